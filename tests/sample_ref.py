"""Float64 NumPy forward filter, backward sample over the band: the reference the path sampling kernels are tested against
(include/kokoro_align_amd.h).

The lattice is posterior_ref's: its ``windows``, ``expand``, moves and veto, and alpha as ``forward_backward`` forms it
(``alphas`` repeats that function's forward loop, because ``forward_backward`` keeps alpha only at the path and as gamma;
tests/test_sample_paths_cpu.py holds the two to the same frame maxima, alpha at the terminal and gamma).  With u = alpha
(any base: only differences enter), sample k is s_{T-1} = s* and, for t = T-1 ... 1 and p = s_t,
    x_j = u_{t-1}(p - j) if p - j is in window t-1 and the move is not vetoed at lab'[p], else -inf         j in [0, max_move)
    w_j = exp(x_j - max x);  tot = w_0 + ... + w_{M-1} in ascending j;  r = U(k, t-1) tot
    s_{t-1} = p - j*, j* the smallest j with w_0 + ... + w_j > r; none (rounding): the largest j with w_j > 0
    U(k, t) = (mix(seed, k T + t) >> 11) 2^-53, mix = oracle.oracle._mix
``fault``: one of FAULTS, a deliberate mistake of the kind a kernel could make.
"""
import numpy as np

import posterior_ref as R
from oracle.oracle import _mix

FAULTS = ("cdf_not_strict", "no_veto", "prev_band", "block_edge", "u_shift")
DELTA = 2.0 ** -26      # a draw is undecidable if U lies within DELTA of a threshold c_j / tot, j < M - 1


def uniforms(seed, K, T):
    """U(k, t) for k in [0, K), t in [0, T): float64 [K, T]."""
    idx = (np.arange(K, dtype=np.uint64)[:, None] * np.uint64(T) + np.arange(T, dtype=np.uint64)[None, :]).reshape(-1)
    return ((_mix(int(seed) & 0xFFFFFFFFFFFFFFFF, idx) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(K, T)


def alphas(lp, labels, beam, mm):
    """(lo, hi, [alpha_t over window t]) in nats: the forward loop of posterior_ref.forward_backward."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0]
    lab = R.expand(labels)
    lo, hi = R.windows(T, len(lab), beam)
    out = []
    plo, prev = 0, np.zeros(1)
    for t in range(T):
        s = np.arange(lo[t], hi[t])
        labs = lab[s]
        cands = []
        for j in range(mm):
            u = s - j
            ok = (u >= plo) & (u < plo + len(prev))
            if j >= 2 and j % 2 == 0:
                ok &= labs != 0
            c = np.full(len(s), -np.inf)
            c[ok] = prev[u[ok] - plo]
            cands.append(c)
        a = (R._lse(np.array(cands)) if len(s) else np.zeros(0)) + lp[t, labs]
        out.append(a)
        plo, prev = lo[t], a
    return lo, hi, out


class Lattice:
    """alpha of one lattice, and the draws on it; every method takes arrays of frames and states of one shape."""

    def __init__(self, lp, labels, beam, mm):
        self.T = np.asarray(lp).shape[0]
        self.lab = R.expand(labels)
        self.mm = mm
        self.lo, self.hi, self.alpha = alphas(lp, labels, beam, mm)
        self.A = np.full((self.T, max(1, int(np.max(self.hi - self.lo)))), -np.inf)
        for t, a in enumerate(self.alpha):
            self.A[t, :len(a)] = a

    def weights(self, t, p, fault=None):
        """w_j [..., M] of the draws from states p at frames t >= 1 into frames t-1 (all zero: no allowed predecessor has mass)."""
        t, p = np.asarray(t, np.int64), np.asarray(p, np.int64)
        q = t - 1
        band = t if fault == "prev_band" else q
        if fault == "block_edge":           # the slab's first row (alpha of t) in place of the checkpoint (alpha of t-1)
            q = np.where(t % R.CK == 0, t, q)
        zero = self.lab[np.clip(p, 0, len(self.lab) - 1)] == 0
        x = np.full(t.shape + (self.mm,), -np.inf)
        for j in range(self.mm):
            u = p - j
            ok = (u >= self.lo[band]) & (u < self.hi[band]) & (u >= self.lo[q]) & (u < self.hi[q])
            if j >= 2 and j % 2 == 0 and fault != "no_veto":
                ok &= ~zero
            x[..., j] = np.where(ok, self.A[q, np.clip(u - self.lo[q], 0, self.A.shape[1] - 1)], -np.inf)
        mx = np.max(x, axis=-1, keepdims=True)
        with np.errstate(invalid="ignore"):
            return np.where(np.isfinite(mx), np.exp(x - np.where(np.isfinite(mx), mx, 0.0)), 0.0)

    def running_sums(self, t, p):
        """(c_j / tot [..., M], w_j) of the draws from ANY states p at frames t >= 1 into frames t-1; the sums run in
        ascending j."""
        w = self.weights(t, p)
        c = np.cumsum(w, axis=-1)
        tot = c[..., -1:]
        return c / np.where(tot > 0, tot, 1.0), w

    def step(self, t, p, u, fault=None):
        """s_{t-1} given s_t = p and the uniforms u."""
        w = self.weights(t, p, fault)
        c = np.cumsum(w, axis=-1)
        r = np.asarray(u)[..., None] * c[..., -1:]
        over = (c >= r) if fault == "cdf_not_strict" else (c > r)
        last = self.mm - 1 - np.argmax((w > 0)[..., ::-1], axis=-1)          # the largest j with w_j > 0 (M - 1 if none: never taken)
        last = np.where(np.any(w > 0, axis=-1), last, 0)
        return np.asarray(p) - np.where(np.any(over, axis=-1), np.argmax(over, axis=-1), last)

    def choice(self, t, p, u):
        """(the reference's s_{t-1}, undecidable?, may an undecidable draw go to state ``got``: a function of got) per draw.
        An undecidable draw may go to either neighbour of a threshold it is near: j itself, or the next j with weight."""
        c, w = self.running_sums(t, p)
        want = self.step(t, p, u)
        near = np.abs(np.asarray(u)[..., None] - c[..., :self.mm - 1]) <= DELTA            # [..., M-1]

        def allowed(got):
            j = np.asarray(p) - got
            ok = np.zeros(np.shape(want), bool)
            for i in range(self.mm - 1):
                nxt = np.full(np.shape(want), -1)
                for i2 in range(self.mm - 1, i, -1):
                    nxt = np.where(w[..., i2] > 0, i2, nxt)
                ok |= near[..., i] & (((j == i) & (w[..., i] > 0)) | ((j == nxt) & (nxt >= 0)))
            return ok
        return want, np.any(near, axis=-1), allowed


def sample_paths(lp, labels, terminal, K, seed, beam, mm, fault=None, lattice=None):
    """int32 [K, T]: the reference's samples."""
    lat = lattice or Lattice(lp, labels, beam, mm)
    T = lat.T
    U = uniforms(seed, K, T)
    paths = np.zeros((K, T), np.int32)
    p = np.full(K, int(terminal), np.int64)
    paths[:, T - 1] = p
    for t in range(T - 1, 0, -1):
        p = lat.step(np.full(K, t), p, U[:, t if fault == "u_shift" else t - 1], fault)
        paths[:, t - 1] = p
    return paths


def _draws(paths):
    K, T = paths.shape
    t = np.broadcast_to(np.arange(1, T, dtype=np.int64), (K, T - 1))
    return t, paths[:, 1:].astype(np.int64), paths[:, :-1].astype(np.int64)


def undecidable_draws(lat, paths, seed):
    """How many draws of ``paths`` (any sampler's, at its own visited states) lie within DELTA of a threshold."""
    K, T = paths.shape
    if T < 2:
        return 0
    t, p, _ = _draws(paths)
    return int(np.sum(lat.choice(t, p, uniforms(seed, K, T)[:, :-1])[1]))


def check_draws(lat, paths, seed, terminal):
    """Every draw of a sampler's paths against the reference, at the sampler's own states: (wrong draws as rows (k, t-1, got,
    want), undecidable count).  A path that diverged at a tie is still checked below it."""
    K, T = paths.shape
    wrong = [(k, T - 1, int(paths[k, T - 1]), int(terminal)) for k in range(K) if paths[k, T - 1] != terminal]
    if T < 2:
        return wrong, 0
    t, p, got = _draws(paths)
    want, tie, allowed = lat.choice(t, p, uniforms(seed, K, T)[:, :-1])
    bad = (got != want) & ~(tie & allowed(got))
    wrong += [(int(k), int(f), int(got[k, f]), int(want[k, f])) for k, f in zip(*np.nonzero(bad))]
    return wrong, int(np.sum(tie))


def valid_path(lat, path, terminal):
    """None, or what is wrong with a path: it ends at the terminal, never moves down, moves less than max_move, never skips
    onto label value 0, stays in every frame's band, and starts within a legal move of the virtual state 0."""
    T = lat.T
    if path[T - 1] != terminal:
        return "does not end at the terminal"
    prev = 0
    for t in range(T):
        p = int(path[t])
        j = p - prev
        if not (lat.lo[t] <= p < lat.hi[t]):
            return f"frame {t}: {p} outside the band"
        if j < 0 or j >= lat.mm:
            return f"frame {t}: move {j}"
        if j >= 2 and j % 2 == 0 and lat.lab[p] == 0:
            return f"frame {t}: a skip onto label value 0"
        prev = p
    return None


def path_probabilities(lp, labels, terminal, beam, mm):
    """{path tuple: probability} by enumerating every path of the band that ends at the terminal (tiny lattices only): the
    enumeration of posterior_ref.brute_force, kept per path."""
    import itertools
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0]
    lab = R.expand(labels)
    lo, hi = R.windows(T, len(lab), beam)
    out = {}
    for moves in itertools.product(range(mm), repeat=T):
        s, score, states, ok = 0, 0.0, [], True
        for t, j in enumerate(moves):
            s += j
            if not (lo[t] <= s < hi[t]) or (j >= 2 and j % 2 == 0 and lab[s] == 0):
                ok = False
                break
            score += lp[t, lab[s]]
            states.append(s)
        if ok and states[-1] == terminal and np.isfinite(score):
            out[tuple(states)] = np.exp(score)
    total = sum(out.values())
    return {k: v / total for k, v in out.items()}
