"""Float64 NumPy forward-backward over the band of the best-path DP: the reference the posterior kernels are tested against.

Definition (include/kokoro_align_amd.h): lab'[2i] = 0, lab'[2i+1] = labels[i], L = 2S+1; window
[lo_t, hi_t) with lo_t = max(0, L t // T - beam // 2), hi_t = min(lo_t + beam, L); moves j in [0, max_move), a move with
j >= 2, j even, into a state whose label is 0 vetoed; virtual state 0 with score 0 before frame 0.
    alpha_t(s) = logsumexp_j alpha_{t-1}(s-j) + lp[t, lab'[s]]
    Z          = alpha_{T-1}(s*), s* = path[T-1]
    beta_t(s)  = logsumexp_j beta_{t+1}(s+j) + lp[t+1, lab'[s+j]],  beta_{T-1} = {s*: 0}
    post[t]    = exp(alpha_t(p_t) + beta_t(p_t) - Z)
Vectorised per frame; raw log domain (float64 holds ~1e5 to 1e-11).
"""
import itertools

import numpy as np

OK, BAD_ARGS, BAD_LABEL, NAN, NONFINITE, ZERO_MASS = 0, -2, -5, -6, -7, -9
CK = 32                                  # frames per block of the kernels' offsets and checkpoints (kPostCk)
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
FAULTS = ("lo_high", "hi_low", "no_veto_fwd", "bwd_drop_move", "stale_row", "late_label", "short_offset", "beta_seed")
DEEP_FAULTS = ("max32",)                 # seen only by the deep inputs at the end of this file (tests/test_posterior_deep_cpu.py)


def windows(T, L, beam):
    t = np.arange(T, dtype=np.int64)
    lo = np.maximum(0, (L * t) // T - beam // 2)
    hi = np.minimum(lo + beam, L)
    return lo, hi


def expand(labels):
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    lab = np.zeros(2 * len(labels) + 1, np.int64)
    lab[1::2] = labels
    return lab


def _lse(stack, max32=False):
    m = np.max(stack, axis=0)
    safe = np.where(np.isfinite(m), m, 0.0)
    if max32:
        # The fault "max32": the maximum taken off the sum is rounded to float32 in log2 units, as a float maximum on the
        # kernels' doubles does.  In exact arithmetic that changes nothing: max32 + log sum exp(x - max32) is the same number.  It
        # bites where exp(x - max32) leaves float64's range and the sum comes out 0 or inf; only there does the faulty value
        # replace the clean one, so that the fault is not drowned in the rounding noise of an absolute alpha of 1e4 nats (one ulp
        # of which is 2e-12, and would move a gamma near 1 by that much whatever the perturbation).
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            clean = safe + np.log(np.sum(np.exp(stack - safe), axis=0))
            m32 = (safe * LOG2E).astype(np.float32).astype(np.float64) * LN2
            faulty = m32 + np.log(np.sum(np.exp(stack - m32), axis=0))
            return np.where(np.isfinite(m), np.where(np.isfinite(faulty), clean, faulty), -np.inf)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), safe + np.log(np.sum(np.exp(stack - safe), axis=0)), -np.inf)


def forward_backward(log_probs, labels, path, beam_size=1000, max_move=4, full=False, fault=None):
    """Returns dict(status, post float64 [T], ll, gamma, alpha_at, fmax) - gamma (list of (lo, array over the window)) only
    with full=True; alpha_at [T] is alpha at the path and fmax [T] the largest alpha of each frame (nats), from which the
    error models below rebuild the kernels' block offsets.  ``fault`` = (name, frame or block): one of FAULTS, a deliberate
    mistake of the kind a kernel could make, for tests/test_posterior_ref_cpu.py."""
    kind, at = fault if fault else (None, None)
    assert kind is None or kind in FAULTS + DEEP_FAULTS, kind
    m32 = kind == "max32"
    lp = np.asarray(log_probs, dtype=np.float64)
    T, V = lp.shape
    lab = expand(labels)
    L = len(lab)
    path = np.asarray(path, dtype=np.int64).reshape(-1)
    nan = np.full(T, np.nan)

    def failed(status, ll=np.nan, last_max=None, last=None):     # every return carries the same keys
        return dict(status=status, post=nan, ll=ll, gamma=None, last_max=last_max, alpha_at=None, fmax=None, last=last)
    if np.any((lab < 0) | (lab >= V)):
        return failed(BAD_LABEL)
    if np.isnan(lp).any():
        return failed(NAN)
    if np.isposinf(lp).any():
        return failed(NONFINITE)
    if len(path) != T or np.any((path < 0) | (path >= L)):
        return failed(BAD_ARGS)
    lo, hi = windows(T, L, beam_size)
    if kind == "lo_high":
        lo = lo.copy()
        lo[at] = min(lo[at] + 1, hi[at])
    if kind == "hi_low":
        hi = hi.copy()
        hi[at] = max(hi[at] - 1, lo[at])
    alpha_at = np.full(T, -np.inf)
    fmax = np.full(T, -np.inf)
    alphas = []
    plo, prev = 0, np.zeros(1)
    for t in range(T):
        s = np.arange(lo[t], hi[t])
        labs = lab[s]
        if kind == "late_label" and t == at and t > 0:          # positions entering the band: the label of one refill ago
            new = s >= hi[t - 1]
            labs = labs.copy()
            labs[new] = lab[np.maximum(s[new] - max(1, hi[t] - hi[t - 1]), 0)]
        row = lp[t - 1] if kind == "stale_row" and t == at and t > 0 else lp[t]
        cands = []
        for j in range(max_move):
            u = s - j
            ok = (u >= plo) & (u < plo + len(prev))
            if j >= 2 and j % 2 == 0 and kind != "no_veto_fwd":
                ok &= labs != 0
            c = np.full(len(s), -np.inf)
            c[ok] = prev[u[ok] - plo]
            cands.append(c)
        a = (_lse(np.array(cands), m32) if len(s) else np.zeros(0)) + row[labs]
        if lo[t] <= path[t] < hi[t]:
            alpha_at[t] = a[path[t] - lo[t]]
        fmax[t] = np.max(a) if len(a) else -np.inf
        if full:
            alphas.append(a)
        plo, prev = lo[t], a
    # short_offset is the crudest of the faults: a whole frame maximum is tens of nats, and anything that looks at the block
    # sees it.  It is here because the offsets are the one part of these kernels a textbook pass does not have at all.
    if kind == "short_offset" and at > 0:       # block ``at``'s offset lacks its last frame maximum: every alpha the kernels
        d = fmax[CK * at - 1] - (fmax[CK * at - 2] if CK * at >= 2 else 0.0)    # hold relative to it comes out short by it
        for t in range(CK * at, min(CK * at + CK, T)):
            alpha_at[t] -= d
            if full:
                alphas[t] = alphas[t] - d
    zero = lab == 0
    ll = alpha_at[T - 1]
    last_max = float(np.max(prev)) if len(prev) else -np.inf     # the last frame's best cell
    a_last = prev
    if ll == -np.inf:
        return failed(ZERO_MASS, -np.inf, last_max, (int(lo[T - 1]), a_last))
    post = np.zeros(T)
    post[T - 1] = 1.0
    sstar = path[T - 1] - (1 if kind == "beta_seed" else 0)
    nxt = np.where(np.arange(lo[T - 1], hi[T - 1]) == sstar, 0.0, -np.inf)   # beta over window T-1
    gamma = [None] * T
    if full:
        gamma[T - 1] = (lo[T - 1], np.exp(alphas[T - 1] + nxt - ll))
    for t in range(T - 2, -1, -1):
        s = np.arange(lo[t], hi[t])
        nlo, nhi = lo[t + 1], hi[t + 1]
        g = nxt + lp[t + 1, lab[nlo:nhi]]
        cands = []
        for j in range(max_move - 1 if kind == "bwd_drop_move" and t == at else max_move):
            u = s + j
            ok = (u >= nlo) & (u < nhi)
            if j >= 2 and j % 2 == 0:
                ok &= ~zero[np.minimum(u, L - 1)]
            c = np.full(len(s), -np.inf)
            c[ok] = g[u[ok] - nlo]
            cands.append(c)
        b = _lse(np.array(cands), m32) if len(s) else np.zeros(0)
        if lo[t] <= path[t] < hi[t]:
            post[t] = np.exp(alpha_at[t] + b[path[t] - lo[t]] - ll)
        if full:
            gamma[t] = (lo[t], np.exp(alphas[t] + b - ll))
        nxt = b
    if kind == "beta_seed":
        post[T - 1] = 0.0                           # the path's last state is not the seeded one
    return dict(status=OK, post=post, ll=float(ll), gamma=gamma if full else None, last_max=last_max, alpha_at=alpha_at, fmax=fmax,
                last=(int(lo[T - 1]), a_last))


def brute_force(log_probs, labels, path, beam_size=1000, max_move=4):
    """(post, ll) by enumerating every path of the band (tiny lattices only)."""
    lp = np.asarray(log_probs, dtype=np.float64)
    T, V = lp.shape
    lab = expand(labels)
    L = len(lab)
    lo, hi = windows(T, L, beam_size)
    path = np.asarray(path, dtype=np.int64)
    total = 0.0
    on_path = np.zeros(T)
    for moves in itertools.product(range(max_move), repeat=T):
        s, score, states, ok = 0, 0.0, [], True
        for t, j in enumerate(moves):
            s += j
            if not (lo[t] <= s < hi[t]) or (j >= 2 and j % 2 == 0 and lab[s] == 0):
                ok = False
                break
            score += lp[t, lab[s]]
            states.append(s)
        if not ok or states[-1] != path[T - 1]:
            continue
        p = np.exp(score)
        total += p
        on_path += p * (np.array(states) == path)
    with np.errstate(divide="ignore", invalid="ignore"):
        return on_path / total, (np.log(total) if total > 0 else -np.inf)


# ---------------------------------------------------------------------------------------
# What the kernels' single-precision steps cost, per output cell, from the float64 reference alone.
# The recurrences run in float64; single precision enters where the design says so:
#   state gamma     (float)arg, arg = log2 gamma: half a float32 ulp of |log2 gamma|, times ln 2 gamma; then the hardware
#                   exp2f, an ulp of its result: 2^-23 gamma
#   label occupancy the same per added cell, 2^-32 per band cell of the bin (32.32 truncation), and the row's float store
#   path posterior  alpha at the path is stored as a float relative to the offset of its 32-frame block (the sum of the
#                   frame maxima before the block's first frame: the largest alpha of the frame before it), and so is
#                   alpha at (T-1, s*), from which Z is formed: half a float32 ulp of each, in log2 units; then the float
#                   store of the posterior
#   Z               that same float at (T-1, s*), and the float64 sums of T offsets on both sides: 2^-53 T max(1, |Z|)
# A tolerance is m x E, m twice the worst ratio |kernel - float64| / E measured on the MI355X over the five posterior GPU
# files (profiles/posterior_accuracy.json, one record per test): 0.983 state, 1.000 label, 0.998 path,
# 1.000 Z, so every m is 2.0.  E bounds every rounding named above and the kernels stay within it: the worst cells are those
# whose float argument rounds by all of its half ulp.  Cells below 2^-120 in the reference must come out below 2^-119 (the
# hardware exp2f flushes what lies below the normal range; nothing near it is asked to be accurate).
# ---------------------------------------------------------------------------------------
M_STATE, M_LABEL, M_PATH, M_Z = 2.0, 2.0, 2.0, 2.0
TINY, TINY_OUT = 2.0 ** -120, 2.0 ** -119


def _hulp32(x):
    """Half a float32 ulp at |x| (0 for a non-finite x)."""
    x = np.abs(np.asarray(x, np.float64))
    fin = np.isfinite(x)
    return np.where(fin, 0.5 * np.spacing(np.where(fin, x, 0.0).astype(np.float32)).astype(np.float64), 0.0)


def state_error_model(g):
    g = np.asarray(g, np.float64)
    with np.errstate(divide="ignore"):
        a = np.log2(g)
    return g * (LN2 * _hulp32(a) + 2.0 ** -23)


def label_error_model(gamma, labels, V):
    """[T, V] from forward_backward(full=True)'s gamma."""
    lab = expand(labels)
    E = np.zeros((len(gamma), V))
    occ = np.zeros((len(gamma), V))
    for t, (lo, g) in enumerate(gamma):
        idx = lab[lo:lo + len(g)]
        np.add.at(E[t], idx, state_error_model(g) + 2.0 ** -32)
        np.add.at(occ[t], idx, g)
    return E + occ * 2.0 ** -24


def block_offsets(ref):
    """[T] the kernels' offset of each frame's block, log2 units: the sum of the frame maxima m_t before the block's first
    frame, which is the largest alpha of the frame before it (alpha_t(s) = C_{t-1} + u_t(s), m_t = max_s u_t(s))."""
    T = len(ref["fmax"])
    first = (np.arange(T) // CK) * CK
    return np.where(first > 0, ref["fmax"][np.maximum(first - 1, 0)], 0.0) * LOG2E


def path_error_model(ref):
    rel = ref["alpha_at"] * LOG2E - block_offsets(ref)
    return ref["post"] * (LN2 * (_hulp32(rel) + _hulp32(rel[-1])) + 2.0 ** -24)


def z_error_model(ref):
    T = len(ref["fmax"])
    rel = ref["alpha_at"][-1] * LOG2E - block_offsets(ref)[-1]
    return float(LN2 * _hulp32(rel) + 2.0 ** -53 * T * max(1.0, abs(ref["ll"])))


def state_tolerance(g):
    return M_STATE * state_error_model(g)


def label_tolerance(gamma, labels, V):
    return M_LABEL * label_error_model(gamma, labels, V)


def path_tolerance(ref):
    return M_PATH * path_error_model(ref)


def z_tolerance(ref):
    return M_Z * z_error_model(ref)


# ---------------------------------------------------------------------------------------
# The per-cell check: every cell the reference puts at 2^-120 or above lies within m x E of it, every cell below that comes
# out in [0, 2^-119); no cell is exempt.  Each *_ratio asserts the second half and returns the worst |got - want| / E of the
# first, which the caller prints, records and holds against its m.
# ---------------------------------------------------------------------------------------
def cells_ratio(got, want, E, what=""):
    got, want, E = (np.asarray(x, np.float64).reshape(-1) for x in (got, want, E))
    big = want >= TINY
    small = got[~big]
    assert np.all((small >= 0.0) & (small < TINY_OUT)), (what, "a cell below 2^-120 in the reference came out at", small.max() if len(small) else None)
    if not big.any():
        return 0.0
    assert np.all(E[big] > 0.0), what
    return float(np.max(np.abs(got[big] - want[big]) / E[big]))     # (a NaN in ``got`` makes this NaN: no m admits it)


def state_ratio(rows, frames, ref, what=""):
    """rows [K, >= window]: the kernel's gamma at ``frames``; ref from forward_backward(full=True)."""
    worst = 0.0
    for k, f in enumerate(frames):
        _, rg = ref["gamma"][int(f)]
        worst = max(worst, cells_ratio(rows[k, :len(rg)], rg, state_error_model(rg), (what, int(f))))
    return worst


def label_ratio(occ, ref, labels, what=""):
    """occ [T, V] of the kernel; ref from forward_backward(full=True) of the same terminal."""
    V = occ.shape[1]
    lab = expand(labels)
    want = np.zeros((len(ref["gamma"]), V))
    for t, (lo, g) in enumerate(ref["gamma"]):
        np.add.at(want[t], lab[lo:lo + len(g)], g)
    return cells_ratio(occ, want, label_error_model(ref["gamma"], labels, V), what)


def path_ratio(post, ref, what=""):
    return cells_ratio(post, ref["post"], path_error_model(ref), what)


def z_ratio(ll, ref):
    return abs(float(ll) - ref["ll"]) / z_error_model(ref)


def ref_at(lp, labels, terminal, beam, mm, fault=None):
    """forward_backward(full=True) of the band's paths that end at ``terminal``."""
    return forward_backward(lp, labels, np.full(np.asarray(lp).shape[0], int(terminal), np.int64), beam, mm, full=True, fault=fault)


# ---------------------------------------------------------------------------------------
# Input families that put mass where the kernels differ from a plain CTC pass (band edges, a sliding label ring, tiny cells).
# Each returns (log-probs float32 [T, V], labels int32 [S]); tests/test_posterior_ref_cpu.py asserts its condition.
# ---------------------------------------------------------------------------------------
def _normalise(logits):
    x = np.asarray(logits, np.float64)
    m = np.max(x, axis=1, keepdims=True)
    return (x - m - np.log(np.sum(np.exp(x - m), axis=1, keepdims=True))).astype(np.float32)


def random_labels(rng, S, V, zero_every=17):
    labels = rng.integers(1, max(V, 2), size=S).astype(np.int32) if V > 1 else np.zeros(S, np.int32)
    if zero_every and S:
        labels[zero_every - 1::zero_every] = 0          # label value 0 at odd positions: the veto of even moves
    return labels


def edge_hugging(T, S, V, beam, seed, boost=12.0):
    """N(0, 1) logits with ``boost`` nats on the label of the band's lowest cell for t < T/2 and of its highest cell after."""
    rng = np.random.default_rng(seed)
    labels = random_labels(rng, S, V)
    lab = expand(labels)
    lo, hi = windows(T, len(lab), beam)
    logits = rng.standard_normal((T, V))
    t = np.arange(T)
    edge = np.where(t < T // 2, lo, hi - 1)
    logits[t, lab[edge]] += boost
    return _normalise(logits), labels


def edge_mass(ref):
    """(lower, upper): the share of frames at which the band's two lowest / two highest cells hold >= 0.5 of gamma."""
    lower = np.mean([g[:2].sum() >= 0.5 for _, g in ref["gamma"]])
    upper = np.mean([g[-2:].sum() >= 0.5 for _, g in ref["gamma"]])
    return float(lower), float(upper)


def sloped(T, S, V, seed, alpha=0.3, zero_every=17):
    """Dirichlet(alpha) rows over labels with value 0 here and there: the family of the older tests, for bands whose slope
    L / T is chosen by the caller (steep: near max_move - 1; flat: far below 1)."""
    rng = np.random.default_rng(seed)
    lp = np.log(np.maximum(rng.dirichlet(np.full(V, alpha), size=T), 1e-300)).astype(np.float32)
    return lp, random_labels(rng, S, V, zero_every)


def band_steps(T, S, beam):
    """How far the window's low end moves per frame: (share of frames it moves >= 2, share of frames it moves at all)."""
    lo, _ = windows(T, 2 * S + 1, beam)
    d = np.diff(lo)
    return (float(np.mean(d >= 2)), float(np.mean(d >= 1))) if len(d) else (0.0, 0.0)


def peaked(T, S, V, beam, mm, seed, floor=-60.0):
    """Near one-hot rows along a random legal path (the others 20 to -floor nats below), labels from half the vocabulary (the
    other columns are -inf throughout), label value 0 first, last and in a run in the middle, and repeated neighbours.
    Returns (lp, labels, terminal): the path's last state."""
    rng = np.random.default_rng(seed)
    used = max(1, V // 2)
    labels = rng.integers(1, max(used, 2), size=S).astype(np.int32) if used > 1 else np.zeros(S, np.int32)
    if S:
        labels[0] = labels[-1] = 0
        labels[S // 2:S // 2 + 3] = 0
        labels[S // 3:S // 3 + 2] = labels[S // 3] if S // 3 < S else 0
    lab = expand(labels)
    L = len(lab)
    lo, hi = windows(T, L, beam)
    s, states = 0, []
    for t in range(T):
        want = min(L - 1, (L * (t + 1)) // T + int(rng.integers(-1, 2)))
        ok = [j for j in range(mm) if lo[t] <= s + j < hi[t] and not (j >= 2 and j % 2 == 0 and lab[s + j] == 0)]
        assert ok, "peaked(): the walk left the band"
        s += min(ok, key=lambda j: abs(s + j - want))
        states.append(s)
    logits = -rng.uniform(20.0, -floor, size=(T, V))
    logits[np.arange(T), lab[states]] = 0.0
    lp = _normalise(logits)
    lp[:, used:] = -np.inf
    return lp, labels, int(states[-1])


def live_terminals(lp, labels, beam, mm):
    """The positions of the last window that some path of the band reaches with mass, best first."""
    T = np.asarray(lp).shape[0]
    got = forward_backward(lp, labels, np.zeros(T, np.int64), beam, mm)
    if got["last"] is None:
        return []
    lo, a = got["last"]
    return [int(lo + k) for k in np.argsort(-a, kind="stable") if np.isfinite(a[k])]


# ---------------------------------------------------------------------------------------
# The cases tests/test_posterior_ref_cpu.py checks the conditions of, for GPU tests of the three calls to run:
# name -> builder of (lp, labels, terminal, beam, max_move).  ``pick`` chooses among the live terminals: 0 the likeliest.
# ---------------------------------------------------------------------------------------
def _sloped_case(T, S, V, beam, mm, seed, pick=0, zero_every=17, alpha=0.3):
    def build():
        lp, labels = sloped(T, S, V, seed, alpha, zero_every)
        live = live_terminals(lp, labels, beam, mm)
        assert live, ("no terminal with mass", T, S, V, beam, mm)
        return lp, labels, live[min(pick, len(live) - 1)], beam, mm
    return build


def _edge_case(T, S, V, beam, mm, seed, back):
    def build():
        lp, labels = edge_hugging(T, S, V, beam, seed)
        return lp, labels, 2 * S - back, beam, mm
    return build


def _peaked_case(T, S, V, beam, mm, seed):
    def build():
        lp, labels, term = peaked(T, S, V, beam, mm, seed)
        return lp, labels, term, beam, mm
    return build


# (T, S, V, beam, max_move): terminal L-1 for even rows, L-2 for odd ones
EDGE_SHAPES = [(400, 150, 39, 16, 4), (400, 150, 39, 64, 4), (300, 140, 64, 9, 3), (200, 230, 39, 32, 4), (400, 150, 80, 64, 4),
               (400, 150, 39, 16, 5), (3000, 1500, 39, 1004, 4), (3000, 1500, 39, 1010, 4)]
# steep: L / T near max_move - 1 (the band slides 2-3 positions a frame); flat: L / T << 1; beams 1, 2, 3 and odd ones
STEEP_SHAPES = [(200, 280, 39, 2, 4), (200, 280, 39, 3, 4), (200, 280, 39, 7, 4), (200, 280, 64, 33, 4), (200, 280, 80, 7, 4),
                (300, 260, 39, 5, 3), (300, 130, 39, 3, 2), (260, 620, 39, 9, 6)]
FLAT_SHAPES = [(300, 10, 39, 1, 4), (300, 10, 39, 2, 4), (300, 10, 39, 3, 4), (300, 10, 39, 5, 3), (640, 3, 39, 1000, 4),
               (300, 10, 80, 1, 4), (300, 10, 39, 2, 6)]
PEAKED_SHAPES = [(200, 60, 39, 16, 4), (150, 100, 64, 64, 3), (300, 40, 80, 9, 4), (260, 120, 39, 1000, 4), (180, 50, 39, 12, 6),
                 (129, 30, 39, 7, 2)]
GEOMETRY_SHAPES = (
    [(T, 5, 39, 1000, 4) for T in (1, 2, 31, 32, 33, 63, 64, 65, 97)] +          # T round the 32-frame block
    [(40, S, 39, 1000, 4) for S in (0, 1, 2)] +
    [(150, 31, 39, 1000, 4), (150, 32, 39, 1000, 4)] +                            # L = 63, 65: a lane more than the wavefront
    [(150, 100, 39, B, 4) for B in (63, 64, 65)] +
    [(600, 511, 39, 1009, 4), (600, 512, 39, 1009, 4), (600, 512, 39, 5000, 4)] + # L = 1023, 1025 round the 1024 slots
    [(700, 600, 39, B, 4) for B in (1008, 1009, 1010)] +                          # the form boundary
    [(100, 30, V, 16, 4) for V in (1, 63, 64, 65)] +
    [(T, 40, 39, 16, 4) for T in (32, 33, 64, 65, 161)] +                         # the block boundary under a sliding window
    [(120, 40, 39, 1000, M) for M in (1, 2, 3, 4, 5, 6)])


def _name(kind, shape, extra=""):
    return kind + "_T%d_S%d_V%d_B%d_M%d" % shape + extra


def fast_form(S, V, beam, mm):
    """Whether the kernels take the one-wavefront form (ka::plan::posterior_fast): band <= 1009, V <= 64, max_move <= 4."""
    return V <= 64 and mm <= 4 and min(beam, 2 * S + 1) <= 1009


def pad_vocabulary(lp, V):
    """The same lattice with unused -inf columns up to V: above 64 columns the kernels take their generic form."""
    out = np.full((lp.shape[0], V), -np.inf, np.float32)
    out[:, :lp.shape[1]] = lp
    return out


def edge_cases():
    cases = {}
    for i, sh in enumerate(EDGE_SHAPES):
        cases[_name("edge", sh, "_back%d" % (i % 2))] = _edge_case(*sh, seed=100 + i, back=i % 2)
    for i, sh in enumerate(STEEP_SHAPES):
        cases[_name("steep", sh)] = _sloped_case(*sh, seed=200 + i, pick=i % 2, zero_every=17 if sh[4] >= 4 else 0)
    for i, sh in enumerate(FLAT_SHAPES):
        cases[_name("flat", sh)] = _sloped_case(*sh, seed=300 + i, pick=i % 2)
    for i, sh in enumerate(PEAKED_SHAPES):
        cases[_name("peaked", sh)] = _peaked_case(*sh, seed=400 + i)
    for i, sh in enumerate(GEOMETRY_SHAPES):
        cases[_name("geom", sh)] = _sloped_case(*sh, seed=500 + i, pick=i % 3, alpha=1.0)
    return cases


def case_shapes():
    """name -> (T, S, V, beam, max_move) of every case of edge_cases()."""
    out = {}
    for kind, shapes in (("edge", EDGE_SHAPES), ("steep", STEEP_SHAPES), ("flat", FLAT_SHAPES), ("peaked", PEAKED_SHAPES),
                         ("geom", GEOMETRY_SHAPES)):
        for i, sh in enumerate(shapes):
            out[_name(kind, sh, "_back%d" % (i % 2) if kind == "edge" else "")] = sh
    return out


def query_frames(T):
    """Every frame of a short lattice; of a long one, the frames round the block boundaries, a spread, and the last block."""
    if T <= 130:
        return np.arange(T, dtype=np.int64)
    f = set([0, 31, 32, 33, 63, 64, 65, T - 1]) | set(range((T - 1) // CK * CK - 1, T)) | set(range(7, T, max(1, T // 23)))
    return np.array(sorted(x for x in f if 0 <= x < T), dtype=np.int64)


def mixed_path(ref, lo_hi, terminal):
    """A path for the path-posterior call: the likeliest state of most frames, the band's lowest cell at every 5th frame, its
    highest at every 7th, position 0 (mostly outside the band) at every 11th; it ends at the terminal."""
    lo, hi = lo_hi
    p = np.array([rlo + int(np.argmax(g)) for rlo, g in ref["gamma"]], np.int64)
    t = np.arange(len(p))
    p[t % 5 == 4] = lo[t % 5 == 4]
    p[t % 7 == 6] = hi[t % 7 == 6] - 1
    p[t % 11 == 10] = 0
    p[-1] = terminal
    return p


# ---------------------------------------------------------------------------------------
# Deep inputs ("magnitude"): rows c = 2^k nats below their neighbours, and single cells masked with a
# large finite constant.  The reference of a deep lattice is forward_backward of the exactly UNSHIFTED float64 rows (row + c), Z
# moved by -sum c_t: adding c_t to every entry of row t changes no posterior, so the reference never sees the magnitude and is
# valid at every rung.  tests/test_posterior_deep_cpu.py asserts the conditions, tests/test_posterior_deep_gpu.py runs the calls.
# ---------------------------------------------------------------------------------------
DEEP_RUNGS = (10, 17, 20, 24, 30, 33, 35, 37, 40, 44)
DEEP_SLACK = 2.0 ** 11      # log2 units: what an ordinary lattice of the deep shapes (T <= 70) adds to an offset beside the shifts
CAP, CAP_FLOOR = 2.0 ** -10, 2.0 ** -20
Z_DEEP_REL = 2.0 ** -40


def deep_rows(base, frames, c):
    """(lp float32 [T, V], shift float64 [T]): ``base`` with the rows at ``frames`` replaced by float32(-c) + d, d a per-label
    offset in {-4, -2, 0, 2, 4} where float32's spacing at c is at most 2 (k <= 24: one d for all those rungs), all zero where
    it exceeds 8; the rows are exactly representable, so lp + shift is the unshifted lattice exactly."""
    lp = np.array(base, np.float32)
    T, V = lp.shape
    assert float(np.float32(c)) == float(c)
    sp = float(np.spacing(np.float32(c)))
    assert sp <= 2.0 or sp > 8.0, c
    d = 2.0 * np.random.default_rng(V).integers(-2, 3, size=V) if sp <= 2.0 else np.zeros(V)
    shift = np.zeros(T)
    for t in frames:
        row = (-float(c) + d).astype(np.float32)
        assert np.array_equal(row.astype(np.float64), -float(c) + d)
        lp[t] = row
        shift[t] = float(c)
    return lp, shift


def deep_unshifted(lp, shift):
    """The float64 rows the reference runs on: row t + shift_t, exact."""
    return np.asarray(lp, np.float64) + np.asarray(shift, np.float64)[:, None]


def deep_ref(lp, shift, labels, terminal, beam, mm, fault=None):
    """ref_at of the unshifted rows; ``ll`` stays the unshifted lattice's, ``z`` is the deep lattice's (ll - sum shift)."""
    ref = ref_at(deep_unshifted(lp, shift), labels, terminal, beam, mm, fault=fault)
    ref["shift"] = np.asarray(shift, np.float64)
    ref["z"] = ref["ll"] - float(np.sum(shift))
    return ref


def shifted_view(ref, shift):
    """What path_error_model, z_error_model and block_offsets read, with the shifts put back: the kernels' offsets and the
    float-stored relative alpha are formed from the shifted maxima."""
    cum = np.cumsum(np.asarray(shift, np.float64))
    return dict(alpha_at=ref["alpha_at"] - cum, fmax=ref["fmax"] - cum, post=ref["post"], ll=ref["ll"] - cum[-1])


def _hulp64(x):
    """Half a float64 ulp at x + DEEP_SLACK for x > 0, else 0."""
    x = np.asarray(x, np.float64)
    return np.where(x > 0.0, 0.5 * np.spacing(np.where(x > 0.0, x + DEEP_SLACK, 1.0)), 0.0)


def deep_roundings(shift):
    """(R [T], h): h = half a float64 ulp of log2 e max c_t, R_t the float64 roundings at that magnitude between the input and a
    cell of frame t, counted from the code:
      5 per deep frame at or before t (forward: the product lp log2 e, e - m_{t-1}, the add to the log-sum-exp; in the frame
        behind it mx + log2 s and e - m_{t-1} again), 3 per deep frame behind t (backward: the product, w + e, mx + log2 s of the
        frame before), 5 per deep frame for Z (the forward pass up to T-1);
      the adds C += m and D += n of every frame behind t (they cancel between alpha, beta and Z up to t), each half an ulp of the
        offset it forms, in units of h;
      6 at the magnitude of Z: (ca + alpha), (D + w), their sum, Z = Ca + u, and the path call's C - Cb and + u."""
    c = np.asarray(shift, np.float64) * LOG2E
    T = len(c)
    if not np.any(c > 0.0):
        return np.zeros(T), 0.0
    h = float(0.5 * np.spacing(np.max(c)))
    deep = c > 0.0
    n_le = np.cumsum(deep)
    n_all = n_le[-1]
    cells = 5.0 * n_le + 3.0 * (n_all - n_le) + 5.0 * n_all
    cmag, dmag = np.cumsum(c), np.cumsum(c[::-1])[::-1]
    adds = _hulp64(cmag) + _hulp64(dmag)                       # frame u's two adds
    behind = np.concatenate([np.cumsum(adds[::-1])[::-1][1:], np.zeros(1)])
    return cells + (behind + 6.0 * _hulp64(cmag[-1])) / h, h


def deep_cost(shift):
    """[T] what a cell of frame t may move by, as a share of its value: ln 2 R_t h."""
    Rn, h = deep_roundings(shift)
    return LN2 * Rn * h


def deep_error_model(call, ref, shift, labels=None, V=None):
    """The call's existing model plus value x deep_cost: "state" -> list over frames of arrays over the window, "label" ->
    [T, V], "path" -> [T] (path_error_model on block_offsets of the shifted maxima: the design's own float store), "z" -> float
    (z_error_model of the shifted values, plus the forward pass's roundings and the add that forms Z)."""
    cost = deep_cost(shift)
    if call == "state":
        return [state_error_model(g) + g * cost[t] for t, (_, g) in enumerate(ref["gamma"])]
    if call == "label":
        lab = expand(labels)
        occ = np.zeros((len(ref["gamma"]), V))
        for t, (lo, g) in enumerate(ref["gamma"]):
            np.add.at(occ[t], lab[lo:lo + len(g)], g)
        return label_error_model(ref["gamma"], labels, V) + occ * cost[:, None]
    if call == "path":
        return path_error_model(shifted_view(ref, shift)) + ref["post"] * cost
    assert call == "z", call
    Rn, h = deep_roundings(shift)
    n_all = float(np.sum(np.asarray(shift) > 0.0))
    return z_error_model(shifted_view(ref, shift)) + LN2 * (5.0 * n_all * h + float(_hulp64(np.sum(shift) * LOG2E)))


def inside_cap(E, value):
    """Is a (case, call) pair compared cell by cell?  Only if E <= 2^-10 value at every cell whose value is >= 2^-20."""
    E, value = (np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in xs]) if isinstance(xs, list) else
                np.asarray(xs, np.float64).reshape(-1) for xs in (E, value))
    big = value >= CAP_FLOOR
    return bool(np.all(E[big] <= CAP * value[big]))


def z_rel_holds(ref, shift):
    """Can the reported Z lie within 2^-40 of the reference, relatively?  Its model from the reference alone says: not where a
    deep frame lies in the last block, whose share of Z goes through the float store of the terminal's relative alpha."""
    return bool(deep_error_model("z", ref, shift) <= Z_DEEP_REL * abs(ref["ll"] - float(np.sum(shift))))


def masked_cells(base, mask, value):
    """(lp with ``value`` at the cells of ``mask`` [T, V] bool, the same lattice with -inf there: the reference's input)."""
    lp, ninf = np.array(base, np.float32), np.array(base, np.float32)
    lp[mask] = np.float32(value)
    ninf[mask] = -np.inf
    return lp, ninf


def masked_mass(ref_value, ref_ninf):
    """The share of the lattice's mass that runs through the masked cells: 1 - Z(-inf there) / Z(the value there), both float64."""
    return float(-np.expm1(ref_ninf["ll"] - ref_value["ll"]))


def deep_row_model(want, shift, which, carried=0.0):
    """A row of ka_ctc_posteriors_resume on a deep chunk ([L] nats, the reference's row less the shifts it carries): the float64
    chain's 2^-53 (frames + 1) max(1, |value|) of fb_resume_ref.row_error_model, plus the roundings of deep_roundings that do
    not cancel in a single row: 5 (alpha_out) or 3 (beta_out) per deep frame, and every frame's add to the offset.  ``carried``:
    the shifts (nats) the chunk's start row (alpha_out) or end row (beta_out) brings from the chunks beside it."""
    want = np.asarray(want, np.float64)
    c = np.asarray(shift, np.float64) * LOG2E
    base = 2.0 ** -53 * (len(c) + 1) * np.maximum(1.0, np.abs(np.where(np.isfinite(want), want, 0.0)))
    if not np.any(c > 0.0) and carried == 0.0:
        return base
    h = float(0.5 * np.spacing(max(np.max(c), carried * LOG2E)))
    mags = carried * LOG2E + (np.cumsum(c) if which == "alpha_out" else np.cumsum(c[::-1]))
    per = 5.0 if which == "alpha_out" else 3.0
    return base + LN2 * (per * float(np.sum(c > 0.0)) * h + float(np.sum(_hulp64(mags))) + 2.0 * float(_hulp64(mags[-1])))


# (T, S, beam, max_move, terminal back from L-1): the window slides under beam 16; 1000 holds every position
DEEP_SHAPES = {"T40_S12_B16_M4": (40, 12, 16, 4, 0), "T70_S20_B16_M4": (70, 20, 16, 4, 1), "T70_S12_B1000_M2": (70, 12, 1000, 2, 0),
               "T40_S20_B1000_M4": (40, 20, 1000, 4, 1)}
DEEP_V = 39


def deep_patterns(T):
    return {"first": [0], "last": [T - 1], "f31": [31], "f32": [32], "f33": [33], "f30_34": list(range(30, 35)),
            "pad8": list(range(T - 8, T)), "lead5": list(range(5)), "all": list(range(T))}


def deep_base(shape):
    """(base log-probs float32 [T, 39]: log-softmax of N(0, 1) logits, labels, terminal, beam, max_move)."""
    T, S, beam, mm, back = DEEP_SHAPES[shape]
    rng = np.random.default_rng(sum(map(ord, shape)))
    labels = random_labels(rng, S, DEEP_V, zero_every=7)
    return _normalise(rng.standard_normal((T, DEEP_V))), labels, 2 * S - back, beam, mm


def deep_case(shape, pattern, k):
    """dict(lp, shift, labels, terminal, beam, mm) of one rung."""
    base, labels, term, beam, mm = deep_base(shape)
    lp, shift = deep_rows(base, deep_patterns(base.shape[0])[pattern], 2.0 ** k)
    return dict(lp=lp, shift=shift, labels=labels, terminal=term, beam=beam, mm=mm)


def deep_ref_key(k):
    """Rungs that share a reference: the rows' offsets d do not depend on k up to 2^24 and are zero above."""
    return "d" if k <= 24 else "zero"


_DEEP_REFS = {}


def deep_built(shape, pattern, k):
    """deep_case with its references: ``ref`` (ref_at of the unshifted rows, shared by the rungs of a deep_ref_key and left
    unchanged), ``path`` (mixed_path through it), ``pref`` (forward_backward along that path) and ``z`` (ll - sum shift)."""
    c = deep_case(shape, pattern, k)
    key = (shape, pattern, deep_ref_key(k))
    if key not in _DEEP_REFS:
        plain = deep_unshifted(c["lp"], c["shift"])
        ref = ref_at(plain, c["labels"], c["terminal"], c["beam"], c["mm"])
        assert ref["status"] == OK, key
        T, L = plain.shape[0], 2 * len(c["labels"]) + 1
        path = mixed_path(ref, windows(T, L, c["beam"]), c["terminal"])
        pref = forward_backward(plain, c["labels"], path, c["beam"], c["mm"])
        assert pref["status"] == OK, key
        _DEEP_REFS[key] = (plain, ref, path, pref)
    plain, ref, path, pref = _DEEP_REFS[key]
    assert np.array_equal(plain, deep_unshifted(c["lp"], c["shift"])), (shape, pattern, k)
    return dict(c, name="%s-%s-k%d" % (shape, pattern, k), shape=shape, pattern=pattern, k=k, plain=plain, ref=ref, path=path, pref=pref,
                z=ref["ll"] - float(np.sum(c["shift"])))


def deep_all(shape):
    return [deep_built(shape, p, k) for p in deep_patterns(DEEP_SHAPES[shape][0]) for k in DEEP_RUNGS]


def deep_caps(c):
    """{call: is the pair compared cell by cell?} for the state, label and path calls of a built case, from the reference alone."""
    ref, shift = c["ref"], c["shift"]
    occ = np.zeros((len(ref["gamma"]), DEEP_V))
    lab = expand(c["labels"])
    for t, (lo, g) in enumerate(ref["gamma"]):
        np.add.at(occ[t], lab[lo:lo + len(g)], g)
    return dict(state=inside_cap(deep_error_model("state", ref, shift), [g for _, g in ref["gamma"]]),
                label=inside_cap(deep_error_model("label", ref, shift, c["labels"], DEEP_V), occ),
                path=inside_cap(deep_error_model("path", c["pref"], shift), c["pref"]["post"]))


MASK_VALUES = (-1e9, -1e30, float(np.finfo(np.float32).min))


def masked_case(shape, value):
    """Single cells of four frames (round a block boundary and at both ends) set to ``value``: the label of the likeliest
    non-blank cell of the frame, so the cell lies beside live alternatives (the blank column among them)."""
    base, labels, term, beam, mm = deep_base(shape)
    ref = ref_at(base, labels, term, beam, mm)
    lab = expand(labels)
    mask = np.zeros(base.shape, bool)
    for t in (3, 31, 32, base.shape[0] - 2):
        lo, g = ref["gamma"][t]
        idx = lab[lo:lo + len(g)]
        mask[t, idx[int(np.argmax(np.where(idx != 0, g, -1.0)))]] = True
    lp, ninf = masked_cells(base, mask, value)
    return lp, ninf, mask, labels, term, beam, mm


# ---------------------------------------------------------------------------------------
# The multipliers of the deep models: twice the worst ratio |kernel - float64| / deep_error_model measured on the MI355X over
# tests/test_posterior_deep_gpu.py, rounded up to two digits (profiles/posterior_accuracy.json, key "deep"; the rule of DESIGN.md
# section 4.21).  Measured: 0.972 state (durations are held to its multiplier: 0.414 and 0.417), 0.999 label, 0.983 path,
# 0.981 Z, 0.494 visit and 0.499 exit_time, 0.254 alpha_out and 0.614 beta_out (a pair of outputs shares the larger of its two
# multipliers).  No ratio exceeds 1: the count of deep_roundings misses no rounding, and is generous where the worst ratio is
# far below 1.
# ---------------------------------------------------------------------------------------
M_DEEP_STATE, M_DEEP_LABEL, M_DEEP_PATH, M_DEEP_Z, M_DEEP_VISIT, M_DEEP_ROW = 2.0, 2.0, 2.0, 2.0, 1.0, 1.3
