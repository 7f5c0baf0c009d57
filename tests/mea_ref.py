"""Float64 NumPy restatement of the maximum-expected-accuracy alignment (include/kokoro_align_amd.h):
the reference ka_ctc_mea_path is tested against.

It takes gamma as an argument - a list of per-frame arrays over the band [lo_t, hi_t) - so it runs on posterior_ref's float64
gamma and on the float32 rows the GPU returned (``rows_to_gamma``) alike.  Backwards, in float64, one add per cell:
    W_{T-1}(p) = gamma_{T-1}(p) if p = s*, else -inf
    W_t(p)     = gamma_t(p) + max_j W_{t+1}(p + j),  j in [0, max_move), p + j in band t+1, not (j even, j >= 2, lab'[p+j] == 0)
    c_t(p)     = the smallest j that attains the maximum
then forwards from the virtual state 0: s_0 the smallest allowed start j < max_move in band 0 that maximises W_0(j),
s_{t+1} = s_t + c_t(s_t); the value is W_0(s_0).
"""
import itertools

import numpy as np

import posterior_ref as R

CK = R.CK
FAULTS = ("no_veto", "next_band", "tie_high", "terminal_free", "start_free", "block_edge")
NINF = -np.inf
LEFT_BAND = -8                                             # mea()'s status for a walk that a seeded fault led out of the band


def _skip(j):
    return j >= 2 and j % 2 == 0


def mea(gamma, lo, hi, labels, terminal, max_move, fault=None):
    """dict(status, path int64 [T], value float, W list of float64 arrays over the bands, code list of int arrays).  ``fault``:
    one of FAULTS, a deliberate mistake of the kind a kernel could make, for tests/test_mea_path_cpu.py:
      no_veto        the label-0 veto of even moves is dropped
      next_band      successors are checked against frame t's band instead of frame t+1's
      tie_high       the largest j on a tie
      terminal_free  W_{T-1} = gamma at every position, not at the terminal alone
      start_free     s_0 anywhere in band 0
      block_edge     the recursion is restarted at every 32-frame edge (W of a block's last frame is its gamma alone)"""
    assert fault is None or fault in FAULTS, fault
    lab = R.expand(labels)
    L = len(lab)
    T = len(gamma)
    Ws, codes = [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        g = np.asarray(gamma[t], np.float64)
        s = np.arange(lo[t], hi[t])
        assert len(g) == len(s), (t, len(g), len(s))
        c = np.zeros(len(s), np.int64)
        if t == T - 1:
            W = g.copy() if fault == "terminal_free" else np.where(s == terminal, g, NINF)
        elif fault == "block_edge" and (t + 1) % CK == 0:
            W = g.copy()
        else:
            nlo, nhi = lo[t + 1], hi[t + 1]
            clo, chi = (lo[t], hi[t]) if fault == "next_band" else (nlo, nhi)
            best = np.full(len(s), NINF)
            for j in range(max_move):
                u = s + j
                ok = (u >= clo) & (u < chi) & (u >= nlo) & (u < nhi)
                if _skip(j) and fault != "no_veto":
                    ok &= lab[np.minimum(u, L - 1)] != 0
                x = np.full(len(s), NINF)
                x[ok] = Ws[t + 1][u[ok] - nlo]
                better = (x > best) | ((x == best) & np.isfinite(x)) if fault == "tie_high" else x > best
                c = np.where(better, j, c)
                best = np.where(better, x, best)
            W = g + best
        Ws[t], codes[t] = W, c
    if fault == "start_free":
        starts = list(range(lo[0], hi[0]))
    else:
        starts = [j for j in range(max_move) if lo[0] <= j < hi[0] and not (_skip(j) and lab[j] == 0)]
    best, s0 = NINF, None
    for j in starts:
        if Ws[0][j - lo[0]] > best:
            best, s0 = Ws[0][j - lo[0]], j
    if s0 is None:
        return dict(status=R.ZERO_MASS, path=np.full(T, -1, np.int64), value=np.nan, W=Ws, code=codes)
    path = np.full(T, -1, np.int64)
    path[0] = s0
    for t in range(T - 1):
        if not lo[t] <= path[t] < hi[t]:                  # only a seeded fault walks out of the band: the rest stays -1
            return dict(status=LEFT_BAND, path=path, value=float(best), W=Ws, code=codes)
        path[t + 1] = path[t] + codes[t][path[t] - lo[t]]
    return dict(status=R.OK, path=path, value=float(best), W=Ws, code=codes)


def rows_to_gamma(rows, band_lo, lo, hi):
    """The float32 rows of ka_ctc_state_posteriors at every frame as mea()'s gamma: row t's first hi_t - lo_t columns, after a
    check that the call's band_lo is the reference band's."""
    assert np.array_equal(np.asarray(band_lo, np.int64), np.asarray(lo, np.int64))
    return [np.asarray(rows[t, :hi[t] - lo[t]], np.float32) for t in range(len(lo))]


def replay(rows, band_lo, labels, terminal, beam, max_move):
    """mea() on the rows of a K = T state-posterior call: what ka_ctc_mea_path must return bit for bit."""
    T = rows.shape[0]
    lo, hi = R.windows(T, 2 * len(labels) + 1, beam)
    return mea(rows_to_gamma(rows, band_lo, lo, hi), lo, hi, labels, terminal, max_move)


def reference(ref, labels, terminal, beam, max_move, fault=None):
    """mea() on the float64 gamma of posterior_ref.ref_at."""
    T = len(ref["gamma"])
    lo, hi = R.windows(T, 2 * len(labels) + 1, beam)
    return mea([g for _, g in ref["gamma"]], lo, hi, labels, terminal, max_move, fault)


def brute_force(gamma, lo, hi, labels, terminal, max_move):
    """(value, path) by enumerating every band path that ends at the terminal (tiny lattices only).  Among the paths of the
    largest value, the one the tie rule picks: the smallest start, then the smallest move at every frame in turn - paths are
    enumerated in that (lexicographic) order and only a strictly larger sum replaces the held one.  A path's sum is formed as
    the recursion forms it, from the last frame down, so equal paths have equal bits."""
    lab = R.expand(labels)
    T = len(gamma)
    best, best_path = NINF, None
    for moves in itertools.product(range(max_move), repeat=T):
        s, states, ok = 0, [], True
        for t, j in enumerate(moves):
            s += j
            if not (lo[t] <= s < hi[t]) or (_skip(j) and lab[s] == 0):
                ok = False
                break
            states.append(s)
        if not ok or states[-1] != terminal:
            continue
        v = 0.0
        for t in range(T - 1, -1, -1):
            v = float(np.float64(gamma[t][states[t] - lo[t]])) + v
        if v > best:
            best, best_path = v, np.array(states, np.int64)
    return best, best_path


def validity(path, lo, hi, labels, terminal, max_move):
    """None if ``path`` is a band path that ends at the terminal, else what is wrong with it."""
    lab = R.expand(labels)
    p = np.asarray(path, np.int64)
    step = np.diff(np.concatenate([np.zeros(1, np.int64), p]))
    if np.any((p < lo) | (p >= hi)):
        return "a state outside its band at frame %d" % int(np.flatnonzero((p < lo) | (p >= hi))[0])
    if np.any((step < 0) | (step >= max_move)):
        return "a step outside [0, max_move) into frame %d" % int(np.flatnonzero((step < 0) | (step >= max_move))[0])
    veto = (step >= 2) & (step % 2 == 0) & (lab[p] == 0)
    if np.any(veto):
        return "a vetoed step into frame %d" % int(np.flatnonzero(veto)[0])
    if p[-1] != terminal:
        return "the path ends at %d, not at the terminal" % int(p[-1])
    return None


def unique_peaked(T, S, V, beam, max_move, seed):
    """posterior_ref.peaked's construction with distinct labels of non-zero value (S <= V - 1), as the sampler's test builds
    it: near one-hot rows along one random legal path, which is then the unique best path and holds all the mass.  Returns
    (lp, labels, states)."""
    rng = np.random.default_rng(seed)
    labels = (1 + rng.permutation(V - 1)[:S]).astype(np.int32)
    lab = R.expand(labels)
    L = len(lab)
    lo, hi = R.windows(T, L, beam)
    s, states = 0, []
    for t in range(T):
        want = min(L - 1, (L * (t + 1)) // T + int(rng.integers(-1, 2)))
        ok = [j for j in range(max_move) if lo[t] <= s + j < hi[t] and not (_skip(j) and lab[s + j] == 0)]
        assert ok, "unique_peaked(): the walk left the band"
        s += min(ok, key=lambda j: abs(s + j - want))
        states.append(s)
    logits = -rng.uniform(30.0, 60.0, size=(T, V))
    logits[np.arange(T), lab[states]] = 0.0
    return R._normalise(logits), labels, np.array(states, np.int64)


# ---------------------------------------------------------------------------------------
# Against the float64 reference.  e = posterior_ref.state_error_model bounds |gamma_kernel - gamma_ref|
# per cell.  W_t is a sum of T - t gammas along a path, each off by at most max_s e(gamma_t'(s)), in float64 adds of values
# below T: |W_kernel - W_ref| <= E_t = sum_{t' >= t} max_s e(gamma_t'(s)) + 2^-52 (T - t) T along any one path.  The kernel
# picks the successor whose W_kernel is largest, so in W_ref its choice is within 2 E_{t+1} of the best allowed successor's
# (each of the two values compared is off by at most E), and its path's sum of gamma_ref within 2 E_0 of the optimum.
# ---------------------------------------------------------------------------------------
M_MEA = 2.0
# Cases of posterior_ref.edge_cases() in which more than 1 % of the reference path's steps are near ties (near_tie_share; the
# peaked family's label value 0 and repeated neighbours make best paths tie exactly, and two edge-hugging lattices cross frames
# of negligible mass).  A near tie cannot fail the check of choices - it is a tolerance - so the GPU test runs these cases
# like the others; the share is a reported property of the inputs, and tests/test_mea_path_cpu.py asserts it on either side
# of the line so that a change of the inputs shows.
NEAR_TIED = ("edge_T200_S230_V39_B32_M4_back1", "edge_T400_S150_V39_B16_M5_back1", "peaked_T200_S60_V39_B16_M4",
             "peaked_T260_S120_V39_B1000_M4", "peaked_T180_S50_V39_B12_M6")


def error_bounds(ref):
    """[T + 1] E_t (E_T = 0) from posterior_ref.ref_at's gamma."""
    T = len(ref["gamma"])
    per = np.array([float(np.max(R.state_error_model(g))) if len(g) else 0.0 for _, g in ref["gamma"]])
    tail = np.concatenate([np.cumsum(per[::-1])[::-1], np.zeros(1)])
    return tail + 2.0 ** -52 * (T - np.arange(T + 1)) * T


def _successors(W_next, p, nlo, nhi, lab, max_move):
    """(j, W_{t+1}(p + j)) of every allowed successor of p."""
    out = []
    for j in range(max_move):
        u = p + j
        if nlo <= u < nhi and not (_skip(j) and lab[u] == 0):
            out.append((j, W_next[u - nlo]))
    return out


def choice_ratio(path, ref, mref, labels, max_move):
    """The worst (best allowed successor's W_ref - the chosen successor's W_ref) / E_{t+1} over the steps of ``path`` (and of
    the start), and the deficit of its sum of gamma_ref to the optimum over E_0.  ``mref`` = reference(ref, ...).  Both are
    held against M_MEA."""
    lab = R.expand(labels)
    T = len(path)
    lo = [g[0] for g in ref["gamma"]]
    hi = [g[0] + len(g[1]) for g in ref["gamma"]]
    E = error_bounds(ref)
    W = mref["W"]
    starts = _successors(W[0], 0, lo[0], hi[0], lab, max_move)
    worst = (max(x for _, x in starts) - W[0][path[0] - lo[0]]) / E[0]
    for t in range(T - 1):
        succ = _successors(W[t + 1], int(path[t]), lo[t + 1], hi[t + 1], lab, max_move)
        got = W[t + 1][path[t + 1] - lo[t + 1]]
        top = max(x for _, x in succ)
        if np.isfinite(top) and E[t + 1] > 0.0:
            worst = max(worst, (top - got) / E[t + 1])
        else:
            assert got == top, (t, got, top)
    total = float(sum(ref["gamma"][t][1][path[t] - lo[t]] for t in range(T)))
    return float(worst), float((mref["value"] - total) / E[0])


def near_tie_share(ref, mref, labels, max_move):
    """The share of the reference path's steps (the start included) at which the best allowed successor beats the second
    best by less than the step's tolerance M_MEA E_{t+1}: where the kernel's path may legitimately leave the reference's."""
    lab = R.expand(labels)
    path = mref["path"]
    T = len(path)
    lo = [g[0] for g in ref["gamma"]]
    hi = [g[0] + len(g[1]) for g in ref["gamma"]]
    E = error_bounds(ref)
    near = 0
    for t in range(-1, T - 1):
        p = 0 if t < 0 else int(path[t])
        xs = sorted((x for _, x in _successors(mref["W"][t + 1], p, lo[t + 1], hi[t + 1], lab, max_move) if np.isfinite(x)), reverse=True)
        if len(xs) >= 2 and xs[0] - xs[1] < M_MEA * E[t + 1]:
            near += 1
    return near / T
