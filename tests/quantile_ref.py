"""Float64 reference of the exact boundary-time quantiles (ka_ctc_boundary_quantiles), the integer
definition applied literally to float32 rows, and what the kernels' roundings may move.

    tau_c = the first frame whose state is >= c        P(tau_c <= t) = P(state_t >= c) = F_t(c)
    F_t(c) = 1 where c <= lo_t (the whole band lies at or above the cut), 0 where c >= hi_t, else sum_{p in [c, hi_t)} gamma_t(p)
    quantile[k, m] = the smallest t in [0, T) with F_t(cuts[k]) >= levels[m], T if there is none

``cdf`` forms F in float64 from posterior_ref's gamma, ``frames_of`` reads the quantile frames off it.  ``integer_quantiles``
is the contract itself: rows as ka_ctc_state_posteriors writes them (float32, position lo_t + j at column j), each cell
truncated to 32.32 fixed point, summed as integers, compared with thr_m = ceil(levels[m] 2^32).  A GPU test holds the kernel
against it without any tolerance.

The margin of F_t(c), per (frame, cut): the kernels add fix(g) of every cell at or above the cut, g the float the state call
writes.  |g - gamma| <= posterior_ref.state_error_model(gamma) and the truncation takes less than
2^-32 of a cell, so the margin is the sum over the cells at or above the cut of state_error_model + 2^-32 (a cell the
reference puts below 2^-120 comes out below 2^-119: it is given that).  Where the band lies at or above the cut, or below
it, F is exact and the margin 0.  A (cut, level) pair whose F comes within 2 x margin of the level at some in-band frame can
cross a frame early or late in the kernel; such a pair is left out of a comparison with the float64 frames (``unsafe``), and
a test caps how many there may be.
"""
import itertools

import numpy as np

import posterior_ref as R

FIX = 4294967296.0                       # 2^32
FAULTS = ("gt", "last_frame", "above_early", "above_late", "floor", "cut_index")


def thresholds(levels, fault=None):
    """thr_m = ceil(levels[m] 2^32) as Python ints (the host's double arithmetic)."""
    lv = np.asarray(levels, np.float64).reshape(-1)
    return [int(np.floor(x * FIX)) if fault == "floor" else int(np.ceil(x * FIX)) for x in lv]


def _region(lo, hi, T, t, c, fault):
    """+1: the band of frame t lies at or above cut c; -1: below it; 0: the cut is strictly inside.  The faults move the
    all-above region a frame: above_early takes it from frame t + 1's band, above_late from frame t - 1's, and between the
    two a cut that is not strictly inside has no cells summed for it."""
    if c >= hi[t]:
        return -1
    if c > lo[t]:
        return 0
    if fault == "above_late" and t > 0 and c > lo[t - 1]:
        return -1                                                                    # (the start value came a frame late)
    return 1


def cdf(gamma, cuts, L, beam, fault=None, with_margin=False):
    """F [T, K] in float64 from forward_backward(full=True)'s gamma; with ``with_margin`` also its margin [T, K] and the mask
    [T, K] of the frames at which the cut is strictly inside the band.  ``fault``: one of FAULTS, a mistake a kernel could make -
      gt           the sum starts above the cut: p > c in place of p >= c
      above_early  the all-above region begins a frame early (frame t is given 1 where frame t + 1's band lies above the cut)
      above_late   ... a frame late (the frame at which the band reaches the cut is lost)
      cut_index    row k is computed for cut k + 1 (the last for itself)
    (last_frame and floor act in ``frames_of`` / ``thresholds``)"""
    T = len(gamma)
    lo, hi = R.windows(T, L, beam)
    cuts = np.asarray(cuts, np.int64).reshape(-1)
    if fault == "cut_index" and len(cuts):
        cuts = np.concatenate([cuts[1:], cuts[-1:]])
    F = np.zeros((T, len(cuts)))
    E = np.zeros((T, len(cuts)))
    inside = np.zeros((T, len(cuts)), bool)
    for t in range(T):
        glo, g = gamma[t]
        assert glo == lo[t] and len(g) == hi[t] - lo[t]
        suffix = np.concatenate([np.cumsum(g[::-1])[::-1], np.zeros(1)])             # suffix[j] = sum of g[j:]
        if with_margin:
            big = g >= R.TINY
            e = np.where(big, R.state_error_model(np.where(big, g, 1.0)), R.TINY_OUT) + 2.0 ** -32
            esuf = np.concatenate([np.cumsum(e[::-1])[::-1], np.zeros(1)])
        for k, c in enumerate(cuts):
            where = _region(lo, hi, T, t, int(c), fault)
            if fault == "above_early" and where == 0 and t + 1 < T and c <= lo[t + 1]:
                where = 1
            if where == 1:
                F[t, k] = 1.0
            elif where == 0:
                j = int(c) - int(lo[t]) + (1 if fault == "gt" else 0)
                F[t, k] = suffix[j]
                inside[t, k] = True
                if with_margin:
                    E[t, k] = esuf[j]
    return (F, E, inside) if with_margin else F


def frames_of(F, levels, fault=None):
    """quantile [K, M] int64 from F [T, K]: the first frame at which F reaches the level, T if none (``last_frame``: the last)."""
    T, K = F.shape
    lv = np.asarray(levels, np.float64).reshape(-1)
    out = np.full((K, len(lv)), T, np.int64)
    for m, x in enumerate(lv):
        hit = F >= x
        any_hit = hit.any(axis=0)
        first = (T - 1 - np.argmax(hit[::-1], axis=0)) if fault == "last_frame" else np.argmax(hit, axis=0)
        out[any_hit, m] = first[any_hit]
    return out


def quantiles(lp, labels, terminal, beam, mm, cuts, levels, fault=None, gamma=None):
    """dict(q [K, M], F, E, inside, unsafe [K, M], ll): the float64 reference, its margin, and the pairs whose F comes within
    2 x margin of the level at a frame where the cut is strictly inside the band."""
    if gamma is None:
        ref = R.ref_at(lp, labels, terminal, beam, mm)
        assert ref["status"] == R.OK
        gamma = ref["gamma"]
    L = 2 * len(np.asarray(labels).reshape(-1)) + 1
    kind = fault[0] if isinstance(fault, tuple) else fault
    F, E, inside = cdf(gamma, cuts, L, beam, fault=kind, with_margin=True)
    lv = np.asarray(levels, np.float64).reshape(-1)
    q = frames_of(F, lv, fault=kind)
    unsafe = np.zeros(q.shape, bool)
    for m, x in enumerate(lv):
        unsafe[:, m] = np.any(inside & (np.abs(F - x) <= 2.0 * E), axis=0)
    return dict(q=q, F=F, E=E, inside=inside, unsafe=unsafe)


def integer_sums(rows, band_lo, cuts, L, beam):
    """F_t(c) [T, K] as Python-int valued uint64: the contract applied to float32 rows [T, >= band width] of
    ka_ctc_state_posteriors at ALL T frames (row t holds gamma_t(lo_t + j) at column j)."""
    rows = np.asarray(rows, np.float32)
    T = rows.shape[0]
    lo, hi = R.windows(T, L, beam)
    assert np.array_equal(np.asarray(band_lo, np.int64).reshape(-1), lo)
    cuts = np.asarray(cuts, np.int64).reshape(-1)
    F = np.zeros((T, len(cuts)), np.uint64)
    for t in range(T):
        w = int(hi[t] - lo[t])
        g = rows[t, :w]
        assert np.all((g >= 0.0) & (g <= 1.0))
        fix = (g * np.float32(FIX)).astype(np.uint64)                                # (a float times 2^32 is exact; then truncation)
        suffix = np.concatenate([np.cumsum(fix[::-1], dtype=np.uint64)[::-1], np.zeros(1, np.uint64)])
        j = np.clip(cuts - lo[t], 0, w)
        F[t] = np.where(cuts <= lo[t], np.uint64(1 << 32), np.where(cuts >= hi[t], np.uint64(0), suffix[j]))
    return F


def integer_quantiles(rows, band_lo, cuts, levels, L, beam, fault=None):
    """quantile [K, M] int32: the smallest t with F_t(cuts[k]) >= ceil(levels[m] 2^32), T if there is none."""
    F = integer_sums(rows, band_lo, cuts, L, beam)
    T, K = F.shape
    thr = thresholds(levels, fault)
    out = np.full((K, len(thr)), T, np.int32)
    for m, x in enumerate(thr):
        hit = F >= np.uint64(x)
        any_hit = hit.any(axis=0)
        out[any_hit, m] = np.argmax(hit, axis=0)[any_hit]
    return out


def float32_rows(gamma, W):
    """Rows [T, W] float32 from the reference's gamma, zero past the band: what the state call would write, to its rounding -
    a stand-in for it where there is no GPU."""
    rows = np.zeros((len(gamma), max(W, 1)), np.float32)
    los = np.zeros(len(gamma), np.int64)
    for t, (lo, g) in enumerate(gamma):
        rows[t, :len(g)] = np.minimum(g, 1.0).astype(np.float32)
        los[t] = lo
    return rows, los


def enumerate_cdf(lp, labels, terminal, beam, mm, cuts):
    """(F [T, K], tau_mass) by enumerating every path of the band that ends at the terminal: the share of path mass with
    tau_c <= t, tau_c the first frame whose state is >= c (tiny lattices only)."""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    lab = R.expand(labels)
    L = len(lab)
    lo, hi = R.windows(T, L, beam)
    cuts = np.asarray(cuts, np.int64).reshape(-1)
    total, F = 0.0, np.zeros((T, len(cuts)))
    for moves in itertools.product(range(mm), repeat=T):
        s, score, states, ok = 0, 0.0, [], True
        for t, j in enumerate(moves):
            s += j
            if not (lo[t] <= s < hi[t]) or (j >= 2 and j % 2 == 0 and lab[s] == 0):
                ok = False
                break
            score += lp[t, lab[s]]
            states.append(s)
        if not ok or states[-1] != terminal or score == -np.inf:
            continue
        p = np.exp(score)
        total += p
        st = np.array(states)
        for k, c in enumerate(cuts):
            reached = np.nonzero(st >= c)[0]
            if len(reached):
                F[reached[0]:, k] += p                                               # tau_c <= t from the first such frame on
    return (F / total) if total > 0 else None


def sample_tau(paths, cuts):
    """tau_c [n_samples, K] of sampled paths: the first frame whose state is >= c, T if there is none."""
    p = np.asarray(paths, np.int64)
    reached = np.maximum.accumulate(p, axis=1)
    c = np.asarray(cuts, np.int64).reshape(-1)
    return np.sum(reached[:, :, None] < c[None, None, :], axis=1, dtype=np.int64)
