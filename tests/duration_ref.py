"""Float64 reference of the expected state durations (ka_ctc_state_durations) and what the kernels'
single-precision steps may cost them.

    D(s) = sum_t gamma_t(s)        B(s) = sum_t t gamma_t(s)

from posterior_ref.forward_backward(full=True)'s gamma.  The kernels add, per cell, the float the state call writes, in
float64.  The error model is the triangle inequality over the per-cell model of that float (posterior_ref.state_error_model
and the rule that goes with it: a cell the reference puts below 2^-120 comes out in [0, 2^-119)), plus the float64 adds, n_s of
them of a relative 2^-53 each on a running sum that never exceeds the total - 2^-52 n_s D(s) bounds them with room:

    E_D(s) = sum_t e(gamma_t(s)) + 2^-52 n_s D(s)      e(g) = state_error_model(g) for g >= 2^-120, else 2^-119
    E_B(s) = sum_t t e(gamma_t(s)) + 2^-52 n_s B(s)    n_s = number of frames whose band holds s

The tolerance is M_DURATION x E with the state call's multiplier.  A position no band holds has
E = 0 and must read exactly 0.
"""
import math

import numpy as np

import posterior_ref as R

M_DURATION = R.M_STATE


def cell_error(g):
    g = np.asarray(g, np.float64)
    return np.where(g >= R.TINY, R.state_error_model(np.where(g >= R.TINY, g, 1.0)), R.TINY_OUT)


def durations(ref, L):
    """dict(D, B, E_D, E_B, n) over [0, L) from forward_backward(full=True)'s result."""
    D, B, E_D, E_B = (np.zeros(L) for _ in range(4))
    n = np.zeros(L, np.int64)
    for t in range(len(ref["gamma"]) - 1, -1, -1):          # (the kernels' order; float64 here is far below the model either way)
        lo, g = ref["gamma"][t]
        s = slice(int(lo), int(lo) + len(g))
        e = cell_error(g)
        D[s] += g
        B[s] += t * g
        E_D[s] += e
        E_B[s] += t * e
        n[s] += 1
    E_D += 2.0 ** -52 * n * D
    E_B += 2.0 ** -52 * n * B
    return dict(D=D, B=B, E_D=E_D, E_B=E_B, n=n)


def duration_ratio(got, want, E, n, what=""):
    """Worst |got - want| / E over the positions some band holds; the others must read exactly 0.0 (asserted here)."""
    got, want, E = (np.asarray(x, np.float64).reshape(-1) for x in (got, want, E))
    inside = np.asarray(n).reshape(-1) > 0
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.all(got[~inside] == 0.0) and not np.any(np.signbit(got[~inside])), (what, "a position outside every band is not 0.0")
    if not inside.any():
        return 0.0
    assert np.all(E[inside] > 0.0), what
    return float(np.max(np.abs(got[inside] - want[inside]) / E[inside]))      # (a NaN in ``got`` makes this NaN: no m admits it)


def sums_ratio(got_D, got_B, dref, T):
    """(|sum D - T| / sum E_D, |sum B - T (T - 1) / 2| / sum E_B): the two identities against the summed model (the second is
    0 for T = 1, where B is 0 exactly)."""
    eD, eB = math.fsum(dref["E_D"]), math.fsum(dref["E_B"])
    rD = abs(math.fsum(np.asarray(got_D, np.float64)) - T) / eD
    dB = abs(math.fsum(np.asarray(got_B, np.float64)) - T * (T - 1) / 2.0)
    return rD, (dB / eB if eB > 0.0 else (0.0 if dB == 0.0 else math.inf))


def sequential_sums(rows, band_lo, L):
    """What the kernels must give bit for bit: the state call's float rows (K = T, frames 0 .. T-1) added in float64, one
    position at a time, over t = T-1 ... 0."""
    T = rows.shape[0]
    lo_t = np.asarray(band_lo, np.int64)
    D, B = np.zeros(L), np.zeros(L)
    for t in range(T - 1, -1, -1):
        lo = int(lo_t[t])
        w = min(rows.shape[1], L - lo)
        g = rows[t, :w].astype(np.float64)
        D[lo:lo + w] += g                                    # (columns past the band hold 0.0: adding them changes no bit)
        B[lo:lo + w] += np.float64(t) * g
    return D, B


def best_paths_histogram(lp, labels, terminal, beam, mm, eps=1e-6):
    """The best path's histogram over [0, L), and the share of best paths that sit at the likeliest cell of every frame.

    posterior_ref.peaked draws labels with value 0 and repeated neighbours, so several paths can emit the same column in
    every frame and tie for the best score exactly (their posteriors are then 1/2, 3/7, ...).  The histogram is therefore the
    mean over every path within ``eps`` nats of the best one: a max-plus forward and backward pass that also counts the best
    paths through each cell.  Without ties it is the one best path's histogram."""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    lab = R.expand(labels)
    L = len(lab)
    lo, hi = R.windows(T, L, beam)
    NINF = -np.inf

    def step(src_lo, src, src_n, s_lo, s_hi, forward):
        """max and count over the moves into (forward) or out of (backward) the cells [s_lo, s_hi)."""
        sc = np.full(s_hi - s_lo, NINF)
        cn = np.zeros(s_hi - s_lo)
        for k, s in enumerate(range(s_lo, s_hi)):
            for j in range(mm):
                u = s - j if forward else s + j
                into = s if forward else u
                if not (src_lo <= u < src_lo + len(src)) or (j >= 2 and j % 2 == 0 and lab[into] == 0):
                    continue
                v = src[u - src_lo]
                if v == NINF:
                    continue
                if v > sc[k] + eps:
                    sc[k], cn[k] = v, src_n[u - src_lo]
                elif v >= sc[k] - eps:
                    cn[k] += src_n[u - src_lo]
        return sc, cn

    fs, fn = [], []
    plo, prev, pn = 0, np.zeros(1), np.ones(1)
    for t in range(T):
        sc, cn = step(plo, prev, pn, lo[t], hi[t], True)
        sc = sc + lp[t, lab[lo[t]:hi[t]]]
        fs.append(sc)
        fn.append(cn)
        plo, prev, pn = lo[t], sc, cn
    best, total = fs[T - 1][terminal - lo[T - 1]], fn[T - 1][terminal - lo[T - 1]]
    hist = np.zeros(L)
    sure = np.zeros(T)
    bs = np.where(np.arange(lo[T - 1], hi[T - 1]) == terminal, 0.0, NINF)
    bn = (bs == 0.0).astype(np.float64)
    for t in range(T - 1, -1, -1):
        on = np.abs(fs[t] + bs - best) <= eps * T
        w = np.where(on, fn[t] * bn, 0.0) / total
        hist[lo[t]:hi[t]] += w
        sure[t] = w.max()
        if t > 0:
            g = bs + lp[t, lab[lo[t]:hi[t]]]
            bs, bn = step(lo[t], g, bn, lo[t - 1], hi[t - 1], False)
    return hist, sure


def peaked_bound(dref):
    """How far D may lie from the best paths' histogram on posterior_ref.peaked inputs: per frame whose band holds s, the
    model's error of a cell that is certain, e(1.0) = 2^-23.  Every other column lies 20 nats or more below the path's, so a
    path that leaves the best ones for a frame weighs e^-20 = 2e-9 at most, and the V/2 live columns times the few moves that
    can do so stay below 2^-23 = 1.2e-7 a frame."""
    return dref["n"] * float(R.state_error_model(1.0))


def likeliest_path(ref):
    """The likeliest state of every frame."""
    return np.array([int(lo) + int(np.argmax(g)) for lo, g in ref["gamma"]], np.int64)


def peaked_boundaries(path, hist, n_phonemes, want=3):
    """Frames b of a path at which the boundary align() would read is one every best path crosses in the same frame: the
    tied-path histogram's prefix sum at the cut is the path's own crossing frame exactly."""
    prefix = np.concatenate([np.zeros(1), np.cumsum(hist)])
    reached = np.maximum.accumulate(path)
    good = []
    for b in range(1, len(path)):
        c = 2 * min(int(path[b]) // 2, n_phonemes)
        if prefix[c] == float(np.searchsorted(reached, c)) and path[b] != path[b - 1]:
            good.append(b)
    return [good[(k + 1) * len(good) // (want + 1)] for k in range(want)] if len(good) >= want else []
