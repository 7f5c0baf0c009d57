"""Float64 reference of the state visit probabilities (ka_ctc_state_visits) and what the kernels'
roundings may cost them.

    exit_t(s) = gamma_t(s) r_t(s)        V(s) = sum_t exit_t(s)        X(s) = sum_t t exit_t(s)

gamma from posterior_ref.forward_backward(full=True); r_t(s) from a backward pass of its own, which repeats that function's
beta recurrence and keeps the recurrence's terms x_j = beta_{t+1}(s+j) + lp[t+1, lab'[s+j]] (-inf outside band t+1 or for a
vetoed move), with the contract's rules: r = 1 at t = T-1 and where x_0 is -inf, r = 0 where no x_j, j >= 1, is finite,
otherwise 1 - exp(x_0 - lse_j x_j) clamped to [0, 1].

The error model, per cell (t, s) and then summed by the triangle inequality.  The kernels add fl(g r) to V and fl(t fl(g r))
to X, g the float the state call writes and r a float64:
  (1) g against gamma            posterior_ref.state_error_model(gamma), times r <= 1
  (2) r against the float64 r    the exponent e = x_0 - lse is a difference of two values of frame t + 1's column.  Each frame
                                 of a backward pass rounds a column by at most 2^-52 (S_u + 4) log2 units, S_u the largest
                                 finite |x| of frame u's column (an add of the emission, then exp, sum, log and add of the
                                 log-sum-exp, which is a convex combination and so does not amplify what it inherits); the
                                 kernels' columns are these less a running offset of at most the same size, so theirs round by
                                 at most twice that.  Reference plus kernel, on both values of the difference: 6 times the sum
                                 over the frames u > t.  Then the kernels' own steps at the cell: lse - n, + n, x_0 - that, each
                                 2^-53 of at most S_{t+1} + 2, and the sum's max_move exp2 and one log2: 2^-52 (S_{t+1} + 2 M + 8)
                                 bounds them.  d r / d e = -ln 2 (1 - r).  Then exp2's ulp and the subtraction from 1: 2^-52.
                                 All of it times gamma; none of it where the rules make r exactly 0 or 1.
  (3) the product g r            2^-53 gamma r
  (4) X only: the product with t 2^-53 t gamma r
  (5) the adds                   n_s of them of a relative 2^-53 each on a running sum that never exceeds the total:
                                 2^-52 n_s V(s), 2^-52 n_s X(s), n_s the number of frames whose band holds s
A cell the reference puts below 2^-120 comes out in [0, 2^-119) (posterior_ref), times an r <= 1: it is given 2^-119.
The tolerance is M_VISIT x E.  A position with E = 0 must have the reference's value exactly, which is then 0.0 or, for X of a
position that only frame 0 leaves, 0.0 as well.
"""
import itertools

import numpy as np

import posterior_ref as R

# twice the worst |kernel - float64| / E measured on the MI355X over tests/test_state_visits_gpu.py, rounded up to two digits
# (profiles/posterior_accuracy.json): 0.945 for visit and for exit_time alike, at cells whose float
# argument rounds by nearly all of its half ulp where r is 1
M_VISIT = 1.9
FAULTS = ("veto_stay", "stay_outside", "skip_last", "t_plus_1", "stale_top", "missed_retire")


def visits(lp, labels, terminal, beam, mm, fault=None):
    """dict(V, X, E_V, E_X, n, r, D, B) over [0, L): the reference, its model, n_s, r as a list of (lo, array over the window)
    and the durations' D and B from the same gamma.  ``fault`` = (name, at): one of FAULTS, a mistake a kernel could make -
      veto_stay      the stay term is read from the vetoable copy of the column: -inf where the label value is 0
      stay_outside   a position that band t+1 no longer holds reads the stay term of the band's nearest cell
      skip_last      frame T-1 is not counted
      t_plus_1       X is weighted with t + 1
      stale_top      block ``at``'s top frame (t = 32 at + 31) takes r from the column of frame t + 2
      missed_retire  the positions that leave the band below frame ``at`` + 1 are never written out (they read 0.0)"""
    kind, at = fault if fault else (None, None)
    assert kind is None or kind in FAULTS, kind
    ref = R.ref_at(lp, labels, terminal, beam, mm)
    assert ref["status"] == R.OK
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    lab = R.expand(labels)
    L = len(lab)
    zero = lab == 0
    lo, hi = R.windows(T, L, beam)
    V, X, D, B, E_V, E_X = (np.zeros(L) for _ in range(6))
    n = np.zeros(L, np.int64)
    rs = [None] * T
    nxt = np.where(np.arange(lo[T - 1], hi[T - 1]) == terminal, 0.0, -np.inf)        # beta over window T-1
    cols = {}                                                                        # t -> (lo, hi, column of frame t)
    inherited = 0.0                                                                  # sum over u > t of S_u + 4
    for t in range(T - 1, -1, -1):
        glo, g = ref["gamma"][t]
        s = np.arange(lo[t], hi[t])
        exact = np.ones(len(s), bool)                                                # r is 0 or 1 by rule
        de = 0.0
        if t == T - 1:
            r = np.ones(len(s))
        else:
            nlo, nhi = lo[t + 1], hi[t + 1]
            col = nxt + lp[t + 1, lab[nlo:nhi]]
            cols[t + 1] = (nlo, nhi, col)
            fin = np.isfinite(col)
            scale = float(np.max(np.abs(col[fin]))) * R.LOG2E if fin.any() else 0.0
            inherited += scale + 4.0
            de = 2.0 ** -52 * (6.0 * inherited + scale + 2.0 * mm + 8.0)

            def terms(nlo, nhi, col):
                out = []
                for j in range(mm):
                    u = s + j
                    ok = (u >= nlo) & (u < nhi)
                    if j >= 2 and j % 2 == 0:
                        ok &= ~zero[np.minimum(u, L - 1)]
                    c = np.full(len(s), -np.inf)
                    c[ok] = col[u[ok] - nlo]
                    out.append(c)
                return np.array(out)
            x = terms(nlo, nhi, col)
            nxt = R._lse(x) if len(s) else np.zeros(0)                               # beta_t, whatever the fault
            if kind == "stale_top" and t == R.CK * at + R.CK - 1 and t + 2 < T:
                x = terms(*cols[t + 2])
            x0 = x[0].copy()
            if kind == "veto_stay":
                x0[zero[s]] = -np.inf
            if kind == "stay_outside" and nhi > nlo:
                out = (s < nlo) | (s >= nhi)
                x0[out] = col[np.clip(s[out], nlo, nhi - 1) - nlo]
            other = np.isfinite(x[1:]).any(axis=0) if mm > 1 else np.zeros(len(s), bool)
            lse = R._lse(np.vstack([x0[None], x[1:]]))
            with np.errstate(invalid="ignore"):
                soft = np.clip(1.0 - np.exp(np.where(np.isfinite(x0), x0 - lse, -np.inf)), 0.0, 1.0)
            r = np.where(~np.isfinite(x0), 1.0, np.where(other, soft, 0.0))
            exact = ~np.isfinite(x0) | ~other
        rs[t] = (int(lo[t]), r)
        eps_r = np.where(exact, 0.0, (1.0 - r) * R.LN2 * de + 2.0 ** -52)
        big = g >= R.TINY
        gs = np.where(big, g, 1.0)
        e = np.where(big, R.state_error_model(gs) * r + g * eps_r + 2.0 ** -53 * g * r, R.TINY_OUT)
        e = np.where(big & exact & (r == 0.0), 0.0, e)
        sl = slice(int(lo[t]), int(hi[t]))
        D[sl] += g
        B[sl] += t * g
        n[sl] += 1
        if kind == "skip_last" and t == T - 1:
            continue
        tw = t + 1 if kind == "t_plus_1" else t
        V[sl] += g * r
        X[sl] += tw * (g * r)
        E_V[sl] += e
        E_X[sl] += t * e + 2.0 ** -53 * t * g * r
    if kind == "missed_retire":
        V[hi[at]:hi[at + 1]] = 0.0
        X[hi[at]:hi[at + 1]] = 0.0
    E_V += 2.0 ** -52 * n * V
    E_X += 2.0 ** -52 * n * X
    return dict(V=V, X=X, E_V=E_V, E_X=E_X, n=n, r=rs, D=D, B=B, gamma=ref["gamma"], ll=ref["ll"], ref=ref)


def visit_ratio(got, want, E, what=""):
    """Worst |got - want| / E over the positions with E > 0; the others must have the reference's value exactly."""
    got, want, E = (np.asarray(x, np.float64).reshape(-1) for x in (got, want, E))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    free = E > 0.0
    assert np.array_equal(got[~free], want[~free]) and not np.any(np.signbit(got[~free])), (what, "a position without a model differs")
    if not free.any():
        return 0.0
    return float(np.max(np.abs(got[free] - want[free]) / E[free]))                   # (a NaN in ``got`` makes this NaN: no m admits it)


def sequential(lp, labels, terminal, beam, mm):
    """(V, X) by enumerating every path of the band that ends at the terminal: the probability-weighted indicator of passing
    through s, and the last frame spent there (tiny lattices only)."""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    lab = R.expand(labels)
    L = len(lab)
    lo, hi = R.windows(T, L, beam)
    total, V, X = 0.0, np.zeros(L), np.zeros(L)
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
        for t, st in enumerate(states):
            if t == T - 1 or states[t + 1] != st:
                V[st] += p
                X[st] += p * t
    return (V / total, X / total) if total > 0 else (None, None)


def single_frame_positions(T, L, beam):
    """The positions that exactly one frame's band holds: there visit must have duration's bits."""
    lo, hi = R.windows(T, L, beam)
    n = np.zeros(L, np.int64)
    for a, b in zip(lo, hi):
        n[a:b] += 1
    return n == 1


def best_paths_visits(lp, labels, terminal, beam, mm, eps=1e-6):
    """The share of the best paths that pass through every position, the mean over every path within ``eps`` nats of the best
    one as duration_ref.best_paths_histogram takes it: a max-plus forward and backward pass that counts the best paths through
    each cell and through each stay; a cell's exits are its paths less those that stay."""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    lab = R.expand(labels)
    L = len(lab)
    lo, hi = R.windows(T, L, beam)
    NINF = -np.inf

    def step(src_lo, src, src_n, s_lo, s_hi, forward):
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
    visit = np.zeros(L)
    bs = np.where(np.arange(lo[T - 1], hi[T - 1]) == terminal, 0.0, NINF)
    bn = (bs == 0.0).astype(np.float64)
    g = gn = None                                                                    # frame t + 1: beta + emission, and its counts
    for t in range(T - 1, -1, -1):
        on = np.abs(fs[t] + bs - best) <= eps * T
        through = np.where(on, fn[t] * bn, 0.0)
        stay = np.zeros(len(through))
        if t < T - 1:
            for k, s in enumerate(range(lo[t], hi[t])):
                if lo[t + 1] <= s < hi[t + 1] and g[s - lo[t + 1]] != NINF and abs(fs[t][k] + g[s - lo[t + 1]] - best) <= eps * T:
                    stay[k] = fn[t][k] * gn[s - lo[t + 1]]
        visit[lo[t]:hi[t]] += (through - stay) / total
        if t > 0:
            g, gn = bs + lp[t, lab[lo[t]:hi[t]]], bn
            bs, bn = step(lo[t], g, bn, lo[t - 1], hi[t - 1], False)
    return visit
