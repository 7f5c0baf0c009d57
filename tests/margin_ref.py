"""Float64 NumPy reference of ``ka_ctc_path_margins`` (include/kokoro_align_amd.h), written from the definition alone: it
shares no code with the product.

    D_t(p) = max_j ( D_{t-1}(p-j) + lp[t, lab'[p]] )        p in band t, p-j in band t-1, veto on lab'[p]
    E_{T-1} = {s*: 0};  E_t(p) = max_j ( E_{t+1}(p+j) + lp[t+1, lab'[p+j]] )   p+j in band t+1, veto on lab'[p+j]
    m = D + E;  through[t] = m_t(path[t]);  alt[t] = max of m_t outside the path's group;  runner_up[t] = lowest arg-max

Every sum is one float64 add of exactly widened operands and every maximum is exact, so the product must match bit for bit.
``FAULTS`` names the mistakes a kernel of this kind can make; each is a keyword of ``margins_ref`` that plants it, so that the
tests can show that their cases would notice it.
"""
import numpy as np

OK, BAD_ARGS, BAD_LABEL, NAN, NONFINITE, ZERO_MASS = 0, -2, -5, -6, -7, -9

FAULTS = (
    "veto_on_source",    # backward pass: the veto read on lab'[p], not on the target lab'[p+j]
    "band_same_frame",   # backward pass: p+j tested against band t, not band t+1
    "keep_group",        # alt: the path's own group not left out
    "tie_highest",       # runner_up: ties to the highest position
    "ignore_unit",       # unit taken as 0
    "seed_all",          # E seeded at every cell of frame T-1
    "open_start",        # the virtual start open to all of band 0
)


def expand(labels):
    lab = np.zeros(2 * len(labels) + 1, np.int64)
    lab[1::2] = np.asarray(labels, np.int64).reshape(-1)
    return lab


def band_of(T, L, beam, band_lo=None):
    """(lo [T], hi [T]) int64: the table's band, or the diagonal's."""
    if band_lo is None:
        lo = np.maximum(0, (L * np.arange(T, dtype=np.int64)) // T - beam // 2)
    else:
        lo = np.asarray(band_lo, np.int64).reshape(-1)
    return lo, np.minimum(lo + beam, L)


def table_valid(band_lo, T, L):
    b = np.asarray(band_lo, np.int64).reshape(-1)
    return len(b) == T and bool(np.all(b >= 0) and np.all(b < L) and np.all(np.diff(b) >= 0))


def _failed(T, status):
    return {"status": status, "through": np.full(T, np.nan), "alt": np.full(T, np.nan), "runner_up": np.full(T, -1, np.int32),
            "score": -np.inf if status == ZERO_MASS else np.nan}


def margins_ref(lp, labels, path, beam, max_move, unit=0, band_lo=None, *, veto_on_source=False, band_same_frame=False,
                keep_group=False, tie_highest=False, ignore_unit=False, seed_all=False, open_start=False, cells=False, forward_only=False):
    """dict(status, through f64 [T], alt f64 [T], runner_up int32 [T], score); with ``cells`` also D, E, m as [T, L] (-inf
    outside the band) and the band (lo, hi).  ``forward_only``: D alone, whatever the terminal."""
    lp32 = np.asarray(lp, np.float32)
    T, V = lp32.shape
    labels = np.asarray(labels, np.int64).reshape(-1)
    path = np.asarray(path, np.int64).reshape(-1)
    lab = expand(labels)
    L = len(lab)
    if len(labels) and (labels.min() < 0 or labels.max() >= V):
        return _failed(T, BAD_LABEL)
    if band_lo is not None and not table_valid(band_lo, T, L):
        return _failed(T, BAD_ARGS)
    if np.isnan(lp32).any():
        return _failed(T, NAN)
    if np.isposinf(lp32).any():
        return _failed(T, NONFINITE)
    if path.min() < 0 or path.max() >= L:
        return _failed(T, BAD_ARGS)
    lo, hi = band_of(T, L, beam, band_lo)
    lpd = lp32.astype(np.float64)
    if ignore_unit:
        unit = 0
    ninf = -np.inf
    pos = np.arange(L, dtype=np.int64)
    zero_label = lab == 0

    def veto(j, on):   # [L] bool: move j is no move where the label read (`on`) is 0
        return zero_label[on] if (j >= 2 and j % 2 == 0) else np.zeros(len(on), bool)

    with np.errstate(invalid="ignore"):
        D = np.full((T, L), ninf)
        prev = np.full(L, ninf)
        if open_start:
            prev[lo[0]:hi[0]] = 0.0
        else:
            prev[0] = 0.0
        plo, phi = (lo[0], hi[0]) if open_start else (0, 1)
        for t in range(T):
            p = pos[lo[t]:hi[t]]
            best = np.full(len(p), ninf)
            e = lpd[t, lab[p]]
            for j in range(max_move):
                if open_start and t == 0 and j > 0:
                    break
                src = p - j
                ok = (src >= plo) & (src < phi) & ~veto(j, p)
                cand = np.where(ok, prev[np.clip(src, 0, L - 1)], ninf) + e
                best = np.maximum(best, cand)
            D[t, lo[t]:hi[t]] = best
            prev = D[t]
            plo, phi = lo[t], hi[t]
        if forward_only:
            return D
        sstar = int(path[T - 1])
        score = float(D[T - 1, sstar])
        if score == ninf:
            return _failed(T, ZERO_MASS)

        E = np.full((T, L), ninf)
        if seed_all:
            E[T - 1, lo[T - 1]:hi[T - 1]] = 0.0
        else:
            E[T - 1, sstar] = 0.0     # (score is finite: s* lies in band T-1)
        for t in range(T - 2, -1, -1):
            p = pos[lo[t]:hi[t]]
            best = np.full(len(p), ninf)
            blo, bhi = (lo[t], hi[t]) if band_same_frame else (lo[t + 1], hi[t + 1])
            for j in range(max_move):
                dst = p + j
                inside = (dst >= blo) & (dst < bhi) & (dst < L)
                dc = np.clip(dst, 0, L - 1)
                ok = inside & ~veto(j, p if veto_on_source else dc)
                cand = np.where(ok, E[t + 1, dc] + lpd[t + 1, lab[dc]], ninf)
                best = np.maximum(best, cand)
            E[t, lo[t]:hi[t]] = best
        m = D + E

    through = np.full(T, ninf)
    alt = np.full(T, ninf)
    runner = np.full(T, -1, np.int32)
    for t in range(T):
        pt = int(path[t])
        if lo[t] <= pt < hi[t]:
            through[t] = m[t, pt]
        p = pos[lo[t]:hi[t]]
        other = p if keep_group else p[(p >> unit) != (pt >> unit)]
        if len(other):
            v = m[t, other]
            a = v.max()
            if a > ninf:
                alt[t] = a
                hit = other[v == a]
                runner[t] = hit[-1] if tie_highest else hit[0]
    out = {"status": OK, "through": through, "alt": alt, "runner_up": runner, "score": score}
    if cells:
        out.update(D=D, E=E, m=m, lo=lo, hi=hi)
    return out


def margin_of(through, alt):
    """through - alt as the front end forms it: +inf where no alternative exists, NaN where both are -inf."""
    with np.errstate(invalid="ignore"):
        return np.asarray(through, np.float64) - np.asarray(alt, np.float64)


def argmax_path(lp, labels, beam, max_move, band_lo=None):
    """A best path of the lattice as the identities want it: the per-frame arg-max of m, ending at the highest reachable
    terminal.  None if no terminal is reachable."""
    lp32 = np.asarray(lp, np.float32)
    T = lp32.shape[0]
    L = 2 * len(np.asarray(labels).reshape(-1)) + 1
    lo, hi = band_of(T, L, beam, band_lo)
    D = margins_ref(lp32, labels, np.zeros(T, np.int64), beam, max_move, 0, band_lo, forward_only=True)
    live = np.flatnonzero(D[T - 1] > -np.inf) if isinstance(D, np.ndarray) else []
    if len(live) == 0:
        return None
    probe = np.zeros(T, np.int64)
    probe[T - 1] = live[-1]
    r = margins_ref(lp32, labels, probe, beam, max_move, 0, band_lo, cells=True)
    path = np.array([int(lo[t] + np.argmax(r["m"][t, lo[t]:hi[t]])) for t in range(T)], np.int64)
    path[T - 1] = live[-1]
    return path


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.int64)
