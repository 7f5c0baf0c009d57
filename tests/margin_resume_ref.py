"""Float64 NumPy reference of ``ka_ctc_margins_resume`` (include/kokoro_align_amd.h), written from the definition alone: it
shares no code with the product (``expand`` and ``band_of`` are margin_ref's helpers).

    D_{-1} = d_in, or {0: 0.0};   D_t(p) = max_j D_{t-1}(p-j) + lp[t, lab'[p]]     p in band t, p-j in band t-1 (t = 0: p-j >= 0
                                                                                   alone: no band applies to d_in), veto on lab'[p]
    E_{T-1} = e_in over band T-1, or {terminal: 0.0};   E_t(p) = max_j E_{t+1}(p+j) + lp[t+1, lab'[p+j]]   p+j in band t+1, veto
    m = D + E;  score = max over band T-1 of m;  d_out = D_{T-1} over band T-1, -inf elsewhere
    e_out[p] = max_j E_0(p+j) + lp[0, lab'[p+j]]    p+j in band 0, veto on lab'[p+j]; p in [max(lo_0-(M-1), 0), hi_0), -inf elsewhere
    rows[k][j] = m_{f_k}(lo_k + j), -inf for j in [hi_k - lo_k, W);  rows_lo[k] = lo_k

Every sum is one float64 add of exactly widened operands and every maximum is exact, so the product must match bit for bit.
``FAULTS`` names the mistakes a kernel of this kind can make; each is a keyword of ``resume_ref`` that plants it.
"""
import numpy as np

from margin_ref import BAD_ARGS, BAD_LABEL, NAN, NONFINITE, OK, ZERO_MASS, band_of, bits, expand, table_valid  # noqa: F401

FAULTS = (
    "e_out_no_emission",   # e_out: E_0 moved back without the emission of frame 0
    "cut_veto_dropped",    # the moves across either cut (d_in -> frame 0, frame 0 -> e_out) without the veto
    "band_on_d_in",        # band 0 applied to d_in: the cells below lo_0 dropped
    "e_in_one_cell",       # e_in seeded at its best cell only
    "d_out_unmasked",      # d_out outside band T-1: what the column held before, not -inf
    "rows_no_offset",      # rows[k][j] = m(j), not m(lo_k + j)
    "row_tail",            # the tail [hi-lo, W) of a row left at 0.0
    "score_at_path_end",   # under an end row: the score read at path[T-1] alone
)


def _failed(T, L, K, W, status, path):
    nan = np.nan
    return {"status": status, "score": -np.inf if status == ZERO_MASS else nan,
            "through": np.full(T, nan), "alt": np.full(T, nan), "runner_up": np.full(T, -1, np.int32),
            "rows": np.full((K, W), nan), "rows_lo": np.full(K, -1, np.int64), "d_out": np.full(L, nan), "e_out": np.full(L, nan)}


def resume_ref(lp, labels, beam, max_move, band_lo=None, path=None, d_in=None, e_in=None, terminal=-1, unit=0, frames=(), *,
               e_out_no_emission=False, cut_veto_dropped=False, band_on_d_in=False, e_in_one_cell=False, d_out_unmasked=False,
               rows_no_offset=False, row_tail=False, score_at_path_end=False, cells=False):
    """dict(status, score, through, alt, runner_up, rows [K, W], rows_lo [K], d_out [L], e_out [L]); through / alt / runner_up
    are None without a path.  ``cells``: also D, E, m as [T, L] (-inf outside the band) and the band (lo, hi)."""
    lp32 = np.asarray(lp, np.float32)
    T, V = lp32.shape
    labels = np.asarray(labels, np.int64).reshape(-1)
    lab = expand(labels)
    L = len(lab)
    frames = np.asarray(frames, np.int64).reshape(-1)
    K, W = len(frames), max(1, min(beam, L))
    M = max_move
    ninf = -np.inf
    if path is not None:
        path = np.asarray(path, np.int64).reshape(-1)
    fail = lambda st: _failed(T, L, K, W, st, path)
    if len(labels) and (labels.min() < 0 or labels.max() >= V):
        return fail(BAD_LABEL)
    if band_lo is not None and not table_valid(band_lo, T, L):
        return fail(BAD_ARGS)
    if np.isnan(lp32).any():
        return fail(NAN)
    if np.isposinf(lp32).any():
        return fail(NONFINITE)
    if path is not None and (path.min() < 0 or path.max() >= L):
        return fail(BAD_ARGS)
    for row in (d_in, e_in):
        if row is not None and (np.isnan(row).any() or np.isposinf(row).any()):
            return fail(BAD_ARGS)
    if e_in is None:
        sstar = int(terminal) if terminal >= 0 else int(path[T - 1])
        if not 0 <= sstar < L:
            return fail(BAD_ARGS)
    lo, hi = band_of(T, L, beam, band_lo)
    lpd = lp32.astype(np.float64)
    zero_label = lab == 0

    def open_move(j, targets, across=False):
        """[len(targets)] bool: may move j land on these positions?  (an even j >= 2 may not land on a label VALUE 0)"""
        if j >= 2 and j % 2 == 0 and not (across and cut_veto_dropped):
            return ~zero_label[targets]
        return np.ones(len(targets), bool)

    with np.errstate(invalid="ignore"):
        # ---- D ----
        if d_in is None:
            start = np.full(L, ninf)
            start[0] = 0.0
        else:
            start = np.asarray(d_in, np.float64).copy()
            if band_on_d_in:
                start[:lo[0]] = ninf
                start[hi[0]:] = ninf
        D = np.full((T, L), ninf)
        for t in range(T):
            prev = start if t == 0 else D[t - 1]
            plo, phi = (0, L) if t == 0 else (lo[t - 1], hi[t - 1])
            p = np.arange(lo[t], hi[t], dtype=np.int64)
            best = np.full(len(p), ninf)
            for j in range(M):
                q = p - j
                ok = (q >= plo) & (q < phi) & open_move(j, p, across=(t == 0))
                best = np.maximum(best, np.where(ok, prev[np.clip(q, 0, L - 1)], ninf))
            D[t, lo[t]:hi[t]] = best + lpd[t, lab[p]]
        # ---- E ----
        E = np.full((T, L), ninf)
        b0, b1 = lo[T - 1], hi[T - 1]
        if e_in is None:
            if b0 <= sstar < b1:
                E[T - 1, sstar] = 0.0
        else:
            e_in = np.asarray(e_in, np.float64)
            if e_in_one_cell:
                v = D[T - 1, b0:b1] + e_in[b0:b1]
                at = b0 + int(np.argmax(v))
                E[T - 1, at] = e_in[at]
            else:
                E[T - 1, b0:b1] = e_in[b0:b1]

        def step_back(Enext, t_next, p, across=False, emission=True):
            """max_j Enext(p+j) + lp[t_next, lab'[p+j]] over the moves into band t_next"""
            best = np.full(len(p), ninf)
            for j in range(M):
                q = p + j
                qc = np.clip(q, 0, L - 1)
                ok = (q >= lo[t_next]) & (q < hi[t_next]) & open_move(j, qc, across=across)
                g = Enext[qc] + (lpd[t_next, lab[qc]] if emission else 0.0)
                best = np.maximum(best, np.where(ok, g, ninf))
            return best

        for t in range(T - 2, -1, -1):
            E[t, lo[t]:hi[t]] = step_back(E[t + 1], t + 1, np.arange(lo[t], hi[t], dtype=np.int64))
        m = D + E
        last = m[T - 1, b0:b1]
        if e_in is not None and score_at_path_end and path is not None:
            score = float(m[T - 1, path[T - 1]])
        else:
            score = float(last.max())
        if score == ninf:
            return fail(ZERO_MASS)
        d_out = np.full(L, ninf)
        if d_out_unmasked:
            d_out = (D[T - 2] if T > 1 else start).copy()
        d_out[b0:b1] = D[T - 1, b0:b1]
        e_out = np.full(L, ninf)
        w0 = max(lo[0] - (M - 1), 0)
        e_out[w0:hi[0]] = step_back(E[0], 0, np.arange(w0, hi[0], dtype=np.int64), across=True, emission=not e_out_no_emission)

    through = alt = runner = None
    if path is not None:
        through, alt, runner = np.full(T, ninf), np.full(T, ninf), np.full(T, -1, np.int32)
        for t in range(T):
            pt = int(path[t])
            if lo[t] <= pt < hi[t]:
                through[t] = m[t, pt]
            alt[t], runner[t] = row_alt(m[t, lo[t]:hi[t]], lo[t], pt, unit)
    rows = np.full((K, W), 0.0 if row_tail else ninf)
    rows_lo = np.zeros(K, np.int64)
    for k, f in enumerate(frames):
        w = hi[f] - lo[f]
        base = 0 if rows_no_offset else lo[f]
        src = m[f, base:base + w]
        rows[k, :len(src)] = src
        rows_lo[k] = lo[f]
    out = {"status": OK, "score": score, "through": through, "alt": alt, "runner_up": runner, "rows": rows, "rows_lo": rows_lo,
           "d_out": d_out, "e_out": e_out}
    if cells:
        out.update(D=D, E=E, m=m, lo=lo, hi=hi)
    return out


def row_alt(row, lo, pt, unit):
    """(alt, runner_up) of a frame read off its row of m (``row[j]`` = m(lo + j)): the maximum outside the group of ``pt`` and
    the lowest position attaining it; (-inf, -1) where there is none."""
    pos = lo + np.arange(len(row), dtype=np.int64)
    other = (pos >> unit) != (pt >> unit)
    if not other.any():
        return -np.inf, -1
    v = np.asarray(row, np.float64)[other]
    a = v.max()
    if a == -np.inf:
        return -np.inf, -1
    return float(a), int(pos[other][v == a][0])


def split_ref(lp, labels, beam, max_move, band_lo, cuts, path=None, terminal=-1, e_in=None, unit=0, frames=(), **fault):
    """The lattice cut at ``cuts`` (ascending, in [1, T)) and run as the header's property 2 says: a forward sweep hands every
    chunk's d_out on, then the chunks run newest first, each ending at its successor's e_out.  Returns a dict in resume_ref's
    form with the chunks' outputs concatenated, ``score`` the last chunk's, ``scores`` every chunk's, and the first non-zero
    status of any chunk.  ``band_lo`` is required (a chunk of the diagonal is no diagonal)."""
    lp = np.asarray(lp, np.float32)
    T = lp.shape[0]
    band_lo = np.asarray(band_lo, np.int64)
    edges = [0] + [int(c) for c in cuts] + [T]
    frames = np.asarray(frames, np.int64).reshape(-1)
    chunks = list(zip(edges[:-1], edges[1:]))
    starts, row = [], None
    free = np.zeros(2 * len(np.asarray(labels).reshape(-1)) + 1)
    for a, b in chunks[:-1]:
        starts.append(row)
        r = resume_ref(lp[a:b], labels, beam, max_move, band_lo[a:b], None, row, free, **fault)
        row = r["d_out"]          # (NaN after a failed chunk: the next chunk fails too)
    starts.append(row)
    parts, end, scores = [None] * len(chunks), e_in, [None] * len(chunks)
    for i in range(len(chunks) - 1, -1, -1):
        a, b = chunks[i]
        last = i == len(chunks) - 1
        sub = frames[(frames >= a) & (frames < b)] - a
        term = terminal if last and e_in is None else -1
        r = resume_ref(lp[a:b], labels, beam, max_move, band_lo[a:b], None if path is None else path[a:b], starts[i], end,
                       term if end is None else -1, unit, sub, **fault)
        parts[i], scores[i], end = r, r["score"], r["e_out"]
    status = next((p["status"] for p in reversed(parts) if p["status"] != OK), OK)
    cat = lambda key: None if parts[0][key] is None else np.concatenate([p[key] for p in parts])
    return {"status": status, "score": scores[-1], "scores": scores, "through": cat("through"), "alt": cat("alt"),
            "runner_up": cat("runner_up"), "rows": np.concatenate([p["rows"] for p in parts]), "rows_lo": cat("rows_lo"),
            "d_out": parts[-1]["d_out"], "e_out": parts[0]["e_out"]}


def same(a, b, keys=("through", "alt", "runner_up", "rows", "rows_lo", "d_out", "e_out")):
    """Do two answers agree bit for bit on ``keys``, the status and the score?"""
    if a["status"] != b["status"] or bits([a["score"]])[0] != bits([b["score"]])[0]:
        return False
    for k in keys:
        x, y = a.get(k), b.get(k)
        if (x is None) != (y is None):
            return False
        if x is None:
            continue
        x, y = np.asarray(x), np.asarray(y)
        if x.shape != y.shape or not (np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y)):
            return False
    return True
