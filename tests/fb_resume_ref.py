"""Float64 reference of the forward-backward under the caller's boundary conditions (ka_ctc_posteriors_resume, DESIGN.md
section 4.37), its planted faults, the cases of the CPU and GPU tests and the tolerances of the rows.

``resume(lp, labels, band_lo, beam, mm, alpha_in, end, path)`` is one call: dense float64 rows over [0, L), -inf = no mass.
``chunked(...)`` cuts a lattice at ``cuts`` and runs the chunks as the callers do: a forward sweep that hands alpha_out on as
the next chunk's alpha_in, then the chunks newest first, each chunk's beta_out the previous chunk's end row.  The reference is
checked against banded_fb_ref.ref_at / dense_gamma of the uncut lattice and against path enumeration
(tests/test_fb_resume_cpu.py), never against the GPU.

Planted faults (FAULTS), each a mistake a kernel could make on the cut:
    alpha_in_banded     band 0 applied to the start row: alpha_in read over [lo_0, hi_0) only
    cut_no_veto_fwd     frame 0's moves from a caller's start row run without the veto
    cut_no_veto_bwd     the emission-free step behind frame 0 runs without the veto
    beta_out_short      beta_out over [lo_0, hi_0) only: max_move-1 cells short
    beta_out_drop_move  the emission-free step misses its last move
    alpha_out_unbanded  cells of alpha_out outside band T-1 left finite (frame T-1 computed without its band)
"""
import itertools

import numpy as np

import banded_fb_ref as B
import posterior_ref as R

FAULTS = ("alpha_in_banded", "cut_no_veto_fwd", "cut_no_veto_bwd", "beta_out_short", "beta_out_drop_move", "alpha_out_unbanded")
NINF = -np.inf


def _lse_rows(stack):
    return R._lse(np.asarray(stack))


def _bad_row(x):
    return x is not None and bool(np.any(np.isnan(x) | np.isposinf(x)))


def is_row(end):
    return np.ndim(end) > 0


def resume(lp, labels, band_lo, beam, mm, alpha_in=None, end=None, path=None, fault=None):
    """One resumed call.  ``end``: an int terminal or a row [L].  Returns dict(status, ll, gamma [T, L] dense, windows (lo, hi),
    occ [T, V], path_post [T] or None, alpha_out [L], beta_out [L], alpha [T, L], beta [T, L], c0, cb, us): c0 the offset the
    start row brings, cb the kernels' offset of the last block and us the terminal's alpha relative to its frame's offset, all in
    log2 units (what the sibling's float-stored Z is formed from)."""
    assert fault is None or fault in FAULTS, fault
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    lab = R.expand(labels)
    L = len(lab)
    failed = lambda st, ll=np.nan: dict(status=st, ll=ll, gamma=None, occ=None, path_post=None, alpha_out=None, beta_out=None)
    if np.any((lab < 0) | (lab >= V)):
        return failed(R.BAD_LABEL)
    lo, hi = B.table_windows(band_lo, L, beam)
    if np.any((lo < 0) | (lo >= L)) or np.any(np.diff(lo) < 0):
        return failed(R.BAD_ARGS)
    if np.isnan(lp).any():
        return failed(R.NAN)
    if np.isposinf(lp).any():
        return failed(R.NONFINITE)
    a_in = None if alpha_in is None else np.asarray(alpha_in, np.float64).reshape(-1)
    b_in = np.asarray(end, np.float64).reshape(-1) if is_row(end) else None
    if _bad_row(a_in) or _bad_row(b_in) or (b_in is None and not 0 <= int(end) < L):
        return failed(R.BAD_ARGS)
    zero = lab == 0
    pos = np.arange(L)
    if a_in is None:
        prev = np.full(L, NINF)
        prev[0] = 0.0
    else:
        prev = a_in.copy()
        prev[:max(lo[0] - (mm - 1), 0)] = NINF      # what frame 0 cannot read
        prev[hi[0]:] = NINF
        if fault == "alpha_in_banded":
            prev[:lo[0]] = NINF
    with np.errstate(invalid="ignore"):
        c0 = float(np.max(prev)) * R.LOG2E if np.isfinite(np.max(prev)) else 0.0
    alpha = np.full((T, L), NINF)
    for t in range(T):
        a, b = (0, L) if fault == "alpha_out_unbanded" and t == T - 1 else (lo[t], hi[t])
        s = pos[a:b]
        cands = []
        for j in range(mm):
            u = s - j
            ok = u >= 0
            if j >= 2 and j % 2 == 0 and not (fault == "cut_no_veto_fwd" and t == 0 and a_in is not None):
                ok = ok & ~zero[s]
            c = np.full(len(s), NINF)
            c[ok] = prev[u[ok]]
            cands.append(c)
        row = np.full(L, NINF)
        row[a:b] = _lse_rows(cands) + lp[t, lab[s]]
        alpha[t] = row
        prev = row
    alpha_out = alpha[T - 1].copy()
    if fault == "alpha_out_unbanded":
        alpha[T - 1, :lo[T - 1]] = NINF
        alpha[T - 1, hi[T - 1]:] = NINF
    beta = np.full((T, L), NINF)
    if b_in is None:
        if lo[T - 1] <= int(end) < hi[T - 1]:
            beta[T - 1, int(end)] = 0.0
    else:
        beta[T - 1, lo[T - 1]:hi[T - 1]] = b_in[lo[T - 1]:hi[T - 1]]

    def step_back(G, a, b, nlo, nhi, veto=True, moves=mm):
        """lse_j G(p + j) over the moves from [a, b) into [nlo, nhi)"""
        s = pos[a:b]
        cands = []
        for j in range(moves):
            u = s + j
            ok = (u >= nlo) & (u < nhi)
            if veto and j >= 2 and j % 2 == 0:
                ok = ok & ~zero[np.minimum(u, L - 1)]
            c = np.full(len(s), NINF)
            c[ok] = G[u[ok]]
            cands.append(c)
        out = np.full(L, NINF)
        out[a:b] = _lse_rows(cands) if len(s) else np.zeros(0)
        return out
    for t in range(T - 2, -1, -1):
        G = beta[t + 1] + np.where(np.isfinite(beta[t + 1]), lp[t + 1, lab], 0.0)
        beta[t] = step_back(G, lo[t], hi[t], lo[t + 1], hi[t + 1])
    G0 = beta[0] + np.where(np.isfinite(beta[0]), lp[0, lab], 0.0)
    wlo = lo[0] if fault == "beta_out_short" else max(lo[0] - (mm - 1), 0)
    beta_out = step_back(G0, wlo, hi[0], lo[0], hi[0], veto=fault != "cut_no_veto_bwd",
                         moves=mm - 1 if fault == "beta_out_drop_move" else mm)
    w = slice(lo[T - 1], hi[T - 1])
    ll = float(_lse_rows((alpha[T - 1, w] + beta[T - 1, w])[:, None])[0])
    if ll == NINF:
        return failed(R.ZERO_MASS, NINF)
    with np.errstate(invalid="ignore"):
        gamma = np.exp(alpha + beta - ll)
    gamma[~np.isfinite(alpha + beta)] = 0.0
    occ = np.zeros((T, V))
    for t in range(T):
        np.add.at(occ[t], lab[lo[t]:hi[t]], gamma[t, lo[t]:hi[t]])
    post = None
    if path is not None:
        p = np.asarray(path, np.int64).reshape(-1)
        inside = (p >= lo) & (p < hi)
        post = np.where(inside, gamma[np.arange(T), np.clip(p, 0, L - 1)], 0.0)
    # the kernels' offsets (log2): C before frame t is c0 + the frame maxima before t; a block's offset is C at its first frame
    fmax = np.max(alpha, axis=1) * R.LOG2E
    first = (T - 1) // R.CK * R.CK
    cb = fmax[first - 1] if first > 0 else c0
    us = (alpha[T - 1, int(end)] * R.LOG2E - cb) if b_in is None else np.nan
    return dict(status=R.OK, ll=ll, gamma=gamma, windows=(lo, hi), occ=occ, path_post=post, alpha_out=alpha_out, beta_out=beta_out,
                alpha=alpha, beta=beta, c0=c0, cb=float(cb), us=float(us))


def gamma_list(gamma, lo, hi):
    """Dense gamma [T, L] as posterior_ref's list of (lo, window) - what R.label_ratio and R.state_ratio read."""
    return [(int(a), gamma[t, a:b]) for t, (a, b) in enumerate(zip(lo, hi))]


def chunk_bounds(T, cuts):
    edges = [0] + [int(c) for c in cuts] + [T]
    assert all(a < b for a, b in zip(edges[:-1], edges[1:])), edges
    return list(zip(edges[:-1], edges[1:]))


def chunked(lp, labels, band_lo, beam, mm, cuts, end, path=None, alpha0=None, fault=None):
    """The lattice cut at ``cuts``: dict(gamma [T, L], occ [T, V], path_post, ll: every chunk's Z, chunks: every chunk's result
    with its alpha_in and end, status: the first failing status or OK)."""
    lp = np.asarray(lp, np.float64)
    band_lo = np.asarray(band_lo, np.int64).reshape(-1)
    T = lp.shape[0]
    bounds = chunk_bounds(T, cuts)
    starts, row = [], alpha0
    for a, b in bounds[:-1]:
        starts.append(row)
        got = resume(lp[a:b], labels, band_lo[a:b], beam, mm, row, np.zeros(2 * len(np.asarray(labels).reshape(-1)) + 1), None, fault)
        if got["status"] != R.OK:
            return dict(status=got["status"], chunks=[got])
        row = got["alpha_out"]
    starts.append(row)
    results = [None] * len(bounds)
    e = end
    for k in range(len(bounds) - 1, -1, -1):
        a, b = bounds[k]
        got = resume(lp[a:b], labels, band_lo[a:b], beam, mm, starts[k], e, None if path is None else np.asarray(path)[a:b], fault)
        got["alpha_in"], got["end"] = starts[k], e
        results[k] = got
        if got["status"] != R.OK:
            return dict(status=got["status"], chunks=results)
        e = got["beta_out"]
    return dict(status=R.OK, gamma=np.concatenate([r["gamma"] for r in results]), occ=np.concatenate([r["occ"] for r in results]),
                path_post=None if path is None else np.concatenate([r["path_post"] for r in results]), ll=[r["ll"] for r in results],
                chunks=results)


def enumerate_resumed(lp, labels, band_lo, beam, mm, alpha_in, end_row):
    """(gamma [T, L], ll) of a tiny resumed lattice from every path: a start cell of alpha_in, T moves inside the windows (the
    veto on all of them, no band on the start cell), the weight of the end row at the last state."""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    lab = R.expand(labels)
    L = len(lab)
    lo, hi = B.table_windows(band_lo, L, beam)
    total, gamma = 0.0, np.zeros((T, L))
    for s0 in range(L):
        if not np.isfinite(alpha_in[s0]):
            continue
        for moves in itertools.product(range(mm), repeat=T):
            s, score, states = s0, alpha_in[s0], []
            for t, j in enumerate(moves):
                s += j
                if s >= L or not (lo[t] <= s < hi[t]) or (j >= 2 and j % 2 == 0 and lab[s] == 0):
                    break
                score += lp[t, lab[s]]
                states.append(s)
            if len(states) != T or not np.isfinite(end_row[states[-1]]):
                continue
            p = np.exp(score + end_row[states[-1]])
            total += p
            gamma[np.arange(T), states] += p
    return gamma / total, float(np.log(total))


# ---------------------------------------------------------------------------------------
# The cases: (T, S, V, beam, max_move), each under the diagonal table and a random table with steps up to max_move-1.  Log-probs
# from R.sloped(..., zero_every=5), so that vetoed cells lie on the cuts.
# ---------------------------------------------------------------------------------------
SHAPES = [(97, 40, 39, 16, 4), (200, 280, 39, 7, 4),            # the one-wavefront form
          (100, 40, 80, 16, 4), (120, 50, 39, 12, 6),           # the generic form
          (130, 60, 39, 1000, 4),                               # a band wider than L
          (65, 20, 39, 9, 3), (129, 30, 39, 7, 2)]
WIDE_SHAPE = (700, 600, 39, 1009, 4)                            # the widest fast band, a start window of 1012 slots: cut at 350
FAR_SHAPE = (40, 1500, 39, 16, 4)                               # tables that start at 2000: the labels far from 0
FAR_LO = 2000
TABLES = ("diagonal", "random")


def cuts_of(T):
    """Single cuts at 1, 31, 32, 33 and T-1 (a chunk's 32-frame blocks then differ from the uncut call's) and a three-way cut that
    holds a one-frame chunk."""
    return [(1,), (31,), (32,), (33,), (T - 1,), (20, 21)]


def case_name(shape, table):
    return "T%d_S%d_V%d_B%d_M%d_" % shape + table


def stepping_table(rng, T, L, mm, lo0):
    """B.random_table's steps in [0, max_move-1], each kept with the probability at which the table climbs about 0.8 L over the T
    frames (the others 0), so that it holds steps of every size and does not outrun the text."""
    steps = np.diff(B.random_table(rng, T, 1 << 40, mm - 1, lo0=0), prepend=0)
    keep = min(1.0, 0.8 * L / T / ((mm - 1) / 2.0))
    steps = np.where(rng.random(T) < keep, steps, 0)
    return np.minimum(lo0 + np.cumsum(steps), L - 1).astype(np.int64)


def build(shape, table):
    """(lp, labels, band_lo, terminal, beam, mm, alpha0, cut sets): alpha0 is None but for FAR_SHAPE, whose lattice starts from a
    row of its own around FAR_LO (the virtual state cannot reach it)."""
    T, S, V, beam, mm = shape
    seed = 7000 + 13 * T + S + (1 if table == "random" else 0)
    lp, labels = R.sloped(T, S, V, seed, zero_every=5)
    L = 2 * S + 1
    rng = np.random.default_rng(seed)
    alpha0 = None
    if shape == FAR_SHAPE:
        band = FAR_LO + 2 * np.arange(T, dtype=np.int64) if table == "diagonal" else B.random_table(rng, T, L, mm - 1, lo0=FAR_LO)
        alpha0 = np.full(L, NINF)
        a, b = FAR_LO - (mm - 1), min(FAR_LO + beam, L)
        alpha0[a:b] = -3.0 * rng.random(b - a) - 700.0     # (absolute values far from 0: the offset must carry them)
        alpha0[a + 1] = NINF
        cuts = cuts_of(T)
    else:
        band = R.windows(T, L, beam)[0] if table == "diagonal" else stepping_table(rng, T, L, mm, lo0=int(rng.integers(0, 2)))
        cuts = [(350,)] if shape == WIDE_SHAPE else cuts_of(T)
    live = resume(lp, labels, band, beam, mm, alpha0, np.zeros(L))
    assert live["status"] == R.OK, (shape, table, "no mass")
    lo, hi = live["windows"]
    a = live["alpha_out"][lo[-1]:hi[-1]]
    terminal = int(lo[-1] + np.argmax(a))
    return lp, labels, band, terminal, beam, mm, alpha0, cuts


def all_cases():
    return [(s, t) for s in SHAPES + [WIDE_SHAPE, FAR_SHAPE] for t in TABLES]


def a_path(ref_gamma, lo, hi, terminal):
    """A path for path_post: R.mixed_path on the uncut reference's windows (likeliest cells, band edges, cells outside it)."""
    return R.mixed_path(dict(gamma=gamma_list(ref_gamma, lo, hi)), (lo, hi), terminal)


# ---------------------------------------------------------------------------------------
# Tolerances of what the call adds.  gamma and the occupancy are held against posterior_ref's models and M_LABEL / M_STATE: the
# rows cross a cut in float64, so no new rounding enters them.  Z of a chunk that ends at a terminal is the sibling's Z, with
# its float-stored relative alpha: posterior_ref's Z model on the chunk's own offsets, and M_Z.  A row cell and a Z formed from
# an end row are float64 log-sum-exp chains: E = 2^-53 (frames of the chunk + 1) max(1, |value|) nats, and m twice the worst
# ratio |kernel - float64| / E measured on the MI355X over tests/test_fb_resume_gpu.py (profiles/fb_resume_accuracy.json, one
# record per test; the rule of DESIGN.md section 4.21).  Measured: 3.738 alpha_out, 4.407 beta_out (a chunk's rows start from the
# rows of the chunks before and after it, which carry their own rounding), 3.738 Z from an end row.
# ---------------------------------------------------------------------------------------
M_ROW_ALPHA, M_ROW_BETA, M_ROW_Z = 7.5, 8.9, 7.5


def row_error_model(want, frames):
    want = np.asarray(want, np.float64)
    return 2.0 ** -53 * (frames + 1) * np.maximum(1.0, np.abs(np.where(np.isfinite(want), want, 0.0)))


def row_ratio(got, want, frames, what=""):
    """The worst |got - want| / E over a row's finite cells; -inf cells must be -inf, and a NaN anywhere fails."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    dead = np.isneginf(want)
    assert np.all(np.isneginf(got[dead])), (what, "a cell without mass came out finite")
    assert not np.isnan(got).any(), what
    if dead.all():
        return 0.0
    return float(np.max(np.abs(got[~dead] - want[~dead]) / row_error_model(want, frames)[~dead]))


def terminal_z_error_model(ref, frames):
    """posterior_ref.z_error_model on a resumed chunk's own offsets: the float store of the terminal's relative alpha, and the
    float64 sums of the offsets."""
    return float(R.LN2 * R._hulp32(ref["us"]) + 2.0 ** -53 * (frames + 1) * max(1.0, abs(ref["ll"])))
