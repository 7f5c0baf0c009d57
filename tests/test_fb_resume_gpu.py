"""ka_ctc_posteriors_resume on the GPU through raw ctypes (tests/fb_resume_harness.py), in both memory
modes, against the float64 reference of tests/fb_resume_ref.py and, bit for bit, against ka_ctc_label_posteriors_banded; then
the Python front doors, ctc_label_posteriors_chunked and StreamingAligner(confidence=True).

The four claims of the header: (1) NULL rows and a terminal are the sibling's bits; (2) alpha_out and beta_out do not depend on
which other outputs are asked for; (3) a lattice's bits do not depend on its batch; (4) cut and resume is the uncut lattice,
within the project's tolerances against the float64 reference of the UNCUT lattice."""
import ctypes

import numpy as np
import pytest

import banded_fb_harness as BH
import banded_fb_ref as B
import determined_ref as DR
import fb_harness as H
import fb_resume_harness as RH
import fb_resume_ref as F
import posterior_ref as R
import track_cases as TC
import track_resume_ref as TR

pytestmark = pytest.mark.gpu

CASES = F.all_cases()
IDS = [F.case_name(s, t) for s, t in CASES]
MODES = ("host", "device")
_cases = {}


@pytest.fixture(scope="module")
def env():
    return H.engine()


def case(shape, table):
    """The case, its uncut float64 reference and a path through it; built once."""
    key = (shape, table)
    if key not in _cases:
        lp, labels, band, term, beam, mm, alpha0, cuts = F.build(shape, table)
        ref = F.resume(lp, labels, band, beam, mm, alpha0, term)
        assert ref["status"] == R.OK
        lo, hi = ref["windows"]
        path = F.a_path(ref["gamma"], lo, hi, term)
        inside = (path >= lo) & (path < hi)
        post = np.where(inside, ref["gamma"][np.arange(len(path)), path], 0.0)
        _cases[key] = dict(lp=lp, labels=labels, band=band, term=term, beam=beam, mm=mm, alpha0=alpha0, cuts=cuts, ref=ref, path=path,
                           post=post, L=2 * len(labels) + 1, chunked={})
    return _cases[key]


def ref_chunks(c, cuts):
    if cuts not in c["chunked"]:
        got = F.chunked(c["lp"], c["labels"], c["band"], c["beam"], c["mm"], cuts, c["term"], c["path"], c["alpha0"])
        assert got["status"] == R.OK
        c["chunked"][cuts] = got
    return c["chunked"][cuts]


def one(eng, _lib, c, a, b, alpha_in, end, mode, want=None, path=True):
    """One chunk [a, b) of a case through the raw call."""
    row = F.is_row(end)
    return RH.run(eng, _lib, [c["lp"][a:b]], [c["labels"]], [c["band"][a:b]], c["beam"], c["mm"], [alpha_in], [end if row else None],
                  [-1 if row else end], [c["path"][a:b]] if path else None, want, device=mode == "device")


def bits(x):
    return np.ascontiguousarray(x).tobytes()


# ---- claim 1 ----
@pytest.mark.parametrize("mode", MODES)
def test_null_rows_are_the_sibling_bit_for_bit(env, mode):
    _, _lib, eng = env
    groups = {}
    for shape, table in CASES:
        c = case(shape, table)
        if c["alpha0"] is None:
            groups.setdefault((shape[2], c["beam"], c["mm"]), []).append(c)
    assert len(groups) >= 6
    for (V, beam, mm), cs in groups.items():
        cs = cs + [dict(cs[0], term=-1), dict(cs[0], term=cs[0]["L"])]        # and two that fail: a terminal outside [0, L)
        lps, labs, tabs, terms = ([c[k] for c in cs] for k in ("lp", "labels", "band", "term"))
        want = BH.run(eng, _lib, "label_posteriors", lps, labs, terms, beam, mm, tables=[np.asarray(t, np.int32) for t in tabs],
                      device=mode == "device")
        got = RH.run(eng, _lib, lps, labs, tabs, beam, mm, None, None, terms, None, dict(path_post=False, alpha_out=False, beta_out=False),
                     device=mode == "device", null_arrays=("alpha_in", "beta_in", "path", "path_post", "alpha_out", "beta_out"))
        assert got.rc == want.rc == _lib.KA_ERR_BAD_ARGS and np.array_equal(got.st, want.st) and list(got.st[-2:]) == [-2, -2]
        assert not np.any(got.st[:-2]), got.st
        assert bits(got.ll.view(np.uint64)) == bits(want.ll.view(np.uint64))
        for i in range(len(cs)):
            assert bits(got.outs[i][0]) == bits(want.outs[i][0]), (V, beam, mm, i)
            assert all(RH.untouched(got, i, name) for name in RH.OUTS[1:])
        assert got.guards_intact() and want.guards_intact()
        # and alone, without a batch around it, through entries that are NULL instead of arrays
        alone = RH.run(eng, _lib, lps[:1], labs[:1], tabs[:1], beam, mm, [None], [None], terms[:1], [None],
                       dict(path_post=False, alpha_out=False, beta_out=False), device=mode == "device")
        assert alone.rc == 0 and bits(alone.outs[0][0]) == bits(want.outs[0][0]) and bits(alone.ll[:1]) == bits(want.ll[:1])


# ---- claim 2 ----
@pytest.mark.parametrize("shape,table", CASES, ids=IDS)
def test_rows_do_not_depend_on_what_else_is_asked_for(env, shape, table):
    _, _lib, eng = env
    c = case(shape, table)
    cuts = c["cuts"][-1]
    ref = ref_chunks(c, cuts)
    for mode in MODES:
        for (a, b), r in zip(F.chunk_bounds(len(c["lp"]), cuts), ref["chunks"]):
            full = one(eng, _lib, c, a, b, r["alpha_in"], r["end"], mode)
            fwd = one(eng, _lib, c, a, b, r["alpha_in"], r["end"], mode, dict(occ=False, path_post=False, beta_out=False), path=False)
            bwd = one(eng, _lib, c, a, b, r["alpha_in"], r["end"], mode, dict(occ=False, path_post=False, alpha_out=False), path=False)
            post = one(eng, _lib, c, a, b, r["alpha_in"], r["end"], mode, dict(occ=False))
            assert full.rc == fwd.rc == bwd.rc == post.rc == 0
            assert bits(fwd.outs[0][2]) == bits(full.outs[0][2]) == bits(post.outs[0][2]), "alpha_out: with and without the backward pass"
            assert bits(bwd.outs[0][3]) == bits(full.outs[0][3]) == bits(post.outs[0][3]), "beta_out: with and without gamma"
            assert bits(post.outs[0][1]) == bits(full.outs[0][1]), "path_post: with and without the occupancy"
            assert bits(fwd.ll) == bits(full.ll) == bits(bwd.ll) == bits(post.ll)
            assert RH.untouched(fwd, 0, "occ") and RH.untouched(fwd, 0, "beta_out") and RH.untouched(bwd, 0, "alpha_out")
            assert all(x.guards_intact() for x in (full, fwd, bwd, post))


# ---- claim 4 ----
def run_chunks(eng, _lib, c, cuts, mode):
    """The chunks as a caller runs them: a forward-only sweep that hands alpha_out on, then newest first with both rows."""
    bounds = F.chunk_bounds(len(c["lp"]), cuts)
    free = np.zeros(c["L"])
    starts, row = [], c["alpha0"]
    for a, b in bounds[:-1]:
        starts.append(row)
        got = one(eng, _lib, c, a, b, row, free, mode, dict(occ=False, path_post=False, beta_out=False), path=False)
        assert got.rc == 0 and got.guards_intact()
        row = got.outs[0][2]
    starts.append(row)
    out, end = [None] * len(bounds), c["term"]
    for k in range(len(bounds) - 1, -1, -1):
        a, b = bounds[k]
        got = one(eng, _lib, c, a, b, starts[k], end, mode)
        assert got.rc == 0 and got.guards_intact(), (cuts, k)
        out[k] = got
        end = got.outs[0][3]
    return bounds, out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,table", CASES, ids=IDS)
def test_cut_and_resume_is_the_uncut_lattice(env, shape, table, mode):
    _, _lib, eng = env
    c = case(shape, table)
    lo, hi = c["ref"]["windows"]
    uncut = dict(gamma=F.gamma_list(c["ref"]["gamma"], lo, hi))
    worst = dict(label=0.0, state=0.0, alpha=0.0, beta=0.0, z_row=0.0, z_term=0.0)
    for cuts in c["cuts"]:
        ref = ref_chunks(c, cuts)
        bounds, out = run_chunks(eng, _lib, c, cuts, mode)
        occ = np.concatenate([o.outs[0][0] for o in out])
        post = np.concatenate([o.outs[0][1] for o in out])
        worst["label"] = max(worst["label"], R.label_ratio(occ, uncut, c["labels"], (cuts, "occupancy")))
        worst["state"] = max(worst["state"], R.cells_ratio(post, c["post"], R.state_error_model(c["post"]), (cuts, "path_post")))
        for (a, b), o, r in zip(bounds, out, ref["chunks"]):
            n = b - a
            worst["alpha"] = max(worst["alpha"], F.row_ratio(o.outs[0][2], r["alpha_out"], n, (cuts, a, "alpha_out")))
            worst["beta"] = max(worst["beta"], F.row_ratio(o.outs[0][3], r["beta_out"], n, (cuts, a, "beta_out")))
            if F.is_row(r["end"]):
                worst["z_row"] = max(worst["z_row"], abs(o.ll[0] - c["ref"]["ll"]) / float(F.row_error_model(c["ref"]["ll"], n)))
            else:
                worst["z_term"] = max(worst["z_term"], abs(o.ll[0] - c["ref"]["ll"]) / F.terminal_z_error_model(r, n))
            if r["alpha_in"] is not None:      # logsumexp(alpha_in + beta_out) over the start row is the chunk's Z
                z0 = float(R._lse((np.asarray(r["alpha_in"]) + o.outs[0][3])[:, None])[0])
                tol = (F.M_ROW_BETA + F.M_ROW_Z) * float(F.row_error_model(o.ll[0], n))     # beta_out's cells, and Z
                if not F.is_row(r["end"]):
                    tol += R.M_Z * F.terminal_z_error_model(r, n)                           # (the sibling's float-stored Z)
                assert abs(z0 - o.ll[0]) <= tol, (cuts, a)
    H.record("resume label occupancy", worst["label"], R.M_LABEL)
    H.record("resume path posterior", worst["state"], R.M_STATE)
    H.record("resume alpha_out", worst["alpha"], F.M_ROW_ALPHA)
    H.record("resume beta_out", worst["beta"], F.M_ROW_BETA)
    H.record("resume Z from an end row", worst["z_row"], F.M_ROW_Z)
    H.record("resume Z at a terminal", worst["z_term"], R.M_Z)


# ---- claim 3, and failures ----
def batch_of(V):
    """Chunks of one V, beam 16 and max_move 4 with rows of every kind, and among them four lattices that fail on their rows."""
    shape = (97, 40, 39, 16, 4) if V == 39 else (100, 40, 80, 16, 4)
    items = []
    for table in F.TABLES:
        c = case(shape, table)
        ref = ref_chunks(c, (33,))
        for (a, b), r in zip(F.chunk_bounds(shape[0], (33,)), ref["chunks"]):
            items.append(dict(lp=c["lp"][a:b], labels=c["labels"], band=c["band"][a:b], alpha_in=r["alpha_in"], end=r["end"], path=c["path"][a:b]))
    if V == 39:
        c = case(F.FAR_SHAPE, "random")
        items.append(dict(lp=c["lp"], labels=c["labels"], band=c["band"], alpha_in=c["alpha0"], end=c["term"], path=c["path"]))
    good = len(items)
    base = items[1]
    L = len(base["alpha_in"])
    nan_row, inf_row = base["alpha_in"].copy(), np.zeros(L)
    nan_row[np.flatnonzero(np.isfinite(nan_row))[0]] = np.nan
    inf_row[int(base["band"][-1])] = np.inf
    unreachable = np.full(L, -np.inf)
    unreachable[0] = 0.0                       # live, but below what frame 0 of a band that starts at base's can read
    items += [dict(base, alpha_in=nan_row), dict(base, end=inf_row), dict(base, alpha_in=np.full(L, np.nan), end=np.full(L, np.nan)),
              dict(base, alpha_in=unreachable)]
    assert base["band"][0] - 3 > 0
    return items, good


def run_items(eng, _lib, items, mode, beam=16, mm=4):
    ends = [it["end"] for it in items]
    return RH.run(eng, _lib, [it["lp"] for it in items], [it["labels"] for it in items], [it["band"] for it in items], beam, mm,
                  [it["alpha_in"] for it in items], [e if F.is_row(e) else None for e in ends], [-1 if F.is_row(e) else e for e in ends],
                  [it["path"] for it in items], None, device=mode == "device")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V", [39, 80])
def test_a_lattice_has_the_same_bits_alone_and_in_a_batch_and_bad_rows_fail_alone(env, V, mode):
    _, _lib, eng = env
    items, good = batch_of(V)
    got = run_items(eng, _lib, items, mode)
    assert got.guards_intact()
    assert list(got.st[:good]) == [0] * good and list(got.st[good:]) == [_lib.KA_ERR_BAD_ARGS] * 3 + [_lib.KA_ERR_ZERO_MASS]
    assert got.rc == _lib.KA_ERR_BAD_ARGS
    for i in range(good, len(items)):          # every requested output of a failed lattice is NaN, rows included
        assert all(RH.all_nan(x) for x in got.outs[i]), i
    assert np.all(np.isnan(got.ll[good:good + 3])) and got.ll[-1] == -np.inf
    for i, it in enumerate(items):
        alone = run_items(eng, _lib, [it], mode)
        assert alone.st[0] == got.st[i] and bits(alone.ll[:1].view(np.uint64)) == bits(got.ll[i:i + 1].view(np.uint64)), i
        assert all(bits(x) == bits(y) for x, y in zip(alone.outs[0], got.outs[i])), i
    other = run_items(eng, _lib, items[:good][::-1], mode)       # other neighbours, another slot each
    for i in range(good):
        assert all(bits(x) == bits(y) for x, y in zip(other.outs[good - 1 - i], got.outs[i])), i


@pytest.mark.parametrize("mode", MODES)
def test_a_chunk_resumed_from_a_failed_chunk_fails(env, mode):
    _, _lib, eng = env
    c = case((97, 40, 39, 16, 4), "diagonal")
    L = c["L"]
    bad = np.full(L, -np.inf)
    bad[1] = np.nan
    first = one(eng, _lib, c, 0, 33, bad, np.zeros(L), mode)
    assert first.rc == first.st[0] == _lib.KA_ERR_BAD_ARGS and all(RH.all_nan(x) for x in first.outs[0]) and np.isnan(first.ll[0])
    second = one(eng, _lib, c, 33, 97, first.outs[0][2], c["term"], mode)
    assert second.rc == _lib.KA_ERR_BAD_ARGS and all(RH.all_nan(x) for x in second.outs[0])
    third = one(eng, _lib, c, 0, 33, None, second.outs[0][3], mode)       # and the other way round, from its beta_out
    assert third.rc == _lib.KA_ERR_BAD_ARGS and all(RH.all_nan(x) for x in third.outs[0])
    assert first.guards_intact() and second.guards_intact() and third.guards_intact()


@pytest.mark.parametrize("mode", MODES)
def test_a_bad_cell_no_frame_reads_fails_too(env, mode):
    """A NaN or +inf ANYWHERE in either row: also below what frame 0 reads, above band 0, and outside band T-1."""
    _, _lib, eng = env
    c = case((97, 40, 39, 16, 4), "diagonal")
    r = ref_chunks(c, (33,))["chunks"]
    a, b, L, mm = 33, 97, c["L"], c["mm"]
    lo0, hi0, loT = int(c["band"][a]), int(c["band"][a]) + c["beam"], int(c["band"][b - 1])
    assert lo0 - (mm - 1) > 0 and hi0 < L and loT > 0
    good = one(eng, _lib, c, a, b, r[1]["alpha_in"], np.zeros(L), mode)
    assert good.rc == 0
    for where, value in ((0, np.nan), (lo0 - mm, np.inf), (hi0, np.nan), (L - 1, np.inf)):
        row = r[1]["alpha_in"].copy()
        row[where] = value
        got = one(eng, _lib, c, a, b, row, np.zeros(L), mode)
        assert got.rc == got.st[0] == _lib.KA_ERR_BAD_ARGS and all(RH.all_nan(x) for x in got.outs[0]), ("alpha_in", where)
        assert F.resume(c["lp"][a:b], c["labels"], c["band"][a:b], c["beam"], mm, row, np.zeros(L))["status"] == R.BAD_ARGS
    for where, value in ((0, np.nan), (loT - 1, np.inf)):
        end = np.zeros(L)
        end[where] = value
        got = one(eng, _lib, c, a, b, r[1]["alpha_in"], end, mode)
        assert got.rc == got.st[0] == _lib.KA_ERR_BAD_ARGS and all(RH.all_nan(x) for x in got.outs[0]), ("beta_in", where)
        assert got.guards_intact()
    row = r[1]["alpha_in"].copy()
    row[0] = -np.inf                                  # -inf is no mass, anywhere
    assert one(eng, _lib, c, a, b, row, np.zeros(L), mode).rc == 0


def test_an_output_row_may_not_overlap_an_input_row(env):
    """Through the single-lattice symbol: alpha_out on top of alpha_in (the in-place update a stream would try) or of beta_in, and
    beta_out likewise, fail with KA_ERR_BAD_ARGS before anything runs; rows side by side in one buffer are fine."""
    _, _lib, eng = env
    c = case((97, 40, 39, 16, 4), "diagonal")
    r = ref_chunks(c, (33,))["chunks"][1]
    a, b, L = 33, 97, c["L"]
    lp = np.ascontiguousarray(c["lp"][a:b], np.float32)
    labels, band = np.ascontiguousarray(c["labels"], np.int32), np.ascontiguousarray(c["band"][a:b], np.int32)

    def call(a_in, b_in, a_out, b_out):
        z = np.full(1, -7.0)
        ptr = lambda x: None if x is None else x.ctypes.data
        rc = eng.lib.ka_ctc_posteriors_resume_f32(eng.handle, lp.ctypes.data, b - a, lp.shape[1], lp.shape[1], labels.ctypes.data, len(labels),
                                                  c["beam"], c["mm"], band.ctypes.data, ptr(a_in), ptr(b_in), -1, None, None, 0, None,
                                                  ptr(a_out), ptr(b_out), z.ctypes.data, _lib.KA_MEM_HOST, None)
        return rc, z[0]
    buf = np.zeros(3 * L)
    rows = buf[:L], buf[L:2 * L], buf[2 * L:]
    rows[0][:] = r["alpha_in"]
    want = rows[0].copy()
    for outs in ((rows[0], None), (None, rows[0]), (rows[1], None), (None, rows[1]), (buf[1:L + 1], None), (None, buf[2 * L - 1:3 * L - 1])):
        rc, z = call(rows[0], rows[1], *outs)
        assert rc == _lib.KA_ERR_BAD_ARGS and z == -7.0 and np.array_equal(rows[0], want) and not np.any(rows[1]), outs
    rc, z = call(rows[0], rows[1], rows[2], None)          # side by side
    full = one(eng, _lib, c, a, b, r["alpha_in"], np.zeros(L), "host")
    assert rc == 0 and z == full.ll[0] and bits(rows[2]) == bits(full.outs[0][2]), "the single call is the batch call"


def test_bad_arguments_write_nothing(env):
    _, _lib, eng = env
    c = case((97, 40, 39, 16, 4), "diagonal")
    args = ([c["lp"]], [c["labels"]], [c["band"]], c["beam"], c["mm"], None, None, [c["term"]])
    no_path = RH.run(eng, _lib, *args, None, None)                                   # path_post without a path
    assert no_path.rc == _lib.KA_ERR_BAD_ARGS and all(RH.untouched(no_path, 0, n) for n in RH.OUTS) and no_path.st[0] == 99
    bad_table = RH.run(eng, _lib, *args[:2], [c["band"][::-1].copy()], *args[3:], [c["path"]], None)
    assert bad_table.rc == bad_table.st[0] == _lib.KA_ERR_BAD_ARGS and all(RH.all_nan(x) for x in bad_table.outs[0])


# ---- workspace ----
@pytest.mark.parametrize("mode", MODES)
def test_workspace_bytes_cover_the_call(env, mode):
    import torch
    _, _lib, eng = env
    lib = _lib.load_library()
    for shape in ((97, 40, 39, 16, 4), (100, 40, 80, 16, 4)):
        c = case(shape, "diagonal")
        mem = _lib.KA_MEM_HOST if mode == "host" else _lib.KA_MEM_DEVICE
        Ts, Ss = (ctypes.c_int64 * 1)(shape[0]), (ctypes.c_int64 * 1)(shape[1])
        need = lib.ka_posteriors_resume_workspace_bytes(1, Ts, Ss, shape[2], shape[3], shape[4], mem)
        sibling = lib.ka_label_posterior_workspace_bytes(1, Ts, Ss, shape[2], shape[3], shape[4], mem)
        rows = 4 * 8 * c["L"] + 2 * 4 * shape[0] + 4 * shape[0] if mode == "host" else 0
        assert sibling + 176 + rows <= need <= sibling + 176 + rows + 12 * 256
        want = one(eng, _lib, c, 0, shape[0], None, np.zeros(c["L"]), mode)          # (the kernels' code is on the device before memory is counted)
        own = _lib.Engine(torch.cuda.current_device())
        try:
            own.reserve(need)
            torch.cuda.synchronize()
            before = torch.cuda.mem_get_info()[0]
            got = one(own, _lib, c, 0, shape[0], None, np.zeros(c["L"]), mode)
            torch.cuda.synchronize()
            assert got.rc == 0 and torch.cuda.mem_get_info()[0] == before
            assert all(bits(x) == bits(y) for x, y in zip(got.outs[0], want.outs[0]))
        finally:
            own.close()


# ---- the Python front doors ----
def test_python_front_doors_are_the_raw_call(env):
    import torch
    ka, _lib, eng = env
    c = case((97, 40, 39, 16, 4), "random")
    r = ref_chunks(c, (33,))["chunks"][1]
    a, b = 33, 97
    raw = one(eng, _lib, c, a, b, r["alpha_in"], c["term"], "host")
    got = ka.ctc_posteriors_resume(c["lp"][a:b], c["labels"], c["band"][a:b], r["alpha_in"], c["term"], c["path"][a:b], beam_size=c["beam"],
                                   max_move=c["mm"])
    assert len(got) == 5 and all(bits(x) == bits(y) for x, y in zip(got[:4], raw.outs[0])) and got[4] == raw.ll[0]
    assert [x.dtype for x in got[:4]] == [np.float32, np.float32, np.float64, np.float64]
    fwd = ka.ctc_posteriors_resume(c["lp"][a:b], c["labels"], c["band"][a:b], r["alpha_in"], ka.free_end_scores(c["L"]), occupancy=False,
                                   rows="alpha", beam_size=c["beam"], max_move=c["mm"])
    assert fwd[0] is None and fwd[1] is None and fwd[3] is None and fwd[2].shape == (c["L"],)
    res, st = ka.ctc_posteriors_resume_batch([c["lp"][a:b]] * 2, [c["labels"]] * 2, [c["band"][a:b]] * 2, [r["alpha_in"], None],
                                             [c["term"], c["L"] + 5], [c["path"][a:b], None], beam_size=c["beam"], max_move=c["mm"],
                                             return_status=True)
    assert st == [0, _lib.KA_ERR_BAD_ARGS] and all(bits(x) == bits(y) for x, y in zip(res[0][:4], raw.outs[0])) and res[1][1] is None
    assert np.all(np.isnan(res[1][0])) and np.all(np.isnan(res[1][2]))
    with pytest.raises(ValueError):
        ka.ctc_posteriors_resume(c["lp"][a:b], c["labels"], c["band"][a:b], None, c["L"] + 5, beam_size=c["beam"], max_move=c["mm"])
    rawd = one(eng, _lib, c, a, b, r["alpha_in"], c["term"], "device")
    dev = ka.ctc_posteriors_resume(torch.from_numpy(c["lp"][a:b]).cuda(), c["labels"], c["band"][a:b], torch.from_numpy(r["alpha_in"]).cuda(),
                                   c["term"], c["path"][a:b], beam_size=c["beam"], max_move=c["mm"])
    assert all(x.is_cuda for x in dev[:4]) and dev[2].dtype == torch.float64
    assert all(bits(x.cpu().numpy()) == bits(y) for x, y in zip(dev[:4], rawd.outs[0])) and dev[4] == rawd.ll[0]


@pytest.mark.parametrize("shape,chunk", [((97, 40, 39, 16, 4), 32), ((100, 40, 80, 16, 4), 33), ((200, 280, 39, 7, 4), 64)])
def test_chunked_label_posteriors_are_the_uncut_call(env, shape, chunk):
    """... within twice R.label_tolerance: two results, each within it of the float64 reference."""
    ka, _lib, eng = env
    c = case(shape, "random")
    lo, hi = c["ref"]["windows"]
    uncut = dict(gamma=F.gamma_list(c["ref"]["gamma"], lo, hi))
    whole, z = ka.ctc_label_posteriors(c["lp"], c["labels"], c["term"], c["beam"], c["mm"], band_lo=c["band"])
    occ, post, zc = ka.ctc_label_posteriors_chunked(c["lp"], c["labels"], c["band"], chunk, c["term"], c["path"], c["beam"], c["mm"])
    tol = R.label_tolerance(uncut["gamma"], c["labels"], shape[2])
    assert occ.shape == whole.shape and occ.dtype == np.float32 and post.shape == (shape[0],)
    assert np.all(np.abs(occ.astype(np.float64) - whole) <= 2.0 * tol)
    H.record("chunked label occupancy", R.label_ratio(occ, uncut, c["labels"]), R.M_LABEL)
    H.record("chunked path posterior", R.cells_ratio(post, c["post"], R.state_error_model(c["post"])), R.M_STATE)
    last = ref_chunks(c, tuple(range(chunk, shape[0], chunk)))["chunks"][-1]
    assert abs(zc - c["ref"]["ll"]) <= R.M_Z * F.terminal_z_error_model(last, len(last["gamma"]))
    assert abs(z - c["ref"]["ll"]) <= R.z_tolerance(B.ref_at(c["lp"], c["labels"], c["term"], c["band"], c["beam"], c["mm"]))
    none = ka.ctc_label_posteriors_chunked(c["lp"], c["labels"], c["band"], shape[0] + 5, c["term"], None, c["beam"], c["mm"])
    assert none[1] is None and bits(none[0]) == bits(whole), "one chunk: the uncut call's bits"


# ---- streaming confidence ----
ST_T, ST_S, ST_BEAM, ST_CHUNK = 192, 40, 16, 32


def stream_input():
    """Peaked rows along a planted path with a flat stretch in the middle: frames [72, 120) say nothing."""
    t = np.arange(ST_T)
    true = np.minimum(t // 3, 2 * ST_S)
    lp, lab = TC.planted(93, ST_T, ST_S, true)
    lp[72:120] = np.float32(-np.log(lp.shape[1]))
    return lp, lab


def stream_plan(lp, lab, period):
    """What every push commits, from the CPU references alone: the number of frames."""
    lo, init, pending, counts = 0, None, 0, []
    for a in range(0, ST_T, ST_CHUNK):
        r = TR.best_path_tracking_resume(lp[a:a + ST_CHUNK], lab, lo, init, TR.END_HIGHEST, ST_BEAM, 4, period)
        det = DR.determined(lp[a:a + ST_CHUNK], lab, r[3], init, ST_BEAM, 4)
        init, lo = r[6], r[7]
        if det >= 0:
            counts.append(pending + det)
            pending = ST_CHUNK - det
        else:
            counts.append(0)
            pending += ST_CHUNK
    return counts


@pytest.mark.parametrize("period", [8, 16])
def test_streaming_confidence(env, period):
    ka, _lib, eng = env
    lp, lab = stream_input()
    plan = stream_plan(lp, lab, period)
    assert any(n > 0 for n in plan) and any(n == 0 for n in plan), plan
    L = 2 * ST_S + 1
    path, _lab, _sc, table = ka.ctc_best_path_tracking(lp, lab, ST_BEAM, 4, period)
    plain = ka.StreamingAligner(lab, ST_BEAM, 4, period)
    conf = ka.StreamingAligner(lab, ST_BEAM, 4, period, confidence=True)
    done, worst = 0, 0.0
    for k, a in enumerate(list(range(0, ST_T, ST_CHUNK)) + [None]):
        want4 = plain.finish() if a is None else plain.push(lp[a:a + ST_CHUNK])
        got = conf.finish() if a is None else conf.push(lp[a:a + ST_CHUNK])
        assert len(got) == 5 and len(want4) == 4
        assert all(bits(x) == bits(y) and x.dtype == y.dtype for x, y in zip(got[:4], want4)), k
        n = got[0].shape[0]
        assert got[4].shape == (n,) and got[4].dtype == np.float32
        if a is not None:
            assert n == plan[k], (k, n, plan)
        if n == 0:
            continue
        pushed = ST_T if a is None else a + ST_CHUNK
        ref = F.resume(lp[:pushed], lab, table[:pushed], ST_BEAM, 4, None, int(path[-1]) if a is None else np.zeros(L), path[:pushed])
        assert ref["status"] == R.OK
        want = ref["path_post"][done:done + n]
        worst = max(worst, R.cells_ratio(got[4], want, R.state_error_model(want), ("push", k)))
        done += n
    assert done == ST_T
    H.record("streaming confidence", worst, R.M_STATE)
