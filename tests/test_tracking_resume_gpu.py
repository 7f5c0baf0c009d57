"""The resumable tracking best path on the GPU (ka_ctc_best_path_tracking_resume[_batch]_f32).  Every
comparison is exact - path, labels, the table, the bits of the scores, of the total and of the last row, entry, next_lo, status -
against tests/track_resume_ref.py (tests/test_tracking_resume_cpu.py asserts that the reference and the cases do what they
say), through the C ABI and both Python front doors, in both kernel forms: a NULL start is the tracking call; a cut lattice
resumed gives the uncut answer; the resumed call over the returned table agrees; batches, failures, bad arguments, the chunked
front end, the workspace figure.
"""
import ctypes

import numpy as np
import pytest

import band_cases as C
import golden_util as G
import track_cases as TC
import track_resume_cases as K
import track_resume_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MODES = ("host", "device")
FORMS = ("wave", "generic")
SENTINEL = -7777
DEAD_BITS = 0x7fc00000
R_END_RULE = {"highest": 0, "best": 1}   # ka_ctc_best_path_tracking's end_rule
SYMBOLS = ("ka_ctc_best_path_tracking_resume_f32", "ka_ctc_best_path_tracking_resume_batch_f32", "ka_tracking_resume_workspace_bytes")


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    lib = _lib.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
    return ka, _lib.default_engine(torch.cuda.current_device())


def bits(x):
    return np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32)


def host(a):
    return np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a)


def widened(lp):
    """72 more columns (that no label names) take V past 64: the generic kernels"""
    return np.concatenate([lp, np.full((lp.shape[0], 72), -1.0, np.float32)], axis=1)


def answers(results, status, total):
    """the results of a Python batch call as the scenarios of track_resume_cases want them"""
    out = []
    for (path, lab, sc, table, entry, final, next_lo), st, tot in zip(results, status, total):
        path, lab, sc, table, final = (host(a) for a in (path, lab, sc, table, final))
        if st == 0:
            out.append(("ok", path, lab, sc, table, np.float32(tot), int(entry), final, int(next_lo)))
        elif st == -1:
            assert entry == -1
            out.append(("empty", final, table, int(next_lo)))
        else:   # the lattice's own failure: no path, a dead row, no low end to go on from
            assert entry == -1 and next_lo == -1 and np.all(bits(final) == DEAD_BITS), st
            out.append(("bad_args",) if st == -2 else ("failed", int(st)))
    return out


def batch(ka, mode, form, lps, labs, first, inits, ends, beam, mm, period):
    if form == "generic":
        lps = [widened(lp) for lp in lps]
    if mode == "host":
        return answers(*ka.ctc_best_path_tracking_resume_batch(lps, labs, first, inits, ends, beam, mm, period, return_status=True))
    import torch
    dlp = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lps]
    return answers(*ka.ctc_best_path_tracking_resume_device(dlp, labs, first, inits, ends, beam, mm, period, return_status=True))


def gpu_run(ka, mode, form):
    def run(lp, lab, first_lo, init, end, beam, mm, period):
        return batch(ka, mode, form, [lp], [lab], [int(first_lo)], [init], [end], beam, mm, period)[0]
    return run


# ---- property 1: a NULL start, first_lo 0, no last row: the tracking call, through the raw C ABI ----
def raw_single(eng, lp, lab, first_lo, init, end, beam, mm, period, final=None, entry=None, next_lo=None, table=True):
    from kokoro_align_amd import _lib
    lp = np.ascontiguousarray(lp, np.float32)
    lab = np.ascontiguousarray(lab, np.int32)
    T, V = lp.shape
    outs = [np.full(T, SENTINEL, np.int32), np.full(T, SENTINEL, np.int32), np.full(T, SENTINEL, np.float32), np.full(T, SENTINEL, np.int32)]
    total = np.zeros(1, np.float32)
    ptr = [a.ctypes.data for a in outs]
    if not table:
        ptr[3] = None
    rc = eng.lib.ka_ctc_best_path_tracking_resume_f32(
        eng.handle, lp.ctypes.data, T, V, V, lab.ctypes.data, len(lab), beam, mm, period, int(first_lo),
        None if init is None else init.ctypes.data, int(end), *ptr, None if final is None else final.ctypes.data,
        None if entry is None else entry.ctypes.data, None if next_lo is None else next_lo.ctypes.data, total.ctypes.data, _lib.KA_MEM_HOST, None)
    return rc, outs, total[0]


def raw_tracking(eng, lp, lab, beam, mm, period, end_rule):
    from kokoro_align_amd import _lib
    lp = np.ascontiguousarray(lp, np.float32)
    lab = np.ascontiguousarray(lab, np.int32)
    T, V = lp.shape
    outs = [np.full(T, SENTINEL, np.int32), np.full(T, SENTINEL, np.int32), np.full(T, SENTINEL, np.float32), np.full(T, SENTINEL, np.int32)]
    total = np.zeros(1, np.float32)
    rc = eng.lib.ka_ctc_best_path_tracking_f32(eng.handle, lp.ctypes.data, T, V, V, lab.ctypes.data, len(lab), beam, mm, period, end_rule,
                                               *[a.ctypes.data for a in outs], total.ctypes.data, _lib.KA_MEM_HOST, None)
    return rc, outs, total[0]


@pytest.mark.parametrize("name", TC.NAMES)
def test_null_start_is_the_tracking_call(env, name):
    ka, eng = env
    lp, lab, beam, mm, period, end_rule = TC.case(name)
    for form in FORMS:
        x = widened(lp) if form == "generic" else lp
        wrc, want, wtot = raw_tracking(eng, x, lab, beam, mm, period, R_END_RULE[end_rule])
        rc, got, tot = raw_single(eng, x, lab, 0, None, K.END_OF[end_rule], beam, mm, period)
        assert rc == wrc and bits(tot)[0] == bits(wtot)[0], (name, form)
        if rc == 0:
            assert all(R.same_bits(g, w) for g, w in zip(got, want)), (name, form)
        else:
            assert all(np.all(a == SENTINEL) for a in got[:3])
    # ... and through the front door
    want = ka.ctc_best_path_tracking(lp, lab, beam, mm, period, end_rule)
    got = ka.ctc_best_path_tracking_resume(lp, lab, 0, None, end_rule, beam, mm, period)
    assert all(R.same_bits(g, w) for g, w in zip(got[:4], want)) and got[4] == 0


# ---- the scenario list: cuts (property 2), depths, block edges, short lattices, single calls ----
GROUPS = {}
for _name in K.SCENARIOS:
    _p = _name.split(":")
    GROUPS.setdefault(_p[1] if _p[0] in ("cut", "uncut") else _p[0], []).append(_name)


@pytest.mark.parametrize("group", list(GROUPS))
def test_scenarios(env, group):
    ka, _ = env
    for name in GROUPS[group]:
        want = K.want(name)
        for mode in MODES:
            for form in FORMS:
                got = K.SCENARIOS[name](gpu_run(ka, mode, form))
                assert K.same_answers(got, want), f"{name} [{mode}, {form}]: {[g[0] for g in got]} against {[w[0] for w in want]}"


# ---- property 3: ctc_best_path_resume over the returned table ----
@pytest.mark.parametrize("name", ["depth1", "depth2", "depth3", "edge1", "edge2", "edge3", "cut:wrap:624", "cut:step70:64", "cut:ninf_best:40",
                                  "cut:gen_mm5:24", "cut:gen_V65:32", "single:end_live", "single:end_dead_in_band", "single:ninf_cells"])
def test_resume_over_the_returned_table(env, name):
    ka, _ = env
    seen = []

    def run(lp, lab, first_lo, init, end, beam, mm, period):
        got = gpu_run(ka, "host", "wave")(lp, lab, first_lo, init, end, beam, mm, period)
        table = got[4] if got[0] == "ok" else got[2]
        (res,), st, tot = ka.ctc_best_path_resume_batch([lp], [lab], [table], [init], [end], beam, mm, return_status=True)
        if got[0] == "ok":
            assert st[0] == 0 and all(R.same_bits(host(g), w) for g, w in zip(res[:3], got[1:4]))
            assert bits(tot[0])[0] == bits(got[5])[0] and res[3] == got[6] and R.same_bits(res[4], got[7])
        else:
            assert st[0] == -1 and R.same_bits(res[4], got[1])
        seen.append(got[0])
        return got
    K.SCENARIOS[name](run)
    assert seen


# ---- batches ----
def mixed_batch():
    """41 lattices of one beam, max_move and period that mix NULL and given start rows, first_lo values and the three kinds of end;
    three of them fail on their own (a bad label, a +inf start cell, a NaN log-prob).  Returns the inputs and those three."""
    rng = np.random.default_rng(435)
    lps, labs, first, inits, ends = [], [], [], [], []
    for i in range(41):
        T, S = int(rng.integers(1, 40)), int(rng.integers(0, 60))
        L = 2 * S + 1
        lp, lab = C.random_lattice(9100 + i, T, S, ninf=(i % 5 == 0))
        lo = int(rng.integers(0, 1 + L // 2)) if i % 4 else 0
        init = None
        if i % 3:
            init = K.free_row(L, max(lo - int(rng.integers(0, 6)), 0), min(lo + int(rng.integers(1, 9)), L))
            init[~np.isnan(init)] = (np.round(rng.standard_normal(int(np.sum(~np.isnan(init)))) * 16) / 8).astype(np.float32)
            if i % 7 == 0:
                init[lo] = -np.inf
        end = (-1, -2, int(rng.integers(0, L)))[i % 3 if i % 4 else 2]
        if end >= 0 and i % 8:   # (mostly a cell that is live at the end)
            row = K.ref_run()(lp, lab, lo, init, R.END_HIGHEST, 24, 4, 8)
            row = row[7] if row[0] == "ok" else row[1]
            if np.any(~np.isnan(row)):
                end = int(rng.choice(np.nonzero(~np.isnan(row))[0]))
        lps.append(lp), labs.append(lab), first.append(lo), inits.append(init), ends.append(end)
    # failures among them: a bad label, a +inf start cell, a NaN log-prob
    bad = next(i for i in range(10, 41) if len(labs[i]) > 2)
    labs[bad] = labs[bad].copy()
    labs[bad][1] = 1000   # (no vocabulary of these tests is that large)
    L = 2 * len(labs[bad + 2]) + 1
    inits[bad + 2] = K.free_row(L, 0, L)
    inits[bad + 2][L // 2] = np.inf
    lps[bad + 4] = lps[bad + 4].copy()
    lps[bad + 4][0, 1] = np.nan
    return lps, labs, first, inits, ends, {bad: ("failed", -5), bad + 2: ("bad_args",), bad + 4: ("failed", -6)}


def test_batch_lattices_get_the_bits_they_have_alone(env):
    """property 4: whatever the neighbours' rows, ends and first_lo are, failures among them"""
    ka, eng = env
    lps, labs, first, inits, ends, failed = mixed_batch()
    run = K.ref_run()
    want = [failed[i] if i in failed else run(lp, lab, lo, init, end, 24, 4, 8)
            for i, (lp, lab, lo, init, end) in enumerate(zip(lps, labs, first, inits, ends))]
    kinds = [w[0] for w in want]
    assert kinds.count("ok") >= 15 and kinds.count("empty") >= 4
    for mode in MODES:
        for form in FORMS:
            got = batch(ka, mode, form, lps, labs, first, inits, ends, 24, 4, 8)
            for i, (g, w) in enumerate(zip(got, want)):
                assert K.same_answers([g], [w]), (mode, form, i, g[0], w[0])
            idx = list(range(10))
            alone = [gpu_run(ka, mode, form)(lps[i], labs[i], first[i], inits[i], ends[i], 24, 4, 8) for i in idx]
            assert K.same_answers(alone, [got[i] for i in idx])


def test_batch_of_both_forms_into_guarded_views(env):
    """one raw batch call whose lattices take both forms (a band of 1010 positions is generic, a short lattice's is not), outputs
    into views with sentinels on both sides"""
    from kokoro_align_amd import _lib
    ka, eng = env
    rng = np.random.default_rng(436)
    beam, mm, period = 1010, 4, 8
    shapes = [(20, 30), (24, 520), (9, 0), (16, 600), (33, 12), (40, 505), (8, 40), (12, 700)]   # L <= 1009: one wavefront
    n = len(shapes)
    lps, labs, first, inits, ends, want = [], [], [], [], [], []
    for i, (T, S) in enumerate(shapes):
        lp, lab = C.random_lattice(9200 + i, T, S)
        L = 2 * S + 1
        lo = 0 if i % 2 == 0 else int(rng.integers(0, min(L, 40)))
        init = None if i % 2 == 0 else K.free_row(L, max(lo - 2, 0), min(lo + 5, L))
        end = (-1, -2)[i % 2]
        lps.append(np.ascontiguousarray(lp)), labs.append(np.ascontiguousarray(lab, np.int32)), first.append(lo), inits.append(init), ends.append(end)
        want.append(K.ref_run()(lp, lab, lo, init, end, beam, mm, period))
    assert all(w[0] == "ok" for w in want)
    g = 3   # guard cells
    Ts = [lp.shape[0] for lp in lps]
    Ls = [2 * len(lab) + 1 for lab in labs]
    outs = [[np.full(T + 2 * g, SENTINEL, dt) for T in Ts] for dt in (np.int32, np.int32, np.float32, np.int32)]
    fins = [np.full(L + 2 * g, SENTINEL, np.float32) for L in Ls]
    arr = lambda ps: (ctypes.c_void_p * n)(*ps)   # noqa: E731
    i64 = lambda xs: (ctypes.c_int64 * n)(*xs)    # noqa: E731
    firsts, endsa = np.array(first, np.int32), np.array(ends, np.int32)
    entry, nxt, status, total = np.full(n + 2, SENTINEL, np.int32), np.full(n + 2, SENTINEL, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    rc = eng.lib.ka_ctc_best_path_tracking_resume_batch_f32(
        eng.handle, n, arr([x.ctypes.data for x in lps]), i64(Ts), C.V, i64([C.V] * n), arr([x.ctypes.data for x in labs]), i64([len(x) for x in labs]),
        beam, mm, period, firsts.ctypes.data, arr([None if x is None else x.ctypes.data for x in inits]), endsa.ctypes.data,
        *[arr([a[g:].ctypes.data for a in o]) for o in outs], arr([a[g:].ctypes.data for a in fins]), entry[1:].ctypes.data, nxt[1:].ctypes.data,
        total.ctypes.data, status.ctypes.data, _lib.KA_MEM_HOST, None)
    assert rc == 0 and not status.any()
    assert entry[0] == entry[-1] == nxt[0] == nxt[-1] == SENTINEL
    for i, w in enumerate(want):
        for o, j in zip(outs, (1, 2, 3, 4)):
            assert np.all(o[i][:g] == SENTINEL) and np.all(o[i][-g:] == SENTINEL) and R.same_bits(o[i][g:-g], w[j]), (i, j)
        assert np.all(fins[i][:g] == SENTINEL) and np.all(fins[i][-g:] == SENTINEL) and R.same_bits(fins[i][g:-g], w[7]), i
        assert bits(total[i])[0] == bits(w[5])[0] and entry[1 + i] == w[6] and nxt[1 + i] == w[8], i


# ---- bad arguments write nothing ----
def test_bad_arguments_write_nothing(env):
    from kokoro_align_amd import _lib
    ka, eng = env
    lp, lab = C.random_lattice(97, 12, 20)
    L = 2 * len(lab) + 1
    cases = [dict(first_lo=-1), dict(first_lo=L), dict(period=0), dict(period=6), dict(period=65540), dict(end=-3), dict(end=L), dict(table=False)]
    for kw in cases:
        final, entry, nxt = np.full(L, SENTINEL, np.float32), np.full(1, SENTINEL, np.int32), np.full(1, SENTINEL, np.int32)
        args = dict(first_lo=0, end=-1, period=4, table=True)
        args.update(kw)
        rc, outs, _ = raw_single(eng, lp, lab, args["first_lo"], None, args["end"], 16, 4, args["period"], final, entry, nxt, args["table"])
        assert rc == _lib.KA_ERR_BAD_ARGS, kw
        assert all(np.all(a == SENTINEL) for a in outs) and np.all(final == SENTINEL) and entry[0] == nxt[0] == SENTINEL, kw
    with pytest.raises(ValueError):
        ka.ctc_best_path_tracking_resume(lp, lab, L, None, "highest", 16, 4, 4)
    with pytest.raises(ValueError):
        ka.ctc_best_path_tracking_chunked(lp, lab, 6, 16, 4, 4)
    with pytest.raises(ValueError):
        ka.ctc_best_path_tracking_chunked(lp, lab, 0, 16, 4, 4)


# ---- the chunked front end ----
@pytest.mark.parametrize("chunk,period", [(256, 16), (64, 16), (256, 64), (64, 64)])
def test_chunked_is_the_tracking_call(env, chunk, period):
    ka, _ = env
    c = G.g2_cases()[0]
    T = 2000
    lp, lab = O.hash_logprobs(T, c["V"], c["seed"]), O.hash_labels(c["S"], c["V"], c["seed"])
    for end_rule in ("highest", "best"):
        want = ka.ctc_best_path_tracking(lp, lab, c["beam"], c["max_move"], period, end_rule)
        got = ka.ctc_best_path_tracking_chunked(lp, lab, chunk, c["beam"], c["max_move"], period, end_rule)
        assert len(got) == 4 and all(R.same_bits(g, w) for g, w in zip(got, want))
    if chunk == 256 and period == 16:
        import torch
        tgot = ka.ctc_best_path_tracking_chunked(torch.from_numpy(lp).cuda(), lab, chunk, c["beam"], c["max_move"], period)
        want = ka.ctc_best_path_tracking(lp, lab, c["beam"], c["max_move"], period)
        assert all(a.is_cuda and R.same_bits(a.cpu().numpy(), w) for a, w in zip(tgot, want))


def test_best_path_file_in_chunks(env, tmp_path):
    """best_path(track_chunk=) writes the file best_path(track_period=) writes"""
    ka, _ = env
    rng = np.random.default_rng(5)
    logits = rng.standard_normal((300, 39)).astype(np.float32)
    np.savez(tmp_path / "a.logits.npz", data=logits)
    (tmp_path / "a.voca.txt").write_text("konnichiwa|k o N n i ch i w a\nsekai|s e k a i\n" * 8)
    ka.best_path(str(tmp_path / "a.logits.npz"), str(tmp_path / "a.voca.txt"), str(tmp_path / "whole.npz"), track_period=16)
    ka.best_path(str(tmp_path / "a.logits.npz"), str(tmp_path / "a.voca.txt"), str(tmp_path / "chunks.npz"), track_period=16, track_chunk=64)
    with np.load(tmp_path / "whole.npz") as a, np.load(tmp_path / "chunks.npz") as b:
        assert sorted(a.files) == sorted(b.files) == ["band_lo", "best_labels", "best_path", "best_scores"]
        assert all(a[k].dtype == b[k].dtype and R.same_bits(a[k], b[k]) for k in a.files)


# ---- workspace ----
def test_workspace_bytes_cover_the_call(env):
    import torch
    ka, _ = env
    from kokoro_align_amd import _lib
    lib = _lib.load_library()
    shapes = [(304, 200, "wave"), (400, 520, "generic")]
    beam = {"wave": 1000, "generic": 1100}
    for mem in (_lib.KA_MEM_HOST, _lib.KA_MEM_DEVICE):
        for T, S, form in shapes:
            L = 2 * S + 1
            Ts, Ss = (ctypes.c_int64 * 1)(T), (ctypes.c_int64 * 1)(S)
            need = lib.ka_tracking_resume_workspace_bytes(1, Ts, Ss, 39, beam[form], 4, mem)
            tracking = lib.ka_tracking_workspace_bytes(1, Ts, Ss, 39, beam[form], 4, mem)
            rows = 2 * L * 4 if mem == _lib.KA_MEM_HOST else 0
            assert tracking + 40 + rows <= need <= tracking + 2 * 256 + rows + 2 * 256
            assert lib.ka_tracking_resume_workspace_bytes(1, Ts, Ss, 39, beam[form], 300, mem) == 0
            assert lib.ka_tracking_resume_workspace_bytes(1, Ts, Ss, 39, beam[form], 4, 7) == 0
            lp, lab = O.hash_logprobs(T, 39, T + S), O.hash_labels(S, 39, T + S)
            init = K.free_row(L, 0, 3)
            want = R.best_path_tracking_resume(lp, lab, 0, init, R.END_BEST, beam[form], 4, 16)
            ka.ctc_best_path_tracking_resume_batch([lp], [lab], 0, [init], "best", beam[form], 4, 16)   # (the kernels' code is on the device before memory is counted)
            eng = _lib.Engine(torch.cuda.current_device())
            try:
                eng.reserve(need)
                outs = [np.empty(T, np.int32), np.empty(T, np.int32), np.empty(T, np.float32), np.empty(T, np.int32), np.empty(L, np.float32)]
                if mem == _lib.KA_MEM_DEVICE:
                    keep = [torch.from_numpy(x).cuda() for x in (lp, lab, init)] + [torch.from_numpy(x).cuda() for x in outs]
                    ptr = [x.data_ptr() for x in keep]
                else:
                    ptr = [x.ctypes.data for x in (lp, lab, init)] + [x.ctypes.data for x in outs]
                entry, nxt, total = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32)
                torch.cuda.synchronize()
                free0 = torch.cuda.mem_get_info()[0]
                rc = lib.ka_ctc_best_path_tracking_resume_f32(eng.handle, ptr[0], T, 39, 39, ptr[1], S, beam[form], 4, 16, 0, ptr[2], -2, ptr[3], ptr[4],
                                                              ptr[5], ptr[6], ptr[7], entry.ctypes.data, nxt.ctypes.data, total.ctypes.data, mem, None)
                assert rc == 0 and torch.cuda.mem_get_info()[0] == free0, (T, S, form, mem)
                got = [x.cpu().numpy() for x in keep[3:]] if mem == _lib.KA_MEM_DEVICE else outs
                assert all(R.same_bits(g, w) for g, w in zip(got, want[:4] + (want[6],)))
                assert entry[0] == want[5] and nxt[0] == want[7] and bits(total)[0] == bits(want[4])[0]
            finally:
                eng.close()
