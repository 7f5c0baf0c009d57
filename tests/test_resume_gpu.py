"""The resumable best path on the GPU (ka_ctc_best_path_resume[_batch]_f32).  Every comparison is exact -
path, labels, the bits of the scores, of the total and of the last row, the entry, the status - against tests/resume_ref.py
(tests/test_resume_cpu.py asserts that the reference and the cases do what they say), through the C ABI and both Python front
doors, in both kernel forms: a NULL start is the banded call; a cut lattice resumed gives the uncut answer; start rows, ends,
batches, the workspace figure, the chunked front end.
"""
import ctypes

import numpy as np
import pytest

import band_cases as C
import golden_util as G
import resume_cases as X
import resume_ref as RR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MODES = ("host", "device")
FORMS = ("wave", "generic")
SENTINEL = -7777
DEAD_BITS = 0x7fc00000


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    lib = _lib.load_library()
    for sym in ("ka_ctc_best_path_resume_f32", "ka_ctc_best_path_resume_batch_f32", "ka_resume_workspace_bytes"):
        assert hasattr(lib, sym), sym
    return ka, _lib.default_engine(torch.cuda.current_device())


def bits(x):
    return np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32)


def widened(lp):
    """72 more columns (that no label names) make V = 80: the generic kernels"""
    return np.concatenate([lp, np.full((lp.shape[0], 72), -1.0, np.float32)], axis=1)


def answers(results, status, total):
    """the results of a Python batch call as the scenarios of resume_cases want them"""
    out = []
    for (path, lab, sc, entry, final), st, tot in zip(results, status, total):
        path, lab, sc, final = (np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in (path, lab, sc, final))
        if st == 0:
            out.append(("ok", path, lab, sc, np.float32(tot), int(entry), final))
        elif st == -1:
            assert entry == -1
            out.append(("empty", final))
        else:   # the lattice's own failure: no path, a dead row
            assert entry == -1 and np.all(bits(final) == DEAD_BITS), st
            out.append(("bad_args",) if st == -2 else ("failed", int(st)))
    return out


def batch(ka, mode, form, lps, labs, los, inits, ends, beam, mm):
    if form == "generic":
        lps = [widened(lp) for lp in lps]
    if mode == "host":
        return answers(*ka.ctc_best_path_resume_batch(lps, labs, los, inits, ends, beam, mm, return_status=True))
    import torch
    dlp = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lps]
    return answers(*ka.ctc_best_path_resume_device(dlp, labs, los, inits, ends, beam, mm, return_status=True))


def gpu_run(ka, mode, form):
    def run(lp, lab, lo, init, end, beam, mm):
        return batch(ka, mode, form, [lp], [lab], [lo], [init], [end], beam, mm)[0]
    return run


def assert_scenario(ka, scenario, what):
    want = scenario(X.ref_run())
    for mode in MODES:
        for form in FORMS:
            got = scenario(gpu_run(ka, mode, form))
            assert X.same_answers(got, want), f"{what} [{mode}, {form}]: {[g[0] for g in got]} against {[w[0] for w in want]}"
    return want


# ---- property 1: a NULL start, the reference's end, no last row: the banded call ----
def raw_single(eng, lp, lab, lo, init, end, beam, mm, final=None, entry=None, outs=None):
    """ka_ctc_best_path_resume_f32 on host buffers"""
    from kokoro_align_amd import _lib
    lp = np.ascontiguousarray(lp, np.float32)
    lab = np.ascontiguousarray(lab, np.int32)
    lo = np.ascontiguousarray(lo, np.int32)
    T, V = lp.shape
    outs = outs or [np.full(T, SENTINEL, np.int32), np.full(T, SENTINEL, np.int32), np.full(T, SENTINEL, np.float32)]
    total = np.zeros(1, np.float32)
    rc = eng.lib.ka_ctc_best_path_resume_f32(eng.handle, lp.ctypes.data, T, V, V, lab.ctypes.data, len(lab), beam, mm, lo.ctypes.data,
                                             None if init is None else init.ctypes.data, int(end), *[a.ctypes.data for a in outs],
                                             None if final is None else final.ctypes.data, None if entry is None else entry.ctypes.data,
                                             total.ctypes.data, _lib.KA_MEM_HOST, None)
    return rc, outs, total[0]


@pytest.mark.parametrize("name", C.NAMES)
def test_null_start_is_the_banded_call(env, name):
    ka, eng = env
    lp, lab, lo, beam, mm = C.case(name)
    want = C.want(name)
    L = 2 * len(lab) + 1
    for init in (None, X.free_row(L, 0, 1)):
        rc, outs, total = raw_single(eng, lp, lab, lo, init, -1, beam, mm)
        if want is None:
            assert rc == -1 and all(np.all(a == SENTINEL) for a in outs)
            continue
        assert rc == 0 and all(RR.same_bits(g, w) for g, w in zip(outs, want[:3])) and bits(total)[0] == bits(want[3])[0], name
    # ... and with the last row and the entry asked for, through the Python front doors, against the reference
    assert_scenario(ka, lambda run: [run(lp, lab, lo, None, RR.END_HIGHEST, beam, mm)], name)


@pytest.mark.parametrize("T,S,V,beam,mm", [(100, 60, 80, 24, 4), (450, 600, 39, 1100, 4), (100, 60, 39, 24, 6)])
def test_null_start_is_the_banded_call_generic_form(env, T, S, V, beam, mm):
    ka, _ = env
    rng = np.random.default_rng(T + V + mm)
    lp = (np.round(rng.standard_normal((T, V)) * 16) / 8).astype(np.float32)
    lab = rng.integers(0, V, size=S).astype(np.int32)
    lo = ka.diagonal_band(T, 2 * S + 1, beam)
    (want,), st, wtot = ka.ctc_best_path_banded_batch([lp], [lab], [lo], beam, mm, return_status=True)
    assert list(st) == [0]
    for init in (None, X.free_row(2 * S + 1, 0, 1)):
        (got,), st, tot = ka.ctc_best_path_resume_batch([lp], [lab], [lo], [init], "highest", beam, mm, return_status=True)
        assert list(st) == [0] and got[3] == 0
        assert all(RR.same_bits(g, w) for g, w in zip(got[:3], want)) and bits(tot[0])[0] == bits(wtot[0])[0]
    # a cut in this form's own shapes
    k = T // 2
    ref = RR.best_path_resume(lp, lab, lo, None, RR.END_HIGHEST, beam, mm)
    out = X.chain(gpu_run(ka, "host", "wave"), lp, lab, lo, k, None, beam, mm)   # ("wave": the log-probs as they are)
    got = X.joined(out)
    assert all(RR.same_bits(g, w) for g, w in zip(got[:3], ref[:3])) and bits(got[3])[0] == bits(ref[3])[0]


# ---- property 2: cut and resume ----
@pytest.mark.parametrize("name", X.CUT_CASES)
def test_cut_and_resume(env, name):
    ka, _ = env
    lp, lab, lo, beam, mm = C.case(name)
    whole = C.want(name)
    for k in X.cuts_of(name):
        want = assert_scenario(ka, X.cut_scenario(name, k), f"{name} cut at {k}")
        got = X.joined(want)
        assert got is not None and whole is not None
        assert all(RR.same_bits(g, w) for g, w in zip(got[:3], whole[:3])) and bits(got[3])[0] == bits(whole[3])[0]
    if name == "ninf":   # live -inf cells in the start rows
        assert any(np.any(np.isneginf(X.cut_scenario(name, k)(X.ref_run())[0][6])) for k in X.cuts_of(name))


@pytest.mark.parametrize("key", X.EDGE_KEYS, ids=lambda k: "lo%d_d%d" % (k[0], k[2]))
def test_cut_at_a_block_edge(env, key):
    ka, _ = env
    want = assert_scenario(ka, X.edge_scenario(key), f"block edge {key}")
    assert len(want) == 3 and want[1][5] == key[0] - key[2]


# ---- start rows and ends ----
@pytest.mark.parametrize("name", list(X.start_row_scenarios()))
def test_start_rows_and_ends(env, name):
    ka, _ = env
    assert_scenario(ka, X.start_row_scenarios()[name], name)


def test_excerpt_through_the_front_door(env):
    import torch
    ka, _ = env
    lp, lab, lo, beam, mm = X.excerpt()
    L = 2 * len(lab) + 1
    want = RR.best_path_resume(lp, lab, lo, ka.free_start_scores(L), RR.END_BEST, beam, mm)
    got = ka.ctc_best_path_resume(lp, lab, lo, ka.free_start_scores(L), "best", beam, mm)
    assert all(isinstance(a, np.ndarray) for a in got[:3]) and got[3] == 50 == want[4] and got[0][-1] == 89
    assert all(RR.same_bits(g, w) for g, w in zip(got[:3] + (got[4],), want[:3] + (want[5],)))
    tgot = ka.ctc_best_path_resume(torch.from_numpy(lp).cuda(), lab, lo, torch.from_numpy(ka.free_start_scores(L)).cuda(), "best", beam, mm)
    assert all(isinstance(tgot[i], torch.Tensor) and tgot[i].is_cuda for i in (0, 1, 2, 4)) and tgot[3] == 50
    assert all(RR.same_bits(tgot[i].cpu().numpy(), want[j]) for i, j in ((0, 0), (1, 1), (2, 2), (4, 5)))
    with pytest.raises(ValueError):
        ka.ctc_best_path_resume(lp[:10], lab, lo[:10], None, L - 1, beam, mm)   # (ten frames from position 0 do not reach it: not live)
    with pytest.raises(ValueError):
        ka.ctc_best_path_resume(lp, lab, lo, ka.free_start_scores(L)[:-1], "best", beam, mm)


def test_end_out_of_range_writes_nothing(env):
    from kokoro_align_amd import _lib
    ka, eng = env
    lp, lab, lo, beam, mm = C.case("const0")
    L = 2 * len(lab) + 1
    for end in (-3, L, L + 5):
        final = np.full(L, SENTINEL, np.float32)
        entry = np.full(1, SENTINEL, np.int32)
        rc, outs, _ = raw_single(eng, lp, lab, lo, None, end, beam, mm, final, entry)
        assert rc == _lib.KA_ERR_BAD_ARGS
        assert all(np.all(a == SENTINEL) for a in outs) and np.all(final == SENTINEL) and entry[0] == SENTINEL
    with pytest.raises(ValueError):
        ka.ctc_best_path_resume(lp, lab, lo, None, L, beam, mm)


def test_failed_lattices_get_a_dead_row_and_spare_their_neighbours(env):
    """a +inf start cell, a bad label, a NaN log-prob, a bad table: each the status of its lattice alone, its last row all dead"""
    from kokoro_align_amd import _lib
    ka, _ = env
    lp, lab, lo, beam, mm = C.case("shifted")
    L = 2 * len(lab) + 1
    pinf = X.free_row(L, 0, 4)
    pinf[2] = np.inf
    bad_lab = lab.copy()
    bad_lab[5] = 1000   # (no vocabulary of these tests is that large)
    nan_lp = lp.copy()
    nan_lp[7, 3] = np.nan
    bad_lo = lo.copy()
    bad_lo[0] = -1
    for mode in MODES:
        for form in FORMS:
            alone = batch(ka, mode, form, [lp], [lab], [lo], [None], [-1], beam, mm)
            lps = [widened(x) if form == "generic" else x for x in (lp, lp, lp, nan_lp, lp, lp)]
            args = (lps, [lab, lab, bad_lab, lab, lab, lab], [lo, lo, lo, lo, bad_lo, lo], [None, pinf, None, None, None, None], [-1] * 6, beam, mm)
            if mode == "host":
                res, st, tot = ka.ctc_best_path_resume_batch(*args, return_status=True)
            else:
                import torch
                res, st, tot = ka.ctc_best_path_resume_device([torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lps], *args[1:], return_status=True)
            assert list(st) == [0, _lib.KA_ERR_BAD_ARGS, _lib.KA_ERR_BAD_LABEL, _lib.KA_ERR_NAN, _lib.KA_ERR_BAD_ARGS, 0], (mode, form, st)
            for i in (1, 2, 3, 4):
                final = res[i][4]
                assert res[i][3] == -1 and np.all(bits(final.cpu().numpy() if hasattr(final, "cpu") else final) == DEAD_BITS), (mode, form, i)
            got = answers(res, st, tot)
            assert X.same_answers([got[0]], alone) and X.same_answers([got[5]], alone), (mode, form)


# ---- batches ----
def mixed_batch():
    """lattices of one V, beam and max_move that mix NULL and given start rows and the three kinds of end, failures among them"""
    rng = np.random.default_rng(434)
    lps, labs, los, inits, ends = [], [], [], [], []
    for i in range(40):
        T, S = int(rng.integers(1, 40)), int(rng.integers(0, 60))
        L = 2 * S + 1
        lp, lab = C.random_lattice(9000 + i, T, S, ninf=(i % 5 == 0))
        lo = np.minimum(np.cumsum(rng.integers(0, 3, T)) + int(rng.integers(0, 1 + L // 2)), L - 1).astype(np.int64)
        init = None
        if i % 3:
            init = X.free_row(L, max(int(lo[0]) - int(rng.integers(0, 6)), 0), min(int(lo[0]) + int(rng.integers(1, 9)), L))
            init[~np.isnan(init)] = (np.round(rng.standard_normal(int(np.sum(~np.isnan(init)))) * 16) / 8).astype(np.float32)
            if i % 7 == 0:
                init[int(lo[0])] = -np.inf
        end = (-1, -2, int(rng.integers(0, L)))[i % 3 if i % 4 else 2]
        if end >= 0 and i % 8:   # (mostly a cell that is live at the end)
            row = X.ref_run()(lp, lab, lo, init, RR.END_HIGHEST, 24, 4)[-1]
            if np.any(~np.isnan(row)):
                end = int(rng.choice(np.nonzero(~np.isnan(row))[0]))
        lps.append(lp), labs.append(lab), los.append(lo), inits.append(init), ends.append(end)
    return lps, labs, los, inits, ends


def test_batch_lattices_get_the_bits_they_have_alone(env):
    ka, _ = env
    lps, labs, los, inits, ends = mixed_batch()
    run = X.ref_run()
    want = [run(lp, lab, lo, init, end, 24, 4) for lp, lab, lo, init, end in zip(lps, labs, los, inits, ends)]
    kinds = [w[0] for w in want]
    assert kinds.count("ok") >= 15 and kinds.count("empty") >= 5
    assert {e for e, w in zip(ends, want) if w[0] == "ok"} >= {-1, -2} and any(e >= 0 and w[0] == "ok" for e, w in zip(ends, want))
    for mode in MODES:
        for form in FORMS:
            got = batch(ka, mode, form, lps, labs, los, inits, ends, 24, 4)
            for i, (g, w) in enumerate(zip(got, want)):
                assert X.same_answers([g], [w]), (mode, form, i, g[0], w[0])
            alone = [gpu_run(ka, mode, form)(lp, lab, lo, init, end, 24, 4) for lp, lab, lo, init, end in list(zip(lps, labs, los, inits, ends))[:8]]
            assert X.same_answers(alone, got[:8])


# ---- the chunked front end ----
@pytest.mark.parametrize("chunk", [256, 250])
def test_chunked_is_the_banded_call(env, chunk):
    ka, _ = env
    c = G.g2_cases()[0]
    T = 2000
    lp, lab = O.hash_logprobs(T, c["V"], c["seed"]), O.hash_labels(c["S"], c["V"], c["seed"])
    lo = ka.diagonal_band(T, 2 * c["S"] + 1, c["beam"])
    want = ka.ctc_best_path_banded(lp, lab, lo, c["beam"], c["max_move"])
    got = ka.ctc_best_path_chunked(lp, lab, lo, chunk, c["beam"], c["max_move"])
    assert len(got) == 3 and all(RR.same_bits(g, w) for g, w in zip(got, want))
    if chunk == 250:
        import torch
        tgot = ka.ctc_best_path_chunked(torch.from_numpy(lp).cuda(), lab, lo, chunk, c["beam"], c["max_move"])
        assert all(a.is_cuda and RR.same_bits(a.cpu().numpy(), w) for a, w in zip(tgot, want))


# ---- workspace ----
def test_workspace_bytes_cover_the_call(env):
    import torch
    ka, _ = env
    from kokoro_align_amd import _lib
    lib = _lib.load_library()
    shapes = [(300, 200, "wave"), (400, 520, "generic")]
    beam = {"wave": 1000, "generic": 1100}
    for mem in (_lib.KA_MEM_HOST, _lib.KA_MEM_DEVICE):
        for T, S, form in shapes:
            L = 2 * S + 1
            Ts, Ss = (ctypes.c_int64 * 1)(T), (ctypes.c_int64 * 1)(S)
            need = lib.ka_resume_workspace_bytes(1, Ts, Ss, 39, beam[form], 4, mem)
            banded = lib.ka_banded_workspace_bytes(1, Ts, Ss, 39, beam[form], 4, mem)
            rows = 2 * L * 4 if mem == _lib.KA_MEM_HOST else 0
            assert banded + 36 + rows <= need <= banded + 2 * 256 + rows + 2 * 256
            assert lib.ka_resume_workspace_bytes(1, Ts, Ss, 39, beam[form], 300, mem) == 0 and lib.ka_resume_workspace_bytes(1, Ts, Ss, 39, beam[form], 4, 7) == 0
            lp, lab = O.hash_logprobs(T, 39, T + S), O.hash_labels(S, 39, T + S)
            lo = np.ascontiguousarray(ka.diagonal_band(T, L, beam[form]), np.int32)
            init = X.free_row(L, 0, 3)
            want = RR.best_path_resume(lp, lab, lo, init, RR.END_BEST, beam[form], 4)
            ka.ctc_best_path_resume_batch([lp], [lab], [lo], [init], "best", beam[form], 4)   # (the kernels' code is on the device before memory is counted)
            eng = _lib.Engine(torch.cuda.current_device())
            try:
                eng.reserve(need)
                outs = [np.empty(T, np.int32), np.empty(T, np.int32), np.empty(T, np.float32), np.empty(L, np.float32)]
                if mem == _lib.KA_MEM_DEVICE:
                    keep = [torch.from_numpy(x).cuda() for x in (lp, lab, lo, init)] + [torch.from_numpy(x).cuda() for x in outs]
                    ptr = [x.data_ptr() for x in keep]
                else:
                    ptr = [x.ctypes.data for x in (lp, lab, lo, init)] + [x.ctypes.data for x in outs]
                entry, total = np.zeros(1, np.int32), np.zeros(1, np.float32)
                torch.cuda.synchronize()
                free0 = torch.cuda.mem_get_info()[0]
                rc = lib.ka_ctc_best_path_resume_f32(eng.handle, ptr[0], T, 39, 39, ptr[1], S, beam[form], 4, ptr[2], ptr[3], -2, ptr[4], ptr[5], ptr[6],
                                                     ptr[7], entry.ctypes.data, total.ctypes.data, mem, None)
                assert rc == 0 and torch.cuda.mem_get_info()[0] == free0, (T, S, form, mem)
                got = [x.cpu().numpy() for x in keep[4:]] if mem == _lib.KA_MEM_DEVICE else outs
                assert all(RR.same_bits(g, w) for g, w in zip(got, want[:3] + (want[5],))) and entry[0] == want[4] and bits(total)[0] == bits(want[3])[0]
            finally:
                eng.close()
