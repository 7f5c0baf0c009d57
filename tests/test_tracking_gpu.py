"""The best path over a self-steering band on the GPU (ka_ctc_best_path_tracking[_batch]_f32).  Every
comparison is exact - path, labels, the bits of the scores and of the total, the table, the status - against tests/track_ref.py
on the inputs of tests/track_cases.py (tests/test_tracking_cpu.py asserts that they do what their names say), in both kernel
forms and both memory modes; the table that comes back is fed to the banded calls of sections 4.29 and 4.30."""
import ctypes
import os

import numpy as np
import pytest

import band_cases as C
import track_cases as K

pytestmark = pytest.mark.gpu

MODES = ("host", "device")
SENTINEL = -7777


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    assert os.path.exists(ka.library_path()), "HIP library not built"
    assert hasattr(_lib.load_library(), "ka_ctc_best_path_tracking_batch_f32")
    return ka, _lib.default_engine(torch.cuda.current_device())


def run(ka, mode, lps, labs, beam, mm, period, end_rule):
    """(results as NumPy arrays, statuses, totals) of one tracking call in the given memory mode; host rows lie at a stride ld > V"""
    if mode == "host":
        wide = []
        for lp in lps:
            buf = np.full((lp.shape[0], lp.shape[1] + 3), np.nan, np.float32)   # (a NaN read from the padding would be a status)
            buf[:, :lp.shape[1]] = lp
            wide.append(buf[:, :lp.shape[1]])
        return ka.ctc_best_path_tracking_batch(wide, labs, beam, mm, period, end_rule, return_status=True)
    import torch
    dlp = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lps]
    res, status, total = ka.ctc_best_path_tracking_device(dlp, labs, beam, mm, period, end_rule, return_status=True)
    return [tuple(a.cpu().numpy() for a in r) for r in res], status, total


def differs(got, total, want, want_total):
    """None when the arrays of `got` and the total are `want`'s in every bit, else what differs first"""
    for g, w, field in zip(got, want, ("path", "labels", "scores", "table")):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape:
            return f"{field} has shape {g.shape}"
        bad = np.nonzero(g.view(np.int32) != w.view(np.int32))[0]
        if bad.size:
            return f"{field} differs at {bad.size} frames, first at frame {int(bad[0])}: got {g[bad[0]]}, want {w[bad[0]]}"
    if np.float32(total).view(np.int32) != np.float32(want_total).view(np.int32):
        return f"total {total!r}, want {want_total!r}"
    return None


# ---- the cases against track_ref ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", K.NAMES)
def test_case_against_track_ref(env, name, mode):
    ka, _ = env
    lp, lab, beam, mm, period, end_rule = K.case(name)
    want = K.want(name)
    res, status, total = run(ka, mode, [lp], [lab], beam, mm, period, end_rule)
    assert list(status) == [0], (name, status)
    why = differs(res[0], total[0], want[:4], want[4])
    assert why is None, f"{name} [{mode}]: {why}"


def test_single_calls_and_both_front_doors(env):
    import torch
    ka, _ = env
    lp, lab, beam, mm, period, end_rule = K.case("mm4_best")
    want = K.want("mm4_best")
    got = ka.ctc_best_path_tracking(lp, lab, beam, mm, period, end_rule)
    assert len(got) == 4 and differs(got, want[4], want[:4], want[4]) is None
    tgot = ka.ctc_best_path_tracking(torch.from_numpy(lp).cuda(), torch.from_numpy(lab).cuda(), beam, mm, period, end_rule)
    assert all(torch.is_tensor(x) and x.is_cuda for x in tgot)
    assert differs([x.cpu().numpy() for x in tgot], want[4], want[:4], want[4]) is None
    # the C single-lattice entry, end_rule by number
    from kokoro_align_amd import _lib
    eng = _lib.default_engine(torch.cuda.current_device())
    T, lpc = lp.shape[0], np.ascontiguousarray(lp)
    outs = [np.empty(T, np.int32), np.empty(T, np.int32), np.empty(T, np.float32), np.empty(T, np.int32)]
    total = ctypes.c_float(0)
    rc = eng.lib.ka_ctc_best_path_tracking_f32(eng.handle, lpc.ctypes.data, T, lpc.shape[1], lpc.shape[1], lab.ctypes.data, len(lab), beam, mm,
                                               period, 1, outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, outs[3].ctypes.data,
                                               ctypes.addressof(total), _lib.KA_MEM_HOST, None)
    assert rc == 0 and differs(outs, total.value, want[:4], want[4]) is None


# ---- a band as wide as the lattice: ctc_best_path at the same beam, for any period ----
@pytest.mark.parametrize("name,period", [("mm4_best", 4), ("ninf", 64), ("step16", 8), ("S0", 4), ("T1", 4), ("gen_mm5", 8), ("gen_V65", 16)])
def test_wide_beam_is_ctc_best_path(env, name, period):
    ka, _ = env
    lp, lab, _, mm, _, _ = K.case(name)
    beam = 2 * (2 * len(lab) + 1)
    ref, ref_status, ref_total = ka.ctc_best_path_batch([lp], [lab], beam, mm, return_status=True)
    assert list(ref_status) == [0]
    for mode in MODES:
        res, status, total = run(ka, mode, [lp], [lab], beam, mm, period, "highest")
        assert list(status) == [0]
        why = differs(res[0], total[0], ref[0] + (np.zeros(lp.shape[0], np.int32),), ref_total[0])
        assert why is None, f"{name} [{mode}]: {why}"


# ---- the round trip: the banded call over the returned table ----
@pytest.mark.parametrize("name", ["step1", "step70", "step504", "ninf", "ninf_list", "wrap", "mm2", "mm3", "beam1", "T5", "rescue3_p8",
                                  "gen_mm5", "gen_V65", "gen_band1010"])
def test_round_trip_through_the_banded_call(env, name):
    ka, _ = env
    lp, lab, beam, mm, period, end_rule = K.case(name)
    assert end_rule == "highest"
    res, status, total = run(ka, "host", [lp], [lab], beam, mm, period, end_rule)
    (again,), st, tot = ka.ctc_best_path_banded_batch([lp], [lab], [res[0][3]], beam, mm, return_status=True)
    assert list(st) == list(status) == [0]
    why = differs(again, tot[0], res[0][:3], total[0])
    assert why is None, f"{name}: {why}"


def test_posteriors_take_the_returned_table(env):
    ka, _ = env
    lp, labels, L, beam, pre = C.rescue(2)
    path, _, _, table = ka.ctc_best_path_tracking(lp, labels, beam, 4, 8)
    assert np.array_equal(table, K.want("rescue2_p8")[3])
    post, ll = ka.ctc_path_posteriors(lp, labels, path, beam, 4, band_lo=table)    # raises unless KA_OK
    assert post.shape == (lp.shape[0],) and np.isfinite(ll) and ll >= float(K.want("rescue2_p8")[4])
    assert ka.band_edge_contact(path, table, beam, L).size < lp.shape[0]


# ---- the rescue case ----
@pytest.mark.parametrize("seed", range(6))
def test_rescue_case(env, seed):
    ka, _ = env
    lp, labels, L, beam, pre = C.rescue(seed)
    (full,), st, full_total = ka.ctc_best_path_batch([lp], [labels], 2 * L, 4, return_status=True)
    assert list(st) == [0]
    for period in (4, 8):
        (got,), st, total = ka.ctc_best_path_tracking_batch([lp], [labels], beam, 4, period, return_status=True)
        assert list(st) == [0]
        why = differs(got[:3], total[0], full, full_total[0])
        assert why is None, (period, why)
    (lost,), st, total = ka.ctc_best_path_tracking_batch([lp], [labels], beam, 4, 16, return_status=True)
    assert list(st) == [0] and int(np.sum(lost[0] != full[0])) > 100


# ---- batches ----
BATCH_BEAM = 1100
_batch = {}


def the_batch(ka):
    """150 one-wavefront and 60 generic small lattices (one call: one beam, 1100, so L <= 1009 picks the form), every seventh
    with a label out of range, and what each returns when it is sent alone."""
    if _batch:
        return _batch
    rng = np.random.default_rng(4321)
    kinds = ["wave"] * 150 + ["generic"] * 60
    rng.shuffle(kinds)
    lps, labs = [], []
    for i, kind in enumerate(kinds):
        T = int(rng.integers(1, 41)) if kind == "wave" else int(rng.integers(2, 14))
        S = int(rng.integers(1, 41)) if kind == "wave" else int(rng.integers(505, 516))
        lp, lab = C.random_lattice(7000 + i, T, S, ninf=(i % 5 == 0))
        if i % 7 == 3:
            lab[int(rng.integers(0, S))] = K.V + (i % 3)
        lps.append(lp)
        labs.append(lab)
    alone = [ka.ctc_best_path_tracking_batch([lp], [lab], BATCH_BEAM, 4, 4, "best" if i % 2 else "highest", return_status=True)
             for i, (lp, lab) in enumerate(zip(lps, labs))]
    _batch.update(lps=lps, labs=labs, alone=alone, kinds=kinds)
    return _batch


@pytest.mark.parametrize("end_rule", ["highest", "best"])
@pytest.mark.parametrize("mode", MODES)
def test_batch_lattices_get_the_bits_they_have_alone(env, mode, end_rule):
    import torch
    from kokoro_align_amd import _lib
    ka, _ = env
    b = the_batch(ka)
    lps, labs, alone = b["lps"], b["labs"], b["alone"]
    n = len(lps)
    mine = [i for i in range(n) if (i % 2 == 1) == (end_rule == "best")]   # the lone calls of this end rule
    statuses = [alone[i][1][0] for i in range(n)]
    assert statuses.count(_lib.KA_ERR_BAD_LABEL) == 30 and statuses.count(0) == n - 30
    # outputs: views into one array per output, a sentinel element between neighbours
    offs = np.concatenate([[1], 1 + np.cumsum([lp.shape[0] + 1 for lp in lps])])
    if mode == "host":
        big = [np.full(offs[-1], SENTINEL, dt) for dt in (np.int32, np.int32, np.float32, np.int32)]
        views = [[a[offs[i]:offs[i] + lps[i].shape[0]] for i in range(n)] for a in big]
        res, status, total = ka.ctc_best_path_tracking_batch(lps, labs, BATCH_BEAM, 4, 4, end_rule, return_status=True, outputs=views)
        out = big
    else:
        big = [torch.full((int(offs[-1]),), SENTINEL, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.float32, torch.int32)]
        views = [[a[int(offs[i]):int(offs[i]) + lps[i].shape[0]] for i in range(n)] for a in big]
        dlp = [torch.from_numpy(x).cuda() for x in lps]
        res, status, total = ka.ctc_best_path_tracking_device(dlp, labs, BATCH_BEAM, 4, 4, end_rule, return_status=True, outputs=views)
        out = [a.cpu().numpy() for a in big]
    assert list(status) == statuses
    for i in range(n):
        sl = slice(offs[i], offs[i] + lps[i].shape[0])
        if statuses[i] != 0:
            # host buffers of a failed lattice are not copied out (its table may hold anything); device buffers are the
            # kernels' own, written within their T elements: the guards below
            assert mode == "device" or all(np.all(a[sl] == SENTINEL) for a in out[:3]), i
        elif i in mine:
            why = differs([a[sl] for a in out], total[i], alone[i][0][0], alone[i][2][0])
            assert why is None, f"lattice {i} ({b['kinds'][i]}) [{mode}]: {why}"
        else:   # the other end rule walks the same table
            assert np.array_equal(out[3][sl], alone[i][0][0][3]), i
    guards = np.concatenate([[0], offs[1:] - 1])
    assert all(np.all(a[guards] == SENTINEL) for a in out)


# ---- statuses ----
@pytest.mark.parametrize("form", ["wave", "generic"])
def test_a_nan_is_a_status_and_never_an_index(env, form):
    from kokoro_align_amd import _lib
    ka, _ = env
    lp, lab = C.random_lattice(90, 40, 30)
    lp = lp.copy()
    lp[5:9, :] = np.nan          # the scores the retarget of frame 8 reads are all NaN
    mm = 4 if form == "wave" else 5
    for mode in MODES:
        res, status, total = run(ka, mode, [lp, K.case("mm3")[0]], [lab, K.case("mm3")[1]], 8, mm, 4, "best")
        assert list(status) == [_lib.KA_ERR_NAN, 0], (form, mode, status)
    with pytest.raises(ValueError):
        ka.ctc_best_path_tracking(lp, lab, 8, mm, 4)


def test_bad_arguments_write_nothing(env):
    import torch
    from kokoro_align_amd import _lib
    from bestpath_harness import tracking_call
    ka, _ = env
    eng = _lib.default_engine(torch.cuda.current_device())
    lp, lab, beam, mm, _, _ = K.case("mm3")
    lpc, T = np.ascontiguousarray(lp), lp.shape[0]

    def call(period, end_rule, null_table=False):
        outs = [np.full(T, SENTINEL, dt) for dt in (np.int32, np.int32, np.float32, np.int32)]
        ptrs = [[a.ctypes.data] for a in outs]
        if null_table:
            ptrs[3] = [None]
        rc, status, _ = tracking_call(eng, [(lpc.ctypes.data, T)], [(lab.ctypes.data, len(lab))], [lpc.shape[1]], lpc.shape[1], beam, mm, period,
                                       end_rule, *ptrs, _lib.KA_MEM_HOST, None)
        assert all(np.all(a == SENTINEL) for a in outs), (period, end_rule, null_table)
        return rc

    for period in (0, -4, 1, 2, 3, 5, 6, 18, 65540, 1 << 20):
        assert call(period, 0) == _lib.KA_ERR_BAD_ARGS, period
    for end_rule in (-1, 2, 7):
        assert call(8, end_rule) == _lib.KA_ERR_BAD_ARGS, end_rule
    assert call(8, 0, null_table=True) == _lib.KA_ERR_BAD_ARGS
    with pytest.raises(KeyError):
        ka.ctc_best_path_tracking(lp, lab, beam, mm, 8, "lowest")
    with pytest.raises(ValueError):
        ka.ctc_best_path_tracking(lp, lab, beam, mm, 6)
    # the limits themselves are fine
    for period in (4, 65536):
        got = ka.ctc_best_path_tracking(lp, lab, beam, mm, period)
        assert got[3][0] == 0 and (period == 4 or not got[3].any())


# ---- workspace ----
def test_workspace_bytes_cover_the_call(env):
    import torch
    ka, _ = env
    from kokoro_align_amd import _lib
    from bestpath_harness import tracking_call
    from oracle import oracle as O
    shapes = [(300, 200, "wave"), (401, 500, "wave"), (400, 520, "generic")]
    beam = {"wave": 1000, "generic": 1100}
    lib = _lib.load_library()
    for mem in (_lib.KA_MEM_HOST, _lib.KA_MEM_DEVICE):
        for T, S, form in shapes:
            Ts, Ss = (ctypes.c_int64 * 1)(T), (ctypes.c_int64 * 1)(S)
            need = lib.ka_tracking_workspace_bytes(1, Ts, Ss, 39, beam[form], 4, mem)
            W = min(beam[form], 2 * S + 1)
            assert need >= (T * 256 if form == "wave" else T * W) + (T * 39 * 4 if mem == _lib.KA_MEM_HOST else 0)
            assert need <= lib.ka_banded_workspace_bytes(1, Ts, Ss, 39, beam[form], 4, mem) - (T * 4 if form == "wave" else 0)
            eng = _lib.Engine(torch.cuda.current_device())
            try:
                eng.reserve(need)
                lp, lab = O.hash_logprobs(T, 39, T + S), O.hash_labels(S, 39, T + S)
                outs = [np.empty(T, np.int32), np.empty(T, np.int32), np.empty(T, np.float32), np.empty(T, np.int32)]
                if mem == _lib.KA_MEM_DEVICE:
                    keep = [torch.from_numpy(x).cuda() for x in (lp, lab)] + [torch.from_numpy(x).cuda() for x in outs]
                    ptr = [x.data_ptr() for x in keep]
                else:
                    ptr = [x.ctypes.data for x in (lp, lab)] + [x.ctypes.data for x in outs]
                want = ka.ctc_best_path_tracking_batch([lp], [lab], beam[form], 4, 16)[0]   # (the kernels' code is on the device before memory is counted)
                torch.cuda.synchronize()
                free0 = torch.cuda.mem_get_info()[0]
                rc, status, _ = tracking_call(eng, [(ptr[0], T)], [(ptr[1], S)], [39], 39, beam[form], 4, 16, 0, [ptr[2]], [ptr[3]], [ptr[4]], [ptr[5]],
                                               mem, None)
                assert rc == 0 and torch.cuda.mem_get_info()[0] == free0, (T, S, form, mem)
                got = [x.cpu().numpy() for x in keep[2:]] if mem == _lib.KA_MEM_DEVICE else outs
                assert all(np.array_equal(g.view(np.int32), w.view(np.int32)) for g, w in zip(got, want))
            finally:
                eng.close()
