"""The best path over a caller-given band on the GPU (ka_ctc_best_path_banded[_batch]_f32).  Every
comparison is exact - path, labels, the bits of the scores and of the total, the status - and there is no tolerance anywhere:
  * with the reference's own band as the table the call returns what ctc_best_path returns on the same engine, in both kernel
    forms and both memory modes;
  * with other tables (tests/band_cases.py; tests/test_banded_cpu.py asserts that they do what their names say) it returns what
    tests/band_ref.py returns;
  * an invalid table is a status of its lattice alone; batches answer every lattice as if it were alone.
"""
import ctypes
import os

import numpy as np
import pytest

import band_cases as C
import band_ref as R
import golden_util as G
from oracle import oracle as O

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
    assert hasattr(_lib.load_library(), "ka_ctc_best_path_banded_batch_f32")
    return ka, _lib.default_engine(torch.cuda.current_device())


def run(ka, mode, lps, labs, bands, beam, mm):
    """(results as NumPy arrays, statuses, totals) of one banded call in the given memory mode; host rows lie at a stride ld > V"""
    if mode == "host":
        wide = []
        for lp in lps:
            buf = np.full((lp.shape[0], lp.shape[1] + 3), np.nan, np.float32)   # (a NaN read from the padding would be a status)
            buf[:, :lp.shape[1]] = lp
            wide.append(buf[:, :lp.shape[1]])
        return ka.ctc_best_path_banded_batch(wide, labs, bands, beam, mm, return_status=True)
    import torch
    dlp = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in lps]
    res, status, total = ka.ctc_best_path_banded_device(dlp, labs, bands, beam, mm, return_status=True)
    return [tuple(a.cpu().numpy() for a in r) for r in res], status, total


def differs(got, total, want):
    """None when (path, labels, scores) and the total are `want`'s in every bit, else what differs first"""
    for g, w, field in zip(got, want[:3], ("path", "labels", "scores")):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape:
            return f"{field} has shape {g.shape}"
        bad = np.nonzero(g.view(np.int32) != w.view(np.int32))[0]
        if bad.size:
            return f"{field} differs at {bad.size} frames, first at frame {int(bad[0])}: got {g[bad[0]]}, want {w[bad[0]]}"
    if np.float32(total).view(np.int32) != np.float32(want[3]).view(np.int32):
        return f"total {total!r}, want {want[3]!r}"
    return None


def assert_diagonal_identity(ka, lps, labs, beam, mm, what):
    """the banded call with diagonal_band == ctc_best_path on the same engine, lattice by lattice, in both memory modes"""
    ref, ref_status, ref_total = ka.ctc_best_path_batch(lps, labs, beam, mm, return_status=True)
    bands = [ka.diagonal_band(lp.shape[0], 2 * len(lab) + 1, beam) for lp, lab in zip(lps, labs)]
    for mode in MODES:
        res, status, total = run(ka, mode, lps, labs, bands, beam, mm)
        assert list(status) == list(ref_status), (what, mode, status, ref_status)
        for i in range(len(lps)):
            if ref_status[i] == 0:
                why = differs(res[i], total[i], ref[i] + (ref_total[i],))
                assert why is None, f"{what} [{mode}] lattice {i}: {why}"


# ---- diagonal identity ----
def test_diagonal_identity_g1(env):
    ka, _ = env
    n_err = 0
    for c in G.g1_cases():
        assert_diagonal_identity(ka, [c["lp"]], [c["labels"]], c["beam"], c["max_move"], f"g1 case {c['idx']}")
        n_err += c["status"] != 0
    assert n_err >= 1   # (the goldens hold empty beams: their status is compared too)


def test_diagonal_identity_g2(env):
    ka, _ = env
    for c in G.g2_cases():
        lp, lab = O.hash_logprobs(c["T"], c["V"], c["seed"]), O.hash_labels(c["S"], c["V"], c["seed"])
        assert_diagonal_identity(ka, [lp], [lab], c["beam"], c["max_move"], f"g2 case {c['idx']}")
        (path, _, _), = ka.ctc_best_path_banded_batch([lp], [lab], [ka.diagonal_band(c["T"], 2 * c["S"] + 1, c["beam"])], c["beam"], c["max_move"])
        assert np.array_equal(path, c["path"])


def test_diagonal_identity_batch_of_64(env):
    ka, _ = env
    rng = np.random.default_rng(64)
    shapes = [(int(rng.integers(300, 521)), int(rng.integers(40, 701))) for _ in range(64)]
    shapes[0], shapes[1] = (520, 700), (300, 40)
    lps = [O.hash_logprobs(T, 39, 6400 + i) for i, (T, S) in enumerate(shapes)]
    labs = [O.hash_labels(S, 39, 6400 + i) for i, (T, S) in enumerate(shapes)]
    assert_diagonal_identity(ka, lps, labs, 1000, 4, "batch of 64")


@pytest.mark.parametrize("T,S,V,beam,mm", [(100, 60, 80, 24, 4), (450, 600, 39, 1100, 4), (100, 60, 39, 24, 6)])
def test_diagonal_identity_generic_form(env, T, S, V, beam, mm):
    ka, _ = env
    rng = np.random.default_rng(T + V + mm)
    lp = (np.round(rng.standard_normal((T, V)) * 16) / 8).astype(np.float32)
    lab = rng.integers(0, V, size=S).astype(np.int32)
    assert_diagonal_identity(ka, [lp], [lab], beam, mm, f"generic T={T} S={S} V={V} beam={beam} max_move={mm}")


# ---- tables against band_ref ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", C.NAMES)
def test_table_against_band_ref(env, name, mode):
    ka, _ = env
    lp, lab, lo, beam, mm = C.case(name)
    want = C.want(name)
    res, status, total = run(ka, mode, [lp], [lab], [lo], beam, mm)
    if want is None:
        assert list(status) == [-1], (name, status)
        with pytest.raises(ValueError):
            ka.ctc_best_path_banded(lp, lab, lo, beam, mm)
        return
    assert list(status) == [0], (name, status)
    why = differs(res[0], total[0], want)
    assert why is None, f"{name} [{mode}]: {why}"


@pytest.mark.parametrize("name", ["const0", "ninf", "ring_wrap", "step64", "step500"])
def test_table_against_band_ref_generic_form(env, name):
    """the same tables through the generic kernels: 72 more columns (that no label names) make V = 80"""
    ka, _ = env
    lp, lab, lo, beam, mm = C.case(name)
    wide = np.concatenate([lp, np.full((lp.shape[0], 72), -1.0, np.float32)], axis=1)
    want = C.want(name)
    for mode in MODES:
        res, status, total = run(ka, mode, [wide], [lab], [lo], beam, mm)
        if want is None:
            assert list(status) == [-1]
            continue
        assert list(status) == [0]
        why = differs(res[0], total[0], want)
        assert why is None, f"{name} generic [{mode}]: {why}"


def test_numpy_and_tensor_front_ends(env):
    import torch
    ka, _ = env
    lp, lab, lo, beam, mm = C.case("shifted")
    want = C.want("shifted")
    got = ka.ctc_best_path_banded(lp, lab, lo, beam, mm)
    assert all(isinstance(a, np.ndarray) for a in got) and differs(got, want[3], want) is None
    tgot = ka.ctc_best_path_banded(torch.from_numpy(lp).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(lo).cuda(), beam, mm)
    assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in tgot)
    assert differs([a.cpu().numpy() for a in tgot], want[3], want) is None
    with pytest.raises(ValueError):
        ka.ctc_best_path_banded(lp, lab, lo[:-1], beam, mm)
    with pytest.raises(ValueError):
        ka.ctc_best_path_banded(lp[0], lab, lo, beam, mm)


# ---- invalid tables ----
def bad_tables(lo, L):
    k = len(lo) // 2
    dec = lo.copy()
    dec[k] = dec[k + 1] + 1          # one step down behind frame k, every entry in range
    assert dec[k] < L and dec[k] >= dec[k - 1]
    neg = lo.copy()
    neg[0] = -1
    top = lo.copy()
    top[-1] = L
    return {"decreasing": dec, "negative": neg, "entry = L": top}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", ["wave", "generic"])
def test_invalid_table_is_a_status_of_its_lattice(env, mode, form):
    ka, eng = env
    from kokoro_align_amd import _lib
    from bestpath_harness import banded_call
    lp, lab, lo, beam, mm = C.case("shifted")
    lp2, lab2, lo2, _, _ = C.case("const0")
    if form == "generic":
        lp, lp2 = (np.concatenate([x, np.full((x.shape[0], 72), -1.0, np.float32)], axis=1) for x in (lp, lp2))
    L = 2 * len(lab) + 1
    (alone, alone2), st, tot = run(ka, mode, [lp, lp2], [lab, lab2], [lo, lo2], beam, mm)
    assert list(st) == [0, 0]
    for what, bad in bad_tables(lo, L).items():
        res, status, total = run(ka, mode, [lp], [lab], [bad], beam, mm)
        assert list(status) == [_lib.KA_ERR_BAD_ARGS], (what, status)
        with pytest.raises(ValueError):
            ka.ctc_best_path_banded(lp, lab, bad, beam, mm)
        # inside a batch: the neighbours keep the bits they have alone
        res, status, total = run(ka, mode, [lp, lp, lp2], [lab, lab, lab2], [lo, bad, lo2], beam, mm)
        assert list(status) == [0, _lib.KA_ERR_BAD_ARGS, 0], (what, status)
        assert differs(res[0], total[0], alone + (tot[0],)) is None and differs(res[2], total[2], alone2 + (tot[1],)) is None, what
    # the call returns the status of the FIRST lattice that failed; a failed lattice's outputs are not written
    empty_lo = C.flat_with_step(lp.shape[0], 5, 100)
    for order, first in (([empty_lo, bad_tables(lo, L)["negative"]], _lib.KA_ERR_EMPTY_BEAM), ([bad_tables(lo, L)["negative"], empty_lo], _lib.KA_ERR_BAD_ARGS)):
        T = lp.shape[0]
        lpc = np.ascontiguousarray(lp)
        bands = [np.ascontiguousarray(b, np.int32) for b in order]
        outs = [[np.full(T, SENTINEL, dt) for _ in range(2)] for dt in (np.int32, np.int32, np.float32)]
        rc, status, _ = banded_call(eng, [(lpc.ctypes.data, T)] * 2, [(lab.ctypes.data, len(lab))] * 2, [b.ctypes.data for b in bands],
                                       [lpc.shape[1]] * 2, lpc.shape[1], beam, mm, *[[a.ctypes.data for a in o] for o in outs], _lib.KA_MEM_HOST, None)
        assert rc == first and sorted(status.tolist()) == [_lib.KA_ERR_BAD_ARGS, _lib.KA_ERR_EMPTY_BEAM]
        assert all(np.all(a == SENTINEL) for o in outs for a in o)


# ---- batches ----
N_WAVE, N_GENERIC, BATCH_BEAM = 1072, 300, 1100
_batch = {}


def the_batch(ka):
    """1072 one-wavefront and 300 generic small lattices (one call: one beam, 1100, so L <= 1009 picks the form) with random
    tables, every seventh failing (empty beam or bad table in turn), and what each returns when it is sent alone."""
    if _batch:
        return _batch
    rng = np.random.default_rng(1372)
    kinds = ["wave"] * N_WAVE + ["generic"] * N_GENERIC
    rng.shuffle(kinds)
    lps, labs, bands = [], [], []
    for i, kind in enumerate(kinds):
        T = int(rng.integers(1, 41)) if kind == "wave" else int(rng.integers(2, 13))
        S = int(rng.integers(0, 41)) if kind == "wave" else int(rng.integers(505, 516))
        lp, lab = C.random_lattice(5000 + i, T, S, ninf=(i % 5 == 0))
        L = 2 * S + 1
        lo = np.minimum(np.cumsum(rng.integers(0, 3, T)) - 1, L - 1).clip(0).astype(np.int64)
        if i % 7 == 3 and T >= 2:
            if (i // 7) % 2 == 0 and L > 8:
                lo[1:] = L - 1            # nothing reaches it: empty beam
            else:
                lo[T // 2] = -1 if (i // 7) % 4 == 1 else L   # bad table
        lps.append(lp)
        labs.append(lab)
        bands.append(lo)
    alone = [ka.ctc_best_path_banded_batch([lp], [lab], [lo], BATCH_BEAM, 4, return_status=True) for lp, lab, lo in zip(lps, labs, bands)]
    _batch.update(lps=lps, labs=labs, bands=bands, alone=alone, kinds=kinds)
    return _batch


@pytest.mark.parametrize("mode", MODES)
def test_batch_lattices_get_the_bits_they_have_alone(env, mode):
    import torch
    ka, _ = env
    b = the_batch(ka)
    lps, labs, bands, alone = b["lps"], b["labs"], b["bands"], b["alone"]
    n = len(lps)
    statuses = [a[1][0] for a in alone]
    assert statuses.count(-1) >= 50 and statuses.count(-2) >= 50 and statuses.count(0) >= 1100
    # outputs: views into one array per output, a sentinel element between neighbours
    offs = np.concatenate([[1], 1 + np.cumsum([lp.shape[0] + 1 for lp in lps])])
    if mode == "host":
        big = [np.full(offs[-1], SENTINEL, dt) for dt in (np.int32, np.int32, np.float32)]
        views = [[a[offs[i]:offs[i] + lps[i].shape[0]] for i in range(n)] for a in big]
        res, status, total = ka.ctc_best_path_banded_batch(lps, labs, bands, BATCH_BEAM, 4, return_status=True, outputs=views)
        out = big
    else:
        big = [torch.full((int(offs[-1]),), SENTINEL, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.float32)]
        views = [[a[int(offs[i]):int(offs[i]) + lps[i].shape[0]] for i in range(n)] for a in big]
        dlp = [torch.from_numpy(x).cuda() for x in lps]
        res, status, total = ka.ctc_best_path_banded_device(dlp, labs, bands, BATCH_BEAM, 4, return_status=True, outputs=views)
        out = [a.cpu().numpy() for a in big]
    assert list(status) == statuses
    for i in range(n):
        sl = slice(offs[i], offs[i] + lps[i].shape[0])
        if statuses[i] == 0:
            why = differs([a[sl] for a in out], total[i], alone[i][0][0] + (alone[i][2][0],))
            assert why is None, f"lattice {i} ({b['kinds'][i]}) [{mode}]: {why}"
        else:
            assert all(np.all(a[sl] == SENTINEL) for a in out), i
    guards = np.concatenate([[0], offs[1:] - 1])
    assert all(np.all(a[guards] == SENTINEL) for a in out)


# ---- workspace ----
def test_workspace_bytes_cover_the_call(env):
    import torch
    ka, _ = env
    from kokoro_align_amd import _lib
    from bestpath_harness import banded_call
    shapes = [(300, 200, "wave"), (401, 500, "wave"), (400, 520, "generic")]
    beam = {"wave": 1000, "generic": 1100}
    for mem in (_lib.KA_MEM_HOST, _lib.KA_MEM_DEVICE):
        for T, S, form in shapes:
            Ts, Ss = (ctypes.c_int64 * 1)(T), (ctypes.c_int64 * 1)(S)
            lib = _lib.load_library()
            need = lib.ka_banded_workspace_bytes(1, Ts, Ss, 39, beam[form], 4, mem)
            W = min(beam[form], 2 * S + 1)
            assert need >= (T * 256 if form == "wave" else T * W) + (T * 39 * 4 if mem == _lib.KA_MEM_HOST else 0)
            assert lib.ka_banded_workspace_bytes(1, Ts, Ss, 39, beam[form], 300, mem) == 0 and lib.ka_banded_workspace_bytes(1, Ts, Ss, 39, beam[form], 4, 7) == 0
            eng = _lib.Engine(torch.cuda.current_device())
            try:
                eng.reserve(need)
                lp, lab = O.hash_logprobs(T, 39, T + S), O.hash_labels(S, 39, T + S)
                lo = np.ascontiguousarray(ka.diagonal_band(T, 2 * S + 1, beam[form]), np.int32)
                outs = [np.empty(T, np.int32), np.empty(T, np.int32), np.empty(T, np.float32)]
                if mem == _lib.KA_MEM_DEVICE:
                    keep = [torch.from_numpy(x).cuda() for x in (lp, lab, lo)] + [torch.from_numpy(x).cuda() for x in outs]
                    ptr = [x.data_ptr() for x in keep]
                else:
                    ptr = [x.ctypes.data for x in (lp, lab, lo)] + [x.ctypes.data for x in outs]
                want = ka.ctc_best_path_batch([lp], [lab], beam[form], 4)[0]
                ka.ctc_best_path_banded_batch([lp], [lab], [lo], beam[form], 4)   # (the kernels' code is on the device before memory is counted)
                torch.cuda.synchronize()
                free0 = torch.cuda.mem_get_info()[0]
                rc, status, _ = banded_call(eng, [(ptr[0], T)], [(ptr[1], S)], [ptr[2]], [39], 39, beam[form], 4, [ptr[3]], [ptr[4]], [ptr[5]], mem,
                                               None)
                assert rc == 0 and torch.cuda.mem_get_info()[0] == free0, (T, S, form, mem)
                got = [x.cpu().numpy() for x in keep[3:]] if mem == _lib.KA_MEM_DEVICE else outs
                assert all(np.array_equal(g.view(np.int32), w.view(np.int32)) for g, w in zip(got, want))
            finally:
                eng.close()


# ---- the rescue case ----
@pytest.mark.parametrize("seed", range(6))
def test_rescue_case(env, seed):
    ka, _ = env
    lp, labels, L, beam, pre = C.rescue(seed)
    T = lp.shape[0]
    (full,), st, full_total = ka.ctc_best_path_batch([lp], [labels], 2 * L, 4, return_status=True)
    assert list(st) == [0]
    band = ka.anchored_band(T, L, [(pre, 0)], beam)
    (got,), st, total = ka.ctc_best_path_banded_batch([lp], [labels], [band], beam, 4, return_status=True)
    assert list(st) == [0]
    why = differs(got, total[0], full + (full_total[0],))
    assert why is None, why
    diag_lo = ka.diagonal_band(T, L, beam)
    (diag,), st, _ = ka.ctc_best_path_banded_batch([lp], [labels], [diag_lo], beam, 4, return_status=True)
    assert list(st) == [0] and int(np.sum(diag[0] != full[0])) > 100 and ka.band_edge_contact(diag[0], diag_lo, beam, L).size > 0
    assert ka.band_edge_contact(got[0], band, beam, L).size == 0
