"""The resumable best path without a GPU: that tests/resume_ref.py, the reference of
tests/test_resume_gpu.py, is band_ref with a free start, end and last row; that cutting a lattice and resuming gives the uncut
answer in every bit; that the crafted cases of tests/resume_cases.py do what their names say; and that every planted fault of
the reference is caught by a scenario the GPU tests run.  The Python names are checked as far as they go without the library.
"""
import numpy as np
import pytest

import band_cases as C
import band_ref as R
import resume_cases as X
import resume_ref as RR

import kokoro_align_amd as ka
from kokoro_align_amd import _lib


def bits(x):
    return np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32)


# ---- the Python surface ----
def test_python_names_and_symbols():
    for name in ("ctc_best_path_resume", "ctc_best_path_resume_batch", "ctc_best_path_resume_device", "ctc_best_path_chunked", "free_start_scores"):
        assert callable(getattr(ka, name))
    for sym in ("ka_ctc_best_path_resume_f32", "ka_ctc_best_path_resume_batch_f32", "ka_resume_workspace_bytes"):
        assert sym in _lib.EXPORTS


def test_free_start_scores():
    row = ka.free_start_scores(9, 2, 5)
    assert row.dtype == np.float32 and row.shape == (9,)
    assert np.array_equal(np.isnan(row), [True, True, False, False, False, True, True, True, True]) and np.all(row[2:5] == 0.0)
    assert np.all(ka.free_start_scores(4) == 0.0)
    assert np.array_equal(bits(ka.free_start_scores(3, 1, 1)), bits(np.full(3, RR.DEAD)))   # (the NaN of the last rows)
    assert bits(RR.DEAD)[0] == 0x7fc00000


# ---- property 1: a NULL start, the reference's end ----
@pytest.mark.parametrize("name", C.NAMES)
def test_null_start_is_band_ref(name):
    lp, lab, lo, beam, mm = C.case(name)
    want = C.want(name)
    L = 2 * len(lab) + 1
    row0 = X.free_row(L, 0, 1)
    for init in (None, row0):
        if want is None:
            with pytest.raises(RR.EmptyBeam) as e:
                RR.best_path_resume(lp, lab, lo, init, RR.END_HIGHEST, beam, mm)
            assert np.all(bits(e.value.final) == 0x7fc00000)
            continue
        got = RR.best_path_resume(lp, lab, lo, init, RR.END_HIGHEST, beam, mm)
        assert all(RR.same_bits(g, w) for g, w in zip(got[:3], want[:3])) and bits(got[3])[0] == bits(want[3])[0]
        assert got[4] == 0
        # the last row: the live cells of band_ref's last frame, dead elsewhere
        pos, sc = R.best_path_banded(lp, lab, lo, beam, mm, return_cells=True)[-1][-1]
        row = np.full(L, RR.DEAD, np.float32)
        row[pos] = sc
        assert RR.same_bits(got[5], row)


# ---- property 2: cut and resume, every cut for T <= 130, every 7th frame above ----
@pytest.mark.parametrize("name", C.NAMES)
def test_cut_and_resume_is_the_uncut_answer(name):
    lp, lab, lo, beam, mm = C.case(name)
    want = C.want(name)
    T = lp.shape[0]
    run = X.ref_run()
    below = []
    for k in (range(1, T) if T <= 130 else range(7, T, 7)):
        out = X.chain(run, lp, lab, lo, k, None, beam, mm)
        got = X.joined(out)
        if want is None:
            assert got is None and out[-1][0] == "empty", (name, k)
            continue
        assert got is not None, (name, k)
        assert all(RR.same_bits(g, w) for g, w in zip(got[:3], want[:3])) and bits(got[3])[0] == bits(want[3])[0], (name, k)
        if out[1][5] < lo[k]:
            below.append(k)
    assert tuple(below) == X.BELOW_CUTS.get(name, ()), (name, below)


def test_the_gpu_cuts_cover_the_prefetch_depth_and_the_tail():
    for name in X.CUT_NAMES:
        T = C.case(name)[0].shape[0]
        assert set(X.cuts_of(name)) >= {k for k in (1, 2, 3, 4, 5, T - 3, T - 2, T - 1) if 1 <= k < T}
    assert sum(len(v) for v in X.BELOW_CUTS.values()) >= 60 and set(X.BELOW_CUTS) <= set(X.CUT_CASES)
    # live -inf cells in a start row: the ninf family's last rows carry them
    lp, lab, lo, beam, mm = C.case("ninf")
    n = 0
    for k in X.cuts_of("ninf"):
        a = RR.best_path_resume(lp[:k], lab, lo[:k], None, RR.END_HIGHEST, beam, mm)
        n += int(np.sum(np.isneginf(a[5])))
    assert n >= 10


# ---- the crafted cases ----
@pytest.mark.parametrize("key", X.EDGE_KEYS, ids=lambda k: "lo%d_d%d" % (k[0], k[2]))
def test_block_edge_cases(key):
    lo_new, S, d = key
    case = X.block_edge(*key)
    lp, lab, lo, init, beam, mm, true = case
    assert lp.shape == (24, 8) and beam == 32 and lo_new % 16 == 0 and lo[X.EDGE_CUT - 1] < lo_new == lo[X.EDGE_CUT]
    assert X.edge_entry_depth(case) == d                       # chunk B's entry lies d below its first low end ...
    out = X.edge_scenario(key)(X.ref_run())
    assert out[1][5] == lo_new - d and lo_new <= out[1][1][0] <= out[1][5] + 3   # ... and its path[0] inside the band
    # the cut answer is the uncut one
    whole = RR.best_path_resume(lp, lab, lo, init, RR.END_HIGHEST, beam, mm)
    got = X.joined(out)
    assert all(RR.same_bits(g, w) for g, w in zip(got[:3], whole[:3])) and bits(got[3])[0] == bits(whole[3])[0]
    assert out[2][5] == whole[4] and RR.same_bits(out[1][6], whole[5])
    if lo_new >= 1024:
        assert 2 * S + 1 > 1024 + beam                           # the wrapped ring


def test_excerpt_case():
    lp, lab, lo, beam, mm = X.excerpt()
    L = 2 * len(lab) + 1
    assert lp.shape == (40, 8) and L == 121 and beam == 2 * L
    free = RR.best_path_resume(lp, lab, lo, ka.free_start_scores(L), RR.END_BEST, beam, mm)
    assert free[4] == 50 and free[0][-1] == 89 and free[3] == np.float32(-5.0)
    fixed = RR.best_path_resume(lp, lab, lo, None, RR.END_BEST, beam, mm)
    assert fixed[4] == 0 and fixed[0][0] == 3 and fixed[3] == np.float32(-47.625)


def test_start_row_scenarios_do_what_their_names_say():
    out = {n: f(X.ref_run()) for n, f in X.start_row_scenarios().items()}
    for n in ("above_hi", "below_reach", "all_dead", "end_dead_in_band", "end_outside_band"):
        assert [o[0] for o in out[n]] == ["empty"], n
    for n in ("above_hi", "below_reach", "all_dead"):
        assert np.all(bits(out[n][0][1]) == 0x7fc00000)
    assert np.any(bits(out["end_dead_in_band"][0][1]) != 0x7fc00000)    # the forward pass ran: the row is written
    assert [o[0] for o in out["pinf"]] == ["bad_args"] and [o[0] for o in out["pinf_outside"]] == ["bad_args"]
    assert out["lowest_reach"][0][0] == "ok" and out["lowest_reach"][0][5] == 17 and out["lowest_reach"][0][1][0] == 20
    assert [o[0] for o in out["end_live"]] == ["ok"] * 3 and len({int(o[1][-1]) for o in out["end_live"]}) == 3
    assert [int(o[1][-1]) for o in out["flat_best"]] == [0, 2]


# ---- every planted fault is caught by a scenario of the GPU tests ----
def gpu_scenarios():
    sc = {("row", n): f for n, f in X.start_row_scenarios().items()}
    sc.update({("edge",) + k: X.edge_scenario(k) for k in X.EDGE_KEYS})
    sc.update({("cut", n, k): X.cut_scenario(n, k) for n in ("ride_lo", "ninf", "T5", "beam1", "mm2") for k in X.cuts_of(n)})
    return sc


def test_planted_faults_are_caught():
    sc = gpu_scenarios()
    good = {key: f(X.ref_run()) for key, f in sc.items()}
    assert all(X.same_answers(f(X.ref_run()), good[key]) for key, f in list(sc.items())[:8])
    caught = {}
    for fault in RR.FAULTS:
        run = X.ref_run(fault)
        caught[fault] = [key for key, f in sc.items() if not X.same_answers(f(run), good[key])]
        assert caught[fault], fault
    # the start-row cells below lo_0 are what the block-edge cuts are for
    assert any(key[0] == "edge" for key in caught["drop_below_lo"])
