"""The resumable tracking best path on the CPU: tests/track_resume_ref.py against tests/track_ref.py and tests/resume_ref.py, the
properties the kernels are tested for, and that the inputs of tests/track_resume_cases.py do what their
names say.  No GPU."""
import numpy as np
import pytest

import resume_ref as RR
import track_cases as TC
import track_resume_cases as K
import track_resume_ref as R

RUN = K.ref_run()


def _bits(a, b):
    return R.same_bits(np.atleast_1d(a), np.atleast_1d(b))


@pytest.mark.parametrize("name", TC.NAMES)
def test_null_start_is_track_ref(name):
    """property 1 on the reference: NULL row, first_lo 0 -> track_ref's bits"""
    want = TC.want(name)
    got, = K.want(f"uncut:{name}")
    if want is None:
        assert got[0] == "empty"
        return
    assert got[0] == "ok"
    for g, w in zip(got[1:6], want[:5]):
        assert _bits(g, w)
    assert got[6] == 0   # entry of a NULL row
    T, P = want[0].shape[0], TC.case(name)[4]
    if T % P:
        assert got[8] == want[3][-1]


@pytest.mark.parametrize("name", TC.NAMES)
def test_cut_and_resume_every_multiple(name):
    """property 2 at every multiple of the period"""
    lp, lab, beam, mm, P, end_rule = TC.case(name)
    uncut, = K.want(f"uncut:{name}")
    for k in K.cuts_of(name, every=True):
        key = f"cut:{name}:{k}"
        out = K.want(key) if key in K.SCENARIOS else K.cut_scenario(name, k)(RUN)
        if uncut[0] != "ok":
            assert K.joined(out) is None
            continue
        assert out[0][0] == "ok" and out[0][8] == uncut[4][k], (name, k)   # A's next_lo is the uncut lo_k
        j = K.joined(out)
        assert j is not None, (name, k)
        for g, w in zip(j[:4], uncut[1:5]):
            assert _bits(g, w), (name, k)
        assert _bits(j[4], uncut[5]) and _bits(j[5], uncut[7]) and j[6] == uncut[8], (name, k)


def test_resume_over_the_returned_table():
    """property 3: resume_ref over a call's table, with the same row and end, gives the call's answer"""
    seen = [0]

    def run(lp, lab, first_lo, init, end, beam, mm, period):
        got = RUN(lp, lab, first_lo, init, end, beam, mm, period)
        if got[0] == "bad_args":
            with pytest.raises(RR.BadArgs):
                RR.best_path_resume(lp, lab, np.zeros(lp.shape[0], np.int64), init, end, beam, mm)
            return got
        table = got[4] if got[0] == "ok" else got[2]
        try:
            want = RR.best_path_resume(lp, lab, table, init, end, beam, mm)
            assert got[0] == "ok"
            for g, w in zip(got[1:4] + got[5:8], want):
                assert _bits(g, w) if np.ndim(g) or isinstance(g, np.floating) else g == w
        except RR.EmptyBeam as e:
            assert got[0] == "empty" and _bits(got[1], e.final)
        seen[0] += 1
        return got
    for name, sc in K.SCENARIOS.items():
        if not name.startswith("cut:wrap") and not name.startswith("uncut:wrap"):
            sc(run)
    assert seen[0] > 500


@pytest.mark.parametrize("d", (1, 2, 3))
def test_depth_cuts(d):
    assert K.depth_of(K.want(f"depth{d}"))[0] == d
    depth, first_lo = K.depth_of(K.want(f"edge{d}"))
    assert depth == d and first_lo == 16
    assert K.joined(K.want(f"edge{d}")) is not None


def test_wrap_cut_has_first_lo_on_the_wrapped_ring():
    k = K.cuts_of("wrap")[-1]
    out = K.want(f"cut:wrap:{k}")
    assert out[0][8] >= 1024 and K.joined(out) is not None


@pytest.mark.parametrize("name", ("step0", "step1", "step16", "step70"))
def test_step_cases_cut_at_their_retarget(name):
    step, at = TC.STEP_OF[name]
    out = K.want(f"cut:{name}:{at}")
    assert out[0][8] - out[0][4][-1] == step   # the retarget that falls on the cut moves lo by the step
    assert out[1][4][0] == out[0][8]


def test_singles_do_what_their_names_say():
    w = {k: K.want(f"single:{k}") for k in K.single_scenarios()}
    assert w["null_row_lo3"][0][0] == "ok" and w["null_row_lo3"][0][6] == 0
    for k in ("null_row_lo4", "null_row_lo1030", "null_row_lo4_generic", "row_above_hi", "row_below_reach"):
        assert w[k][0][0] == "empty" and np.all(np.isnan(w[k][0][1])), k
    assert w["null_row_lo4"][0][3] == 4 and np.all(w["null_row_lo4"][0][2] == 4)   # no live cell keeps the low end
    assert w["row_lowest_reach"][0][0] == "ok" and w["row_lowest_reach"][0][6] == 9
    assert [a[0] for a in w["first_lo_top"]] == ["ok"] * 3
    for k in ("ninf_cells", "ninf_cells_generic"):
        assert [a[0] for a in w[k]] == ["ok", "ok"]
    assert w["pinf"][0] == ("bad_args",) and w["pinf_outside"][0] == ("bad_args",) and w["pinf_generic"][0] == ("bad_args",)
    assert [a[0] for a in w["end_live"]] == ["ok"] * 3
    for k in ("end_dead_in_band", "end_dead_generic", "end_outside_band", "end_dead_T8"):
        a, = w[k]
        assert a[0] == "empty" and not np.all(np.isnan(a[1])) and a[3] >= 0, k   # the forward pass's outputs are there
    for T in (4, 8):
        assert [a[0] for a in K.want(f"short:T{T}")] == ["ok", "ok"]
    assert K.joined(K.want("short:T8:4")) is not None


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_planted_fault_changes_a_scenario(fault):
    run = K.ref_run(fault)
    for name, sc in K.SCENARIOS.items():
        if name.split(":")[1 if ":" in name else 0] in ("wrap", "step504", "gen_band1010"):
            continue   # (the long ones: the short ones catch every fault)
        if not K.same_answers(sc(run), K.want(name)):
            return
    pytest.fail(f"no scenario sees the fault {fault}")


def test_off_phase_cuts_steer_another_band():
    """why ctc_best_path_tracking_chunked wants chunks that are multiples of the period"""
    differ = tried = 0
    for name in TC.NAMES:
        lp, lab, beam, mm, P, end_rule = TC.case(name)
        T = lp.shape[0]
        uncut, = K.want(f"uncut:{name}")
        if T > 64 or uncut[0] != "ok":
            continue
        for k in range(1, T):
            if k % P == 0:
                continue
            out = K.chain(RUN, lp, lab, k, 0, None, K.END_OF[end_rule], beam, mm, P)
            tried += 1
            if len(out) < 2 or out[1][0] != "ok" or not _bits(np.concatenate([out[0][4], out[1][4]]), uncut[4]):
                differ += 1
    assert tried > 300 and differ > tried // 2
