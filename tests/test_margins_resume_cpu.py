"""tests/margin_resume_ref.py and tests/margin_resume_cases.py on their own, without a GPU: the reference agrees with
tests/margin_ref.py where the two overlap, a lattice cut into chunks that exchange their rows gives the uncut answer bit for
bit (the header's property 2) on every case, its state rows reproduce through / alt / runner_up (property 3), and every planted
fault changes the answer on the cases that claim to catch it.  tests/test_margins_resume_gpu.py runs the same cases through
the kernels."""
import numpy as np
import pytest

import margin_cases as C
import margin_ref as R
import margin_resume_cases as MC
import margin_resume_ref as RR


@pytest.mark.parametrize("name", ["T33", "units", "stairs", "mm4_zeros", "gen_mm5", "ninf", "outside", "step16"])
def test_without_rows_the_reference_is_margin_refs(name):
    c = C.case(name)
    for unit in (0, 1):
        got = RR.resume_ref(c["lp"], c["labels"], c["beam"], c["mm"], c["band_lo"], c["path"], unit=unit)
        assert C.same(got, C.want(name, unit)), (name, unit)


@pytest.mark.parametrize("name", MC.NAMES)
def test_a_cut_lattice_gives_the_uncut_answer(name):
    c, u = MC.case(name), MC.uncut(name)
    assert c["cuts"] and all(len(cut) >= 1 for cut in c["cuts"])
    for cut in c["cuts"]:
        s = MC.split(name, cut)
        assert RR.same(s, u, MC.CUT_KEYS), (name, cut)          # (same() compares the status and the last chunk's score too)
        if u["status"] == RR.OK and c["end"] is None:
            assert all(z == u["score"] for z in s["scores"])    # eighths: every chunk's score is the uncut score exactly


def test_the_cases_cover_what_they_are_named_for():
    T = lambda n: MC.case(n)["lp"].shape[0]
    assert {T(n) for n in ("T2", "T3", "T33", "T65", "T70")} == {2, 3, 33, 65, 70}
    cuts = {k for n in ("T33", "T65", "T70") for cut in MC.case(n)["cuts"] for k in cut}
    assert {1, 31, 32, 33, 64, 69} <= cuts and any(len(cut) == 2 for cut in MC.case("T65")["cuts"])
    assert (32, 33) in MC.case("T70")["cuts"] and np.isneginf(MC.case("T70")["lp"]).any()
    for n, step in (("step0", 0), ("step1", 1), ("step16", 16), ("step70", 70), ("step504", 504)):
        c = MC.case(n)
        (k,), = c["cuts"]
        assert c["band_lo"][k] - c["band_lo"][k - 1] == step, n
    assert MC.uncut("gap")["status"] == RR.ZERO_MASS and all(MC.uncut(n)["status"] == RR.OK for n in MC.NAMES if n != "gap")
    w = MC.case("wrap")
    (k,), = w["cuts"]
    assert 2 * len(w["labels"]) + 1 == 1201 and w["band_lo"][k] < 1024 < w["band_lo"][k] + w["beam"]
    assert [MC.fast_form(MC.case(n)) for n in ("gen_V65", "gen_mm5", "gen_band1010", "T65")] == [False, False, False, True]
    assert [MC.case(n)["mm"] for n in ("mm1", "mm2", "mm3", "mm4_zeros")] == [1, 2, 3, 4]
    assert MC.case("beam1")["beam"] == 1 and len(MC.case("S0")["labels"]) == 0
    assert np.all(MC.case("free_end")["e_in"] == 0) and np.isneginf(MC.case("holes_end")["e_in"]).any()
    # a row with a tail: a band cut short by the lattice's end
    u = MC.uncut("gen_band1010")
    g = MC.case("gen_band1010")
    assert u["rows_lo"][-1] + g["beam"] > 2 * len(g["labels"]) + 1 and np.isneginf(u["rows"][-1, -1]) and np.isfinite(u["rows"][-1]).any()


@pytest.mark.parametrize("name", MC.NAMES)
def test_a_state_row_reproduces_its_frames_through_alt_and_runner_up(name):
    c, u = MC.case(name), MC.uncut(name)
    if u["status"] != RR.OK:
        return
    for k, f in enumerate(c["frames"]):
        lo, pt = int(u["rows_lo"][k]), int(c["path"][f])
        row = u["rows"][k]
        w = min(lo + c["beam"], 2 * len(c["labels"]) + 1) - lo
        assert np.all(np.isneginf(row[w:]))
        th = row[pt - lo] if lo <= pt < lo + w else -np.inf
        assert R.bits([th])[0] == R.bits([u["through"][f]])[0], (name, f)
        alt, runner = RR.row_alt(row[:w], lo, pt, c["unit"])
        assert R.bits([alt])[0] == R.bits([u["alt"][f]])[0] and runner == u["runner_up"][f], (name, f)
        if c["end"] is None:       # values are absolute: no cell beats the score, and the path's own cells attain it on a best path
            assert np.all(row <= u["score"])


def _noticed(name, fault):
    c, u = MC.case(name), MC.uncut(name)
    kw = {fault: True}
    return not RR.same(MC.uncut(name, **kw), u) or any(not RR.same(MC.split(name, cut, **kw), u, MC.CUT_KEYS) for cut in c["cuts"])


@pytest.mark.parametrize("name", MC.NAMES)
def test_every_fault_a_case_claims_changes_its_answer(name):
    for fault in MC.case(name)["catches"]:
        assert fault in RR.FAULTS and _noticed(name, fault), (name, fault)


def test_every_fault_is_claimed_by_a_case():
    claimed = {f for n in MC.NAMES for f in MC.case(n)["catches"]}
    assert claimed == set(RR.FAULTS)


def test_failures_of_the_reference():
    c = MC.case("T33")
    L = 2 * len(c["labels"]) + 1
    args = (c["lp"], c["labels"], c["beam"], c["mm"], c["band_lo"], c["path"])
    bad = np.zeros(L)
    bad[L - 1] = np.nan             # (a cell no frame reads)
    for kw in (dict(d_in=bad), dict(e_in=bad), dict(terminal=L), dict(e_in=np.where(np.arange(L) == 0, np.inf, 0.0))):
        r = RR.resume_ref(*args, frames=[3], **kw)
        assert r["status"] == RR.BAD_ARGS and np.isnan(r["rows"]).all() and np.all(r["rows_lo"] == -1) and np.isnan(r["d_out"]).all()
    r = RR.resume_ref(*args, d_in=np.full(L, -np.inf))
    assert r["status"] == RR.ZERO_MASS and r["score"] == -np.inf


# ---- what StreamingAligner(confidence="margin") relies on: a determined frame's free-end margin is never negative ----
# Every live cell's line runs through the committed state of a determined frame, so the best complete path to any live cell
# passes there: m at the committed state is the maximum over all live cells, which no other state's m can exceed.
def _prefix_margins(lp, lab, table, beam, mm):
    import resume_ref as BR
    path = BR.best_path_resume(lp, lab, table, None, BR.END_HIGHEST, beam, mm)[0]
    r = RR.resume_ref(lp, lab, beam, mm, table, path, None, np.zeros(2 * len(lab) + 1))
    assert r["status"] == RR.OK
    return R.margin_of(r["through"], r["alt"])


def test_a_determined_frames_free_end_margin_is_not_negative():
    import determined_ref as DR
    import track_cases as TC
    T, S, beam, mm, period = 128, 20, 16, 4, 8
    lp, lab = TC.planted(91, T, S, np.minimum(np.arange(T) // 3, 2 * S))
    assert not np.isinf(lp).any() and np.all(lp * 8 == np.round(lp * 8))
    seen = 0
    for n in range(32, T + 1, 32):          # the self-steering band, as the aligner walks it
        table = DR.tracking_table(lp[:n], lab, 0, None, beam, mm, period)
        det = int(DR.tracking_determined(lp[:n], lab, 0, None, beam, mm, period))
        margin = _prefix_margins(lp[:n], lab, table, beam, mm)
        assert np.all(margin[:max(det, 0)] >= 0), n
        seen += max(det, 0)
    assert seen > 0
    for name in ("T65", "mm3", "stairs"):    # a caller's table
        c = MC.case(name)
        if np.isinf(c["lp"]).any():
            continue
        det = int(DR.determined(c["lp"], c["labels"], c["band_lo"], None, c["beam"], c["mm"]))
        margin = _prefix_margins(c["lp"], c["labels"], c["band_lo"], c["beam"], c["mm"])
        assert det > 0 and np.all(margin[:det] >= 0), name
