"""Inputs of the resumed-margin tests (tests/test_margins_resume_cpu.py asserts on tests/margin_resume_ref.py that the cuts
compose and that every planted fault shows on the cases that claim it; tests/test_margins_resume_gpu.py runs them through the
kernels).

A case is a lattice of tests/margin_cases.py (log-probs in eighths: every sum exact, ties common, label value 0 arms the
veto) under a TABLE (the diagonal's own where the parent case has none: a chunk of a diagonal is no diagonal) with
    cuts      the ways it is cut: tuples of ascending frames in [1, T)
    end       None (the path's last state), "free" (an end row of zeros), "holes" (an end row in eighths with -inf holes)
    frames    the query frames of its state rows
    catches   the faults of margin_resume_ref.FAULTS the case is meant to notice
"""
import numpy as np

import margin_cases as C
import margin_ref as R
import margin_resume_ref as RR

# what any cut lattice with state rows notices; what an end row adds
CORE = ("e_out_no_emission", "d_out_unmasked", "rows_no_offset")
ROW_END = ("e_in_one_cell",)


def end_row(kind, L, seed=0):
    if kind is None:
        return None
    if kind == "free":
        return np.zeros(L, np.float64)
    rng = np.random.default_rng(seed)
    row = -rng.integers(0, 17, size=L) / 8.0
    row[rng.random(L) < 0.3] = -np.inf
    return row


def _from(name, cuts, end=None, frames=None, catches=CORE, unit=0, table=None):
    def make():
        c = C.case(name)
        T, L = c["lp"].shape[0], 2 * len(c["labels"]) + 1
        tab = c["band_lo"] if c["band_lo"] is not None else R.band_of(T, L, c["beam"])[0]
        if table is not None:
            tab = table(T, L, c["beam"])
        fr = frames
        if fr is None:       # around every cut, and both ends
            fr = sorted({0, T - 1} | {t for cut in cuts for k in cut for t in (k - 1, k) if 0 <= t < T})
        return dict(lp=c["lp"], labels=c["labels"], path=c["path"], beam=c["beam"], mm=c["mm"], band_lo=np.ascontiguousarray(tab, np.int32),
                    cuts=[tuple(k for k in cut if 0 < k < T) for cut in cuts], end=end, e_in=end_row(end, L, len(name)),
                    frames=np.asarray(fr, np.int64), unit=unit, catches=tuple(catches), parent=name)
    return make


def _step(name, catches):
    import track_cases as TC
    return _from(name, [(TC.STEP_OF[name][1],)], catches=catches)


CASES = {
    # the 32-frame block borders and one-frame chunks
    "T2": _from("T2", [(1,)], catches=("e_out_no_emission",)),
    "T3": _from("T3", [(1,), (2,), (1, 2)], catches=("e_out_no_emission", "d_out_unmasked")),
    "T33": _from("T33", [(1,), (31,), (32,)]),
    "T65": _from("T65", [(1,), (31,), (32,), (33,), (64,), (20, 45)]),
    "T70": _from("ninf", [(1,), (31,), (32,), (33,), (69,), (32, 33)]),          # (-inf log-probs; a middle chunk of one frame)
    # tables that step at the cut frame: d_in cells below lo_0 matter.  (Under the beam of 1009 of these lattices a step of 504
    # still leaves cells in reach; "gap" steps past the whole band and past the moves, which leaves none: zero mass)
    "step0": _step("step0", ("e_out_no_emission",)), "step1": _step("step1", ("e_out_no_emission", "rows_no_offset")),
    "step16": _step("step16", ("rows_no_offset", "cut_veto_dropped")), "step70": _step("step70", ("rows_no_offset", "cut_veto_dropped")),
    "step504": _step("step504", ("rows_no_offset",)),
    "gap": _from("T65", [(32,)], catches=(), table=lambda T, L, beam: np.where(np.arange(T) < 32, 0, beam + 3)),
    "stairs": _from("stairs", [(35,), (36,), (6, 12)], catches=("e_out_no_emission", "rows_no_offset", "band_on_d_in")),
    "wrap": _from("wrap", [(1120,)], frames=[0, 1100, 1119, 1120, 1140, 1299]),   # (the band crosses slot 1023 -> 0 at the cut)
    # forms and shapes
    "beam1": _from("beam1", [(10,)], catches=("d_out_unmasked",)), "S0": _from("S0", [(4,)], catches=()),
    "mm1": _from("mm1", [(10,)], catches=()), "mm2": _from("mm2", [(30,)]), "mm3": _from("mm3", [(30,)], catches=CORE + ("band_on_d_in",)),
    "mm4_zeros": _from("mm4_zeros", [(29,), (30,), (31,)], catches=CORE + ("cut_veto_dropped",)),
    "gen_V65": _from("gen_V65", [(32,)]), "gen_mm5": _from("gen_mm5", [(31,), (33,)], catches=CORE + ("band_on_d_in",)),
    "gen_band1010": _from("gen_band1010", [(200,)], frames=[0, 199, 200, 399], catches=CORE + ("row_tail",)),
    # rows and ends
    "free_end": _from("T65", [(32,), (64,)], end="free", catches=CORE + ROW_END + ("row_tail",)),
    "holes_end": _from("units", [(24,), (47,)], end="holes", unit=1, catches=CORE + ROW_END + ("score_at_path_end",)),
    "beam_ge_L": _from("beam_ge_2L", [(15,)], catches=("e_out_no_emission",)),
    # paths the lattice did not choose
    "outside": _from("outside", [(25,)]), "disconnected": _from("disconnected", [(25,)], end="free", catches=CORE + ROW_END + ("score_at_path_end",)),
}
NAMES = list(CASES)
_made, _want = {}, {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


def fast_form(c):
    return C.fast_form(c)


def uncut(name, **fault):
    """margin_resume_ref's answer for the whole lattice in one call (computed once; planted faults are not kept)"""
    c = case(name)
    if fault or name not in _want:
        r = RR.resume_ref(c["lp"], c["labels"], c["beam"], c["mm"], c["band_lo"], c["path"], None, c["e_in"], -1, c["unit"], c["frames"], **fault)
        if fault:
            return r
        _want[name] = r
    return _want[name]


def split(name, cut, **fault):
    c = case(name)
    return RR.split_ref(c["lp"], c["labels"], c["beam"], c["mm"], c["band_lo"], cut, c["path"], -1, c["e_in"], c["unit"], c["frames"], **fault)


# what property 2 promises of a cut lattice: everything but the rows handed across the cuts, which belong to single chunks
CUT_KEYS = ("through", "alt", "runner_up", "rows", "rows_lo", "d_out", "e_out")
