"""The deep inputs of tests/posterior_ref.py ("magnitude"), on the CPU: rows 2^k nats below their
neighbours and single cells masked with a large finite constant.  What is asserted here is what tests/test_posterior_deep_gpu.py
relies on: the rows are exact, the reference does not see the magnitude, which (case, call) pairs are compared cell by cell is
decided from the reference alone and listed, and a ninth seeded fault - every maximum of the log-sum-exp rounded through
float32, as a float maximum on doubles does - breaks the ladder from k = 35 and moves nothing on the older families."""
import numpy as np
import pytest

import posterior_ref as R

SHAPES = list(R.DEEP_SHAPES)
CASES = R.edge_cases()


def test_the_ladder_the_patterns_and_the_shapes_are_the_issues():
    assert R.DEEP_RUNGS == (10, 17, 20, 24, 30, 33, 35, 37, 40, 44)
    shapes = R.DEEP_SHAPES.values()
    assert {s[0] for s in shapes} == {40, 70} and {s[1] for s in shapes} == {12, 20}
    assert {s[3] for s in shapes} == {2, 4} and {s[4] for s in shapes} == {0, 1}                    # max_move; terminals L-1, L-2
    assert any(s[2] == 16 and 2 * s[1] + 1 > 16 for s in shapes) and any(s[2] >= 2 * s[1] + 1 for s in shapes)
    for T in (40, 70):
        p = R.deep_patterns(T)
        assert p["first"] == [0] and p["last"] == [T - 1] and (p["f31"], p["f32"], p["f33"]) == ([31], [32], [33])
        assert p["f30_34"] == [30, 31, 32, 33, 34] and p["pad8"] == list(range(T - 8, T)) and p["lead5"] == [0, 1, 2, 3, 4]
        assert p["all"] == list(range(T))
    assert R.fast_form(20, R.DEEP_V, 1000, 4) and not R.fast_form(20, 80, 1000, 4)                   # V = 39, and padded to 80


@pytest.mark.parametrize("shape", SHAPES)
def test_deep_rows_are_exact_and_their_sum_stays_inside_float32(shape):
    base = R.deep_base(shape)[0]
    for c in R.deep_all(shape):
        lp, shift = c["lp"], c["shift"]
        deep = shift > 0
        assert lp.dtype == np.float32 and np.all(np.isfinite(lp)) and deep.sum() == len(R.deep_patterns(len(lp))[c["pattern"]])
        assert np.array_equal(lp[~deep], base[~deep]) and np.all(shift[deep] == 2.0 ** c["k"])
        d = lp[deep].astype(np.float64) + 2.0 ** c["k"]                          # exact: the rows are -c + d in float32
        assert np.all(np.abs(d) <= 4.0) and np.all(d == np.round(d))
        assert np.all(d == 0.0) == (c["k"] >= 30) and np.array_equal(c["plain"][deep], d)
        assert np.sum(np.abs(lp.astype(np.float64))) < 2.0 ** 60 < np.finfo(np.float32).max


@pytest.mark.parametrize("shape", SHAPES)
def test_the_reference_is_shift_invariant_up_to_2_to_the_30(shape):
    """forward_backward on the SHIFTED float64 rows against the unshifted reference.  The shifted pass holds absolute alpha and
    beta of magnitude sum c: each of its about 4 operations a frame on either side rounds by an ulp of that, so a cell may move
    by (8 T + 8) ulp64(sum c) of its value."""
    worst = 0.0
    for c in R.deep_all(shape):
        if c["k"] > 30:
            continue
        T = len(c["lp"])
        got = R.ref_at(c["lp"].astype(np.float64), c["labels"], c["terminal"], c["beam"], c["mm"])
        assert got["status"] == R.OK
        tol = (8 * T + 8) * np.spacing(np.sum(c["shift"]))
        assert abs(got["ll"] - c["z"]) <= tol, c["name"]
        for (lo, g), (rlo, rg) in zip(got["gamma"], c["ref"]["gamma"]):
            assert lo == rlo
            big = rg >= R.CAP_FLOOR
            worst = max(worst, float(np.max(np.abs(g[big] - rg[big]) / (rg[big] * tol + 1e-15))))
    print(shape, "worst shifted-reference error in units of its bound:", worst)
    assert worst <= 1.0


def test_the_deep_model_is_the_old_one_without_a_shift_and_grows_with_it():
    c = R.deep_built("T40_S12_B16_M4", "f31", 10)
    zero = np.zeros_like(c["shift"])
    Rn, h = R.deep_roundings(zero)
    assert not Rn.any() and h == 0.0
    for E, (_, g) in zip(R.deep_error_model("state", c["ref"], zero), c["ref"]["gamma"]):
        assert np.array_equal(E, R.state_error_model(g))
    assert np.array_equal(R.deep_error_model("label", c["ref"], zero, c["labels"], R.DEEP_V), R.label_error_model(c["ref"]["gamma"], c["labels"], R.DEEP_V))
    assert np.array_equal(R.deep_error_model("path", c["pref"], zero), R.path_error_model(c["pref"]))
    assert R.deep_error_model("z", c["ref"], zero) == R.z_error_model(c["ref"])
    Rn, h = R.deep_roundings(c["shift"])
    assert h == 0.5 * np.spacing(R.LOG2E * 2.0 ** 10) and np.all(Rn >= 5 + 5 + 6)             # one deep frame: alpha or beta, Z, the sums
    costs = [float(np.max(R.deep_cost(R.deep_built("T40_S12_B16_M4", "f31", k)["shift"]))) for k in R.DEEP_RUNGS]
    assert all(a < b for a, b in zip(costs, costs[1:]))


def test_which_pairs_are_compared_cell_by_cell():
    """The cap is a condition on the reference: E <= 2^-10 value wherever value >= 2^-20.  Listed per call; expected outside:
    the upper rungs for every call, and every pattern from k = 17 for the path call (the float store of alpha relative to its
    block's offset: half a float32 ulp of c log2 e)."""
    outside = dict(state=[], label=[], path=[])
    for shape in SHAPES:
        for c in R.deep_all(shape):
            for call, inside in R.deep_caps(c).items():
                if not inside:
                    outside[call].append(c["name"])
                assert inside or c["k"] >= (17 if call == "path" else 33) or (call == "path" and c["pattern"] == "all"), (call, c["name"])
                if c["k"] >= 40 or (call == "path" and c["k"] >= 17):
                    assert not inside, (call, c["name"])
                if c["k"] <= 30 and call != "path":
                    assert inside, (call, c["name"])
    for call, names in outside.items():
        print(call, "- outside the cap:", len(names), "of", len(SHAPES) * 9 * len(R.DEEP_RUNGS))
        for n in names:
            print("   ", n)


def test_where_z_can_hold_2_to_the_minus_40():
    """The reported Z goes through the float store of the terminal's alpha relative to its block's offset (z_error_model), so
    2^-40 of |Z| is within reach only where |Z| is large and no deep frame lies in the last block.  Listed."""
    held, lost = [], []
    for shape in SHAPES:
        T = R.DEEP_SHAPES[shape][0]
        for c in R.deep_all(shape):
            ok = R.z_rel_holds(c["ref"], c["shift"])
            (held if ok else lost).append(c["name"])
            in_last_block = bool(np.any(c["shift"][(T - 1) // R.CK * R.CK:] > 0))
            if c["k"] >= 30:
                assert ok == (not in_last_block), c["name"]
    print("Z within 2^-40 |Z| is asserted for", len(held), "cases; not for", len(lost))
    for n in lost:
        print("   ", n)
    assert len(held) >= 80


# ---- the ninth fault ----
def _max32_margin(c):
    """How far max32 moves the state posteriors or Z of a deep case, in deep tolerances; inf for a non-finite value or a status."""
    bad = R.ref_at(c["lp"].astype(np.float64), c["labels"], c["terminal"], c["beam"], c["mm"], fault=("max32", None))
    if bad["status"] != R.OK or not np.isfinite(bad["ll"]):
        return np.inf
    best = abs(bad["ll"] - c["z"]) / (R.M_Z * R.deep_error_model("z", c["ref"], c["shift"]))
    for (_, g), (_, rg), E in zip(bad["gamma"], c["ref"]["gamma"], R.deep_error_model("state", c["ref"], c["shift"])):
        if not np.all(np.isfinite(g)):
            return np.inf
        best = max(best, float(np.max(np.abs(g - rg) / np.maximum(R.M_STATE * E, R.M_STATE * R.TINY))))
    return best


@pytest.mark.parametrize("k", [k for k in R.DEEP_RUNGS if k >= 35])
def test_max32_breaks_the_ladder_from_2_to_the_35(k):
    """On every shape some pattern of the rung gives a non-finite value, a status or five tolerances (the rule of
    tests/test_posterior_ref_cpu.py's faults: some family sees it).  Which patterns do depends on how float32 happens to round
    the rung's maxima: 2^35 log2 e rounds by 459 nats, inside exp's range, so one deep frame alone passes there, and eight
    (3670 nats) do not; from 2^37 (1835 nats) every pattern breaks."""
    margins = {(s, p): _max32_margin(R.deep_built(s, p, k)) for s in SHAPES for p in R.deep_patterns(R.DEEP_SHAPES[s][0])}
    print(k, {"%s-%s" % key: float(f"{v:.3g}") for key, v in margins.items()})
    for s in SHAPES:
        assert max(v for (s2, _), v in margins.items() if s2 == s) >= 5.0, (k, s, margins)
    if k >= 37:
        assert all(v >= 5.0 for v in margins.values()), (k, {key: v for key, v in margins.items() if v < 5.0})


@pytest.mark.parametrize("name", list(CASES))
def test_max32_moves_nothing_on_the_older_families(name):
    """Why 211 posterior tests could not see it: on every family of edge_cases() the fault moves no posterior by more than the
    existing faults' noise floor, 2e-13, and Z by no more than that share of itself."""
    lp, labels, term, beam, mm = CASES[name]()
    ref = R.ref_at(lp, labels, term, beam, mm)
    bad = R.ref_at(lp, labels, term, beam, mm, fault=("max32", None))
    assert ref["status"] == bad["status"] == R.OK
    worst = max(float(np.max(np.abs(g - rg))) if len(g) else 0.0 for (_, g), (_, rg) in zip(bad["gamma"], ref["gamma"]))
    print(name, "max32 moves gamma by", worst, "and Z by", abs(bad["ll"] - ref["ll"]))
    assert worst <= 2e-13 and abs(bad["ll"] - ref["ll"]) <= 2e-13 * max(1.0, abs(ref["ll"]))


# ---- masked cells ----
MASK_VALUES = R.MASK_VALUES


@pytest.mark.parametrize("value", MASK_VALUES)
@pytest.mark.parametrize("shape", SHAPES)
def test_masked_cells_lie_beside_live_alternatives_and_carry_no_mass(shape, value):
    lp, ninf, mask, labels, term, beam, mm = R.masked_case(shape, value)
    assert mask.sum() == 4 and np.all(lp[mask] == np.float32(value)) and np.all(np.isneginf(ninf[mask])) and np.array_equal(lp[~mask], ninf[~mask])
    assert not mask[:, 0].any()
    want = R.ref_at(ninf, labels, term, beam, mm)
    full = R.ref_at(lp, labels, term, beam, mm)
    assert want["status"] == full["status"] == R.OK and np.isfinite(want["ll"])      # the terminal is reached without a masked cell
    share = R.masked_mass(full, want)
    print(shape, value, "mass through the masked cells:", share)
    assert 0.0 <= share < R.TINY
