"""State visit probabilities, CPU side: the float64 reference (visit_ref.py) against enumeration of every band path, what
follows from max_move 2 and 3, the best paths' visited set on peaked inputs, the seeded faults on every input family of the
GPU tests, the conditions of those inputs, the host helpers on a hand-made path, and the C-ABI / Python boundary of the
feature (no compute: there is no GPU)."""
import ctypes
import functools

import numpy as np
import pytest

import duration_ref as DR
import posterior_ref as R
import visit_ref as VR
from fb_harness import assert_declared_exported_bound

NEW_SYMBOLS = ("ka_ctc_state_visits_f32", "ka_ctc_state_visits_batch_f32", "ka_state_visit_workspace_bytes")
BIT_CASE = "steep_T200_S280_V39_B2_M4"
# one case per family and form among those the GPU file runs (T <= 700).  The peaked ones are those with the narrowest bands: on
# a wider one the cells that leave the band lie below 2^-120, where no figure is asked of a kernel and stay_outside cannot show.
FAMILY_CASES = ["edge_T400_S150_V39_B16_M4_back0", "edge_T400_S150_V80_B64_M4_back0", "steep_T200_S280_V39_B7_M4",
                "steep_T260_S620_V39_B9_M6", "flat_T300_S10_V39_B2_M4", "flat_T300_S10_V39_B2_M6", "peaked_T129_S30_V39_B7_M2",
                "peaked_T300_S40_V80_B9_M4", "geom_T161_S40_V39_B16_M4", "geom_T100_S30_V65_B16_M4"]


@functools.lru_cache(maxsize=None)
def _case(name):
    lp, labels, terminal, beam, mm = R.edge_cases()[name]()
    return lp, labels, terminal, beam, mm, VR.visits(lp, labels, terminal, beam, mm)


def _tiny_cases():
    rng = np.random.default_rng(2711)
    cases = []
    for mm in (1, 2, 3, 4, 5, 6):
        for T, S, beam in ((6, 4, 1000), (5, 3, 4), (6, 2, 2), (4, 4, 4), (1, 1, 1000), (6, 0, 1000), (5, 4, 2)):
            V = 5
            lp = np.log(rng.dirichlet(np.ones(V), size=T)).astype(np.float32)
            labels = rng.integers(1, V, size=S).astype(np.int32)
            if S >= 2:
                labels[int(rng.integers(0, S))] = 0                        # label value 0: the veto of even moves
            if T >= 3:
                lp[int(rng.integers(0, T)), int(rng.integers(1, V))] = -np.inf
            cases.append((lp, labels, beam, mm))
    return cases


def test_reference_is_the_enumerated_visit_probability():
    checked, below = 0, 0
    for lp, labels, beam, mm in _tiny_cases():
        T, L = lp.shape[0], 2 * len(labels) + 1
        assert T <= 6 and L <= 9
        for terminal in R.live_terminals(lp, labels, beam, mm)[:3]:
            want_V, want_X = VR.sequential(lp, labels, terminal, beam, mm)
            assert want_V is not None
            got = VR.visits(lp, labels, terminal, beam, mm)
            np.testing.assert_allclose(got["V"], want_V, rtol=0, atol=1e-12)
            np.testing.assert_allclose(got["X"], want_X, rtol=0, atol=1e-11)
            assert got["V"][terminal] == 1.0 and np.all(got["V"][terminal + 1:] == 0.0)
            assert np.all(got["V"] <= got["D"]) and np.all(got["X"] <= got["B"]) and np.all(got["V"] >= 0.0)
            # first = last - frames + 1 on every path: E[first; visited] = X - D + V is an expectation of a frame index
            first = got["X"] - got["D"] + got["V"]
            assert np.all(first >= -1e-12) and np.all(first <= got["X"] + 1e-12)
            checked += 1
            below += terminal < L - 1
    assert checked >= 40 and below >= 10                                   # terminals below L - 1 among them


def test_max_move_two_visits_every_position_up_to_the_terminal():
    lp, labels = R.sloped(120, 40, 39, 77)
    terminal = R.live_terminals(lp, labels, 1000, 2)[0]
    v = VR.visits(lp, labels, terminal, 1000, 2)
    tol = VR.M_VISIT * v["E_V"]
    assert np.all(np.abs(v["V"][1:terminal + 1] - 1.0) <= tol[1:terminal + 1])
    glo, g0 = v["gamma"][0]
    assert glo == 0 and abs(v["V"][0] - g0[0]) <= tol[0] and 0.0 < g0[0] < 1.0   # position 0 is visited only at frame 0


def test_max_move_three_visits_every_phoneme_up_to_the_terminal():
    lp, labels = R.sloped(200, 40, 39, 3)
    terminal = R.live_terminals(lp, labels, 16, 3)[0]
    v = VR.visits(lp, labels, terminal, 16, 3)
    odd = np.arange(1, terminal + 1, 2)
    assert len(odd) >= 30 and np.all(np.abs(v["V"][odd] - 1.0) <= VR.M_VISIT * v["E_V"][odd])
    assert np.min(v["V"][0:terminal:2]) < 0.9                              # ... but not every blank


@pytest.mark.parametrize("shape", R.PEAKED_SHAPES[:4], ids=lambda s: "T%d_S%d_V%d_B%d_M%d" % s)
def test_peaked_visits_are_the_best_paths_visited_set(shape):
    T, S, V, beam, mm = shape
    lp, labels, terminal = R.peaked(T, S, V, beam, mm, seed=7)
    v = VR.visits(lp, labels, terminal, beam, mm)
    best = VR.best_paths_visits(lp, labels, terminal, beam, mm)
    hist, _ = DR.best_paths_histogram(lp, labels, terminal, beam, mm)
    assert np.all((best > 0.0) == (hist > 0.0)) and np.all(best <= 1.0 + 1e-12) and best[terminal] == 1.0
    assert np.mean((best == 0.0) | (best == 1.0)) > 0.5                    # most positions are on every best path or on none
    # (duration_ref.peaked_bound: a path that leaves the best ones weighs e^-20 a frame)
    assert np.all(np.abs(v["V"] - best) <= VR.M_VISIT * (v["E_V"] + v["n"] * float(R.state_error_model(1.0))))


def _fault_sites(name, v):
    """(fault, at) for every seeded fault, at a frame or block where the case lets it show."""
    lp, labels, terminal, beam, mm = _case(name)[:5]
    T, L = lp.shape[0], 2 * len(labels) + 1
    _, hi = R.windows(T, L, beam)
    moved = [t for t in range(T - 1) if hi[t + 1] > hi[t] and v["V"][hi[t]:hi[t + 1]].max() > 0.01]
    assert moved and T > 2 * R.CK, name
    return [("veto_stay", 0), ("stay_outside", 0), ("skip_last", 0), ("t_plus_1", 0), ("missed_retire", moved[len(moved) // 2])] + \
           [("stale_top", k) for k in range((T - 2) // R.CK)]


@pytest.mark.parametrize("name", FAMILY_CASES)
def test_every_seeded_fault_shows(name):
    lp, labels, terminal, beam, mm, v = _case(name)
    shown = {}
    for fault in _fault_sites(name, v):
        bad = VR.visits(lp, labels, terminal, beam, mm, fault=fault)
        over_V = np.abs(bad["V"] - v["V"]) > VR.M_VISIT * v["E_V"]
        over_X = np.abs(bad["X"] - v["X"]) > VR.M_VISIT * v["E_X"]
        shown[fault[0]] = shown.get(fault[0], False) or bool(over_V.any() or over_X.any())
        if fault[0] == "t_plus_1":
            assert not over_V.any() and over_X.any()
    assert set(shown) == set(VR.FAULTS) and all(shown.values()), (name, shown)


def test_the_family_cases_span_both_forms_and_all_five_families():
    shapes = R.case_shapes()
    assert all(shapes[k][0] <= 700 for k in FAMILY_CASES)
    forms = {(k.split("_")[0], R.fast_form(*shapes[k][1:])) for k in FAMILY_CASES}
    assert forms == {(f, x) for f in ("edge", "steep", "flat", "peaked", "geom") for x in (True, False)}


def test_conditions_of_the_inputs():
    # the bit test's case: at least half of the positions are held by exactly one frame
    T, S, _, beam, _ = R.case_shapes()[BIT_CASE]
    single = VR.single_frame_positions(T, 2 * S + 1, beam)
    assert single.sum() == 398 and len(single) == 561
    v = _case(BIT_CASE)[5]
    assert np.array_equal(v["n"] == 1, single) and np.array_equal(v["V"][single], v["D"][single])      # r is 1 by rule there
    assert np.sum(single & (v["V"] > 0.0)) >= 100
    # the model is positive wherever a visit is, and small against a probability
    for name in FAMILY_CASES:
        v = _case(name)[5]
        assert np.all(v["E_V"][v["V"] > 0.0] > 0.0) and v["E_V"].max() < 1e-4, name
        assert np.all(v["V"] <= v["D"]) and np.all(v["X"] <= v["B"]) and v["V"].max() <= 1.0 + 1e-9, name
        # r takes values inside (0, 1) and both exact ones
        r = np.concatenate([x for _, x in v["r"]])
        assert np.any((r > 0.01) & (r < 0.99)) and np.any(r == 1.0), name


# ---- the host helpers ----
def _indicator(path, L):
    """V, X and D of one path."""
    V, X, D = np.zeros(L), np.zeros(L), np.zeros(L)
    for t, s in enumerate(path):
        D[s] += 1
        if t == len(path) - 1 or path[t + 1] != s:
            V[s], X[s] = 1.0, float(t)
    return V, X, D


def test_phoneme_visits_split_odd_and_even_positions():
    import kokoro_align_amd as ka
    labels, blanks = ka.phoneme_visits([0.5, 1.0, 0.25, 0.0, 1.0])
    assert np.array_equal(labels, [1.0, 0.0]) and np.array_equal(blanks, [0.5, 0.25, 1.0])
    assert labels.dtype == blanks.dtype == np.float64
    with pytest.raises(ValueError):
        ka.phoneme_visits([1.0, 0.5])


def test_phoneme_spans_on_a_hand_made_path():
    import kokoro_align_amd as ka
    #        t:  0  1  2  3  4  5  6  7
    path = [0, 1, 1, 3, 3, 3, 5, 6]                                    # S = 3, L = 7; positions 2 and 4 are jumped over
    V, X, D = _indicator(path, 7)
    first, last = ka.phoneme_spans(V, X, D)
    assert np.array_equal(last[[0, 1, 3, 5, 6]], [0.0, 2.0, 5.0, 6.0, 7.0])
    assert np.array_equal(first[[0, 1, 3, 5, 6]], [0.0, 1.0, 3.0, 6.0, 7.0])
    assert np.all(np.isnan(first[[2, 4]])) and np.all(np.isnan(last[[2, 4]]))
    with pytest.raises(ValueError):
        ka.phoneme_spans(V, X, D[:-1])
    # a mixture of two paths: the means given that the position is visited
    V2, X2, D2 = _indicator([0, 1, 2, 3, 3, 3, 5, 6], 7)
    first, last = ka.phoneme_spans(0.5 * (V + V2), 0.5 * (X + X2), 0.5 * (D + D2))
    assert last[1] == 1.5 and first[1] == 1.0 and last[2] == 2.0 and first[2] == 2.0 and np.isnan(last[4])


def test_segment_expected_match_on_a_hand_made_path():
    import kokoro_align_amd as ka
    path = [0, 1, 1, 3, 3, 3, 5, 6]
    V, _, _ = _indicator(path, 7)
    labels = [4, 0, 7]                                                 # the second phoneme has label value 0: not counted
    # boundaries read at 0, 3, 6 (and 9 >= T): text 0, 1, 2, then S = 3
    expected, count = ka.segment_expected_match(V, labels, path, [3, 6, 9])
    assert np.array_equal(count, [1, 0, 1]) and np.array_equal(expected, [1.0, 0.0, 1.0])
    assert expected.dtype == np.float64 and count.dtype == np.int64
    soft = np.array([1.0, 0.25, 1.0, 0.5, 1.0, 0.75, 1.0])
    expected, count = ka.segment_expected_match(soft, [4, 5, 7], path, [3, 20])
    assert np.array_equal(count, [1, 2]) and np.array_equal(expected, [0.25, 1.25])
    expected, count = ka.segment_expected_match(soft, [4, 5, 7], path, [20])            # one segment: the whole transcript
    assert np.array_equal(count, [3]) and np.array_equal(expected, [1.5])
    with pytest.raises(ValueError):
        ka.segment_expected_match(soft[:-2], [4, 5, 7], path, [3])


# ---- the C-ABI / Python boundary ----
def test_new_symbols_declared_exported_and_bound():
    assert_declared_exported_bound(NEW_SYMBOLS)


def test_workspace_bytes_are_the_duration_calls():
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    arr = lambda n, v: (ctypes.c_int64 * n)(*[v] * n)
    assert L.ka_state_visit_workspace_bytes(2, arr(2, 5000), arr(2, 500), 64, 1000, 300, 1) == 0
    assert L.ka_state_visit_workspace_bytes(2, arr(2, 0), arr(2, 50), 64, 1000, 4, 1) == 0
    assert L.ka_state_visit_workspace_bytes(2, arr(2, 5000), arr(2, 500), 64, 1000, 4, 7) == 0
    for V, mm in ((64, 4), (80, 4), (39, 6)):
        for n in (1, 3, 2000):
            for mem in (0, 1):
                got = L.ka_state_visit_workspace_bytes(n, arr(n, 700), arr(n, 300), V, 1000, mm, mem)
                assert got > 0 and got == L.ka_state_duration_workspace_bytes(n, arr(n, 700), arr(n, 300), V, 1000, mm, mem)


def test_python_functions_are_exported_and_reject_bad_lists():
    import kokoro_align_amd as ka
    for name in ("ctc_state_visits", "ctc_state_visits_batch", "ctc_state_visits_device", "phoneme_visits", "phoneme_spans",
                 "segment_expected_match"):
        assert callable(getattr(ka, name)), name
    assert ka.ctc_state_visits_batch([], [], []) == []
    assert ka.ctc_state_visits_batch([], [], [], return_status=True) == ([], [])
    with pytest.raises(ValueError):
        ka.ctc_state_visits_batch([np.zeros((3, 4), np.float32)], [[1]], [])
