"""Expected state durations, CPU side: the float64 reference (duration_ref.py) against brute-force enumeration, its
identities, the best path's histogram on peaked inputs, the three host helpers on hand-made arrays, and the C-ABI / Python
boundary of the feature (no compute: there is no GPU)."""
import ctypes
import itertools

import numpy as np
import pytest

import duration_ref as DR
import posterior_ref as R
from fb_harness import assert_declared_exported_bound

NEW_SYMBOLS = ("ka_ctc_state_durations_f32", "ka_ctc_state_durations_batch_f32", "ka_state_duration_workspace_bytes")


def _enumerated(lp, labels, terminal, beam, mm):
    """D and B by enumerating every path of the band that ends at the terminal: the path-probability-weighted count of
    frames in s, and of their indices."""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    lab = R.expand(labels)
    L = len(lab)
    lo, hi = R.windows(T, L, beam)
    total, D, B = 0.0, np.zeros(L), np.zeros(L)
    for moves in itertools.product(range(mm), repeat=T):
        s, score, states, ok = 0, 0.0, [], True
        for t, j in enumerate(moves):
            s += j
            if not (lo[t] <= s < hi[t]) or (j >= 2 and j % 2 == 0 and lab[s] == 0):
                ok = False
                break
            score += lp[t, lab[s]]
            states.append(s)
        if not ok or states[-1] != terminal or score == -np.inf:
            continue
        p = np.exp(score)
        total += p
        for t, st in enumerate(states):
            D[st] += p
            B[st] += p * t
    return (D / total, B / total) if total > 0 else (None, None)


def _tiny_cases():
    rng = np.random.default_rng(2205)
    cases = []
    for mm in (1, 2, 3, 4, 5):
        for T, S, beam in ((6, 4, 1000), (5, 3, 4), (6, 2, 3), (4, 4, 5), (1, 1, 1000), (6, 0, 1000)):
            V = 5
            lp = np.log(rng.dirichlet(np.ones(V), size=T)).astype(np.float32)
            labels = rng.integers(1, V, size=S).astype(np.int32)
            if S >= 2:
                labels[int(rng.integers(0, S))] = 0                        # label value 0: the veto of even moves
            if T >= 3:
                lp[int(rng.integers(0, T)), int(rng.integers(1, V))] = -np.inf
            cases.append((lp, labels, beam, mm))
    return cases


def test_reference_is_the_enumerated_expected_count():
    checked = 0
    for lp, labels, beam, mm in _tiny_cases():
        T, L = lp.shape[0], 2 * len(labels) + 1
        assert T <= 6 and L <= 9
        for terminal in R.live_terminals(lp, labels, beam, mm)[:3]:
            want_D, want_B = _enumerated(lp, labels, terminal, beam, mm)
            assert want_D is not None
            ref = R.ref_at(lp, labels, terminal, beam, mm)
            assert ref["status"] == R.OK
            got = DR.durations(ref, L)
            np.testing.assert_allclose(got["D"], want_D, rtol=0, atol=1e-12)
            np.testing.assert_allclose(got["B"], want_B, rtol=0, atol=1e-11)
            checked += 1
    assert checked >= 30


@pytest.mark.parametrize("name", ["edge_T400_S150_V39_B16_M4_back0", "steep_T200_S280_V39_B7_M4", "flat_T300_S10_V39_B2_M4",
                                  "geom_T150_S100_V39_B64_M4", "geom_T120_S40_V39_B1000_M6"])
def test_reference_identities(name):
    lp, labels, terminal, beam, mm = R.edge_cases()[name]()
    T, L = lp.shape[0], 2 * len(labels) + 1
    d = DR.durations(R.ref_at(lp, labels, terminal, beam, mm), L)
    assert abs(d["D"].sum() - T) <= 1e-9 * T
    assert abs(d["B"].sum() - T * (T - 1) / 2) <= 1e-9 * T * T
    lo, hi = R.windows(T, L, beam)
    n = np.zeros(L, np.int64)
    for a, b in zip(lo, hi):
        n[a:b] += 1
    assert np.array_equal(d["n"], n) and np.all(d["D"][n == 0] == 0.0)
    import kokoro_align_amd as ka
    tau = ka.expected_crossing_frames(d["D"], np.arange(L + 1))
    assert tau[0] == 0.0 and abs(tau[-1] - T) <= 1e-9 * T and np.all(np.diff(tau) >= 0.0)
    # the model is positive wherever a band reaches, and small against a frame
    assert np.all(d["E_D"][n > 0] > 0.0) and d["E_D"].max() < 1e-3


@pytest.mark.parametrize("shape", R.PEAKED_SHAPES[:4], ids=lambda s: "T%d_S%d_V%d_B%d_M%d" % s)
def test_peaked_durations_are_the_best_paths_histogram(shape):
    T, S, V, beam, mm = shape
    lp, labels, terminal = R.peaked(T, S, V, beam, mm, seed=7)
    L = 2 * S + 1
    ref = R.ref_at(lp, labels, terminal, beam, mm)
    d = DR.durations(ref, L)
    hist, sure = DR.best_paths_histogram(lp, labels, terminal, beam, mm)
    assert abs(hist.sum() - T) < 1e-9 and np.mean(sure == 1.0) > 0.5          # most frames have one best cell; ties are counted
    assert np.all(np.abs(d["D"] - hist) <= DR.M_DURATION * (d["E_D"] + DR.peaked_bound(d)))
    import kokoro_align_amd as ka
    path = DR.likeliest_path(ref)
    assert path[-1] == terminal and np.all(np.diff(path) >= 0)
    ends = DR.peaked_boundaries(path, hist, S)
    assert len(ends) == 3
    start, end = ka.segment_boundary_shift(d["D"], path, ends + [T + 5], S)
    tol = DR.M_DURATION * float(np.sum(d["E_D"] + DR.peaked_bound(d)))
    assert start.shape == end.shape == (4,) and np.all(np.abs(start) <= tol) and np.all(np.abs(end) <= tol) and end[3] == 0.0


def test_cell_error_switches_at_the_flush_threshold():
    g = np.array([1.0, 0.5, R.TINY, R.TINY / 2, 0.0])
    e = DR.cell_error(g)
    assert np.array_equal(e[:3], R.state_error_model(g[:3])) and np.all(e[3:] == R.TINY_OUT)


def test_sequential_sums_follow_descending_frames():
    rows = np.array([[0.25, 0.5, 0.0], [1.0, 2.0 ** -24, 0.0], [0.75, 0.0, 0.0]], np.float32)
    D, B = DR.sequential_sums(rows, [0, 1, 2], 4)
    assert np.array_equal(D, [0.25, 1.5, 2.0 ** -24 + 0.75, 0.0])
    assert np.array_equal(B, [0.0, 1.0, 2.0 ** -24 + 1.5, 0.0])


# ---- the host helpers ----
def test_phoneme_durations_split_odd_and_even_positions():
    import kokoro_align_amd as ka
    labels, blanks = ka.phoneme_durations([0.5, 3.0, 0.25, 2.0, 1.25])
    assert np.array_equal(labels, [3.0, 2.0]) and np.array_equal(blanks, [0.5, 0.25, 1.25])
    assert labels.dtype == blanks.dtype == np.float64
    labels, blanks = ka.phoneme_durations([4.0])                       # S = 0: one blank
    assert labels.shape == (0,) and np.array_equal(blanks, [4.0])
    with pytest.raises(ValueError):
        ka.phoneme_durations([1.0, 2.0])


def test_expected_crossing_frames_reads_the_prefix_sum():
    import kokoro_align_amd as ka
    d = [0.5, 3.0, 0.25, 2.0, 1.25]
    tau = ka.expected_crossing_frames(d, [0, 1, 2, 5, 3])
    assert np.array_equal(tau, [0.0, 0.5, 3.5, 7.0, 3.75])             # a cut at 0 is crossed at once, one at L never before T
    assert ka.expected_crossing_frames(d, []).shape == (0,)
    for bad in ([-1], [6]):
        with pytest.raises(ValueError):
            ka.expected_crossing_frames(d, bad)


def test_segment_boundary_shift_on_a_hand_made_path():
    import kokoro_align_amd as ka
    #        t:  0  1  2  3  4  5  6  7
    path = [0, 1, 1, 2, 3, 3, 3, 4]                                    # S = 2, L = 5
    d = [1.5, 1.5, 1.0, 3.5, 0.5]                                      # prefix: 0, 1.5, 3.0, 4.0, 7.5, 8.0
    # boundaries read at 0, 3, 6 (and 9 >= T): text 0, 1, 1 -> cuts 0, 2, 2; the path crosses them at frames 0, 3, 3
    start, end = ka.segment_boundary_shift(d, path, [3, 6, 9], 2)
    assert np.array_equal(start, [0.0, 0.0, 0.0])                      # E[tau_0] = 0 at frame 0; E[tau_2] = 3.0 against frame 3
    assert np.array_equal(end, [0.0, 0.0, 0.0])                        # ... and 0 for the boundary at 9 >= T
    start, end = ka.segment_boundary_shift([1.5, 2.5, 1.0, 2.5, 0.5], path, [3, 6, 9], 2)
    assert np.array_equal(start, [0.0, 1.0, 1.0]) and np.array_equal(end, [1.0, 1.0, 0.0])   # E[tau_2] = 4.0: a frame later
    # the text index is clipped to n_phonemes: position 4 reads as text 2 whatever n_phonemes below it says
    start, end = ka.segment_boundary_shift(d, path, [7], 1)
    assert np.array_equal(start, [0.0]) and np.array_equal(end, [3.0 - 3.0])   # min(4 // 2, 1) = 1 -> cut 2, crossed at 3
    start, end = ka.segment_boundary_shift(d, path, [7], 2)
    assert np.array_equal(end, [7.5 - 7.0])                            # cut 4: E[tau_4] = 7.5, crossed at frame 7
    start, end = ka.segment_boundary_shift(d, path, [20], 2)           # one segment to the end
    assert np.array_equal(start, [0.0]) and np.array_equal(end, [0.0])


# ---- the C-ABI / Python boundary ----
def test_new_symbols_declared_exported_and_bound():
    assert_declared_exported_bound(NEW_SYMBOLS)


def _ws(n, T, S, V=64, beam=1000, mm=4, mem=1):
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    arr = lambda v: (ctypes.c_int64 * n)(*[v] * n)
    return L.ka_state_duration_workspace_bytes(n, arr(T), arr(S), V, beam, mm, mem)


def test_workspace_bytes():
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    assert _ws(2, 5000, 500, mm=300) == 0 and _ws(2, 0, 50) == 0 and _ws(2, 5000, 500, mem=7) == 0
    arr = lambda n, v: (ctypes.c_int64 * n)(*[v] * n)
    for V, mm in ((64, 4), (80, 4), (39, 6)):
        for n in (1, 3, 2000):
            dev, host = _ws(n, 700, 300, V=V, mm=mm), _ws(n, 700, 300, V=V, mm=mm, mem=0)
            # the label call's slots (both descriptors have one size); host mode stages the inputs and 2 x [L] doubles per lattice
            assert dev == L.ka_label_posterior_workspace_bytes(n, arr(n, 700), arr(n, 300), V, 1000, mm, 1)
            up = lambda b: (b + 255) // 256 * 256
            assert host == dev + n * (up(700 * V * 4) + up(300 * 4) + 2 * up(601 * 8))
    head = lambda n: up(n * 120) + up(n * 16)                 # descriptors and results
    assert _ws(3000, 700, 300) - head(3000) == _ws(1024, 700, 300) - head(1024)      # bounded by the slots, not by n


def test_python_functions_are_exported_and_reject_bad_lists():
    import kokoro_align_amd as ka
    for name in ("ctc_state_durations", "ctc_state_durations_batch", "ctc_state_durations_device", "phoneme_durations",
                 "expected_crossing_frames", "segment_boundary_shift"):
        assert callable(getattr(ka, name)), name
    assert ka.ctc_state_durations_batch([], [], []) == []
    assert ka.ctc_state_durations_batch([], [], [], return_status=True) == ([], [])
    with pytest.raises(ValueError):
        ka.ctc_state_durations_batch([np.zeros((3, 4), np.float32)], [[1]], [])
