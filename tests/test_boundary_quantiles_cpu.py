"""Exact boundary-time quantiles, CPU side: the float64 reference (quantile_ref.py) against enumeration of every band path,
the seeded faults on the input families of the GPU tests, the conditions of those inputs, the host helpers on a hand-made
path, and the C-ABI / Python boundary of the feature (no compute: there is no GPU)."""
import ctypes
import functools

import numpy as np
import pytest

import posterior_ref as R
import quantile_ref as QR
import test_state_visits_cpu as VC
from fb_harness import assert_declared_exported_bound

NEW_SYMBOLS = ("ka_ctc_boundary_quantiles_f32", "ka_ctc_boundary_quantiles_batch_f32", "ka_boundary_quantile_workspace_bytes")
FAMILY_CASES = list(VC.FAMILY_CASES)
LEVELS = (0.05, 0.5, 0.95)
MAX_UNSAFE = 0.02                                  # the share of a case's (cut, level) pairs that may lie at a near-tie


@functools.lru_cache(maxsize=None)
def family(name):
    """(lp, labels, terminal, beam, mm, cuts, reference) of a family case: cuts at every even position of [0, L]."""
    lp, labels, terminal, beam, mm = R.edge_cases()[name]()
    ref = R.ref_at(lp, labels, terminal, beam, mm)
    assert ref["status"] == R.OK
    cuts = np.arange(0, 2 * len(labels) + 2, 2, dtype=np.int64)
    return lp, labels, terminal, beam, mm, cuts, ref


@functools.lru_cache(maxsize=None)
def family_quantiles(name):
    lp, labels, terminal, beam, mm, cuts, ref = family(name)
    return QR.quantiles(lp, labels, terminal, beam, mm, cuts, LEVELS, gamma=ref["gamma"])


def test_reference_is_the_enumerated_crossing_time_distribution():
    checked, below, inside = 0, 0, 0
    levels = (2.0 ** -10, 0.05, 0.3, 0.5, 0.7, 0.95, 1.0 - 2.0 ** -10)
    for lp, labels, beam, mm in VC._tiny_cases():
        T, L = lp.shape[0], 2 * len(labels) + 1
        assert T <= 6 and L <= 9
        cuts = np.arange(L + 1)
        for terminal in R.live_terminals(lp, labels, beam, mm)[:3]:
            want = QR.enumerate_cdf(lp, labels, terminal, beam, mm, cuts)
            assert want is not None
            got = QR.quantiles(lp, labels, terminal, beam, mm, cuts, levels)
            np.testing.assert_allclose(got["F"], want, rtol=0, atol=1e-12)
            # the frames, away from an enumerated value that ties with a level to the last bits
            clear = np.array([[not np.any(np.abs(want[:, k] - x) <= 1e-12) for x in levels] for k in range(L + 1)])
            assert np.array_equal(got["q"][clear], QR.frames_of(want, levels)[clear]) and clear.mean() > 0.9
            assert np.all(got["q"][0] == 0) and np.all(got["q"][terminal + 1:] == T) and np.all(got["q"][L] == T)
            assert np.all(np.diff(got["q"], axis=1) >= 0) and np.all(np.diff(got["q"], axis=0) >= 0)
            assert np.all(np.diff(want, axis=0) >= -1e-12)                  # the true F never falls in t
            checked += 1
            below += terminal < L - 1
            inside += int(got["inside"].any())
    assert checked >= 40 and below >= 10 and inside >= 20                   # terminals below L - 1 among them


def test_integer_definition_follows_the_float64_reference_on_rounded_rows():
    # float32 roundings of the reference's own gamma: the integer definition gives the float64 frames at every safe pair
    for name in FAMILY_CASES[:4]:
        lp, labels, terminal, beam, mm, cuts, ref = family(name)
        q = family_quantiles(name)
        L = 2 * len(labels) + 1
        rows, los = QR.float32_rows(ref["gamma"], min(beam, L))
        got = QR.integer_quantiles(rows, los, cuts, LEVELS, L, beam)
        safe = ~q["unsafe"]
        assert got.dtype == np.int32 and np.array_equal(got[safe], q["q"][safe]), name


def _floor_site(name):
    """A (cut, level) at which floor in place of ceil shows: the level half a unit above an attained sum k 2^-32."""
    lp, labels, terminal, beam, mm, cuts, ref = family(name)
    L = 2 * len(labels) + 1
    rows, los = QR.float32_rows(ref["gamma"], min(beam, L))
    F = QR.integer_sums(rows, los, cuts, L, beam)
    base = QR.integer_quantiles(rows, los, cuts, (0.5,), L, beam)[:, 0]
    lo, hi = R.windows(lp.shape[0], L, beam)
    for k, c in enumerate(cuts):
        t = int(base[k])
        if t < lp.shape[0] and lo[t] < c < hi[t]:
            level = (int(F[t, k]) + 0.5) / QR.FIX
            if 2.0 ** -10 <= level <= 1.0 - 2.0 ** -10:
                return rows, los, cuts[k:k + 1], level, L, beam, t
    return None


def test_every_seeded_fault_shows():
    shown = dict.fromkeys(QR.FAULTS, 0)
    for name in FAMILY_CASES:
        lp, labels, terminal, beam, mm, cuts, ref = family(name)
        want = family_quantiles(name)["q"]
        for fault in QR.FAULTS:
            if fault == "floor":
                site = _floor_site(name)
                if site is None:
                    continue
                rows, los, cut, level, L, beam, t = site
                assert float(int(level * QR.FIX)) != level * QR.FIX             # k + 1/2: ceil and floor differ
                good = QR.integer_quantiles(rows, los, cut, (level,), L, beam)
                bad = QR.integer_quantiles(rows, los, cut, (level,), L, beam, fault="floor")
                assert bad[0, 0] == t
                shown[fault] += int(not np.array_equal(good, bad))
            else:
                bad = QR.quantiles(lp, labels, terminal, beam, mm, cuts, LEVELS, fault=fault, gamma=ref["gamma"])["q"]
                shown[fault] += int(not np.array_equal(bad, want))
    assert all(n >= 1 for n in shown.values()), shown


def test_conditions_of_the_inputs():
    shapes = R.case_shapes()
    forms = {(k.split("_")[0], R.fast_form(*shapes[k][1:])) for k in FAMILY_CASES}
    assert forms == {(f, x) for f in ("edge", "steep", "flat", "peaked", "geom") for x in (True, False)}
    for name in FAMILY_CASES:
        lp, labels, terminal, beam, mm, cuts, ref = family(name)
        q = family_quantiles(name)
        T = lp.shape[0]
        pairs = q["q"].size
        left_out = int(q["unsafe"].sum())
        print(name, "pairs", pairs, "left out", left_out)
        assert left_out <= MAX_UNSAFE * pairs, (name, left_out, pairs)
        k, m = np.nonzero(~q["unsafe"] & (q["q"] < T))
        crossing_inside = q["inside"][q["q"][k, m], k]
        assert crossing_inside.any(), name                                  # a crossing strictly inside the band, at a safe pair
        assert q["E"].max() < 1e-4 and np.all(q["E"][q["inside"]] > 0.0), name


# ---- the host helpers ----
def test_boundary_cuts_are_sorted_unique_and_clamped():
    import kokoro_align_amd as ka
    #        t:  0  1  2  3  4  5  6  7
    path = [0, 1, 1, 3, 3, 3, 5, 6]                                     # S = 3
    # boundaries read at 0, 3, 4, 6 (9 >= T is not read): text 0, 1, 1, 2 -> cuts 0, 2, 2, 4
    cuts = ka.boundary_cuts(path, [3, 4, 6, 9], 3)
    assert cuts.dtype == np.int64 and np.array_equal(cuts, [0, 2, 4])
    assert np.array_equal(ka.boundary_cuts(path, [7], 2), [0, 4])       # 6 // 2 = 3 clamped to n_phonemes = 2
    assert np.array_equal(ka.boundary_cuts(path, [20], 3), [0])


def test_segment_boundary_interval_on_a_hand_made_path():
    import kokoro_align_amd as ka
    path = [0, 1, 1, 3, 3, 3, 5, 6]
    cuts = np.array([0, 2, 4, 6], np.int64)
    quant = np.array([[0, 0, 0], [2, 3, 4], [5, 6, 6], [7, 7, 8]], np.int32)
    start, end = ka.segment_boundary_interval(quant, cuts, path, [3, 6, 9], 3)
    assert start.dtype == end.dtype == np.int64 and start.shape == end.shape == (3, 3)
    assert np.array_equal(start, [[0, 0, 0], [2, 3, 4], [5, 6, 6]])
    assert np.array_equal(end, [[2, 3, 4], [5, 6, 6], [8, 8, 8]])         # b = 9 >= T = 8: T
    # the layout of segment_boundary_spread's quantiles
    paths = np.array([path] * 4, np.int32)
    sq, _, eq, _ = ka.segment_boundary_spread(paths, path, [3, 6, 9], 3)
    assert sq.shape == start.shape and eq.shape == end.shape and np.all(eq[2] == 8.0)
    with pytest.raises(ValueError):
        ka.segment_boundary_interval(quant[[0, 1, 3]], cuts[[0, 1, 3]], path, [3, 6, 9], 3)      # cut 4 is missing
    with pytest.raises(ValueError):
        ka.segment_boundary_interval(quant[:3], cuts, path, [3], 3)


def test_bad_cuts_and_levels_raise_before_any_call():
    import kokoro_align_amd as ka
    lp, labels = np.zeros((5, 4), np.float32), [1, 2]
    for bad in ([2, 1], [1, 1], [-1, 2], [0, 6]):
        with pytest.raises(ValueError):
            ka.ctc_boundary_quantiles_batch([lp], [labels], [4], [bad])
    for bad in ((), tuple(np.linspace(0.1, 0.9, 9)), (0.5, 0.5), (0.9, 0.1), (2.0 ** -11, 0.5), (0.5, 1.0), (float("nan"),)):
        with pytest.raises(ValueError):
            ka.ctc_boundary_quantiles_batch([lp], [labels], [4], [[0, 2]], q=bad)
    with pytest.raises(ValueError):
        ka.ctc_boundary_quantiles_batch([lp], [labels], [4], [])
    with pytest.raises(ValueError):
        ka.ctc_boundary_quantiles_batch([], [], [], [], q=(0.9, 0.1))
    assert ka.ctc_boundary_quantiles_batch([], [], [], []) == []
    assert ka.ctc_boundary_quantiles_batch([], [], [], [], return_status=True) == ([], [])


# ---- the C-ABI / Python boundary ----
def test_new_symbols_declared_exported_and_bound():
    assert_declared_exported_bound(NEW_SYMBOLS)
    import kokoro_align_amd as ka
    for name in ("ctc_boundary_quantiles", "ctc_boundary_quantiles_batch", "ctc_boundary_quantiles_device", "boundary_cuts",
                 "segment_boundary_interval"):
        assert callable(getattr(ka, name)), name


def test_workspace_bytes():
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    arr = lambda n, v: (ctypes.c_int64 * n)(*[v] * n)
    quant = L.ka_boundary_quantile_workspace_bytes
    assert quant(2, arr(2, 700), arr(2, 300), arr(2, 5), 0, 64, 1000, 4, 1) == 0       # M outside [1, 8]
    assert quant(2, arr(2, 700), arr(2, 300), arr(2, 5), 9, 64, 1000, 4, 1) == 0
    assert quant(2, arr(2, 700), arr(2, 300), arr(2, -1), 3, 64, 1000, 4, 1) == 0      # K < 0, K > 2S+2
    assert quant(2, arr(2, 700), arr(2, 300), arr(2, 603), 3, 64, 1000, 4, 1) == 0
    assert quant(2, arr(2, 700), arr(2, 300), arr(2, 5), 3, 64, 1000, 4, 7) == 0
    assert quant(2, arr(2, 0), arr(2, 300), arr(2, 5), 3, 64, 1000, 4, 1) == 0
    for V, mm in ((64, 4), (80, 4), (39, 6)):
        for n in (1, 3, 2000):
            for mem in (0, 1):
                base = L.ka_state_duration_workspace_bytes(n, arr(n, 700), arr(n, 300), V, 1000, mm, mem)
                none = quant(n, arr(n, 700), arr(n, 300), arr(n, 0), 3, V, 1000, mm, mem)
                some = quant(n, arr(n, 700), arr(n, 300), arr(n, 602), 8, V, 1000, mm, mem)
                assert base > 0 and none > 0 and some > none
                # device buffers: the slots of a duration call, wider descriptors, the thresholds and a generic slot's row -
                # bounded by the slots, not by the batch
                if mem == _lib.KA_MEM_DEVICE:
                    assert 0 <= none - base <= n * 64 + 1024 + 512 * 8 * 1024
