"""The best path over a caller-given band, without a GPU: tests/band_ref.py is pinned to the C oracle
on the reference's own band, the band helpers of the package are checked, the rescue case of the issue is shown on the
reference, the inputs of tests/test_banded_gpu.py are shown to do what their names say, and five planted faults of band_ref
are each shown to change a result on one of those inputs."""
import numpy as np
import pytest

import band_cases as C
import band_ref as R
import golden_util as G
from oracle import oracle as O

import kokoro_align_amd as ka


def same(got, want):
    """path, labels, scores (as bits) and total of two results"""
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and
            np.array_equal(np.asarray(got[2]).view(np.int32), np.asarray(want[2]).view(np.int32)) and
            np.float32(got[3]).view(np.int32) == np.float32(want[3]).view(np.int32))


def assert_ref_is_oracle(lp, labels, beam, mm, what):
    T, L = lp.shape[0], 2 * len(labels) + 1
    lo = ka.diagonal_band(T, L, beam)
    try:
        want = O.ctc_best_path_c(lp, labels, beam, mm, return_total=True)
    except ValueError:
        with pytest.raises(ValueError):
            R.best_path_banded(lp, labels, lo, beam, mm)
        return False
    got = R.best_path_banded(lp, labels, lo, beam, mm, return_total=True)
    assert same(got, want), what
    return True


# ---- 1. band_ref with the diagonal table is the pinned oracle ----
def test_ref_equals_oracle_on_g1():
    n_ok = n_err = 0
    for c in G.g1_cases():
        ok = assert_ref_is_oracle(c["lp"], c["labels"], c["beam"], c["max_move"], f"g1 case {c['idx']}")
        assert ok == (c["status"] == 0)
        n_ok += ok
        n_err += not ok
    assert n_ok >= 5


def test_ref_equals_oracle_on_g2():
    for c in G.g2_cases():
        lp = O.hash_logprobs(c["T"], c["V"], c["seed"])
        labels = O.hash_labels(c["S"], c["V"], c["seed"])
        assert assert_ref_is_oracle(lp, labels, c["beam"], c["max_move"], f"g2 case {c['idx']}")


def test_ref_equals_oracle_on_200_random_lattices():
    rng = np.random.default_rng(4290)
    n_ok = n_err = n_ninf = n_zero = 0
    for k in range(200):
        V = int(rng.integers(2, 12))
        S = int(rng.integers(0, 40))
        T = int(rng.integers(1, 90))
        beam = int(rng.choice([4, 5, 8, 13, 33, 1000]))
        mm = int(rng.integers(2, 6))
        lp = np.round(rng.standard_normal((T, V)) * 2, int(rng.integers(0, 3))).astype(np.float32)   # (few decimals: ties)
        if rng.random() < 0.3:
            lp = np.where(rng.random((T, V)) < 0.2, -np.inf, lp).astype(np.float32)
            n_ninf += 1
        labels = rng.integers(0, V, size=S).astype(np.int32)
        n_zero += bool(np.any(labels == 0))
        ok = assert_ref_is_oracle(lp, labels, beam, mm, f"random lattice {k}: T={T} S={S} V={V} beam={beam} max_move={mm}")
        n_ok += ok
        n_err += not ok
    assert n_ok >= 100 and n_err >= 1 and n_ninf >= 20 and n_zero >= 50, (n_ok, n_err, n_ninf, n_zero)


# ---- 2. the helpers ----
@pytest.mark.parametrize("T,L,beam", [(1, 1, 1000), (7, 31, 4), (240, 121, 24), (50000, 10001, 1000), (500000, 200001, 1000), (13, 401, 7)])
def test_diagonal_band_is_the_formula(T, L, beam):
    got = ka.diagonal_band(T, L, beam)
    assert got.dtype == np.int64 and got.shape == (T,)
    if T <= 50000:
        assert got.tolist() == R.diagonal_lo(T, L, beam)
    else:   # L t exceeds 2^31: spot checks in Python integers, every 997th frame and the ends
        for t in list(range(0, T, 997)) + [T - 2, T - 1]:
            assert int(got[t]) == max(0, L * t // T - beam // 2), t
        assert np.all(np.diff(got) >= 0) and got[-1] == (L * (T - 1)) // T - beam // 2


def test_anchored_band_without_anchors_is_diagonal():
    for T, L, beam in [(240, 121, 24), (1, 5, 4), (97, 1401, 300), (500000, 200001, 1000)]:
        assert np.array_equal(ka.anchored_band(T, L, [], beam), np.clip(ka.diagonal_band(T, L, beam), 0, L - 1))
        assert np.array_equal(ka.anchored_band(T, L, [], beam), ka.diagonal_band(T, L, beam))


def test_anchored_band_is_monotone_and_in_range():
    rng = np.random.default_rng(7)
    for _ in range(200):
        T = int(rng.integers(2, 400))
        L = 2 * int(rng.integers(0, 300)) + 1
        beam = int(rng.choice([1, 4, 24, 300, 1000]))
        k = int(rng.integers(0, min(6, T - 1) + 1))
        frames = np.sort(rng.choice(np.arange(1, T), size=k, replace=False))
        pos = np.sort(rng.integers(0, L + 1, size=k))
        lo = ka.anchored_band(T, L, list(zip(frames.tolist(), pos.tolist())), beam)
        assert lo.shape == (T,) and lo.dtype == np.int64
        assert lo.min() >= 0 and lo.max() <= L - 1 and np.all(np.diff(lo) >= 0)
        for f, p in zip(frames.tolist(), pos.tolist()):   # the centre passes through every anchor
            assert lo[f] == min(max(p - beam // 2, 0), L - 1)
    for bad in ([(5, 3), (5, 4)], [(6, 3), (5, 4)], [(5, 9), (8, 4)], [(0, 0)], [(10, 2)]):
        with pytest.raises(ValueError):
            ka.anchored_band(10, 21, bad, 4)


def test_band_around_path_keeps_the_path_inside():
    for name in ("const0", "shifted", "ring_wrap", "ninf"):
        lp, lab, lo, beam, mm = C.case(name)
        path, L = C.want(name)[0], 2 * len(lab) + 1
        for b in (1, 2, 7, beam):
            band = ka.band_around_path(path, L, b)
            assert np.all(np.diff(band) >= 0) and band.min() >= 0 and band.max() <= L - 1
            assert np.all((band <= path) & (path < np.minimum(band + b, L))), (name, b)


def test_band_edge_contact_on_hand_made_cases():
    L, beam = 101, 10
    lo = np.array([0, 0, 5, 20, 50, 91, 95], np.int64)           # hi = 10, 10, 15, 30, 60, 101, 101
    path = np.array([0, 6, 5, 24, 59, 91, 100], np.int64)
    # frame 0: on lo = 0, a clamped end: no.  1: within 3 of hi - 1 = 9: yes.  2: on lo = 5: yes.  3: 4 above lo, 5 below hi - 1: no.
    # 4: on hi - 1: yes.  5: on lo = 91 (hi clamped to L): yes, by lo.  6: on hi - 1 = L - 1, clamped, and 5 above lo: no.
    assert ka.band_edge_contact(path, lo, beam, L).tolist() == [1, 2, 4, 5]
    assert ka.band_edge_contact(path, lo, beam, L, max_move=1).tolist() == [2, 4, 5]
    assert ka.band_edge_contact(path, lo, beam, L, max_move=5).tolist() == [1, 2, 3, 4, 5]
    # the diagonal band of a path along the diagonal: no contact; of a path held at 0: contact once lo > 0
    T = 200
    diag = ka.diagonal_band(T, L, beam)
    assert ka.band_edge_contact(L * np.arange(T) // T, diag, beam, L).size == 0
    held = ka.band_edge_contact(np.maximum(diag, 0), diag, beam, L)
    assert held.tolist() == np.nonzero(diag > 0)[0].tolist()


# ---- 3. the rescue case ----
@pytest.mark.parametrize("seed", range(6))
def test_rescue_case(seed):
    lp, labels, L, beam, pre = C.rescue(seed)
    T = lp.shape[0]
    full = R.best_path_banded(lp, labels, np.zeros(T, np.int64), 2 * L, 4, return_total=True)
    diag_lo = ka.diagonal_band(T, L, beam)
    diag = R.best_path_banded(lp, labels, diag_lo, beam, 4, return_total=True)
    assert int(np.sum(diag[0] != full[0])) > 100 and diag[3] < full[3] - 100
    assert ka.band_edge_contact(diag[0], diag_lo, beam, L).size > 0
    anchored = R.best_path_banded(lp, labels, ka.anchored_band(T, L, [(pre, 0)], beam), beam, 4, return_total=True)
    assert same(anchored, full)


# ---- 4. the inputs of the GPU families do what their names say ----
def test_every_case_has_a_valid_table():
    for name in C.NAMES:
        lp, lab, lo, beam, mm = C.case(name)
        L = 2 * len(lab) + 1
        assert lo.shape == (lp.shape[0],) and lo.min() >= 0 and lo.max() < L and np.all(np.diff(lo) >= 0), name


def test_edge_cases_ride_their_edges():
    lp, lab, lo, beam, mm = C.case("ride_hi")
    path = C.want("ride_hi")[0]
    assert int(np.sum(path == lo + beam - 1)) >= 10 and np.all(np.diff(lo)[4:] == mm - 1)
    lp, lab, lo, beam, mm = C.case("ride_lo")
    path = C.want("ride_lo")[0]
    assert int(np.sum((path == lo) & (lo > 0))) >= 10
    lp, lab, lo, beam, mm = C.case("shifted")
    assert int(np.sum(C.want("shifted")[0] - lo <= 2)) >= 10


def test_better_cell_lies_outside():
    lp, lab, lo, beam, mm = C.case("better_outside")
    L = 2 * len(lab) + 1
    cells = R.best_path_banded(lp, lab, lo, beam + 1, mm, return_cells=True)[3]   # one position wider at the high edge
    better = 0
    for t, (pos, sc) in enumerate(cells):
        hi = min(lo[t] + beam, L)
        outside = sc[pos == hi]
        inside = sc[pos < hi]
        better += bool(outside.size and inside.size and outside[0] > inside.max())
    assert better >= 10
    # and the band's answer is not the wider band's
    assert not np.array_equal(C.want("better_outside")[0], R.best_path_banded(lp, lab, lo, beam + 1, mm)[0])


def test_statuses_of_the_cases():
    empty = {n for n in C.NAMES if C.want(n) is None}
    assert empty == {"no_overlap", "step500", "step1100", "mm1"}
    lp, lab, lo, beam, mm = C.case("no_overlap")
    assert np.max(np.diff(lo)) == beam + mm
    # the steps with survivors end above the step; the ring case passes slot 1023 -> 0 inside its band
    for s in C.STEPS:
        if f"step{s}" not in empty:
            assert C.want(f"step{s}")[0][-1] >= s
    assert C.want("step1009")[0][-1] >= 1024 and C.want("step1009")[0][349] <= 1023
    lp, lab, lo, beam, mm = C.case("ring_wrap")
    path = C.want("ring_wrap")[0]
    assert np.any((lo < 1023) & (lo + beam > 1024) & (lo > 700)) and path[0] < 4 and path[-1] == 1400


# ---- 5. five planted faults: each changes a result on some case ----
@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_changes_a_result(fault):
    changed = []
    for name in C.NAMES:
        lp, lab, lo, beam, mm = C.case(name)
        want = C.want(name)
        try:
            got = R.best_path_banded(lp, lab, lo, beam, mm, fault=fault, return_total=True)
        except ValueError:
            got = None
        if (got is None) != (want is None) or (got is not None and not same(got, want)):
            changed.append(name)
    assert changed, fault
