"""The best path over a self-steering band, without a GPU: the properties that follow from the recurrence
are shown on tests/track_ref.py (the table is a valid table, the banded reference over it returns the same answer, a band as
wide as the lattice gives the pinned C oracle's answer, a valid lattice never loses every state), the rescue case of the issue
is measured on the reference, the inputs of tests/test_tracking_gpu.py are shown to do what their names say, and six planted
faults of track_ref are each shown to change a result on one of those inputs."""
import ctypes
import os
import re

import numpy as np
import pytest

import band_cases as C
import band_ref as B
import golden_util as G
import track_cases as K
import track_ref as R
from oracle import oracle as O

import kokoro_align_amd as ka

PERIODS = (4, 8, 16, 64)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def same(got, want):
    """path, labels, scores (as bits) and total of two results"""
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(bits(got[2]), bits(want[2])) and
            bits(got[3]) == bits(want[3]))


def assert_properties(lp, labels, beam, mm, period, what, wide=True, best=True):
    """properties 1 - 4 of the issue on one lattice (labels valid, no NaN, beam >= 1)"""
    T, L = lp.shape[0], 2 * len(labels) + 1
    got = R.best_path_tracking(lp, labels, beam, mm, period, return_total=True)   # 4. never a ValueError
    table = got[3]
    # 1. a valid table, constant between multiples of the period
    assert table.dtype == np.int32 and table.shape == (T,) and table[0] == 0, what
    assert table.min() >= 0 and table.max() < L and np.all(np.diff(table) >= 0), what
    assert np.all(np.nonzero(np.diff(table))[0] % period == period - 1), what
    # 2. the round trip
    again = B.best_path_banded(lp, labels, table, beam, mm, return_total=True)
    assert same((got[0], got[1], got[2], got[4]), again), what
    # the "best" end is the banded recurrence's too: same cells, another terminal
    if best:
        got = R.best_path_tracking(lp, labels, beam, mm, period, "best", return_total=True, return_cells=True)
        pos, sc = got[5][-1]
        assert np.array_equal(got[3], table) and got[0][-1] == pos[int(np.argmax(sc))] and bits(got[4]) == bits(sc[int(np.argmax(sc))]), what
    # 3. a band as wide as the lattice: zeros, and the pinned oracle's answer at the same beam
    if wide:
        got = R.best_path_tracking(lp, labels, 2 * L, mm, period, return_total=True)
        assert not got[3].any(), what
        assert same((got[0], got[1], got[2], got[4]), O.ctc_best_path_c(lp, labels, 2 * L, mm, return_total=True)), what


# ---- 1. the properties ----
def test_properties_on_g1():
    n = 0
    for c in G.g1_cases():
        period = PERIODS[n % 4]
        assert_properties(c["lp"], c["labels"], c["beam"], c["max_move"], period, f"g1 case {c['idx']} period {period}")
        n += 1
    assert n >= 100


@pytest.mark.parametrize("idx", range(6))
def test_properties_on_g2(idx):
    c = G.g2_cases()[idx]
    lp = O.hash_logprobs(c["T"], c["V"], c["seed"])
    labels = O.hash_labels(c["S"], c["V"], c["seed"])
    # (the lattice-wide band costs T x L in NumPy: on the two smallest)
    assert_properties(lp, labels, c["beam"], c["max_move"], (16, 64, 4, 8, 16, 64)[idx], f"g2 case {c['idx']}", wide=idx in (1, 4), best=False)


def test_properties_on_200_random_lattices():
    rng = np.random.default_rng(4320)
    n_ninf = n_zero = n_moved = 0
    for k in range(200):
        V = int(rng.integers(2, 12))
        S = int(rng.integers(0, 60))
        T = int(rng.integers(1, 140))
        beam = int(rng.choice([1, 2, 3, 4, 5, 8, 13, 33, 1000]))
        mm = int(rng.integers(2, 6))
        period = int(rng.choice(PERIODS))
        lp = (np.round(rng.standard_normal((T, V)) * 16) / 8).astype(np.float32)   # (eighths: ties)
        if rng.random() < 0.3:
            lp = np.where(rng.random((T, V)) < 0.2, -np.inf, lp).astype(np.float32)
            n_ninf += 1
        labels = rng.integers(0, V, size=S).astype(np.int32)
        n_zero += bool(np.any(labels == 0))
        assert_properties(lp, labels, beam, mm, period, f"random lattice {k}: T={T} S={S} V={V} beam={beam} max_move={mm} period={period}")
        n_moved += bool(R.best_path_tracking(lp, labels, beam, mm, period)[3].any())
    assert n_ninf >= 20 and n_zero >= 50 and n_moved >= 50, (n_ninf, n_zero, n_moved)


# ---- 2. the rescue case, as the issue measured it ----
@pytest.mark.parametrize("seed", range(6))
def test_rescue_case(seed):
    lp, labels, L, beam, pre = C.rescue(seed)
    T = lp.shape[0]
    full = B.best_path_banded(lp, labels, np.zeros(T, np.int64), 2 * L, 4, return_total=True)
    assert full[3] == np.float32(-30.0)
    for period in (4, 8):
        got = R.best_path_tracking(lp, labels, beam, 4, period, return_total=True)
        assert same((got[0], got[1], got[2], got[4]), full), period
        assert same(B.best_path_banded(lp, labels, got[3], beam, 4, return_total=True), full), period
    diag = B.best_path_banded(lp, labels, ka.diagonal_band(T, L, beam), beam, 4)
    assert int(np.sum(diag[0] != full[0])) > 100
    lost = R.best_path_tracking(lp, labels, beam, 4, 16, return_total=True)   # 16 frames x 0.83 positions > beam / 2
    assert int(np.sum(lost[0] != full[0])) > 100 and lost[4] < -150


# ---- 3. the inputs of the GPU families do what their names say ----
def test_every_case_has_an_answer_and_a_valid_table():
    for name in K.NAMES:
        lp, lab, beam, mm, period, end_rule = K.case(name)
        w = K.want(name)
        assert w is not None, name
        L = 2 * len(lab) + 1
        assert w[3][0] == 0 and w[3].max() < L and np.all(np.diff(w[3]) >= 0), name
        assert np.all(np.nonzero(np.diff(w[3]))[0] % period == period - 1), name


def test_step_cases_move_by_their_step():
    for name, (step, at) in K.STEP_OF.items():
        lp, lab, beam, mm, period, end_rule = K.case(name)
        table, cells = K.want(name)[3], K.want(name)[5]
        assert at == period and period <= lp.shape[0] - 1 < 2 * period   # one retarget
        moves = np.nonzero(np.diff(table))[0]
        assert (moves.tolist() == [at - 1] and table[at] == step) if step else moves.size == 0, name
        pos, sc = cells[at - 2]
        assert pos[int(np.argmax(sc))] == beam // 2 + step, name
    # no single retarget moves further than the arg-max cell allows: 504 is the most a band of 1009 can do, with the arg-max in
    # its top cell; 31 blocks of 16 pass the low end
    lp, lab, beam, mm, period, end_rule = K.case("step504")
    assert beam == 1009 and K.STEP_OF["step504"][0] == beam - 1 - beam // 2 and (504 >> 4) == 31
    assert K.STEP_OF["step70"][0] >= 64 and K.STEP_OF["step16"][0] == 16


def test_tie_and_ninf_cases_are_what_they_say():
    lp, lab, beam, mm, period, end_rule = K.case("tie")
    for t in range(period, lp.shape[0], period):
        pos, sc = K.want("tie")[5][t - 2]
        assert pos.size > 8 and np.all(sc == sc[0]) and pos[0] == 0
    assert not K.want("tie")[3].any()
    # two cells tie for the maximum, two positions apart, and the lower one steers
    for name in ("step16", "step70"):
        lp, lab, beam, mm, period, end_rule = K.case(name)
        pos, sc = K.want(name)[5][period - 2]
        top = beam // 2 + K.STEP_OF[name][0]
        assert pos[sc == sc.max()].tolist() == [top, top + 2] and K.want(name)[3][period] == top - beam // 2
    for name in ("ninf_list", "ninf_list_best"):
        pos, sc = K.want(name)[5][14]
        assert pos.tolist() == [7, 9, 10, 11] and np.all(np.isneginf(sc)) and K.want(name)[3][15] == 6   # lo itself is dead
        pos, sc = K.want(name)[5][-1]
        assert pos[0] == 7 and np.all(np.isneginf(sc))
    assert K.want("ninf_list")[0][-1] == 11 and K.want("ninf_list_best")[0][-1] == 7


def test_forms_and_edges_of_the_cases():
    fast = lambda lp, lab, beam, mm: lp.shape[1] <= 64 and mm <= 4 and min(beam, 2 * len(lab) + 1) <= 1009   # noqa: E731
    for name in K.NAMES:
        lp, lab, beam, mm, period, end_rule = K.case(name)
        assert fast(lp, lab, beam, mm) != name.startswith("gen_"), name
    assert K.case("gen_V65")[0].shape[1] == 65 and K.case("gen_mm5")[3] == 5 and K.case("gen_band1010")[2] == 1010
    assert K.want("gen_band1010")[3][-1] == 504
    for name, T in (("T1", 1), ("T2", 2), ("T3", 3), ("T5", 5)):
        assert K.case(name)[0].shape[0] == T
    assert K.case("T3")[0].shape[0] < K.case("T3")[4] and K.case("T9_p8")[0].shape[0] == 9
    assert len(K.case("S0")[1]) == 0 and K.case("beam1")[2] == 1
    lp, lab, beam, mm, period, end_rule = K.case("beam_ge_2L")
    assert beam >= 2 * (2 * len(lab) + 1)
    assert {K.case(n)[3] for n in ("mm1", "mm2", "mm3", "mm4_best")} == {1, 2, 3, 4}
    # the ring case's band passes slot 1023 -> 0
    lo = K.want("wrap")[3].astype(np.int64)
    assert np.any((lo < 1023) & (lo + K.case("wrap")[2] > 1024))
    # the two end rules differ where the audio ends early
    assert K.want("short_best")[0][-1] == 41 and K.want("short_highest")[0][-1] > 41
    assert np.array_equal(K.want("short_best")[3], K.want("short_highest")[3])


# ---- 4. six planted faults: each changes a result on some case ----
@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_changes_a_result(fault):
    changed = []
    for name in K.NAMES:
        lp, lab, beam, mm, period, end_rule = K.case(name)
        w = K.want(name)
        try:
            got = R.best_path_tracking(lp, lab, beam, mm, period, end_rule, fault=fault, return_total=True)
        except ValueError:
            got = None
        if got is None or not (same((got[0], got[1], got[2], got[4]), (w[0], w[1], w[2], w[4])) and np.array_equal(got[3], w[3])):
            changed.append(name)
    assert changed, fault


# ---- 5. the boundary ----
def test_symbols_and_argument_checks():
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    for name in ("ka_ctc_best_path_tracking_f32", "ka_ctc_best_path_tracking_batch_f32", "ka_tracking_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    header = open(os.path.join(ROOT, "include", "kokoro_align_amd.h")).read()
    assert re.search(r"int ka_ctc_best_path_tracking_batch_f32\(", header)
    # the workspace: the banded call's without the copy of the table in the one-wavefront form, the same in the generic form
    Ts, Ss = (ctypes.c_int64 * 1)(4001), (ctypes.c_int64 * 1)(700)
    for mem in (_lib.KA_MEM_HOST, _lib.KA_MEM_DEVICE):
        fast_t, fast_b = L.ka_tracking_workspace_bytes(1, Ts, Ss, 39, 300, 4, mem), L.ka_banded_workspace_bytes(1, Ts, Ss, 39, 300, 4, mem)
        assert 0 < fast_t <= fast_b - 4004 * 4
        gen_t, gen_b = L.ka_tracking_workspace_bytes(1, Ts, Ss, 39, 300, 5, mem), L.ka_banded_workspace_bytes(1, Ts, Ss, 39, 300, 5, mem)
        assert 0 < gen_t == gen_b
    H = _lib.KA_MEM_HOST
    assert L.ka_tracking_workspace_bytes(1, Ts, Ss, 39, 300, 300, H) == 0 and L.ka_tracking_workspace_bytes(1, Ts, Ss, 39, 300, 4, 7) == 0
    assert L.ka_tracking_workspace_bytes(-1, Ts, Ss, 39, 300, 4, H) == 0 and L.ka_tracking_workspace_bytes(1, None, Ss, 39, 300, 4, H) == 0
