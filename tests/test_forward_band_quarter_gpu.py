"""forward_ck's mask behind a band step: the first frame of a new band masks only the quarter of a lane's
sixteen cells that holds the position which left on the lo side, lo_old & 15, where lo went one further; every other band
change masks all sixteen as before.  What can go wrong is a matter of which cell that is (every value of lo & 15, the quarter
boundaries 3 -> 4, 7 -> 8, 11 -> 12, the halo cells 13..15, and 15 -> 0 with its re-labelled lane), of how often the band steps
(every frame, every second, every fifth: cfg2's rhythm) and of what else falls on that frame (a checkpoint, the last frame, each
place in the loop's eight frames).  Lattices whose band moves by more than one position or too rarely for the steps to bound
the leaks keep the full passes and are here to show that they still do.

Every case states, from the band arithmetic of tests/pbt_ref.py, that it produces the situation it is named for.  Outputs are
compared as bits with the C oracle, every in-band cell of every checkpoint row with the float32 reference (the harness of
test_forward_pair_gather_gpu.py and test_forward_checkpoints_gpu.py).  V = 64 with contiguous rows takes the block path, V = 39
the row-by-row path; a transcript with a label 0 runs the other instance of the kernel, both beside each other in one launch.

lo clamped at 0 "while hi moves" does not exist: hi = min(lo + beam, L) is a function of lo.  What exists is floor(L t / T)
moving while the band stays, and the first frames of every case here are that.
"""
import functools

import numpy as np
import pytest

import pbt_ref as P
import test_forward_checkpoints_gpu as C
import test_forward_pair_gather_gpu as G
from oracle import oracle as O

MAX_MOVE = 4


def _ends_behind_a_step(S, beam, around):
    """The T nearest `around` whose last frame is the first frame of a new band."""
    for T in sorted(range(around - 20, around + 21), key=lambda x: abs(x - around)):
        lo, _ = P.band(T, 2 * S + 1, beam)
        if lo[T - 1] == lo[T - 2] + 1:
            return T
    raise AssertionError("no such T")


T_END = _ends_behind_a_step(100, 40, 300)
# name -> (T, S, beam)
SHAPES = {
    "every_5th": (1000, 100, 40),
    "every_2nd": (400, 100, 24),
    "every_frame": (201, 100, 24),
    "by_two": (150, 150, 30),
    "slow": (400, 20, 16),
    "ends_behind_step": (T_END, 100, 40),
}
SHAPES.update({f"T_mod_8_is_{T % 8}": (T, 100, 40) for T in range(600, 608)})


def steps(T, S, beam):
    """(frames t after which lo moves, by how much, lo & 15 of the position that leaves, lo, hi)"""
    lo, hi = P.band(T, 2 * S + 1, beam)
    t = np.nonzero(lo[1:] != lo[:-1])[0]
    return t, lo[t + 1] - lo[t], lo[t] & 15, lo, hi


def steps_mask(T, S, beam):
    """forward_ck_body's own rule: the band steps often enough for the steps' masks to bound the leaks."""
    L = 2 * S + 1
    period = 8 if P.WAVE_RING - min(beam, L) >= 8 * (MAX_MOVE - 1) else 4
    return L // T != 0 or (period - 1) * (L % T) >= T


def test_the_cases_are_what_their_names_say():
    for name, gaps in (("every_5th", {4, 5}), ("every_2nd", {1, 2}), ("every_frame", {1})):
        t, by, left, lo, hi = steps(*SHAPES[name])
        assert set(by) == {1} and set(np.diff(t)) == gaps and steps_mask(*SHAPES[name]), name
        assert set(left) == set(range(16)), name                       # every cell, the quarter boundaries and the halos among them
        # 15 -> 0 re-labels a lane: lo >> 4 moves
        assert np.any((left == 15) & ((lo[t + 1] >> 4) != (lo[t] >> 4))), name
        # floor(L t / T) moves while lo is still 0: the band, hi included, stays
        L, T = 2 * SHAPES[name][1] + 1, SHAPES[name][0]
        early = np.nonzero((L * np.arange(1, t[0]) // T) != (L * np.arange(t[0] - 1) // T))[0]
        assert early.size >= 5 and not lo[:t[0] + 1].any() and np.all(hi[:t[0] + 1] == hi[0]), name
        # hi stays at L while lo moves on
        late = t[hi[t] == L]
        assert late.size >= 5 and np.all(hi[late + 1] == L), name
    t, by, left, lo, hi = steps(*SHAPES["every_5th"])
    assert np.any((t + 1) % P.CK == P.CK - 1)                           # the first frame of a new band is a checkpoint frame
    assert {int(x) for x in (t + 1) % 8} == set(range(8))               # ... and every one of the loop's eight frames
    t, by, left, lo, hi = steps(*SHAPES["by_two"])
    assert 2 in set(by) and SHAPES["by_two"][1] * 2 + 1 >= 2 * SHAPES["by_two"][0]
    t, by, left, lo, hi = steps(*SHAPES["slow"])
    assert not steps_mask(*SHAPES["slow"]) and set(by) == {1} and np.diff(t).min() > 8
    T, S, beam = SHAPES["ends_behind_step"]
    t, by, left, lo, hi = steps(T, S, beam)
    assert t[-1] + 1 == T - 1 and by[-1] == 1
    assert sorted(SHAPES[f"T_mod_8_is_{r}"][0] % 8 for r in range(8)) == list(range(8))


@functools.lru_cache(maxsize=None)
def case(name, V, zero):
    """(lp, labels, oracle outputs, reference with checkpoint rows); computed once, never written to."""
    T, S, beam = SHAPES[name]
    seed = 9000 + T + V
    lp = O.hash_logprobs(T, V, seed)
    lab = O.hash_labels(S, V, seed)
    if zero:
        lab = lab.copy()
        lab[1::3] = 0
    assert lp.shape == (T, V) and lp.strides == (4 * V, 4) and lp.dtype == np.float32      # ld == V: 64 takes the block path
    want = O.ctc_best_path_c(lp, lab, beam, MAX_MOVE, return_total=True)
    ref = P.best_path_with_moves(lp, lab, beam, MAX_MOVE, maps=False)
    assert np.array_equal(ref.path, want[0]) and np.float32(ref.total).view(np.int32) == want[3].view(np.int32)
    lp.setflags(write=False)
    lab.setflags(write=False)
    return lp, lab, want, ref


@pytest.mark.gpu
@pytest.mark.parametrize("V", [64, 39])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_outputs_and_checkpoint_rows_bit_for_bit(name, V):
    import torch
    assert torch.cuda.is_available()
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    T, S, beam = SHAPES[name]
    eng = _lib.default_engine(torch.cuda.current_device())
    eng.set_mode("wave")
    eng.set_tile_width(0)
    eng.set_backtrace("serial")
    try:
        plain, zero = case(name, V, False), case(name, V, True)
        # both instances of the kernel beside each other in one launch
        res, status, total = ka.ctc_best_path_batch([plain[0], zero[0]], [plain[1], zero[1]], beam, MAX_MOVE, return_status=True)
        G.check_outputs(res[0], status[0], total[0], plain[2], f"{name} V={V}, launch of two")
        G.check_outputs(res[1], status[1], total[1], zero[2], f"{name} V={V} with label 0, launch of two")
        # each alone: outputs again and every in-band cell of its checkpoint rows
        for (lp, lab, want, ref), what in ((plain, "alone"), (zero, "with label 0, alone")):
            res, status, total = ka.ctc_best_path_batch([lp], [lab], beam, MAX_MOVE, return_status=True)
            G.check_outputs(res[0], status[0], total[0], want, f"{name} V={V} {what}")
            assert len(ref.rows) == (T - 1) // P.CK
            img, R = C.check(eng, "wave", f"{name} V={V}", ref, what)
            C.check_dead_slots(f"{name} V={V}", ref, img, R, what)
    finally:
        eng.set_mode("auto")
        eng.set_backtrace("auto")
        eng.set_tile_width(0)
