"""forward_ck's four-row block path with two frames per emission gather.  A lattice with V = 64 and
contiguous rows (ld == 64) takes it; its label cells then fetch the emissions of frames 2p and 2p + 1 with one 8-byte LDS read,
requested in the odd frame before.  What can go wrong is a matter of where a frame falls: the last frame inside a pair, a block
of four rows or a 32-frame chunk (a half-used last pair reads a row past T - 1), and the parity of the frame after which a lane
is re-labelled (after an even frame the pair still owes its second half, after an odd frame both).  Transcripts that hold a
label 0 run the other instance of the kernel, which reads the same LDS image one frame at a time.

Every output is compared as bits with the C oracle, every in-band cell of every checkpoint row with the float32 reference of
tests/pbt_ref.py (the helpers of test_forward_checkpoints_gpu.py).  All inputs come from the oracle's hash generators.
"""
import functools

import numpy as np
import pytest

import pbt_ref as P
import test_forward_checkpoints_gpu as C
from oracle import oracle as O

V, MAX_MOVE = 64, 4
# (T, S, beam): the last frame at every place of a pair, a block and a chunk
SHORT = [(T, 3, 1000) for T in (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 65)]
# L = 1201 > 1024, so lo crosses 16-position block boundaries and lanes are re-labelled: with the band moving about every half
# frame (602), every 2-3 frames (3001) and every fifth frame, cfg2's rhythm (6007).  At T = 601 and T = 6005 every re-labelling
# falls on one parity of the frame (lo is then 2 t - 501 and t // 5 - 500 nearly throughout: T = 600, 6004 and 6006 likewise);
# these are the nearest T above that have both (the first test below), 6007 odd like 6005.
RELABEL = [(602, 600, 1000), (3001, 600, 1000), (6007, 600, 1000)]
STATIC = [(257, 40, 1000)]      # L < beam: the band never moves, periodic mask only
SHAPES = SHORT + RELABEL + STATIC


def relabel_frames(T, S, beam):
    """Frames t after which lanes are re-labelled: lo >> 4 of frame t + 1 differs from that of frame t."""
    lo, _ = P.band(T, 2 * S + 1, beam)
    return np.nonzero((lo[1:] >> 4) != (lo[:-1] >> 4))[0]


@functools.lru_cache(maxsize=None)
def case(T, S, beam, zero):
    """(lp, labels, oracle outputs, reference with checkpoint rows); computed once, never written to."""
    seed = 7000 + T
    lp = O.hash_logprobs(T, V, seed)
    lab = O.hash_labels(S, V, seed)
    if zero:
        lab = lab.copy()
        lab[1::3] = 0
    assert lp.shape == (T, V) and lp.strides == (4 * V, 4) and lp.dtype == np.float32      # ld == 64: the block path
    want = O.ctc_best_path_c(lp, lab, beam, MAX_MOVE, return_total=True)
    ref = P.best_path_with_moves(lp, lab, beam, MAX_MOVE, maps=False)
    assert np.array_equal(ref.path, want[0]) and np.float32(ref.total).view(np.int32) == want[3].view(np.int32)
    lp.setflags(write=False)
    lab.setflags(write=False)
    return lp, lab, want, ref


@pytest.mark.parametrize("T,S,beam", RELABEL)
def test_lanes_are_relabelled_after_even_and_after_odd_frames(T, S, beam):
    """A property of the inputs: both parities of the re-labelling frame occur (the re-gather differs between them)."""
    t = relabel_frames(T, S, beam)
    assert np.any(t % 2 == 0) and np.any(t % 2 == 1), (T, S, t[:8])
    assert 2 * S + 1 > P.WAVE_RING


def test_the_static_case_never_moves_its_band():
    for T, S, beam in STATIC:
        lo, hi = P.band(T, 2 * S + 1, beam)
        assert not lo.any() and np.all(hi == 2 * S + 1)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def check_outputs(res, status, total, want, what):
    assert int(status) == 0, what
    for got, w, name in zip(res, want[:3], ("path", "best_labels", "best_scores")):
        assert same_bits(got, w), f"{what}: {name} differs"
    assert np.float32(total).view(np.int32) == want[3].view(np.int32), f"{what}: total {total!r}, want {want[3]!r}"


@pytest.mark.gpu
@pytest.mark.parametrize("T,S,beam", SHAPES)
def test_outputs_and_checkpoint_rows_bit_for_bit(T, S, beam):
    import torch
    assert torch.cuda.is_available()
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    eng = _lib.default_engine(torch.cuda.current_device())
    eng.set_mode("wave")
    eng.set_tile_width(0)
    eng.set_backtrace("serial")
    try:
        plain, zero = case(T, S, beam, False), case(T, S, beam, True)
        # both instances of the kernel beside each other in one launch
        res, status, total = ka.ctc_best_path_batch([plain[0], zero[0]], [plain[1], zero[1]], beam, MAX_MOVE, return_status=True)
        check_outputs(res[0], status[0], total[0], plain[2], f"T={T} S={S}, launch of two")
        check_outputs(res[1], status[1], total[1], zero[2], f"T={T} S={S} with label 0, launch of two")
        # each alone: outputs again and every in-band cell of its checkpoint rows
        for (lp, lab, want, ref), what in ((plain, "alone"), (zero, "with label 0, alone")):
            res, status, total = ka.ctc_best_path_batch([lp], [lab], beam, MAX_MOVE, return_status=True)
            check_outputs(res[0], status[0], total[0], want, f"T={T} S={S} {what}")
            assert len(ref.rows) == (T - 1) // P.CK
            img, R = C.check(eng, "wave", f"T={T} S={S}", ref, what)
            C.check_dead_slots(f"T={T} S={S}", ref, img, R, what)
    finally:
        eng.set_mode("auto")
        eng.set_backtrace("auto")
        eng.set_tile_width(0)
