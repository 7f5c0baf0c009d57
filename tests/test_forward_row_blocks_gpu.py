"""The two ways log-prob rows reach forward_ck's frame loop (ka_wave_forward.hpp), and the frames on
which it applies the band mask.

A lattice with V = 64, ld = 64 and a 16-byte aligned base takes its rows in blocks of four: one 16-byte load per lane per four
frames, LDS double-buffered as [2][4][64], the blank emissions read from the block's registers, rows past T - 1 delivered as
zeros by the buffer descriptor's range check.  Every other lattice goes row by row as before.  So the cases are about WHERE a
block ends and WHO is eligible:

  residues   T = 1 .. 100 with last blocks of 1, 2 and 3 rows, T below one block, block ends on checkpoint frames (32, 64)
  relabel    beam 32 over L = 601 (T = 400 and 397): lanes are re-labelled - and regather from the row of the block that
             holds frame t + 1 - with frame t + 1 at every row of both LDS buffers
  steps      a 1000-wide band over L = 1201 with floor(L t / T) moving every k-th frame, k = 1 .. 9: up to k = 7 the band steps
             often enough that the periodic mask pass is dropped (checkpoint frames keep theirs), k = 8 and 9 keep it
  mixed      in one launch of V = 64 lattices: eligible ones beside a view with ld = 80, a view whose base is only 4-byte
             aligned and a transcript with label 0 (the other kernel instance); V = 39 lattices with ld = 39 and with ld = 64
             (NaN in the padding columns) in a launch of their own - one launch has one V
  nonfinite  -inf and NaN in the last row of a partial block; NaN behind row T - 1 in the same allocation

Each case runs through the checkpointed one-wavefront form; path, labels, scores and total are compared with the C oracle bit
for bit.  The tests without the gpu mark assert from the oracle and from the band formula that the cases do what their names
say; they need no GPU.
"""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O

V = 64
MM = 4
RESIDUE_T = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 36, 63, 64, 65, 100)
RELABEL_BEAM = 32
RELABEL = {400: (400, 300, 61), 397: (397, 300, 62)}      # T: (T, S, seed)
STEP_S, STEP_BEAM, STEP_SEED = 600, 1000, 71      # seed 71: the first one tried (see test_step_cases_...)
STEP_K = tuple(range(1, 10))


@functools.lru_cache(maxsize=None)
def lattice(T, S, seed, v=V, zero=None):
    lp = O.hash_logprobs(T, v, seed)
    lab = O.hash_labels(S, v, seed)
    if zero:
        lab = np.where(np.arange(S) % zero == 1, 0, lab).astype(np.int32)
    lp.setflags(write=False)
    lab.setflags(write=False)
    return lp, lab


@functools.lru_cache(maxsize=None)
def want(T, S, seed, beam, v=V, zero=None):
    lp, lab = lattice(T, S, seed, v, zero)
    return O.ctc_best_path_c(lp, lab, beam, MM, return_total=True)


def residue_case(T):
    return T, min(T, 5), 100 + T


def step_case(k):
    return k * (2 * STEP_S + 1), STEP_S, STEP_SEED + k


def band(T, L, beam):
    """lo[t], hi[t] of align.py:64-65"""
    t = np.arange(T, dtype=np.int64)
    lo = np.maximum(L * t // T - beam // 2, 0)
    hi = np.where(L - lo < beam, L, lo + beam)
    return lo, hi


def drops_periodic_mask(T, L, beam, max_move=MM):
    """forward_ck's condition, restated: the periodic pass runs every P = 8 frames when the ring of 1024 slots has at least
    8 (max_move - 1) dead ones, else every 4; it is dropped when floor(L t / T) moves at least every P - 1 frames."""
    P = 8 if 1024 - min(beam, L) >= 8 * (max_move - 1) else 4
    return L // T >= 1 or (P - 1) * (L % T) >= T


# ---- the cases do what their names say (no GPU) ----
def test_residue_cases_cover_every_last_block_and_both_sides_of_a_checkpoint():
    assert {T % 4 for T in RESIDUE_T} == {0, 1, 2, 3}
    assert {1, 2, 3} <= set(RESIDUE_T)                       # below one block
    assert {31, 32, 33, 63, 64, 65} <= set(RESIDUE_T)        # a block ends on the checkpoint frames 31 and 63
    assert any(T % 8 == 4 for T in RESIDUE_T)                # the eight-frame loop ends after its first block
    for T in RESIDUE_T:
        _, S, seed = residue_case(T)
        assert len(want(T, S, seed, 1000)[0]) == T


def test_relabel_cases_regather_from_every_row_of_both_buffers():
    phases = {}
    for T, S, seed in RELABEL.values():
        lo, _ = band(T, 2 * S + 1, RELABEL_BEAM)
        crossed = np.nonzero((lo[1:] >> 4) != (lo[:-1] >> 4))[0] + 1  # frames t + 1 whose band starts in a new block of 16
        assert len(crossed) >= 30
        assert {int(t) % 4 for t in crossed - 1} == {0, 1, 2, 3}      # the frame t in which the lanes are re-labelled
        assert {int(t) % 4 for t in crossed} == {0, 1, 2, 3}          # frame t + 1: row (t + 1) % 4 ..
        assert {int(t) // 4 % 2 for t in crossed} == {0, 1}           # .. of buffer ((t + 1) / 4) % 2
        phases[T] = {int(t) % 8 for t in crossed}
        assert want(T, S, seed, RELABEL_BEAM)[0][-1] > 400            # the path follows the band up
    assert phases[397] == set(range(8))                               # T = 397: every row of each buffer (T = 400: four of eight)


def test_step_cases_drop_the_periodic_mask_up_to_k_7_and_touch_the_high_edge():
    L = 2 * STEP_S + 1
    assert L == 1201 and 1024 - STEP_BEAM == 8 * (MM - 1)             # the ring's gap is just wide enough for eight frames
    assert [drops_periodic_mask(step_case(k)[0], L, STEP_BEAM) for k in STEP_K] == [True] * 7 + [False] * 2
    for k in STEP_K:
        T, S, seed = step_case(k)
        lo, hi = band(T, L, STEP_BEAM)
        moves = np.nonzero(np.diff(L * np.arange(T, dtype=np.int64) // T))[0]
        assert np.diff(moves).max() == k and hi.max() - hi.min() > 150    # a band step every k-th frame; hi travels
        if k <= 7:
            path = want(T, S, seed, STEP_BEAM)[0]
            assert (hi - 1 - path).min() <= 3, k                      # (seed 71 + k; the contact is in the closing frames)


def test_mixed_cases_are_what_they_say():
    assert (lattice(130, 70, 82, V, 4)[1] == 0).any()
    assert not (lattice(130, 70, 81)[1] == 0).any()


# ---- the kernels ----
@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    assert os.path.exists(ka.library_path()), "HIP library not built"
    eng = _lib.default_engine(torch.cuda.current_device())
    eng.set_mode("wave")
    eng.set_backtrace("serial")
    eng.set_tile_width(0)
    yield ka, _lib, torch
    eng.set_mode("auto")
    eng.set_backtrace("auto")


def run(env, lps, labs, beam):
    """One launch over device tensors as they are (base address and row pitch included): results as arrays, statuses, totals."""
    _, _, torch = env
    from kokoro_align_amd.align import DeviceBatch
    batch = DeviceBatch(lps, [torch.from_numpy(np.array(x, dtype=np.int32)).cuda() for x in labs], beam, MM)
    status = batch.run(raise_on_error=False)
    res = [tuple(x.cpu().numpy() for x in r) for r in batch.results()]
    return res, list(status), batch.total.copy()


def differs(got, total, w):
    path, labels, scores, wtotal = w[:4]
    for g, x, field in zip(got, (path, labels, scores), ("path", "labels", "scores")):
        if g.shape != x.shape:
            return f"{field} has shape {g.shape}"
        bad = np.nonzero(g.view(np.int32) != x.view(np.int32))[0]
        if bad.size:
            t = int(bad[0])
            return f"{field} differs at {bad.size} frames, first at frame {t} (row {t % 4} of its block): got {g[t]}, want {x[t]}"
    if np.float32(total).view(np.int32) != np.float32(wtotal).view(np.int32):
        return f"total {total!r}, want {wtotal!r}"
    return None


def aligned(torch, lp):
    """a contiguous device copy: torch's allocator hands out addresses that are multiples of 16"""
    x = torch.from_numpy(np.array(lp, dtype=np.float32)).cuda()
    assert x.data_ptr() % 16 == 0 and x.stride(0) == lp.shape[1]
    return x


def view_at(torch, lp, ld, offset, fill=float("nan")):
    """lp as a [T, V] view with row pitch `ld` that starts `offset` floats into a `fill`ed buffer with eight spare rows"""
    T, v = lp.shape
    buf = torch.full((offset + (T + 8) * ld,), fill, dtype=torch.float32, device="cuda")
    x = buf[offset:offset + T * ld].view(T, ld)[:, :v]
    x.copy_(torch.from_numpy(np.array(lp, dtype=np.float32)))
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("T", RESIDUE_T)
def test_last_blocks_of_every_length(env, T):
    _, S, seed = residue_case(T)
    lp, lab = lattice(T, S, seed)
    res, status, total = run(env, [aligned(env[2], lp)], [lab], 1000)
    assert status == [0]
    why = differs(res[0], total[0], want(T, S, seed, 1000))
    assert why is None, f"T={T}: {why}"


@pytest.mark.gpu
def test_all_residues_in_one_launch_from_host_memory(env):
    """the host form: the library's own copies of the rows, whatever their alignment"""
    ka = env[0]
    cases = [residue_case(T) for T in RESIDUE_T]
    res, status, total = ka.ctc_best_path_batch([lattice(*c)[0] for c in cases], [lattice(*c)[1] for c in cases], 1000, MM, return_status=True)
    assert list(status) == [0] * len(cases)
    for i, (T, S, seed) in enumerate(cases):
        why = differs([np.asarray(x) for x in res[i]], total[i], want(T, S, seed, 1000))
        assert why is None, f"T={T}: {why}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RELABEL))
def test_relabelling_at_every_block_phase(env, name):
    T, S, seed = RELABEL[name]
    lp, lab = lattice(T, S, seed)
    res, status, total = run(env, [aligned(env[2], lp)], [lab], RELABEL_BEAM)
    assert status == [0]
    why = differs(res[0], total[0], want(T, S, seed, RELABEL_BEAM))
    assert why is None, why


@pytest.mark.gpu
@pytest.mark.parametrize("k", STEP_K)
def test_band_steps_every_kth_frame(env, k):
    T, S, seed = step_case(k)
    lp, lab = lattice(T, S, seed)
    res, status, total = run(env, [aligned(env[2], lp)], [lab], STEP_BEAM)
    assert status == [0]
    why = differs(res[0], total[0], want(T, S, seed, STEP_BEAM))
    assert why is None, f"k={k}: {why}"


@pytest.mark.gpu
def test_ineligible_lattices_beside_eligible_ones(env):
    torch = env[2]
    specs = [(130, 70, 81, None), (97, 40, 83, None), (130, 70, 82, 4), (65, 20, 84, None), (36, 12, 85, None)]
    lats = [lattice(T, S, seed, V, zero) for T, S, seed, zero in specs]
    lps = [aligned(torch, lats[0][0]),
           view_at(torch, lats[1][0], 80, 0),        # ld = 80
           aligned(torch, lats[2][0]),               # label 0: the other kernel instance
           view_at(torch, lats[3][0], 64, 1),        # base 4 bytes past a multiple of 16
           aligned(torch, lats[4][0])]
    assert lps[1].stride(0) == 80 and lps[3].stride(0) == 64 and lps[3].data_ptr() % 16 == 4
    res, status, total = run(env, lps, [x[1] for x in lats], 1000)
    assert status == [0] * len(specs)
    for i, (T, S, seed, zero) in enumerate(specs):
        why = differs(res[i], total[i], want(T, S, seed, 1000, V, zero))
        assert why is None, f"lattice {i}: {why}"


@pytest.mark.gpu
def test_narrow_vocabulary_with_and_without_padding_columns(env):
    torch = env[2]
    specs = [(130, 70, 91), (97, 40, 92), (33, 9, 93)]
    lats = [lattice(T, S, seed, 39) for T, S, seed in specs]
    lps = [aligned(torch, lats[0][0]), view_at(torch, lats[1][0], 64, 0), view_at(torch, lats[2][0], 64, 0)]
    assert lps[0].stride(0) == 39 and lps[1].stride(0) == 64 and lps[1].data_ptr() % 16 == 0
    res, status, total = run(env, lps, [x[1] for x in lats], 1000)
    assert status == [0] * len(specs)                # the NaN in columns 39 .. 63 is never read
    for i, (T, S, seed) in enumerate(specs):
        why = differs(res[i], total[i], want(T, S, seed, 1000, 39))
        assert why is None, f"lattice {i}: {why}"


@pytest.mark.gpu
def test_non_finite_values_in_and_behind_the_last_partial_block(env):
    _, _lib, torch = env
    T, S, seed = 7, 5, 107                            # rows 4 .. 6 are a last block of three
    lp, lab = lattice(T, S, seed)
    ninf, nan = lp.copy(), lp.copy()
    ninf[T - 1, 9] = -np.inf                          # the lattice goes to the exact kernels: the oracle's result
    nan[T - 1, 63] = np.nan                           # an explicit error
    behind = view_at(torch, lp, 64, 0)                # NaN from row T on, in the same allocation
    assert behind.data_ptr() % 16 == 0 and behind.stride(0) == 64
    res, status, total = run(env, [aligned(torch, ninf), aligned(torch, nan), behind, aligned(torch, lp)], [lab] * 4, 1000)
    assert status == [0, _lib.KA_ERR_NAN, 0, 0]
    w_inf = O.ctc_best_path_c(ninf, lab, 1000, MM, return_total=True)
    for i, w in ((0, w_inf), (2, want(T, S, seed, 1000)), (3, want(T, S, seed, 1000))):
        why = differs(res[i], total[i], w)
        assert why is None, f"lattice {i}: {why}"
