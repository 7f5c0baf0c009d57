"""State posteriors at chosen frames, CPU side: the C-ABI / Python boundary of the feature (no compute: there is no GPU), the
host-only boundary confidence of align()'s text boundaries on hand-built posteriors, and the float64 reference's gamma
against the occupancy and path-posterior references it must agree with."""
import ctypes
import re

import numpy as np
import pytest

import occupancy_ref as Q
import posterior_ref as R
from fb_harness import assert_declared_exported_bound, header_text
from oracle import oracle as O

NEW_SYMBOLS = ("ka_ctc_state_posteriors_f32", "ka_ctc_state_posteriors_batch_f32", "ka_state_posterior_workspace_bytes")


def test_new_symbols_declared_exported_and_bound():
    assert_declared_exported_bound(NEW_SYMBOLS)


def test_version_is_104():
    from kokoro_align_amd import _lib
    assert _lib.load_library().ka_version() == 104
    assert int(re.search(r"#define KA_VERSION (\d+)", header_text()).group(1)) == 104


def _ws(n, T, S, K, V=64, beam=1000, mm=4, mem=1):
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    arr = lambda v: (ctypes.c_int64 * n)(*[v] * n)
    return L.ka_state_posterior_workspace_bytes(n, arr(T), arr(S), arr(K), V, beam, mm, mem)


def test_workspace_bytes_unsupported_shapes_are_zero():
    assert _ws(2, 5000, 500, 10, mm=300) == 0          # max_move above 255
    assert _ws(2, 5000, 500, -1) == 0                  # a negative frame count
    assert _ws(2, 100, 50, 101) == 0                   # more frames than the lattice has
    assert _ws(2, 0, 50, 0) == 0                       # no frames at all
    assert _ws(2, 5000, 500, 10, mem=7) == 0           # no such memory mode
    assert _ws(1, 5000, 500, 0) > 0                    # K = 0 is legal


def test_workspace_is_bounded_by_resident_slots_for_8192_cfg2():
    big = _ws(8192, 50000, 5000, 200)
    assert 0 < big <= 16 << 30
    # beyond the resident slots only descriptors and frame lists grow
    assert _ws(2048, 50000, 5000, 200) - _ws(1024, 50000, 5000, 200) < (1 << 20) + 1024 * 2048   # (a lattice: 200 frames, 1792 B aligned)
    one = _ws(1, 50000, 5000, 200)
    assert one >= (50000 // 32) * 1024 * 8             # the checkpointed columns
    assert one < 64 << 20                              # ... and no alpha lattice
    # host buffers: the staged log-probs and labels, the gamma rows and band_lo
    assert _ws(1, 50000, 5000, 200, mem=0) >= one + 50000 * 64 * 4 + 200 * 1000 * 4 + 200 * 8
    # the same slots as the label posteriors
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    occ = L.ka_label_posterior_workspace_bytes(1, (ctypes.c_int64 * 1)(50000), (ctypes.c_int64 * 1)(5000), 64, 1000, 4, 1)
    assert abs(one - occ) < 1 << 20


def test_public_api_exists():
    import kokoro_align_amd as ka
    for name in ("ctc_state_posteriors", "ctc_state_posteriors_batch", "ctc_state_posteriors_device", "boundary_frames",
                 "segment_boundary_confidence"):
        assert callable(getattr(ka, name)), name


def test_boundary_frames():
    import kokoro_align_amd as ka
    got = ka.boundary_frames(np.array([40, 12, 12, 90, 100, 130]), 100)
    assert got.dtype == np.int64 and got.tolist() == [0, 12, 40, 90]
    assert ka.boundary_frames([], 10).tolist() == [0]
    assert ka.boundary_frames([0, 5], 10).tolist() == [0, 5]


def _onehot_rows(T, frames, states, W, lo):
    g = np.zeros((len(frames), W), np.float32)
    for k, s in enumerate(states):
        g[k, s - lo[k]] = 1.0
    return g


def test_boundary_confidence_one_hot_rows_give_one():
    import kokoro_align_amd as ka
    T, n_ph = 20, 6
    path = np.minimum(np.arange(T) // 2, 12)           # states 0..9
    seg_ends = np.array([5, 11, 30])
    frames = ka.boundary_frames(seg_ends, T)             # [0, 5, 11]
    lo = np.array([0, 1, 3], np.int64)
    gamma = _onehot_rows(T, frames, path[frames], 8, lo)
    p_start, p_end = ka.segment_boundary_confidence(gamma, lo, frames, path, seg_ends, n_ph)
    assert p_start.dtype == np.float64 and p_end.dtype == np.float64
    assert p_start.tolist() == [1.0, 1.0, 1.0] and p_end.tolist() == [1.0, 1.0, 1.0]


def test_boundary_confidence_split_mass_and_the_text_index_map():
    import kokoro_align_amd as ka
    path = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9])      # T = 10
    frames = np.array([0, 4, 8], np.int64)
    lo = np.array([0, 2, 6], np.int64)
    W = 6
    gamma = np.zeros((3, W), np.float32)
    gamma[0, :3] = [0.5, 0.25, 0.25]                     # states 0, 1 (text 0) and 2 (text 1); path[0] = 0: text 0
    gamma[1, :4] = [0.125, 0.125, 0.5, 0.25]             # states 2, 3 (text 1), 4 (text 2), 5 (text 2); path[4] = 4: text 2
    gamma[2, :4] = [0.1, 0.2, 0.3, 0.4]                  # states 6, 7 (text 3), 8, 9 (text 4 -> clipped to n_ph = 3)
    p_start, p_end = ka.segment_boundary_confidence(gamma, lo, frames, path, [4, 8], n_phonemes=3)
    np.testing.assert_allclose(p_start, [0.75, 0.75])
    # segment 0 ends at 4 (text 2: 0.75); segment 1 ends at 8: path[8] // 2 = 4, clipped to 3 -> every state of text >= 3
    np.testing.assert_allclose(p_end, [0.75, 1.0])
    p_start, p_end = ka.segment_boundary_confidence(gamma, lo, frames, path, [4, 8], n_phonemes=4)
    np.testing.assert_allclose(p_end, [0.75, 0.7], rtol=1e-6)   # unclipped: text 4 is states 8 and 9


def test_boundary_confidence_end_past_the_frames_is_one():
    import kokoro_align_amd as ka
    path = np.arange(10)
    frames = np.array([0, 6], np.int64)
    lo = np.array([0, 4], np.int64)
    gamma = np.full((2, 4), 0.25, np.float32)
    p_start, p_end = ka.segment_boundary_confidence(gamma, lo, frames, path, [6, 10], 5)
    assert p_end[1] == 1.0
    assert ka.segment_boundary_confidence(gamma, lo, frames, path, [6, 25], 5)[1][1] == 1.0
    assert p_start[0] == pytest.approx(0.5) and p_end[0] == pytest.approx(0.5)


def test_boundary_confidence_missing_frame_raises():
    import kokoro_align_amd as ka
    path = np.arange(10)
    frames = np.array([0, 6], np.int64)
    gamma = np.full((2, 4), 0.25, np.float32)
    with pytest.raises(ValueError):
        ka.segment_boundary_confidence(gamma, np.array([0, 4]), frames, path, [5, 10], 5)


def test_reference_gamma_sums_to_the_occupancy_and_holds_the_path_posterior():
    rng = np.random.default_rng(17)
    for T, S, V, beam, mm in [(60, 20, 9, 12, 4), (50, 15, 6, 1000, 3), (45, 12, 12, 8, 6), (40, 10, 5, 1000, 2)]:
        lp = np.log(rng.dirichlet(np.ones(V), size=T)).astype(np.float32)
        labels = rng.integers(1, V, size=S).astype(np.int32)
        labels[::5] = 0
        lp[rng.integers(0, T), rng.integers(0, V)] = -np.inf
        path = O.ctc_best_path_c(lp, labels, beam, mm)[0]
        s = int(path[-1])
        ref = R.forward_backward(lp, labels, np.full(T, s), beam, mm, full=True)
        assert ref["status"] == R.OK
        lab = R.expand(labels)
        occ = Q.occupancy(lp, labels, s, beam, mm)["occ"]
        post = R.forward_backward(lp, labels, path, beam, mm)["post"]
        lo_w, hi_w = R.windows(T, len(lab), beam)
        for t, (lo, g) in enumerate(ref["gamma"]):
            assert lo == lo_w[t] and len(g) == hi_w[t] - lo_w[t]
            row = np.zeros(V)
            np.add.at(row, lab[lo:lo + len(g)], g)
            assert np.max(np.abs(row - occ[t])) < 1e-12
            assert abs(g.sum() - 1.0) < 1e-9
            if lo <= path[t] < lo + len(g):
                assert abs(g[path[t] - lo] - post[t]) < 1e-12


def test_state_posteriors_without_a_gpu_is_a_loud_error():
    """No device: the call raises, never a silent CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import kokoro_align_amd as ka
    lp = np.log(np.full((4, 3), 1 / 3, np.float32))
    with pytest.raises((ka.KAError, ValueError)):
        ka.ctc_state_posteriors(lp, np.array([1], np.int32), 2, [0, 3])


def test_bad_frames_raise_before_any_call():
    import kokoro_align_amd as ka
    lp = np.log(np.full((4, 3), 1 / 3, np.float32))
    for frames in ([2, 1], [1, 1], [0, 4], [-1, 2]):
        with pytest.raises(ValueError):
            ka.ctc_state_posteriors(lp, np.array([1], np.int32), 2, frames)
