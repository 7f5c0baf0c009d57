"""Best-path posteriors and lattice log-likelihood, CPU side: the float64 reference (tests/posterior_ref.py) against brute-force
path enumeration and its own invariants, and the C-ABI / Python boundary of the feature (no compute: there is no GPU)."""
import ctypes
import re

import numpy as np
import pytest

import posterior_ref as R
from fb_harness import assert_declared_exported_bound, header_text, tiny as _tiny
from oracle import oracle as O

NEW_SYMBOLS = ("ka_ctc_path_posteriors_f32", "ka_ctc_path_posteriors_batch_f32", "ka_posterior_workspace_bytes")


def _some_path(rng, T, L, beam, mm):
    lo, hi = R.windows(T, L, beam)
    return np.array([rng.integers(lo[t], hi[t]) if hi[t] > lo[t] else 0 for t in range(T)], np.int32)


@pytest.mark.parametrize("mm", [1, 2, 3, 4, 5, 6])
def test_reference_matches_brute_force(mm):
    rng = np.random.default_rng(100 + mm)
    checked = 0
    for trial in range(40):
        T = int(rng.integers(1, 7 if mm <= 3 else 6))
        S = int(rng.integers(0, 5))
        V = int(rng.integers(2, 6))
        beam = int(rng.choice([2, 3, 5, 1000]))
        lp, labels = _tiny(rng, T, S, V, zero_label=trial % 3 == 0, ninf=trial % 4 == 1)
        L = 2 * S + 1
        path = _some_path(rng, T, L, beam, mm)
        want_post, want_ll = R.brute_force(lp, labels, path, beam, mm)
        got = R.forward_backward(lp, labels, path, beam, mm)
        if want_ll == -np.inf:
            assert got["status"] == R.ZERO_MASS and got["ll"] == -np.inf
            continue
        assert got["status"] == R.OK
        assert abs(got["ll"] - want_ll) < 1e-9
        np.testing.assert_allclose(got["post"], want_post, atol=1e-12)
        checked += 1
    assert checked >= 10


def test_gamma_sums_to_one_and_last_frame_is_one():
    rng = np.random.default_rng(7)
    for T, S, V, beam, mm in [(40, 12, 8, 10, 4), (30, 9, 5, 1000, 3), (25, 6, 12, 7, 6)]:
        lp, labels = _tiny(rng, T, S, V, zero_label=True)
        path = O.ctc_best_path_c(lp, labels, beam, mm)[0]
        got = R.forward_backward(lp, labels, path, beam, mm, full=True)
        assert got["status"] == R.OK
        assert got["post"][-1] == 1.0
        for lo, g in got["gamma"]:
            assert abs(g.sum() - 1.0) < 1e-9
        assert np.all((got["post"] >= 0) & (got["post"] <= 1 + 1e-12))


def test_likelihood_bounds_the_viterbi_score():
    for T, V, S, beam, mm, seed in [(300, 39, 60, 1000, 4, 1), (200, 12, 40, 16, 4, 2), (150, 64, 50, 20, 2, 3)]:
        lp = O.hash_logprobs(T, V, seed)
        labels = O.hash_labels(S, V, seed)
        path, _, _, total, _ = O.ctc_best_path_c(lp, labels, beam, mm, return_total=True)
        got = R.forward_backward(lp, labels, path, beam, mm)
        assert got["status"] == R.OK
        assert got["ll"] >= float(total) - 1e-3


def test_reference_statuses():
    lp = np.log(np.full((5, 4), 0.25, np.float32))
    labels = np.array([1, 2], np.int32)
    path = np.zeros(5, np.int32)
    assert R.forward_backward(lp, np.array([4], np.int32), path)["status"] == R.BAD_LABEL
    bad = lp.copy()
    bad[2, 1] = np.nan
    assert R.forward_backward(bad, labels, path)["status"] == R.NAN
    bad[2, 1] = np.inf
    assert R.forward_backward(bad, labels, path)["status"] == R.NONFINITE
    assert R.forward_backward(lp, labels, np.full(5, 5, np.int32))["status"] == R.BAD_ARGS
    dead = lp.copy()
    dead[:, 0] = -np.inf                       # the terminal (a blank) is reached only through -inf
    got = R.forward_backward(dead, labels, path)
    assert got["status"] == R.ZERO_MASS and got["ll"] == -np.inf and np.isnan(got["post"]).all()


def test_new_symbols_declared_exported_and_bound():
    from kokoro_align_amd import _lib
    lib = assert_declared_exported_bound(NEW_SYMBOLS)
    assert lib.ka_version() >= 101
    assert _lib.KA_ERR_ZERO_MASS == -9
    assert re.search(r"#define KA_ERR_ZERO_MASS \(-9\)", header_text())


def test_workspace_bytes_without_a_device():
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    T = (ctypes.c_int64 * 2)(50000, 3000)
    S = (ctypes.c_int64 * 2)(5000, 700)
    dev = L.ka_posterior_workspace_bytes(2, T, S, 64, 1000, 4, 1)
    host = L.ka_posterior_workspace_bytes(2, T, S, 64, 1000, 4, 0)
    assert dev >= (50000 // 32 + 3000 // 32) * 8          # the forward offsets: a double per 32 frames
    assert dev < 1 << 20                                   # ... and no alpha lattice
    assert host >= dev + 53000 * 64 * 4                    # host buffers are staged
    generic = L.ka_posterior_workspace_bytes(2, T, S, 80, 1000, 4, 1)
    assert generic >= dev + (10001 + 1401) * 16            # the generic form's four columns
    assert L.ka_posterior_workspace_bytes(2, T, S, 64, 1000, 300, 1) == 0


def test_public_api_exists():
    import kokoro_align_amd as ka
    for name in ("ctc_path_posteriors", "ctc_path_posteriors_batch", "ctc_path_posteriors_device", "segment_confidence"):
        assert callable(getattr(ka, name)), name


def test_segment_confidence_uses_align_ranges():
    import kokoro_align_amd as ka
    post = np.array([1.0, 0.5, 0.25, 1.0, 0.75, 0.5], np.float32)
    mean, low = ka.segment_confidence(post, np.array([2, 2, 5, 9]))
    np.testing.assert_allclose(mean[[0, 2, 3]], [0.75, (0.25 + 1.0 + 0.75) / 3, 0.5])
    np.testing.assert_allclose(low[[0, 2, 3]], [0.5, 0.25, 0.5])
    assert np.isnan(mean[1]) and np.isnan(low[1])


def test_posteriors_without_a_gpu_is_a_loud_error():
    """No device: the call raises, never a silent CPU fallback (fails without the feature: there is no such entry point)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import kokoro_align_amd as ka
    lp = np.log(np.full((4, 3), 1 / 3, np.float32))
    with pytest.raises((ka.KAError, ValueError)):
        ka.ctc_path_posteriors(lp, np.array([1], np.int32), np.array([0, 1, 1, 2], np.int32))
