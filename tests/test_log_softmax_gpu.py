"""ka_log_softmax_f32 against float64: vocabulary sizes round the wavefront's 64 lanes, row counts round the four rows of a
workgroup, padded and in-place buffers, wide rows, and the overflow / -inf behaviour of the float32 NumPy expression it
restates (kokoro_align/align.py:116-117), which the header promises.  Tolerance = M_LOG_SOFTMAX x E_ref, E_ref = that NumPy
expression's own distance from float64 over all rows of one vocabulary size (tests/producer_ref.py)."""
import json
import os

import numpy as np
import pytest

import producer_ref as R

pytestmark = pytest.mark.gpu

NAN_FILL = 0x7FC0BEEF
V_SWEEP = (1, 2, 38, 39, 63, 64, 65, 127, 128, 129, 1000)
T_SWEEP = (1, 2, 3, 4, 5, 1023)


def _record(**kw):
    print(json.dumps(kw))
    path = os.environ.get("KA_ACCURACY_OUT")
    if path:
        with open(path, "at") as f:
            f.write(json.dumps(kw) + "\n")


def _rows(rng, T, V):
    """N(0, 3) logits; every fifth row has one or a few logits 80 above the rest (x - mean up to 80: exp stays finite)"""
    x = (3.0 * rng.standard_normal((T, V))).astype(np.float32)
    for t in range(0, T, 5):
        x[t] = rng.uniform(-0.5, 0.5, V)
        x[t, rng.integers(0, V, size=1 + (t // 5) % 3)] += 80.0
    return x


def _run(x, ld_in, ld_out, in_place=False):
    """-> (log-probs [T, V], True if every padding element of both buffers kept its bits)"""
    import torch
    from kokoro_align_amd import _lib
    lib = _lib.load_library()
    T, V = x.shape
    buf = np.empty((T, ld_in), dtype=np.float32)
    buf.view(np.int32)[:] = NAN_FILL
    buf[:, :V] = x
    d_in = torch.from_numpy(buf).cuda()
    if in_place:
        d_out, ld_out = d_in, ld_in
    else:
        d_out = torch.empty((T, ld_out), dtype=torch.float32, device="cuda")
        d_out.view(torch.int32).fill_(NAN_FILL)
    assert lib.ka_log_softmax_f32(d_in.data_ptr(), d_out.data_ptr(), T, V, ld_in, ld_out, None) == 0
    torch.cuda.synchronize()
    got_in, got_out = d_in.cpu().numpy(), d_out.cpu().numpy()
    clean = bool(np.all(got_in.view(np.int32)[:, V:] == NAN_FILL) and np.all(got_out.view(np.int32)[:, V:] == NAN_FILL))
    if not in_place:
        clean = clean and np.array_equal(got_in.view(np.int32)[:, :V], x.view(np.int32))     # the input is read only
    return got_out[:, :V].copy(), clean


@pytest.mark.parametrize("V", V_SWEEP)
def test_log_softmax_against_float64(V):
    rng = np.random.default_rng(V)
    e_ref = err = 0.0
    for T in T_SWEEP:
        x = _rows(rng, T, V)
        want, want32 = R.log_softmax(x), R.log_softmax_f32(x)
        assert np.isfinite(want32).all()
        e_ref = max(e_ref, float(np.abs(want32 - want).max()))
        for ld_in, ld_out, in_place in ((V, V, False), (V + 3, V, False), (V, V + 5, False), (V + 3, V + 5, False), (V, V, True),
                                        (V + 7, V + 7, True)):
            got, clean = _run(x, ld_in, ld_out, in_place)
            assert clean, f"V={V} T={T} ld_in={ld_in} ld_out={ld_out} in_place={in_place}: padding (or the input) was written"
            assert np.isfinite(got).all()
            err = max(err, float(np.abs(got - want).max()))
    tol = R.log_softmax_tolerance(e_ref)
    _record(test=f"log_softmax[V={V}]", e_ref=e_ref, kernel_error=err, ratio=err / e_ref if e_ref else None, m=R.M_LOG_SOFTMAX, tolerance=tol)
    assert err <= tol


@pytest.mark.parametrize("V", V_SWEEP)
def test_log_softmax_overflow_and_minus_infinity_follow_numpy(V):
    """A logit 100 above the rest overflows exp in float32: NumPy's row is -inf (or, for V = 1, 0).  A -inf logit makes the
    mean -inf: NumPy's row is NaN.  The kernel must give the same pattern, row by row, and ordinary rows between them."""
    rng = np.random.default_rng(100 + V)
    x = _rows(rng, 23, V)
    for t in (1, 6, 12):
        x[t, rng.integers(0, V)] += 100.0
    for t in (3, 12, 17):
        x[t, rng.integers(0, V)] = -np.inf
    x[19, :] = -np.inf
    want32 = R.log_softmax_f32(x)
    for in_place in (False, True):
        got, clean = _run(x, V + 3, V + 5, in_place)
        assert clean
        for kind in (np.isnan, np.isneginf, np.isposinf):
            assert np.array_equal(kind(got), kind(want32)), f"V={V} in_place={in_place}: {kind.__name__} pattern differs from NumPy's"
        fin = np.isfinite(want32)
        ok = np.all(fin, axis=1)
        want = R.log_softmax(x[ok])
        e_ref = float(np.abs(want32[ok] - want).max())
        assert float(np.abs(got[ok] - want).max()) <= R.log_softmax_tolerance(e_ref)
    if V >= 38:
        assert np.isneginf(want32[1]).all() and np.isnan(want32[3]).all() and np.isnan(want32[19]).all()


def test_log_softmax_rejects_bad_arguments():
    import torch
    from kokoro_align_amd import _lib
    lib = _lib.load_library()
    a = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    for args in ((None, a.data_ptr(), 4, 8, 8, 8), (a.data_ptr(), None, 4, 8, 8, 8), (a.data_ptr(), a.data_ptr(), 4, 8, 7, 8),
                 (a.data_ptr(), a.data_ptr(), 4, 8, 8, 7), (a.data_ptr(), a.data_ptr(), 4, 0, 8, 8), (a.data_ptr(), a.data_ptr(), -1, 8, 8, 8)):
        assert lib.ka_log_softmax_f32(*args, None) == -2
    assert lib.ka_log_softmax_f32(a.data_ptr(), a.data_ptr(), 0, 8, 8, 8, None) == 0
