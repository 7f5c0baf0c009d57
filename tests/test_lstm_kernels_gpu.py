"""The LSTM kernels (ka_lstm_layer_f32, ka_lstm_layer0_f32, ka_lstm_step_f32) called through the C ABI and the whole network
in its three device routes, against the float64 references of tests/producer_ref.py.

Tolerance = m x E_ref, E_ref = the distance of a float32 CPU computation of the same thing from float64 on the same input
(computed in the test); m and the tolerance functions live in producer_ref.py, where tests/test_producer_ref_cpu.py checks
that they are a fifth or less of what each kernel fault moves.  Every test prints its figures before it asserts; with
KA_ACCURACY_OUT=<file> they are also appended to that file as JSON lines (the source of profiles/producer_accuracy.json).
"""
import ctypes
import json
import os

import numpy as np
import pytest

import producer_ref as R

pytestmark = pytest.mark.gpu

NAN_FILL = 0x7FC0BEEF           # a quiet NaN with a payload: what `out` holds where nobody writes
KA_ERR_BAD_ARGS = -2


def _record(**kw):
    print(json.dumps(kw))
    path = os.environ.get("KA_ACCURACY_OUT")
    if path:
        with open(path, "at") as f:
            f.write(json.dumps(kw) + "\n")


def _lib():
    from kokoro_align_amd import _lib as L
    return L.load_library()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(a, ld, fill=np.nan):
    """[rows, cols] -> [rows, ld] float32 with NaN in the padding columns."""
    out = np.full((a.shape[0], ld), fill, dtype=np.float32)
    out[:, :a.shape[1]] = a
    return out


def _nan_filled(rows, ld):
    import torch
    t = torch.empty((rows, ld), dtype=torch.float32, device="cuda")
    t.view(torch.int32).fill_(NAN_FILL)
    return t


def _check_layer_output(got, ref, ref32, own, name):
    """owned rows against float64 within m x E_ref, everything else bit-unchanged, no NaN among the owned values"""
    h2 = ref.shape[1]
    bits = got.view(np.int32)
    assert np.all(bits[~own] == NAN_FILL), f"{name}: a row no sequence owns was written"
    assert np.all(bits[:, h2:] == NAN_FILL), f"{name}: a padding column was written"
    if not own.any():
        return
    assert not np.isnan(got[own, :h2]).any(), f"{name}: NaN in an owned row (an unowned input row leaked in, or a row was never written)"
    e_ref = float(np.abs(ref32[own] - ref[own]).max())
    err = float(np.abs(got[own, :h2].astype(np.float64) - ref[own]).max())
    tol = R.lstm_layer_tolerance(e_ref)
    _record(test=name, e_ref=e_ref, kernel_error=err, ratio=err / e_ref if e_ref else None, m=R.M_LSTM_LAYER, tolerance=tol)
    assert err <= tol, f"{name}: max |kernel - float64| = {err:.3g} > {tol:.3g} = {R.M_LSTM_LAYER} x E_ref"


def _run_layer(case, ld_in, ldo):
    import torch
    lib = _lib()
    out = _nan_filled(case["rows"], ldo)
    off, ln = _dev(case["seq_off"].astype(np.int32)), _dev(case["seq_len"].astype(np.int32))
    w_hh = _dev(case["w_hh"])
    if "x" in case:
        x, w_ih, bias = _dev(_padded(case["x"], ld_in)), _dev(case["w_ih"]), _dev(case["bias"])
        rc = lib.ka_lstm_layer0_f32(x.data_ptr(), ld_in, 40, w_ih.data_ptr(), bias.data_ptr(), w_hh.data_ptr(), out.data_ptr(), ldo,
                                    off.data_ptr(), ln.data_ptr(), len(case["seq_len"]), 128, None)
    else:
        gin = _dev(_padded(case["gin"], ld_in))
        rc = lib.ka_lstm_layer_f32(gin.data_ptr(), ld_in, w_hh.data_ptr(), out.data_ptr(), ldo, off.data_ptr(), ln.data_ptr(),
                                   len(case["seq_len"]), 128, None)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


LD_COMBOS = ((1024, 256), (1032, 260), (1024, 260), (1032, 256))


@pytest.mark.parametrize("pattern", R.LENGTH_PATTERNS)
@pytest.mark.parametrize("nseq", R.NSEQ_SWEEP)
def test_lstm_layer_geometry(nseq, pattern):
    """ka_lstm_layer_f32 on input projections the test supplies: sequence counts at the tile edges, length patterns, tables
    scattered over the frame buffer in non-monotone order with unowned rows (row 0 among them) that hold NaN, padded ldg / ldo."""
    k = R.NSEQ_SWEEP.index(nseq) * len(R.LENGTH_PATTERNS) + R.LENGTH_PATTERNS.index(pattern)
    ldg, ldo = LD_COMBOS[k % 4]
    case = R.layer_case(pattern, nseq, 100 + k)
    assert np.all(np.diff(case["seq_len"]) <= 0) and not case["own"][0]
    got = _run_layer(case, ldg, ldo)
    _check_layer_output(got, R.layer_reference(case), R.layer_reference(case, dtype=np.float32), case["own"],
                        f"layer[{pattern},nseq={nseq},ldg={ldg},ldo={ldo}]")


@pytest.mark.parametrize("x_in", ("mfcc", "unit"))
@pytest.mark.parametrize("pattern", ("one_long", "straddle", "zero_tail"))
@pytest.mark.parametrize("nseq", (1, 16, 17, 33, 150))
def test_lstm_layer0_geometry(nseq, pattern, x_in):
    """ka_lstm_layer0_f32 (input projection inside the step): MFCC-scale x at default-initialisation weights, the saturated
    regime it runs in, and order-1 x, where its W_hh fragments show; ldx 40 and 48, the same scattered tables."""
    k = (1, 16, 17, 33, 150).index(nseq) * 3 + ("one_long", "straddle", "zero_tail").index(pattern)
    ldx, ldo = (40, 48)[k % 2], (256, 260)[(k // 2) % 2]
    case = R.layer_case(pattern, nseq, 300 + k, x_in=x_in)
    got = _run_layer(case, ldx, ldo)
    _check_layer_output(got, R.layer_reference(case), R.layer_reference(case, dtype=np.float32), case["own"],
                        f"layer0[{x_in},{pattern},nseq={nseq},ldx={ldx},ldo={ldo}]")


def _exact_limits(got, ref, name):
    """where the float64 value IS 0, 1 or -1 (a gate at its limit, not a rounding), the kernel's must be too"""
    lim = (ref == 0.0) | (ref == 1.0) | (ref == -1.0)
    assert np.array_equal(got[lim].astype(np.float64), ref[lim] + 0.0), f"{name}: a saturated gate missed its limit"
    return int(lim.sum())


def test_lstm_layer_saturated_gates():
    """Sequences of 1 .. 4 steps whose pre-activations are mostly +-30, +-100, +-1e4 and +-inf (the accumulator's initial
    value: the float64 result is finite wherever they sit).  h = sigmoid(o) tanh(c) with c = 0 at the start cannot reach +-1
    within 4 steps, so the exact limit seen here is 0 (o at -1e4 or -inf); +-1 is asserted in the step test below."""
    rng = np.random.default_rng(41)
    lens = np.sort(rng.integers(1, 5, size=40))[::-1].copy()
    off, rows = R.scatter(lens, rng)
    own = R.owned_rows(rows, off, lens)
    gin = np.full((rows, 1024), np.nan, dtype=np.float32)
    gin[own] = R.saturating_gates(rng, (int(own.sum()), 1024))
    assert np.isposinf(gin).any() and np.isneginf(gin).any()
    case = dict(gin=gin, seq_off=off, seq_len=lens, rows=rows, own=own,
                w_hh=(2.5 * rng.uniform(-0.088, 0.088, (2, 512, 128))).astype(np.float32))
    got = _run_layer(case, 1032, 260)
    with np.errstate(all="ignore"):
        ref, ref32 = R.layer_reference(case), R.layer_reference(case, dtype=np.float32)
    assert np.isfinite(ref[own]).all()
    n = _exact_limits(got[own, :256], ref[own], "layer, saturated")
    assert n > 100
    _check_layer_output(got, ref, ref32, own, "layer[saturated gates]")


@pytest.mark.parametrize("H", (8, 100, 128))
def test_lstm_step(H):
    """ka_lstm_step_f32: arbitrary incoming c and h, fewer running sequences than the tables hold, padded strides everywhere,
    saturated gates (incoming c of +-1e4 under a forget gate at +inf gives h = +-1 exactly)."""
    import torch
    lib = _lib()
    rng = np.random.default_rng(50 + H)
    n_tab, n, frames = 9, 6, 23
    ldg, ldo = 8 * H + 8, 2 * H + 4
    rec_stride, state_stride, rows_stride = n_tab * 4 * H + 16, n_tab * H + 8, n_tab + 3
    gin = _padded(R.saturating_gates(rng, (frames, 8 * H)), ldg)
    gin[::2, :8 * H] = (2.0 * rng.standard_normal((len(gin[::2]), 8 * H))).astype(np.float32)
    rec = np.full(2 * rec_stride, np.nan, dtype=np.float32)
    c = np.full(2 * state_stride, np.nan, dtype=np.float32)
    h = np.full(2 * state_stride, np.nan, dtype=np.float32)
    rows = np.full(2 * rows_stride, -1, dtype=np.int32)
    pick = rng.permutation(frames)
    for d in (0, 1):
        rec[d * rec_stride:d * rec_stride + n_tab * 4 * H] = rng.standard_normal(n_tab * 4 * H)
        cc = 1.5 * rng.standard_normal((n_tab, H))
        cc[0, :], cc[1, :] = 1e4, -1e4
        c[d * state_stride:d * state_stride + n_tab * H] = cc.reshape(-1)
        h[d * state_stride:d * state_stride + n_tab * H] = rng.uniform(-1, 1, n_tab * H)
        rows[d * rows_stride:d * rows_stride + n_tab] = pick[d * n_tab:d * n_tab + n_tab]
    for d in (0, 1):                       # sequences 0 and 1: forget and output gates wide open, c stays at +-1e4
        for s in (0, 1):
            r = rows[d * rows_stride + s]
            gin[r, d * 4 * H + H:d * 4 * H + 2 * H] = np.inf
            gin[r, d * 4 * H + 3 * H:d * 4 * H + 4 * H] = 1e4
            gin[r, d * 4 * H:d * 4 * H + H] = -np.inf
    out0 = _nan_filled(frames, ldo)
    d_gin, d_rec, d_c, d_h, d_rows = _dev(gin), _dev(rec), _dev(c), _dev(h), _dev(rows)
    rc = lib.ka_lstm_step_f32(d_gin.data_ptr(), ldg, d_rec.data_ptr(), rec_stride, d_c.data_ptr(), d_h.data_ptr(), state_stride,
                              out0.data_ptr(), ldo, d_rows.data_ptr(), rows_stride, n, H, None)
    assert rc == 0
    torch.cuda.synchronize()
    got_c, got_h, got_out = d_c.cpu().numpy(), d_h.cpu().numpy(), out0.cpu().numpy()

    def view(a, stride, width):
        return np.stack([a[d * stride:d * stride + n_tab * width].reshape(n_tab, width) for d in (0, 1)])
    args = (gin, view(rec, rec_stride, 4 * H), view(c, state_stride, H), view(h, state_stride, H), np.zeros((frames, 2 * H)),
            view(rows, rows_stride, 1)[:, :, 0], n)
    with np.errstate(all="ignore"):
        rc64, rh64, ro64 = R.lstm_step(*args)
        rc32, rh32, _ = R.lstm_step(*args, dtype=np.float32)
    # untouched: the states of sequences n.., the gaps between the directions, rows nobody names, padding columns
    keep_c, keep_h = np.ones(c.shape, bool), np.ones(h.shape, bool)
    written = np.zeros((frames, ldo), bool)
    for d in (0, 1):
        keep_c[d * state_stride:d * state_stride + n * H] = False
        keep_h[d * state_stride:d * state_stride + n * H] = False
        for s in range(n):
            written[rows[d * rows_stride + s], d * H:(d + 1) * H] = True
    assert np.array_equal(got_c.view(np.int32)[keep_c], c.view(np.int32)[keep_c])
    assert np.array_equal(got_h.view(np.int32)[keep_h], h.view(np.int32)[keep_h])
    assert np.all(got_out.view(np.int32)[~written] == NAN_FILL)
    gc, gh = view(got_c, state_stride, H)[:, :n], view(got_h, state_stride, H)[:, :n]
    assert np.isfinite(gc).all() and np.isfinite(gh).all()
    assert _exact_limits(gh, rh64[:, :n], f"step H={H}") >= 4 * H
    assert np.all(gh[:, 0] == 1.0) and np.all(gh[:, 1] == -1.0)
    for d in (0, 1):
        for s in range(n):
            assert np.array_equal(got_out[rows[d * rows_stride + s], d * H:(d + 1) * H], gh[d, s])
    # c of sequences 0 / 1 is +-1e4 (one float32 ulp there is 1e-3): compared relative to its magnitude
    scale = np.maximum(1.0, np.abs(rc64[:, :n]))
    e_ref = max(float(np.abs(rh32[:, :n] - rh64[:, :n]).max()), float((np.abs(rc32[:, :n] - rc64[:, :n]) / scale).max()))
    err = max(float(np.abs(gh - rh64[:, :n]).max()), float((np.abs(gc - rc64[:, :n]) / scale).max()))
    tol = R.lstm_layer_tolerance(e_ref)
    _record(test=f"step[H={H}]", e_ref=e_ref, kernel_error=err, ratio=err / e_ref, m=R.M_LSTM_LAYER, tolerance=tol)
    assert err <= tol


def test_lstm_calls_reject_what_the_kernels_are_not_built_for():
    """KA_ERR_BAD_ARGS and nothing launched: `out` keeps its fill."""
    import torch
    lib = _lib()
    case = R.layer_case("equal", 3, 1, x_in="unit")
    out = _nan_filled(case["rows"], 256)
    g = _dev(np.zeros((case["rows"], 1024), np.float32))
    x = _dev(np.zeros((case["rows"], 40), np.float32))
    w_hh, w_ih, bias = _dev(case["w_hh"]), _dev(case["w_ih"]), _dev(case["bias"])
    off, ln = _dev(case["seq_off"].astype(np.int32)), _dev(case["seq_len"].astype(np.int32))
    P = lambda t: t.data_ptr()
    layer_ok = [P(g), 1024, P(w_hh), P(out), 256, P(off), P(ln), 3, 128, None]
    layer0_ok = [P(x), 40, 40, P(w_ih), P(bias), P(w_hh), P(out), 256, P(off), P(ln), 3, 128, None]
    st = _dev(np.zeros(2 * 3 * 128, np.float32))
    rec = _dev(np.zeros(2 * 3 * 512, np.float32))
    rows = _dev(np.ones(6, np.int32))
    step_ok = [P(g), 1024, P(rec), 3 * 512, P(st), P(st), 3 * 128, P(out), 256, P(rows), 3, 3, 128, None]

    def bad(fn, ok, **changes):
        args = list(ok)
        for i, v in changes.items():
            args[int(i[1:])] = v
        assert fn(*args) == KA_ERR_BAD_ARGS, (fn.__name__, changes)
    for h_bad in (64, 127, 256):
        bad(lib.ka_lstm_layer_f32, layer_ok, a8=h_bad, a1=8 * 256, a4=2 * 256)
        bad(lib.ka_lstm_layer0_f32, layer0_ok, a11=h_bad, a7=2 * 256)
    for n_in in (39, 41, 0):
        bad(lib.ka_lstm_layer0_f32, layer0_ok, a2=n_in, a1=48)
    bad(lib.ka_lstm_layer_f32, layer_ok, a1=1023)
    bad(lib.ka_lstm_layer_f32, layer_ok, a4=255)
    bad(lib.ka_lstm_layer0_f32, layer0_ok, a1=39)
    bad(lib.ka_lstm_layer0_f32, layer0_ok, a7=255)
    bad(lib.ka_lstm_layer_f32, layer_ok, a7=-1)
    bad(lib.ka_lstm_step_f32, step_ok, a1=1023)
    bad(lib.ka_lstm_step_f32, step_ok, a8=255)
    bad(lib.ka_lstm_step_f32, step_ok, a12=0)
    for i in (0, 2, 3, 5, 6):
        bad(lib.ka_lstm_layer_f32, layer_ok, **{f"a{i}": None})
    for i in (0, 3, 4, 5, 6, 8, 9):
        bad(lib.ka_lstm_layer0_f32, layer0_ok, **{f"a{i}": None})
    for i in (0, 2, 4, 5, 7, 9):
        bad(lib.ka_lstm_step_f32, step_ok, **{f"a{i}": None})
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy().view(np.int32) == NAN_FILL)
    assert lib.ka_lstm_layer_f32(*layer_ok) == 0 and lib.ka_lstm_layer0_f32(*layer0_ok) == 0 and lib.ka_lstm_step_f32(*step_ok) == 0
    torch.cuda.synchronize()


ROUTES = (("persistent, layer-0 projection inside", dict(persistent=True, fuse_layer0=True)),
          ("persistent, projection as a GEMM", dict(persistent=True, fuse_layer0=False)),
          ("per step", dict(persistent=False)))


@pytest.mark.parametrize("kind,scale", R.NETWORK_FAMILIES)
def test_network_routes_against_float64(kind, scale):
    """lstm_logits_device in its three routes on 44 segments of 0 .. 1400 frames: trained-scale weights on MFCC-scale input,
    and the order-1 input at default initialisation on which one W_hh element moves the logits least (the ceiling of m)."""
    import torch
    from kokoro_align_amd.model import AudioToChar, lstm_logits_device, segment_logits
    state, data, ends = R.network_family(kind, scale)
    ref = R.network_logits(state, data, ends)
    cpu = AudioToChar().eval()
    cpu.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    starts = np.concatenate([[0], ends[:-1]])
    want32 = np.concatenate([g.numpy() for g in segment_logits(cpu, [data[a:b] for a, b in zip(starts, ends) if b > a], device="cpu")], 0)
    e_ref = float(np.abs(want32 - ref).max())
    tol = R.network_tolerance(e_ref)
    gpu = AudioToChar().eval()
    gpu.load_state_dict(cpu.state_dict())
    gpu = gpu.cuda()
    errs = {}
    for name, kw in ROUTES:
        got = lstm_logits_device(gpu, data, ends, **kw).cpu().numpy()
        assert got.shape == ref.shape and np.isfinite(got).all()
        errs[name] = float(np.abs(got - ref).max())
        _record(test=f"network[{kind},x{scale}]", route=name, e_ref=e_ref, kernel_error=errs[name], ratio=errs[name] / e_ref,
                m=R.M_LSTM_NETWORK, tolerance=tol)
    assert 0.0 < e_ref <= R.E_REF_MAX
    assert all(v <= tol for v in errs.values()), (errs, tol)
