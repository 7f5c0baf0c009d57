"""The yardstick of the producer tests (tests/producer_ref.py) is checked here, without a GPU: the float64 references are
right (torch.nn.LSTM in float64, the reference-made g7 logits), the input families are well-conditioned (float32 stays
within 5e-6 of float64: a CONDITION on the inputs, not a measurement of the kernels), and the tolerance the GPU tests apply
- taken from the same functions - is at least five times smaller than what each kernel fault moves."""
import functools

import numpy as np
import pytest

import producer_ref as R
from golden_util import g7
from oracle import oracle as O


def _torch_network(state, dtype):
    import torch
    from kokoro_align_amd.model import AudioToChar
    model = AudioToChar().eval().to(dtype)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items()})
    return model


def _torch_logits(state, data, ends, dtype):
    import torch
    from kokoro_align_amd.model import segment_logits
    starts = np.concatenate([[0], ends[:-1]])
    segs = [torch.from_numpy(data[a:b]).to(dtype) for a, b in zip(starts, ends) if b > a]
    model = _torch_network(state, dtype)
    with torch.no_grad():
        from torch.nn.utils.rnn import pack_sequence
        logits, lengths = model(pack_sequence(segs, enforce_sorted=False))
    return np.concatenate([logits[:n, j].numpy() for j, n in enumerate(lengths.tolist())], 0)


@functools.lru_cache(maxsize=None)
def _family(kind, scale):
    state, data, ends = R.network_family(kind, scale)
    ref = R.network_logits(state, data, ends)
    e_ref = float(np.abs(_torch_logits(state, data, ends, __import__("torch").float32) - ref).max())
    return state, data, ends, ref, e_ref


# ------------------------------------------------------------------------------------------
# the reference is right
# ------------------------------------------------------------------------------------------
def test_network_reference_equals_torch_lstm_in_float64():
    import torch
    rng = np.random.default_rng(7)
    lens = np.array([1, 40, 0, 7, 129, 16, 17, 2, 300])
    ends = np.cumsum(lens)
    for scale, data in ((1.0, rng.standard_normal((int(lens.sum()), 40)).astype(np.float32)), (2.5, R.mfcc_like(rng, int(lens.sum())))):
        state = R.trained_scale_state(3, scale)
        want = _torch_logits(state, data, ends, torch.float64)
        got = R.network_logits(state, data, ends)
        assert got.dtype == np.float64 and got.shape == want.shape == (int(lens.sum()), 39)
        assert np.abs(got - want).max() <= 1e-12


def test_network_reference_reproduces_the_reference_made_logits():
    """g7: logits the reference computed in float32 (|logit| <= 0.2, eps 6e-8 relative, a few hundred accumulated roundings
    per logit): 1e-6 is ten times the float32 network's measured distance from float64 and a hundredth of the 1e-4 the device
    tests grant."""
    g = g7()
    segs = [O.hash_logprobs(n, 40, sd) * np.float32(g["scale"]) + np.float32(g["offset"]) for n, sd in zip(g["lens"], g["seeds"])]
    got = R.network_logits(g["state"], np.concatenate(segs, 0), np.cumsum(g["lens"]))
    worst = float(np.abs(got - np.concatenate(g["logits"], 0)).max())
    print("g7: max |float64 reference - reference-made float32 logits| =", worst)
    assert worst <= 1e-6


def test_layer_and_step_references_agree_with_the_network_reference():
    """lstm_layer0 = projection + lstm_layer, and lstm_step iterated = lstm_layer: three statements of one recurrence."""
    case = R.layer_case("straddle", 17, 5, x_in="unit")
    a = R.layer_reference(case)
    own = case["own"]
    gin = np.full((case["rows"], 8 * R.H), np.nan)
    gin[own] = case["x"][own].astype(np.float64) @ case["w_ih"].reshape(-1, 40).astype(np.float64).T + case["bias"].reshape(-1).astype(np.float64)
    b = R.lstm_layer(gin, case["w_hh"], case["seq_off"], case["seq_len"])
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isnan(a[:, 0]), ~own)
    assert np.abs(a[own] - b[own]).max() <= 1e-13
    off, ln = case["seq_off"], case["seq_len"]
    n = len(ln)
    c = np.zeros((2, n, R.H))
    h = np.zeros((2, n, R.H))
    out = np.full((case["rows"], 2 * R.H), np.nan)
    w = case["w_hh"].astype(np.float64)
    for t in range(int(ln.max())):
        run = int((ln > t).sum())
        rows = np.stack([off + t, off + ln - 1 - t])
        rec = np.einsum("dsk,dgk->dsg", h, w)
        c, h, out = R.lstm_step(np.nan_to_num(gin), rec, c, h, out, rows, run)
    assert np.abs(out[own] - b[own]).max() <= 1e-13 and np.isnan(out[~own]).all()


def test_log_softmax_references():
    rng = np.random.default_rng(2)
    x = (3.0 * rng.standard_normal((50, 39))).astype(np.float32)
    a, b = R.log_softmax(x), R.log_softmax_f32(x)
    assert a.dtype == np.float64 and b.dtype == np.float32
    assert np.abs(np.exp(a).sum(-1) - 1.0).max() <= 1e-14
    assert np.abs(a - b).max() <= 4e-6
    x[3, 5] += 100.0                     # exp overflows in float32: the whole row is -inf, as in the reference
    x[7, 0] = -np.inf                    # the mean is -inf: the whole row is NaN
    b = R.log_softmax_f32(x)
    assert np.all(np.isneginf(b[3])) and np.all(np.isnan(b[7])) and np.isfinite(np.delete(b, [3, 7], 0)).all()
    assert np.isfinite(R.log_softmax(x)[3]).all()


# ------------------------------------------------------------------------------------------
# the inputs are well-conditioned
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,scale", R.NETWORK_FAMILIES)
def test_network_families_are_well_conditioned(kind, scale):
    state, data, ends, ref, e_ref = _family(kind, scale)
    e_np = float(np.abs(R.network_logits(state, data, ends, dtype=np.float32) - ref).max())
    print(f"{kind} x{scale}: {len(ends)} segments, {ref.shape[0]} frames, E_ref (float32 PyTorch CPU) = {e_ref:.3g}, float32 NumPy = {e_np:.3g}")
    assert len(ends) >= 40 and int(np.diff(np.concatenate([[0], ends])).max()) == 1400
    assert 0.0 < e_ref <= R.E_REF_MAX and e_np <= R.E_REF_MAX


LAYER_CASES = [("one_long", 33, False), ("straddle", 150, False), ("one_long", 33, "mfcc"), ("zero_tail", 150, "mfcc"),
               ("one_long", 33, "unit"), ("straddle", 150, "unit")]


@pytest.mark.parametrize("pattern,nseq,x_in", LAYER_CASES)
def test_layer_families_are_well_conditioned(pattern, nseq, x_in):
    case = R.layer_case(pattern, nseq, 100 + nseq, x_in=x_in)
    ref = R.layer_reference(case)
    e_ref = float(np.nanmax(np.abs(R.layer_reference(case, dtype=np.float32) - ref)))
    print(f"{pattern} nseq={nseq} x_in={x_in}: E_ref (float32 NumPy) = {e_ref:.3g}")
    assert 0.0 < e_ref <= R.E_REF_MAX


# ------------------------------------------------------------------------------------------
# the tolerance separates good from bad
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", R.WEIGHT_FAULTS + R.STRUCTURE_FAULTS)
@pytest.mark.parametrize("kind,scale", R.NETWORK_FAMILIES)
def test_network_tolerance_is_a_fifth_of_every_fault(kind, scale, fault):
    state, data, ends, ref, e_ref = _family(kind, scale)
    if fault in R.WEIGHT_FAULTS:
        bad = R.network_logits(R.with_weight_fault(state, fault), data, ends)
    else:
        bad = R.network_logits(state, data, ends, fault=fault)
    shift = float(np.abs(bad - ref).max())
    tol = R.network_tolerance(e_ref)
    print(f"{kind} x{scale} {fault}: shift {shift:.3g}, tolerance {tol:.3g}, ratio {shift / tol:.3g}")
    assert shift >= 5.0 * tol


def _visible(x_in, fault):
    if fault in ("one_w_ih_column", "one_bias_element"):
        return bool(x_in)              # ka_lstm_layer_f32 takes finished input projections: it has no W_ih and no bias
    if fault in ("one_w_hh_element", "w_hh_k124_127"):
        return x_in != "mfcc"          # saturated gates: W_hh cannot be seen at MFCC scale, the order-1 family covers it
    return True


@pytest.mark.parametrize("pattern,nseq,x_in,fault", [c + (f,) for c in LAYER_CASES for f in R.WEIGHT_FAULTS + R.STRUCTURE_FAULTS
                                                     if _visible(c[2], f)])
def test_layer_tolerance_is_a_fifth_of_every_fault(pattern, nseq, x_in, fault):
    """Per kernel call.  Not every fault can be seen in every family, which is why the GPU tests run all three: W_ih and the
    bias exist in the fused layer-0 call only, and at MFCC scale every gate of that call is saturated - W_hh is invisible
    there (a zeroed element moves the output by 1e-13) and is caught on the order-1 input."""
    case = R.layer_case(pattern, nseq, 100 + nseq, x_in=x_in)
    ref = R.layer_reference(case)
    tol = R.lstm_layer_tolerance(np.nanmax(np.abs(R.layer_reference(case, dtype=np.float32) - ref)))
    bad = dict(case)
    if fault == "one_w_hh_element":
        bad["w_hh"] = case["w_hh"].copy()
        bad["w_hh"][0, 2 * R.H + 37, 53] = 0.0
    elif fault == "w_hh_k124_127":
        bad["w_hh"] = case["w_hh"].copy()
        bad["w_hh"][0, :, 124:128] = 0.0
    elif fault == "one_w_ih_column":
        bad["w_ih"] = case["w_ih"].copy()
        bad["w_ih"][0, :, 7] = 0.0
    elif fault == "one_bias_element":
        bad["bias"] = case["bias"].copy()
        bad["bias"][0, 3 * R.H + 5] = 0.0
    got = R.layer_reference(bad, fault=fault if fault in R.STRUCTURE_FAULTS else None)
    own = case["own"]
    shift = float(np.max(np.abs(np.nan_to_num(got[own], nan=9.0) - ref[own])))
    print(f"{pattern} nseq={nseq} x_in={x_in} {fault}: shift {shift:.3g}, tolerance {tol:.3g}, ratio {shift / tol:.3g}")
    assert shift >= 5.0 * tol
