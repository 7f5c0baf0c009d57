"""Plain NumPy references of the kernels that PRODUCE the dynamic program's input, written from the equations in
include/kokoro_align_amd.h: the bidirectional LSTM (ka_lstm_layer_f32, ka_lstm_layer0_f32, ka_lstm_step_f32), the whole
AudioToChar network and the mean-subtracted log-softmax (ka_log_softmax_f32).  Explicit loops over time, no torch.

Every function runs in float64 by default - the yardstick - and in float32 on request (``dtype=np.float32``): the float32
run is the "restatement" whose own distance from float64, E_ref, is the unit the GPU tests' tolerances are counted in
(``lstm_layer_tolerance``, ``network_tolerance``, ``log_softmax_tolerance`` below: the ONE place both the CPU tests and the
GPU tests take them from).  The input builders give the families the tests run on; the faults are the kernel mistakes the
tolerance has to tell from rounding (tests/test_producer_ref_cpu.py).
"""
import numpy as np

H = 128        # hidden size of the persistent kernel
N_IN = 40      # MFCC coefficients
TILE = 16      # sequences per workgroup of the persistent kernel

# m of "tolerance = m x E_ref": twice the worst ratio max|kernel - float64| / E_ref measured on the MI355X
# (profiles/producer_accuracy.json)
M_LSTM_LAYER = 9.0      # ka_lstm_layer_f32 / ka_lstm_layer0_f32 / ka_lstm_step_f32 against the float32 NumPy restatement's E_ref
M_LSTM_NETWORK = 3.9    # lstm_logits_device (three routes) against the float32 PyTorch CPU network's E_ref
M_LOG_SOFTMAX = 3.2     # ka_log_softmax_f32 against the float32 NumPy restatement's E_ref
E_REF_MAX = 5e-6        # conditioning: a family whose float32 restatement is further than this from float64 is no yardstick


def lstm_layer_tolerance(e_ref):
    return M_LSTM_LAYER * float(e_ref)


def network_tolerance(e_ref):
    return M_LSTM_NETWORK * float(e_ref)


def log_softmax_tolerance(e_ref):
    return M_LOG_SOFTMAX * float(e_ref)


# ------------------------------------------------------------------------------------------
# the cell
# ------------------------------------------------------------------------------------------
def sigmoid(x):
    """1 / (1 + exp(-x)) without overflow; exact 0 and 1 at -inf and +inf."""
    x = np.asarray(x)
    e = np.exp(-np.abs(x))
    one = x.dtype.type(1)
    return np.where(x >= 0, one / (one + e), e / (one + e))


def cell(gates, c, swap_fg=False):
    """gates [..., 4H] in PyTorch order (i, f, g, o), c [..., H] -> (c', h')."""
    h = gates.shape[-1] // 4
    i, f, g, o = (gates[..., k * h:(k + 1) * h] for k in range(4))
    if swap_fg:
        f, g = g, f
    cn = sigmoid(f) * c + sigmoid(i) * np.tanh(g)
    return cn, sigmoid(o) * np.tanh(cn)


# ------------------------------------------------------------------------------------------
# one layer, both directions (ka_lstm_layer_f32)
# ------------------------------------------------------------------------------------------
def lstm_layer(gin, w_hh, seq_off, seq_len, dtype=np.float64, fault=None):
    """gin [rows, >= 8H] (forward | backward input projections, bias included), w_hh [2, 4H, H], seq_off / seq_len [nseq]
    (sorted by length, longest first, as the kernel requires) -> out [rows, 2H]; rows no sequence owns hold NaN.
    Rows of gin that no sequence owns are never read.  ``fault``: None, "swap_fg", "backward_off_by_one" (the backward
    direction READS one row further up) or "overrun" (a sequence shorter than its tile of 16 takes one step too many and
    writes it over the neighbouring row)."""
    gin = np.asarray(gin)
    w_hh = np.asarray(w_hh, dtype=dtype)
    seq_off = np.asarray(seq_off, dtype=np.int64)
    seq_len = np.asarray(seq_len, dtype=np.int64)
    h = w_hh.shape[2]
    rows = gin.shape[0]
    out = np.full((rows, 2 * h), np.nan, dtype=dtype)
    nseq = len(seq_len)
    max_len = int(seq_len.max()) if nseq else 0
    for d in (0, 1):
        wt = np.ascontiguousarray(w_hh[d].T)                    # [H, 4H]
        hs = np.zeros((nseq, h), dtype=dtype)
        cs = np.zeros((nseq, h), dtype=dtype)
        for t in range(max_len):
            run = np.nonzero(seq_len > t)[0]
            r_out = seq_off[run] + t if d == 0 else seq_off[run] + seq_len[run] - 1 - t
            r_in = r_out
            if fault == "backward_off_by_one" and d == 1:
                r_in = np.minimum(r_out + 1, rows - 1)
            gates = gin[r_in, d * 4 * h:(d + 1) * 4 * h].astype(dtype) + hs[run] @ wt
            cs[run], hs[run] = cell(gates, cs[run], swap_fg=fault == "swap_fg")
            out[r_out, d * h:(d + 1) * h] = hs[run]
        if fault == "overrun":
            for s in range(nseq):
                n, o = int(seq_len[s]), int(seq_off[s])
                if n <= 0 or n >= int(seq_len[(s // TILE) * TILE]):
                    continue                                    # the tile's loop ends with its longest member
                r_last, r_next = (o + n - 1, o + n) if d == 0 else (o, o - 1)
                if not 0 <= r_next < rows:
                    continue
                gates = gin[r_last, d * 4 * h:(d + 1) * 4 * h].astype(dtype) + hs[s] @ wt
                out[r_next, d * h:(d + 1) * h] = cell(gates, cs[s])[1]
    return out


def owned_rows(rows, seq_off, seq_len):
    m = np.zeros(rows, dtype=bool)
    for o, n in zip(np.asarray(seq_off).tolist(), np.asarray(seq_len).tolist()):
        m[o:o + n] = True
    return m


def lstm_layer0(x, w_ih, bias, w_hh, seq_off, seq_len, dtype=np.float64, fault=None):
    """ka_lstm_layer0_f32: x [rows, >= 40], w_ih [2, 4H, 40] (or [8H, 40]), bias [2, 4H] = b_ih + b_hh; otherwise as lstm_layer."""
    x = np.asarray(x)
    w_ih = np.asarray(w_ih, dtype=dtype).reshape(-1, N_IN)
    bias = np.asarray(bias, dtype=dtype).reshape(-1)
    own = owned_rows(x.shape[0], seq_off, seq_len)
    gin = np.full((x.shape[0], w_ih.shape[0]), np.nan, dtype=dtype)
    gin[own] = x[own, :N_IN].astype(dtype) @ w_ih.T + bias
    return lstm_layer(gin, w_hh, seq_off, seq_len, dtype=dtype, fault=fault)


# ------------------------------------------------------------------------------------------
# one step (ka_lstm_step_f32)
# ------------------------------------------------------------------------------------------
def lstm_step(gin, rec, c, h, out, rows, n, dtype=np.float64):
    """gin [frames, >= 8H], rec [2, n_tab, 4H], c / h [2, n_tab, H], out [frames, >= 2H], rows [2, n_tab] int, n <= n_tab
    running sequences -> (c', h', out') as new arrays: entries of sequences n.. and rows nobody names are the caller's."""
    c = np.array(c, dtype=dtype)
    h = np.array(h, dtype=dtype)
    out = np.array(out, dtype=dtype)
    hd = c.shape[2]
    for d in (0, 1):
        for s in range(n):
            r = int(rows[d][s])
            gates = np.asarray(gin[r, d * 4 * hd:(d + 1) * 4 * hd], dtype=dtype) + np.asarray(rec[d][s], dtype=dtype)
            c[d, s], h[d, s] = cell(gates, c[d, s])
            out[r, d * hd:(d + 1) * hd] = h[d, s]
    return c, h, out


# ------------------------------------------------------------------------------------------
# the whole network (AudioToChar: 2 bidirectional layers + Linear)
# ------------------------------------------------------------------------------------------
def network_logits(state, data, ends, dtype=np.float64, fault=None, fault_layer=0):
    """state: name -> array with torch.nn.LSTM's keys (lstm.weight_ih_l0, ..._reverse, dense.weight, dense.bias); data
    [rows, n_in]; ends = cumulative segment ends (empty segments allowed) -> logits [ends[-1], vocab] in row order."""
    ends = np.asarray(ends, dtype=np.int64).reshape(-1)
    total = int(ends[-1]) if len(ends) else 0
    starts = np.concatenate([[0], ends[:-1]])
    lens = ends - starts
    order = np.argsort(-lens, kind="stable")
    off, ln = starts[order], lens[order]
    inp = np.asarray(data)[:total].astype(dtype)
    layer = 0
    while f"lstm.weight_ih_l{layer}" in state:
        sfx = [f"_l{layer}", f"_l{layer}_reverse"]
        w_ih = np.concatenate([np.asarray(state["lstm.weight_ih" + s], dtype=dtype) for s in sfx], 0)
        bias = np.concatenate([np.asarray(state["lstm.bias_ih" + s], dtype=dtype) + np.asarray(state["lstm.bias_hh" + s], dtype=dtype)
                               for s in sfx], 0)
        w_hh = np.stack([np.asarray(state["lstm.weight_hh" + s], dtype=dtype) for s in sfx], 0)
        gin = inp @ w_ih.T + bias
        inp = lstm_layer(gin, w_hh, off, ln, dtype=dtype, fault=fault if layer == fault_layer else None)
        layer += 1
    return inp @ np.asarray(state["dense.weight"], dtype=dtype).T + np.asarray(state["dense.bias"], dtype=dtype)


# ------------------------------------------------------------------------------------------
# log-softmax (ka_log_softmax_f32)
# ------------------------------------------------------------------------------------------
def log_softmax(x):
    """float64, max-subtracted: the mathematical value (the mean the kernel subtracts cancels)."""
    x = np.asarray(x, dtype=np.float64)
    z = x - np.max(x, axis=-1, keepdims=True)
    return z - np.log(np.sum(np.exp(z), axis=-1, keepdims=True))


def log_softmax_f32(x):
    """The float32 NumPy expression the kernel restates (mean-subtracted, NOT max-subtracted): its overflow to -inf and its
    NaN rows are part of the contract."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        centred = x - np.mean(x, axis=-1, keepdims=True)
        return centred - np.log(np.sum(np.exp(centred), axis=-1, keepdims=True))


# ------------------------------------------------------------------------------------------
# input builders
# ------------------------------------------------------------------------------------------
def mfcc_like(rng, n):
    """[n, 40] float32 at the scale of real MFCCs: c0 = -300 +- 100, the other coefficients decaying from +-60."""
    sd = np.concatenate([[100.0], 60.0 * np.exp(-np.arange(N_IN - 1) / 8.0)])
    mean = np.concatenate([[-300.0], np.zeros(N_IN - 1)])
    return (mean + sd * rng.standard_normal((n, N_IN))).astype(np.float32)


def trained_scale_state(seed, scale, hidden=H, n_in=N_IN, vocab=39):
    """torch.nn.LSTM / Linear default initialisation (uniform +-1/sqrt(hidden), +-1/sqrt(fan_in)) with the LSTM weight matrices
    multiplied by ``scale`` and +1 on the forget gate's bias: the magnitudes of a trained network.  float32 arrays."""
    rng = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(hidden)
    st = {}
    for layer, fan in ((0, n_in), (1, 2 * hidden)):
        for sfx in (f"_l{layer}", f"_l{layer}_reverse"):
            st["lstm.weight_ih" + sfx] = (scale * rng.uniform(-k, k, (4 * hidden, fan))).astype(np.float32)
            st["lstm.weight_hh" + sfx] = (scale * rng.uniform(-k, k, (4 * hidden, hidden))).astype(np.float32)
            b = rng.uniform(-k, k, 4 * hidden)
            b[hidden:2 * hidden] += 1.0
            st["lstm.bias_ih" + sfx] = b.astype(np.float32)
            st["lstm.bias_hh" + sfx] = rng.uniform(-k, k, 4 * hidden).astype(np.float32)
    kd = 1.0 / np.sqrt(2 * hidden)
    st["dense.weight"] = rng.uniform(-kd, kd, (vocab, 2 * hidden)).astype(np.float32)
    st["dense.bias"] = rng.uniform(-kd, kd, vocab).astype(np.float32)
    return st


# (input, LSTM weight scale): MFCC-scale input at the magnitudes of a trained network, and the order-1 input at default
# initialisation that the older LSTM tests use (the family where one W_hh element moves the logits least)
NETWORK_FAMILIES = (("mfcc", 1.0), ("mfcc", 2.5), ("mfcc", 5.0), ("unit", 1.0))


FAMILY_SEEDS = {("mfcc", 1.0): 10, ("mfcc", 2.5): 25, ("mfcc", 5.0): 51, ("unit", 1.0): 510}


def network_family(kind, scale):
    """(state, data, ends) of the whole-network tests: 44 segments of 1 .. 1400 frames, two of them empty, in no particular
    order.  Above scale 5 the recurrence turns chaotic (float32 and float64 part ways): no tolerance test means anything there,
    and AT scale 5 it depends on the draw (E_ref 1.4e-6 .. 1.3e-5 over six seeds): the seed was chosen on the CPU, by the
    conditioning test alone, before a kernel ran on it."""
    seed = FAMILY_SEEDS[(kind, scale)]
    rng = np.random.default_rng(1000 + seed)
    lens = np.concatenate([[1400, 1, 2, 0, 15, 16, 17, 511, 512, 0], rng.integers(3, 300, size=34)])
    lens = lens[rng.permutation(len(lens))]
    n = int(lens.sum())
    data = mfcc_like(rng, n) if kind == "mfcc" else (1.0 + 2.0 * rng.standard_normal((n, N_IN))).astype(np.float32)
    return trained_scale_state(seed, scale), data, np.cumsum(lens)


# ------------------------------------------------------------------------------------------
# launch geometry of the persistent kernel: sequence tables scattered over a frame buffer
# ------------------------------------------------------------------------------------------
LENGTH_PATTERNS = ("equal", "ones", "one_long", "straddle", "zero_tail")
NSEQ_SWEEP = (1, 15, 16, 17, 31, 32, 33, 150)


def seq_lengths(pattern, nseq, rng):
    """Lengths sorted longest first, as the kernel requires."""
    if pattern == "equal":
        ln = np.full(nseq, 37)
    elif pattern == "ones":
        ln = np.ones(nseq, dtype=np.int64)
    elif pattern == "one_long":                 # the longest segment the silence splitter allows among short ones
        ln = np.concatenate([[1400], rng.integers(1, 60, size=nseq - 1)])
    elif pattern == "straddle":                 # every tile of 16 holds 16 different lengths, its neighbours continue the run
        ln = 2 + np.arange(nseq)
    elif pattern == "zero_tail":                # empty entries at the sorted tail (a whole tile of them from 33 sequences on)
        ln = rng.integers(1, 50, size=nseq)
        ln[:max(1, nseq // 3 if nseq < 33 else 17)] = 0
    else:
        raise ValueError(pattern)
    return np.sort(np.asarray(ln, dtype=np.int64))[::-1].copy()


def scatter(lens, rng):
    """(seq_off, rows): the sequences laid into a frame buffer in random order with gaps of 0 .. 2 unowned rows between them,
    row 0 and the last rows unowned; an empty sequence's offset points into somebody else's rows."""
    off = np.zeros(len(lens), dtype=np.int64)
    cur = 1
    for i in rng.permutation(len(lens)):
        off[i] = cur
        if lens[i] > 0:
            cur += int(lens[i]) + int(rng.integers(0, 3))
    rows = cur + 2
    off[lens == 0] = rng.integers(0, rows, size=int((lens == 0).sum()))
    return off, rows


def layer_case(pattern, nseq, seed, x_in=False):
    """One call of ka_lstm_layer_f32 (gin ~ N(0, 1.5), weights x2.5) or, ``x_in`` = "mfcc" / "unit", of ka_lstm_layer0_f32:
    on MFCC-scale x at default-initialisation weights - pre-activations of +-90, every gate saturated, what the fused
    projection sees in production, where W_ih, the bias and the row addressing are what can go wrong and W_hh cannot be seen -
    or on x ~ N(1, 2) with weights x2.5, where W_hh's fragments in that instantiation of the kernel can.  A dict of float32 /
    int arrays without padding columns (the GPU test adds them); rows nobody owns hold NaN."""
    rng = np.random.default_rng(seed)
    scale = 1.0 if x_in == "mfcc" else 2.5
    lens = seq_lengths(pattern, nseq, rng)
    off, rows = scatter(lens, rng)
    own = owned_rows(rows, off, lens)
    k = 1.0 / np.sqrt(H)
    case = dict(seq_off=off, seq_len=lens, rows=rows, own=own,
                w_hh=(scale * rng.uniform(-k, k, (2, 4 * H, H))).astype(np.float32))
    if x_in:
        case["x"] = np.full((rows, N_IN), np.nan, dtype=np.float32)
        n = int(own.sum())
        case["x"][own] = mfcc_like(rng, n) if x_in == "mfcc" else (1.0 + 2.0 * rng.standard_normal((n, N_IN))).astype(np.float32)
        case["w_ih"] = (scale * rng.uniform(-k, k, (2, 4 * H, N_IN))).astype(np.float32)
        b = rng.uniform(-2 * k, 2 * k, (2, 4 * H))
        b[:, H:2 * H] += 1.0
        case["bias"] = b.astype(np.float32)
    else:
        case["gin"] = np.full((rows, 8 * H), np.nan, dtype=np.float32)
        case["gin"][own] = (1.5 * rng.standard_normal((int(own.sum()), 8 * H))).astype(np.float32)
    return case


def layer_reference(case, dtype=np.float64, fault=None):
    if "x" in case:
        return lstm_layer0(case["x"], case["w_ih"], case["bias"], case["w_hh"], case["seq_off"], case["seq_len"], dtype=dtype, fault=fault)
    return lstm_layer(case["gin"], case["w_hh"], case["seq_off"], case["seq_len"], dtype=dtype, fault=fault)


SATURATING = (30.0, -30.0, 100.0, -100.0, 1e4, -1e4, np.inf, -np.inf)


def saturating_gates(rng, shape):
    """float32 pre-activations: a third of them N(0, 2), the rest drawn from +-30, +-100, +-1e4, +-inf."""
    g = (2.0 * rng.standard_normal(shape)).astype(np.float32)
    pick = rng.integers(0, 3 * len(SATURATING), size=shape)
    sat = np.asarray(SATURATING, dtype=np.float32)
    m = pick < 2 * len(SATURATING)
    g[m] = sat[pick[m] % len(SATURATING)]
    return g


# ------------------------------------------------------------------------------------------
# faults the tolerance must tell from rounding
# ------------------------------------------------------------------------------------------
WEIGHT_FAULTS = ("one_w_hh_element", "w_hh_k124_127", "one_w_ih_column", "one_bias_element")
STRUCTURE_FAULTS = ("swap_fg", "backward_off_by_one", "overrun")


def with_weight_fault(state, name):
    """A copy of ``state`` with one fault in the forward direction.  The W_hh faults are a kernel's (a fragment in the wrong
    lane or a k-step left out), and one kernel runs every layer: they sit in both layers.  W_ih and the bias enter the kernel
    in layer 0 only (the fused projection)."""
    st = {k: np.array(v) for k, v in state.items()}
    if name == "one_w_hh_element":
        for layer in (0, 1):
            st[f"lstm.weight_hh_l{layer}"][2 * H + 37, 53] = 0.0    # gate g of unit 37, k = 53: one lane of one fragment
    elif name == "w_hh_k124_127":
        for layer in (0, 1):
            st[f"lstm.weight_hh_l{layer}"][:, 124:128] = 0.0        # the last k-step, a VGPR-resident fragment
    elif name == "one_w_ih_column":
        st["lstm.weight_ih_l0"][:, 7] = 0.0
    elif name == "one_bias_element":
        st["lstm.bias_ih_l0"][3 * H + 5] = 0.0
        st["lstm.bias_hh_l0"][3 * H + 5] = 0.0
    else:
        raise ValueError(name)
    return st
