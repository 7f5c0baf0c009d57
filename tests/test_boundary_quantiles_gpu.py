"""Exact boundary-time quantiles on the GPU: ka_ctc_boundary_quantiles against the integer definition
applied to the rows of ka_ctc_state_posteriors at all T frames (bit for bit, nothing left out), against the float64 reference
on the input families of posterior_ref.edge_cases() (all pairs but those at a near-tie, whose number is capped), the orderings,
peaked inputs, the path sampler, reused workspace slots in both memory modes, the argument checks and the Python layer.

The four large shapes of the bit-for-bit test are those the feature's request names.  Three of them (T=96 S=400, T=130 S=700,
T=40 S=600) have L / T above max_move - 1, so no path can follow the band and every terminal has zero mass: they are run as
stated and must fail as the state call fails, with -1 over [K, M].  Beside each stands a lattice of the same S, V and beam_size
with enough frames for a path to follow the band (T=300, 520, 450; max_move 2: T=900; max_move 6: T=260), which is where the
scan, the run of cuts and the ring do their work."""
import numpy as np
import pytest

import posterior_ref as R
import quantile_ref as QR
from fb_harness import engine, record, state_call
from quantile_harness import SENTINEL, quant_call, quant_call_one, written
from sample_harness import sample_call
from test_boundary_quantiles_cpu import FAMILY_CASES, LEVELS, MAX_UNSAFE, family, family_quantiles

pytestmark = pytest.mark.gpu

LEVELS8 = (2.0 ** -10, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0 - 2.0 ** -10)
# (T, S, V, beam, max_move, fast form, a path can follow the band)
BIT_SHAPES = [(96, 400, 39, 300, 4, True, False), (300, 400, 39, 300, 4, True, True),          # 300 cells and cuts in the band
              (130, 700, 39, 200, 4, True, False), (520, 700, 39, 200, 4, True, True),        # L = 1401: the ring wraps
              (40, 600, 39, 1100, 4, False, False), (450, 600, 39, 1100, 4, False, True),      # generic by band width, W > 1024
              (100, 60, 80, 16, 4, False, True),                                                # generic by V
              (900, 400, 39, 300, 2, True, True), (130, 60, 80, 16, 2, False, True),           # max_move 2
              (260, 600, 39, 1100, 6, False, True), (100, 60, 80, 16, 6, False, True)]         # max_move 6


@pytest.fixture(scope="module")
def env():
    return engine()


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _definition(eng, _lib, lp, labels, terminal, cuts, levels, beam, mm):
    """The integer definition on the state call's rows at all T frames: (quantile [K, M] or None for a failed lattice, Z, status)."""
    T, L = lp.shape[0], 2 * len(labels) + 1
    (rows,), (los,), z, st, rc = state_call(eng, _lib, [lp], [labels], [terminal], [np.arange(T)], beam, mm)
    if st[0] != 0:
        return None, z[0], int(st[0])
    return QR.integer_quantiles(rows, los, cuts, levels, L, beam), z[0], 0


def _check_against_definition(eng, _lib, lp, labels, terminal, cuts, levels, beam, mm, what, device=False):
    K, M = len(cuts), len(levels)
    want, zs, status = _definition(eng, _lib, lp, labels, terminal, cuts, levels, beam, mm)
    (buf,), z, st, rc = quant_call(eng, _lib, [lp], [labels], [terminal], [cuts], levels, beam, mm, pad=3, device=device)
    got = written(buf, K, M)
    assert st[0] == status and rc == status, (what, st, rc, status)
    if status != 0:
        assert np.all(got == -1), what
        assert (z[0] == -np.inf) if status == _lib.KA_ERR_ZERO_MASS else np.isnan(z[0]), what
        return None
    assert _same(z[0], zs), what
    diff = np.argwhere(got != want)
    assert len(diff) == 0, (what, len(diff), diff[:6], got[tuple(diff[:6].T)], want[tuple(diff[:6].T)])
    return got


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=lambda s: "T%d_S%d_V%d_B%d_M%d" % s[:5])
def test_bit_for_bit_the_integer_definition_on_the_state_rows(env, shape):
    _, _lib, eng = env
    T, S, V, beam, mm, fast, live = shape
    assert R.fast_form(S, V, beam, mm) == fast
    lp, labels = R.sloped(T, S, V, 4000 + T + S)
    L = 2 * S + 1
    terms = R.live_terminals(lp, labels, beam, mm)
    assert bool(terms) == live, shape
    terminal = terms[0] if live else L - 1
    cuts = np.arange(L + 1)
    got = _check_against_definition(eng, _lib, lp, labels, terminal, cuts, LEVELS8, beam, mm, shape)
    if not live:
        return
    lo, hi = R.windows(T, L, beam)
    assert np.all(got[0] == 0) and np.all(got[terminal + 1:] == T)
    assert np.all(np.diff(got, axis=1) >= 0) and np.all(np.diff(got, axis=0) >= 0)
    # the shape does what it is here for: crossings strictly inside the band at many cuts, a spread between the outer levels
    k = np.arange(1, terminal + 1)
    inside = (lo[got[k, 3]] < k) & (k < hi[got[k, 3]])
    assert inside.sum() >= min(len(k), 100) // 2 and np.any(got[k, -1] > got[k, 0]), shape
    if L > 1024 and fast:
        assert np.any(inside & (k > 1024))                                  # cuts inside the band after the ring has wrapped


@pytest.mark.parametrize("V", [39, 80], ids=["one_wavefront", "generic"])
def test_the_smallest_lattices_and_a_low_terminal(env, V):
    _, _lib, eng = env
    pad = lambda lp: R.pad_vocabulary(lp, V) if V != 39 else lp
    for T in (1, 2, 33):
        # S = 0: one blank holds every frame - cut 0 reads 0, cut 1 = L reads T
        lp0 = pad(R.sloped(T, 1, 39, 5 + T)[0])
        buf, z, rc = quant_call_one(eng, _lib, lp0, np.zeros(0, np.int32), 0, [0, 1], LEVELS8, 64, 4, pad=2)
        got = written(buf, 2, 8)
        assert rc == 0 and np.all(got[0] == 0) and np.all(got[1] == T)
        # K = 0: only Z
        lp, labels = R.sloped(T, 7, 39, 900 + T, alpha=1.0, zero_every=5)
        live = R.live_terminals(lp, labels, 64, 4)
        lp = pad(lp)
        (rows,), _, zs, st, _ = state_call(eng, _lib, [lp], [labels], [live[0]], [np.arange(T)], 64, 4)
        buf, z, rc = quant_call_one(eng, _lib, lp, labels, live[0], [], LEVELS, 64, 4)
        assert rc == 0 and st[0] == 0 and _same(z, zs[0]) and np.all(buf == SENTINEL)
        for terminal in live[:3]:
            _check_against_definition(eng, _lib, lp, labels, terminal, np.arange(16), LEVELS8, 64, 4, (T, terminal))
    # a terminal below L - 1: the cuts above it read T, in both memory modes
    lp, labels = R.sloped(90, 30, 39, 77, alpha=1.0, zero_every=5)
    live = [s for s in R.live_terminals(lp, labels, 16, 4) if s < 2 * 30 - 2]
    assert live
    for device in (False, True):
        got = _check_against_definition(eng, _lib, pad(lp), labels, live[0], np.arange(62), LEVELS8, 16, 4, ("low", device), device)
        assert np.all(got[live[0] + 1:] == 90) and np.all(got[live[0]] < 90)


_results = {}


def _kernel(env, name):
    """One quantile call per family case (cuts at every even position, LEVELS), shared by the tests below."""
    if name not in _results:
        _, _lib, eng = env
        lp, labels, terminal, beam, mm, cuts, ref = family(name)
        (buf,), z, st, rc = quant_call(eng, _lib, [lp], [labels], [terminal], [cuts], LEVELS, beam, mm)
        assert rc == 0 and st[0] == 0, (name, rc, st)
        _results[name] = (written(buf, len(cuts), len(LEVELS)), z[0])
    return _results[name]


@pytest.mark.parametrize("name", FAMILY_CASES)
def test_family_cases_against_the_float64_reference(env, name):
    _, _lib, eng = env
    lp, labels, terminal, beam, mm, cuts, ref = family(name)
    q = family_quantiles(name)
    got, z = _kernel(env, name)
    safe = ~q["unsafe"]
    left_out = int(q["unsafe"].sum())
    differ = int(np.sum(got[safe] != q["q"][safe]))
    moved = int(np.sum(got[~safe] != q["q"][~safe]))
    print(name, "pairs", got.size, "left out", left_out, "of them differing", moved, "safe pairs differing", differ)
    record("quantile_left_out", left_out / got.size, MAX_UNSAFE)
    record("quantile_mismatch", differ / got.size, 0.0)
    record("z", R.z_ratio(z, ref), R.M_Z)
    # the pairs left out may differ, but by a frame at which F is within the margin of the level: never out of order
    assert np.all(np.diff(got, axis=1) >= 0) and np.all(np.diff(got, axis=0) >= 0)
    # and the kernel is the integer definition here too
    _check_against_definition(eng, _lib, lp, labels, terminal, cuts, LEVELS, beam, mm, name)


@pytest.mark.parametrize("shape", R.PEAKED_SHAPES, ids=lambda s: "T%d_S%d_V%d_B%d_M%d" % s)
def test_peaked_inputs_give_the_best_paths_crossing_frames(env, shape):
    """posterior_ref.peaked's repeated labels and runs of label 0 leave several best paths of one score, so the best path is
    unique per CUT, not per frame: at a cut that every best path crosses at the same frame, F is below 2^-12 before that frame
    and above 1 - 2^-12 from it on (a path off the best ones weighs e^-20 a frame), and all eight levels read that frame."""
    _, _lib, eng = env
    T, S, V, beam, mm = shape
    lp, labels, terminal = R.peaked(T, S, V, beam, mm, seed=7)
    ref = R.ref_at(lp, labels, terminal, beam, mm)
    L = 2 * S + 1
    cuts = np.arange(L + 1)
    F = QR.cdf(ref["gamma"], cuts, L, beam)
    sharp = np.all((F < 2.0 ** -12) | (F > 1.0 - 2.0 ** -12), axis=0)
    assert sharp[1:terminal + 1].mean() >= 0.8, shape
    path = np.array([lo + int(np.argmax(g)) for lo, g in ref["gamma"]])    # a best path's state at every frame, to a tie
    want = np.sum(np.maximum.accumulate(path)[:, None] < cuts[None, :], axis=0)       # the first frame with path[t] >= c, T if none
    assert np.array_equal(want[sharp], QR.frames_of(F, (0.5,))[sharp, 0])
    (buf,), z, st, rc = quant_call(eng, _lib, [lp], [labels], [terminal], [cuts], LEVELS8, beam, mm)
    got = written(buf, L + 1, 8)
    assert rc == 0 and np.array_equal(got[sharp], np.repeat(want[sharp, None], 8, axis=1)), np.argwhere(got != want[:, None])[:6]
    assert np.all(np.diff(got, axis=1) >= 0) and np.all(np.diff(got, axis=0) >= 0)


def test_the_sampled_crossing_times_have_these_quantiles(env):
    _, _lib, eng = env
    lp, labels = R.sloped(120, 40, 39, 2024, alpha=0.6)
    beam, mm = 64, 4
    terminal = R.live_terminals(lp, labels, beam, mm)[0]
    L = 2 * 40 + 1
    cuts = np.arange(L + 1)
    levels = (0.05, 0.25, 0.5, 0.75, 0.95)
    buf, z, rc = quant_call_one(eng, _lib, lp, labels, terminal, cuts, levels, beam, mm)
    assert rc == 0
    q = written(buf, L + 1, len(levels)).astype(np.int64)
    taus = []
    for seed in range(8):
        (paths,), zs, st, rc = sample_call(eng, _lib, [lp], [labels], [terminal], 64, 1000 + seed, beam, mm)
        assert rc == 0 and _same(zs[0], z)
        taus.append(QR.sample_tau(paths, cuts))
    tau = np.concatenate(taus)                                              # [512, K]
    assert tau.shape == (512, L + 1) and np.any(q[:, -1] - q[:, 0] >= 3)    # (the posterior is spread: intervals of several frames)
    for m, level in enumerate(levels):
        se = np.sqrt(level * (1.0 - level) / 512)
        at = np.mean(tau <= q[None, :, m], axis=0)
        before = np.mean(tau <= q[None, :, m] - 1, axis=0)
        assert np.all(at >= level - 5 * se), (level, np.flatnonzero(at < level - 5 * se)[:8])
        assert np.all(before <= level + 5 * se), (level, np.flatnonzero(before > level + 5 * se)[:8])


def _small(rng, V, T=None, S=None):
    T, S = T or int(rng.integers(30, 60)), S or int(rng.integers(3, 20))
    lp, labels = R.sloped(T, S, 39, int(rng.integers(1 << 30)), alpha=0.5, zero_every=5)
    lp = R.pad_vocabulary(lp, V) if V != 39 else lp
    return lp, labels, R.live_terminals(lp, labels, 64, 4)[0]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("V,slots,pairs", [(39, 1024, 48), (80, 512, 24)], ids=["one_wavefront_1072", "generic_536"])
def test_a_reused_slot_gives_the_bits_of_a_lattice_sent_alone(env, V, slots, pairs, device):
    """Lattice slots + k runs on slot k after lattice k (launch_fb_ck: lattice i on workgroup i mod grid): after a wider and
    longer one with more cuts, which every third time failed after its forward pass or before it.  The outputs are views of
    wider buffers, whose other columns and rows stay as they were."""
    _, _lib, eng = env
    rng = np.random.default_rng(V)
    first, second = [], []
    for k in range(pairs):
        lp, labels, term = _small(rng, V, T=int(rng.integers(48, 65)), S=int(rng.integers(24, 40)))        # band 49 ... 64
        if k % 3 == 1:
            lp = lp.copy()
            lp[:, 0] = -np.inf                            # zero mass: found after the forward pass
            term = 2 * len(labels)
        elif k % 6 == 2:
            labels = labels.copy()
            labels[0] = V                                 # a bad label: found before anything runs
        first.append((lp, labels, term, np.arange(2 * len(labels) + 2)))                                     # every position
        lp, labels, term = _small(rng, V, T=int(rng.integers(20, 40)), S=int(rng.integers(2, 10)))          # band 5 ... 19
        second.append((lp, labels, term, np.arange(0, 2 * len(labels) + 2, 2)))                              # every even one
    pool = []
    for _ in range(8):
        lp, labels, term = _small(rng, V, T=int(rng.integers(16, 33)), S=int(rng.integers(1, 8)))
        pool.append((lp, labels, term, np.arange(1, 2 * len(labels) + 2, 3)))
    lats = first + [pool[i % len(pool)] for i in range(slots - pairs)] + second
    assert len(lats) == slots + pairs and all(R.fast_form(len(x[1]), V, 64, 4) == (V <= 64) for x in lats)
    lps, labs, terms, cuts = ([x[i] for x in lats] for i in range(4))
    M = len(LEVELS)
    bufs, z, st, rc = quant_call(eng, _lib, lps, labs, terms, cuts, LEVELS, 64, 4, pad=2, device=device)
    want = [(_lib.KA_ERR_ZERO_MASS if i % 3 == 1 else _lib.KA_ERR_BAD_LABEL if i % 6 == 2 else 0) for i in range(pairs)]
    assert list(st[:pairs]) == want and np.all(st[pairs:] == 0) and rc == want[1]
    for i in range(pairs):
        got = written(bufs[i], len(cuts[i]), M)
        if want[i]:
            assert np.all(got == -1) and ((z[i] == -np.inf) if want[i] == _lib.KA_ERR_ZERO_MASS else np.isnan(z[i])), i
    alone = {}
    for i in list(range(pairs)) + list(range(pairs, len(lats))):
        if i < pairs and want[i]:
            continue
        lp, labels, term, c = lats[i]
        if id(lp) not in alone:
            (b1,), z1, st1, _ = quant_call(eng, _lib, [lp], [labels], [term], [c], LEVELS, 64, 4)
            assert st1[0] == 0
            alone[id(lp)] = (written(b1, len(c), M), z1[0])
        q1, z1 = alone[id(lp)]
        assert np.array_equal(written(bufs[i], len(c), M), q1), (i, "reused" if i >= slots else "first or filler")
        assert _same(z[i], z1), i
    for i in range(len(lats) - 3, len(lats)):             # a few of those on an inherited slot against the definition
        lp, labels, term, c = lats[i]
        want_q, _, _ = _definition(eng, _lib, lp, labels, term, c, LEVELS, 64, 4)
        assert np.array_equal(written(bufs[i], len(c), M), want_q), i


def test_bad_arguments_fail_the_call_before_anything_is_launched(env):
    _, _lib, eng = env
    rng = np.random.default_rng(5)
    lp, labels, term = _small(rng, 39, T=40, S=10)
    good = dict(cuts=[0, 4, 8, 21], levels=LEVELS)

    def refused(**kw):
        args = {**good, **kw}
        (buf,), z, st, rc = quant_call(eng, _lib, [lp], [labels], [term], [args["cuts"]], args["levels"], 64, 4, pad=1,
                                       ld_q=args.get("ld_q"), M=args.get("M"))
        assert rc == _lib.KA_ERR_BAD_ARGS and np.all(buf == SENTINEL) and st[0] == 99, kw

    for cuts in ([4, 0], [0, 4, 4], [-1, 4], [0, 22]):                       # out of order, repeated, out of range (L = 21)
        refused(cuts=cuts)
    refused(M=0)
    refused(levels=tuple(np.linspace(0.1, 0.9, 9)))                         # M = 9
    for levels in ((2.0 ** -11, 0.5), (0.5, 1.0 - 2.0 ** -11), (0.5, 0.5), (0.9, 0.1), (float("nan"), 0.5)):
        refused(levels=levels)
    refused(ld_q=2)                                                         # ld_q < M
    (buf,), z, st, rc = quant_call(eng, _lib, [lp], [labels], [term], [good["cuts"]], LEVELS, 64, 4)
    assert rc == 0 and st[0] == 0 and np.all(written(buf, 4, 3)[0] == 0) and np.all(written(buf, 4, 3)[3] == 40)


def test_no_side_effects_on_the_best_path_call(env):
    ka, _lib, eng = env
    rng = np.random.default_rng(9)
    lp, labels, term = _small(rng, 39, T=300, S=120)
    before = ka.ctc_best_path(lp, labels, 64, 4)
    for V in (39, 80):
        x = _small(rng, V, T=200, S=90)
        assert quant_call(eng, _lib, [x[0]], [x[1]], [x[2]], [np.arange(0, 182, 2)], LEVELS, 64, 4)[3] == 0
    after = ka.ctc_best_path(lp, labels, 64, 4)
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def test_python_layer_gives_the_raw_calls_results(env):
    import torch
    ka, _lib, eng = env
    rng = np.random.default_rng(12)
    lats = [_small(rng, 39), _small(rng, 39, T=70, S=30), _small(rng, 39, T=1, S=2)]
    lps, labs, terms = ([x[i] for x in lats] for i in range(3))
    cuts = [np.arange(0, 2 * len(x) + 2, 2) for x in labs]
    bufs, z, st, rc = quant_call(eng, _lib, lps, labs, terms, cuts, LEVELS, 64, 4)
    assert rc == 0
    raw = [written(b, len(c), 3) for b, c in zip(bufs, cuts)]
    batch = ka.ctc_boundary_quantiles_batch(lps, labs, terms, cuts, LEVELS, 64, 4)
    dev, dst = ka.ctc_boundary_quantiles_device([torch.from_numpy(x).cuda() for x in lps], [torch.from_numpy(x).cuda() for x in labs],
                                                terms, cuts, LEVELS, 64, 4, return_status=True)
    assert dst == [0, 0, 0]
    for i in range(3):
        for q, ll in (batch[i], ka.ctc_boundary_quantiles(lps[i], labs[i], terms[i], cuts[i], LEVELS, 64, 4)):
            assert q.dtype == np.int32 and isinstance(ll, float) and np.array_equal(q, raw[i]) and ll == z[i]
        q, ll = dev[i]
        assert q.dtype == torch.int32 and q.is_cuda and np.array_equal(q.cpu().numpy(), raw[i]) and ll == z[i]
    # the default levels are LEVELS
    q, _ = ka.ctc_boundary_quantiles(lps[1], labs[1], terms[1], cuts[1], beam_size=64)
    assert np.array_equal(q, raw[1])
    # failures raise, or come back as statuses
    bad = lps[0].copy()
    bad[3, 3] = np.nan
    with pytest.raises(ValueError):
        ka.ctc_boundary_quantiles(bad, labs[0], terms[0], cuts[0], LEVELS, 64, 4)
    res, status = ka.ctc_boundary_quantiles_batch([bad, lps[1]], [labs[0], labs[1]], [terms[0], terms[1]], cuts[:2], LEVELS, 64, 4,
                                                  return_status=True)
    assert status == [_lib.KA_ERR_NAN, 0] and np.all(res[0][0] == -1) and np.isnan(res[0][1]) and np.array_equal(res[1][0], raw[1])
    # the caller's tensors: views into a wider one keep its other columns
    wide = torch.full((len(cuts[0]), 7), -5, dtype=torch.int32, device="cuda")
    (q, ll), = ka.ctc_boundary_quantiles_device([torch.from_numpy(lps[0]).cuda()], [labs[0]], [terms[0]], [cuts[0]], LEVELS, 64, 4,
                                                out=[wide[:, 2:5]])
    host = wide.cpu().numpy()
    assert np.array_equal(host[:, 2:5], raw[0]) and np.all(host[:, :2] == -5) and np.all(host[:, 5:] == -5)
    # the helpers on the call's own output, with the best path and the sampler's spread beside it
    path = np.asarray(ka.ctc_best_path(lps[1], labs[1], 64, 4)[0]).reshape(-1)
    seg_ends = [20, 45, 70]
    bc = ka.boundary_cuts(path, seg_ends, len(labs[1]))
    q, _ = ka.ctc_boundary_quantiles(lps[1], labs[1], int(path[-1]), bc, LEVELS, 64, 4)
    start, end = ka.segment_boundary_interval(q, bc, path, seg_ends, len(labs[1]))
    assert start.shape == end.shape == (3, 3) and np.all(start[0] == 0) and np.all(end[2] == 70)
    assert np.all(np.diff(start, axis=1) >= 0) and np.all(end[:2] >= start[:2])
