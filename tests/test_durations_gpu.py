"""Expected state durations on the GPU: ka_ctc_state_durations against the float64 reference per
position on the input families of posterior_ref.edge_cases(), the two sum identities, Z against the label call's, the bits
of a sequential float64 sum over the state call's rows, positions outside every band, failed lattices, memory modes, reused
workspace slots and the Python layer.  Every figure held against the model is printed through fb_harness.record."""
import functools

import numpy as np
import pytest

import duration_ref as DR
import posterior_ref as R
from duration_harness import GUARD, SENTINEL, duration_call, duration_call_one
from fb_harness import engine, label_call, record, state_call

pytestmark = pytest.mark.gpu

CASES = R.edge_cases()
SHAPES = R.case_shapes()
NAMES = [k for k, sh in SHAPES.items() if sh[0] <= 700]           # (the two 3000-frame lattices lie outside this file's sizes)
NAN64 = 0x7ff8000000000000


@pytest.fixture(scope="module")
def env():
    return engine()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


@functools.lru_cache(maxsize=None)
def _reference(name):
    lp, labels, terminal, beam, mm = CASES[name]()
    ref = R.ref_at(lp, labels, terminal, beam, mm)
    assert ref["status"] == R.OK, name
    return lp, labels, terminal, beam, mm, ref, DR.durations(ref, 2 * len(labels) + 1)


_results = {}


def _kernel(env, name):
    """One call per case, shared by the tests below."""
    if name not in _results:
        _, _lib, eng = env
        lp, labels, terminal, beam, mm = _reference(name)[:5]
        (dur,), (tsum,), z, st, rc = duration_call(eng, _lib, [lp], [labels], [terminal], beam, mm)
        assert rc == 0 and st[0] == 0, (name, rc, st)
        L = 2 * len(labels) + 1
        assert np.all(dur[L:] == SENTINEL) and np.all(tsum[L:] == SENTINEL)
        _results[name] = (dur[:L], tsum[:L], z[0])
    return _results[name]


def test_the_cases_cover_both_forms_and_every_family():
    forms = {(k.split("_")[0], R.fast_form(*SHAPES[k][1:])) for k in NAMES}
    assert forms == {(f, x) for f in ("edge", "steep", "flat", "peaked", "geom") for x in (True, False)}


@pytest.mark.parametrize("name", NAMES)
def test_every_position_lies_within_the_model(env, name):
    dref = _reference(name)[6]
    dur, tsum, _ = _kernel(env, name)
    rD = DR.duration_ratio(dur, dref["D"], dref["E_D"], dref["n"], name)
    # (position 0's only frame can be frame 0 and T = 1 has no other: B is then 0 exactly, with a model of 0)
    held = (dref["n"] > 0) & (dref["E_B"] > 0.0)
    assert np.all(tsum[~held] == 0.0), name
    rB = DR.duration_ratio(tsum, dref["B"], dref["E_B"], held, name) if held.any() else 0.0
    record("duration", rD, DR.M_DURATION)
    record("time_sum", rB, DR.M_DURATION)


@pytest.mark.parametrize("name", NAMES)
def test_sums_and_log_likelihood(env, name):
    _, _lib, eng = env
    lp, labels, terminal, beam, mm, ref, dref = _reference(name)
    dur, tsum, z = _kernel(env, name)
    rD, rB = DR.sums_ratio(dur, tsum, dref, lp.shape[0])
    _, z_label, st, _ = label_call(eng, _lib, [lp], [labels], [terminal], beam, mm)
    assert st[0] == 0 and _same(z, z_label[0]), (name, z, z_label[0])
    record("duration_sum", rD, DR.M_DURATION)
    record("time_sum_sum", rB, DR.M_DURATION)
    record("z", R.z_ratio(z, ref), R.M_Z)


@pytest.mark.parametrize("name", ["edge_T200_S230_V39_B32_M4_back1", "steep_T200_S280_V80_B7_M4", "peaked_T200_S60_V39_B16_M4",
                                  "steep_T260_S620_V39_B9_M6"])
def test_bits_of_a_sequential_sum_over_the_state_rows(env, name):
    _, _lib, eng = env
    lp, labels, terminal, beam, mm = _reference(name)[:5]
    T, L = lp.shape[0], 2 * len(labels) + 1
    (rows,), (lo,), z_s, st, rc = state_call(eng, _lib, [lp], [labels], [terminal], [np.arange(T)], beam, mm)
    assert rc == 0 and st[0] == 0
    want_D, want_B = DR.sequential_sums(rows, lo, L)
    dur, tsum, z = _kernel(env, name)
    assert np.array_equal(_bits(dur), _bits(want_D)), (name, np.flatnonzero(_bits(dur) != _bits(want_D))[:8])
    assert np.array_equal(_bits(tsum), _bits(want_B)), (name, np.flatnonzero(_bits(tsum) != _bits(want_B))[:8])
    assert _same(z, z_s[0])


def _gapped(V, mm, seed):
    """A lattice whose band (2 wide, 3 positions a frame; generic: 4 a frame under max_move 6) never holds every third
    position, nor the last three: L = 3 T + 1 (4 T + 1)."""
    step = 3 if mm <= 4 else 4
    T = 60
    S = step * T // 2
    lp, labels = R.sloped(T, S, 39, seed, alpha=1.0, zero_every=0)
    lp = R.pad_vocabulary(lp, V) if V != 39 else lp
    return lp, labels, R.live_terminals(lp, labels, 2, mm)[0], 2, mm


@pytest.mark.parametrize("V,mm", [(39, 4), (80, 4), (39, 6)], ids=["one_wavefront", "generic_V80", "generic_M6"])
def test_positions_outside_every_band_read_zero(env, V, mm):
    _, _lib, eng = env
    lp, labels, terminal, beam, mm = _gapped(V, mm, seed=V + mm)
    L = 2 * len(labels) + 1
    assert R.fast_form(len(labels), V, beam, mm) == (V <= 64 and mm <= 4)
    ref = R.ref_at(lp, labels, terminal, beam, mm)
    dref = DR.durations(ref, L)
    assert ref["status"] == R.OK and np.sum(dref["n"] == 0) >= L // 4
    for device in (False, True):
        (dur,), (tsum,), z, st, rc = duration_call(eng, _lib, [lp], [labels], [terminal], beam, mm, device=device)
        assert rc == 0 and np.all(dur[L:] == SENTINEL) and np.all(tsum[L:] == SENTINEL)
        assert not np.any(dur[:L] == SENTINEL) and not np.any(tsum[:L] == SENTINEL)            # the sentinel is overwritten
        record("duration", DR.duration_ratio(dur[:L], dref["D"], dref["E_D"], dref["n"]), DR.M_DURATION)   # (asserts the zeros)
        assert np.all(tsum[:L][dref["n"] == 0] == 0.0)


def _small(rng, V, T=None, S=None):
    T, S = T or int(rng.integers(30, 60)), S or int(rng.integers(3, 20))
    lp, labels = R.sloped(T, S, 39, int(rng.integers(1 << 30)), alpha=0.5, zero_every=5)
    lp = R.pad_vocabulary(lp, V) if V != 39 else lp
    return lp, labels, R.live_terminals(lp, labels, 64, 4)[0]


@pytest.mark.parametrize("V", [39, 80], ids=["one_wavefront", "generic"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_failed_lattices_beside_good_ones(env, V, device):
    _, _lib, eng = env
    rng = np.random.default_rng(31 + V)
    good = _small(rng, V)
    lats, want = [good], [0]
    lp, labels, term = _small(rng, V)
    bad = labels.copy()
    bad[len(bad) // 2] = V
    lats.append((lp, bad, term)); want.append(_lib.KA_ERR_BAD_LABEL)
    for value, code in ((np.nan, _lib.KA_ERR_NAN), (np.inf, _lib.KA_ERR_NONFINITE)):
        lp, labels, term = _small(rng, V)
        lp = lp.copy()
        lp[lp.shape[0] // 2, 3] = value
        lats.append((lp, labels, term)); want.append(code)
    lp, labels, term = _small(rng, V)
    lats.append((lp, labels, 2 * len(labels) + 1)); want.append(_lib.KA_ERR_BAD_ARGS)
    lats.append((lp, labels, -1)); want.append(_lib.KA_ERR_BAD_ARGS)
    lp, labels, term = _small(rng, V)
    lp = lp.copy()
    lp[:, 0] = -np.inf                                    # the last blank is reached only through -inf emissions
    lats.append((lp, labels, 2 * len(labels))); want.append(_lib.KA_ERR_ZERO_MASS)
    lats.append(good); want.append(0)
    lps, labs, terms = ([x[i] for x in lats] for i in range(3))
    durs, sums, z, st, rc = duration_call(eng, _lib, lps, labs, terms, 64, 4, device=device)
    assert rc == want[1] and list(st) == want
    for i, (lp, labels, term) in enumerate(lats):
        L = 2 * len(labels) + 1
        assert np.all(durs[i][L:] == SENTINEL) and np.all(sums[i][L:] == SENTINEL), i          # nothing written beyond [0, L)
        if want[i]:
            assert np.all(_bits(durs[i][:L]) == NAN64) and np.all(_bits(sums[i][:L]) == NAN64), i
            assert (z[i] == -np.inf) if want[i] == _lib.KA_ERR_ZERO_MASS else np.isnan(z[i]), i
    (alone,), (alone_b,), z1, _, _ = duration_call(eng, _lib, [good[0]], [good[1]], [good[2]], 64, 4)
    for i in (0, len(lats) - 1):
        assert np.array_equal(_bits(durs[i]), _bits(alone)) and np.array_equal(_bits(sums[i]), _bits(alone_b)) and z[i] == z1[0]
    dref = DR.durations(R.ref_at(*good, 64, 4), len(alone) - GUARD)
    record("duration", DR.duration_ratio(alone[:-GUARD], dref["D"], dref["E_D"], dref["n"]), DR.M_DURATION)


@pytest.mark.parametrize("V", [39, 80], ids=["one_wavefront", "generic"])
def test_null_time_sum_strided_rows_and_the_smallest_lattices(env, V):
    _, _lib, eng = env
    rng = np.random.default_rng(77 + V)
    lp, labels, term = _small(rng, V)
    L = 2 * len(labels) + 1
    dur, tsum, z, rc = duration_call_one(eng, _lib, lp, labels, term, 64, 4)
    assert rc == 0 and np.all(dur[L:] == SENTINEL) and np.all(tsum[L:] == SENTINEL)
    dur0, tsum0, z0, rc = duration_call_one(eng, _lib, lp, labels, term, 64, 4, time_sum=False)
    assert rc == 0 and np.array_equal(_bits(dur0), _bits(dur)) and np.all(tsum0 == SENTINEL) and z0 == z
    dur1, tsum1, z1, rc = duration_call_one(eng, _lib, lp, labels, term, 64, 4, ld=V + 5)      # the other columns hold NaN
    assert rc == 0 and np.array_equal(_bits(dur1), _bits(dur)) and np.array_equal(_bits(tsum1), _bits(tsum)) and z1 == z
    # a batch with a NULL array, and one with a NULL entry, on both sides of the memory modes
    for device in (False, True):
        (d2, d3), none, zz, st, rc = duration_call(eng, _lib, [lp, lp], [labels, labels], [term, term], 64, 4, time_sum=False, device=device)
        assert rc == 0 and none is None and np.array_equal(_bits(d2), _bits(dur)) and np.array_equal(_bits(d3), _bits(dur))
        (d2, d3), (s2, s3), zz, st, rc = duration_call(eng, _lib, [lp, lp], [labels, labels], [term, term], 64, 4, time_sum=[False, True],
                                                       device=device)
        assert rc == 0 and np.all(s2 == SENTINEL) and np.array_equal(_bits(s3), _bits(tsum)) and np.array_equal(_bits(d2), _bits(dur))
        assert zz[0] == zz[1] == z
    # S = 0 (one blank holds every frame) and T = 1, alone and together
    for T, S in ((1, 0), (1, 2), (37, 0)):
        lp1 = R.pad_vocabulary(R.sloped(T, 1, 39, 5 + T + S)[0], V) if V != 39 else R.sloped(T, 1, 39, 5 + T + S)[0]
        labels1 = np.arange(1, S + 1, dtype=np.int32)
        term1 = R.live_terminals(lp1, labels1, 64, 4)[0]
        dur, tsum, z, rc = duration_call_one(eng, _lib, lp1, labels1, term1, 64, 4)
        dref = DR.durations(R.ref_at(lp1, labels1, term1, 64, 4), 2 * S + 1)
        assert rc == 0 and np.all(dur[2 * S + 1:] == SENTINEL)
        if S == 0:
            assert dur[0] == T and tsum[0] == T * (T - 1) / 2                                   # gamma is 1.0 exactly in every frame
        if T == 1:
            assert dur[term1] == 1.0 and dur[:2 * S + 1].sum() == 1.0 and np.all(tsum[:2 * S + 1] == 0.0)
        record("duration", DR.duration_ratio(dur[:2 * S + 1], dref["D"], dref["E_D"], dref["n"]), DR.M_DURATION)


@pytest.mark.parametrize("V,slots,pairs", [(39, 1024, 48), (80, 512, 24)], ids=["one_wavefront_1072", "generic_536"])
def test_a_reused_slot_gives_the_bits_of_a_lattice_sent_alone(env, V, slots, pairs):
    """Lattice slots + k runs on slot k after lattice k (launch_fb_ck: lattice i on workgroup i mod grid): after a wider and
    longer one, which every third time failed after its forward pass or before it."""
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
        first.append((lp, labels, term))
        second.append(_small(rng, V, T=int(rng.integers(20, 40)), S=int(rng.integers(2, 10))))               # band 5 ... 19
    pool = [_small(rng, V, T=int(rng.integers(16, 33)), S=int(rng.integers(1, 8))) for _ in range(8)]
    lats = first + [pool[i % len(pool)] for i in range(slots - pairs)] + second
    assert len(lats) > slots and all(R.fast_form(len(x[1]), V, 64, 4) == (V <= 64) for x in lats)
    lps, labs, terms = ([x[i] for x in lats] for i in range(3))
    durs, sums, z, st, rc = duration_call(eng, _lib, lps, labs, terms, 64, 4)
    assert all(st[i] == (_lib.KA_ERR_ZERO_MASS if i % 3 == 1 else _lib.KA_ERR_BAD_LABEL if i % 6 == 2 else 0) for i in range(pairs))
    assert np.all(st[pairs:] == 0)
    alone = {}
    worst = 0.0
    for i in range(pairs, len(lats)):
        lp, labels, term = lats[i]
        if id(lp) not in alone:
            (d1,), (s1,), z1, st1, _ = duration_call(eng, _lib, [lp], [labels], [term], 64, 4)
            assert st1[0] == 0
            alone[id(lp)] = (d1, s1, z1[0])
        d1, s1, z1 = alone[id(lp)]
        assert np.array_equal(_bits(durs[i]), _bits(d1)) and np.array_equal(_bits(sums[i]), _bits(s1)), (i, "reused" if i >= slots else "filler")
        assert _same(z[i], z1), i
        if i >= len(lats) - 4:                            # a few of those on an inherited slot against the reference
            dref = DR.durations(R.ref_at(lp, labels, term, 64, 4), 2 * len(labels) + 1)
            worst = max(worst, DR.duration_ratio(durs[i][:-GUARD], dref["D"], dref["E_D"], dref["n"], i))
    record("duration", worst, DR.M_DURATION)


def test_no_side_effects_on_the_best_path_call(env):
    ka, _lib, eng = env
    rng = np.random.default_rng(9)
    lp, labels, term = _small(rng, 39, T=300, S=120)
    before = ka.ctc_best_path(lp, labels, 64, 4)
    for V in (39, 80):
        x = _small(rng, V, T=200, S=90)
        assert duration_call(eng, _lib, [x[0]], [x[1]], [x[2]], 64, 4)[4] == 0
    after = ka.ctc_best_path(lp, labels, 64, 4)
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def test_python_layer_gives_the_raw_calls_results(env):
    import torch
    ka, _lib, eng = env
    rng = np.random.default_rng(12)
    lats = [_small(rng, 39), _small(rng, 39, T=70, S=30), _small(rng, 39, T=1, S=2)]
    lps, labs, terms = ([x[i] for x in lats] for i in range(3))
    durs, sums, z, st, rc = duration_call(eng, _lib, lps, labs, terms, 64, 4)
    assert rc == 0
    batch = ka.ctc_state_durations_batch(lps, labs, terms, 64, 4)
    dev, dst = ka.ctc_state_durations_device([torch.from_numpy(x).cuda() for x in lps], [torch.from_numpy(x).cuda() for x in labs], terms, 64, 4,
                                             return_status=True)
    assert dst == [0, 0, 0]
    for i in range(3):
        for d, s, ll in (batch[i], ka.ctc_state_durations(lps[i], labs[i], terms[i], 64, 4)):
            assert d.dtype == s.dtype == np.float64 and isinstance(ll, float)
            assert np.array_equal(_bits(d), _bits(durs[i][:-GUARD])) and np.array_equal(_bits(s), _bits(sums[i][:-GUARD])) and ll == z[i]
        d, s, ll = dev[i]
        assert d.dtype == s.dtype == torch.float64 and d.is_cuda and s.is_cuda
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(durs[i][:-GUARD])) and np.array_equal(_bits(s.cpu().numpy()), _bits(sums[i][:-GUARD]))
        assert ll == z[i]
    # failures raise, or come back as statuses
    bad = lps[0].copy()
    bad[3, 3] = np.nan
    with pytest.raises(ValueError):
        ka.ctc_state_durations(bad, labs[0], terms[0], 64, 4)
    with pytest.raises(ValueError):
        ka.ctc_state_durations(lps[0], labs[0], 2 * len(labs[0]) + 1, 64, 4)
    res, status = ka.ctc_state_durations_batch([bad, lps[1]], [labs[0], labs[1]], [terms[0], terms[1]], 64, 4, return_status=True)
    assert status == [_lib.KA_ERR_NAN, 0] and np.all(np.isnan(res[0][0])) and np.isnan(res[0][2])
    assert np.array_equal(_bits(res[1][0]), _bits(durs[1][:-GUARD]))
    # the caller's tensors
    L0 = 2 * len(labs[0]) + 1
    out = [(torch.full((L0,), -7.0, dtype=torch.float64, device="cuda"), torch.full((L0,), -7.0, dtype=torch.float64, device="cuda"))]
    (d, s, ll), = ka.ctc_state_durations_device([torch.from_numpy(lps[0]).cuda()], [labs[0]], [terms[0]], 64, 4, out=out)
    assert d is out[0][0] and s is out[0][1] and np.array_equal(_bits(d.cpu().numpy()), _bits(durs[0][:-GUARD]))


def test_boundary_shift_is_zero_on_a_peaked_lattice(env):
    ka, _lib, eng = env
    T, S, V, beam, mm = 200, 60, 39, 16, 4
    lp, labels, terminal = R.peaked(T, S, V, beam, mm, seed=7)
    L = 2 * S + 1
    ref = R.ref_at(lp, labels, terminal, beam, mm)
    dref = DR.durations(ref, L)
    hist, _ = DR.best_paths_histogram(lp, labels, terminal, beam, mm)
    path = DR.likeliest_path(ref)
    ends = DR.peaked_boundaries(path, hist, S)
    assert len(ends) == 3
    dur, tsum, ll = ka.ctc_state_durations(lp, labels, terminal, beam, mm)
    record("duration", DR.duration_ratio(dur, dref["D"], dref["E_D"], dref["n"]), DR.M_DURATION)
    start, end = ka.segment_boundary_shift(dur, path, ends + [T + 5], S)
    tol = DR.M_DURATION * float(np.sum(dref["E_D"] + DR.peaked_bound(dref)))
    assert np.all(np.abs(start) <= tol) and np.all(np.abs(end) <= tol) and end[3] == 0.0, (start, end, tol)
    labs_d, blanks_d = ka.phoneme_durations(dur)
    assert abs(labs_d.sum() + blanks_d.sum() - T) <= DR.M_DURATION * float(dref["E_D"].sum())
