"""State visit probabilities on the GPU: ka_ctc_state_visits against the float64 reference per position
on the input families of posterior_ref.edge_cases(), Z against the label call's, the exact facts against the duration call on
the same input, T round the 32-frame block, failed lattices, memory modes, reused workspace slots and the Python layer.  Every
figure held against the model is printed through fb_harness.record."""
import functools

import numpy as np
import pytest

import posterior_ref as R
import visit_ref as VR
from duration_harness import duration_call
from fb_harness import engine, label_call, record
from visit_harness import GUARD, SENTINEL, visit_call, visit_call_one

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
    return lp, labels, terminal, beam, mm, VR.visits(lp, labels, terminal, beam, mm)


_results = {}


def _kernel(env, name):
    """One visit call and one duration call per case, shared by the tests below."""
    if name not in _results:
        _, _lib, eng = env
        lp, labels, terminal, beam, mm = _reference(name)[:5]
        (vis,), (xt,), z, st, rc = visit_call(eng, _lib, [lp], [labels], [terminal], beam, mm)
        assert rc == 0 and st[0] == 0, (name, rc, st)
        L = 2 * len(labels) + 1
        assert np.all(vis[L:] == SENTINEL) and np.all(xt[L:] == SENTINEL)
        (dur,), (tsum,), zd, st, rc = duration_call(eng, _lib, [lp], [labels], [terminal], beam, mm)
        assert rc == 0 and st[0] == 0 and _same(z[0], zd[0]), name
        _results[name] = (vis[:L], xt[:L], z[0], dur[:L], tsum[:L])
    return _results[name]


def _ratios(vis, xt, v, what=""):
    return VR.visit_ratio(vis, v["V"], v["E_V"], what), VR.visit_ratio(xt, v["X"], v["E_X"], what)


def _exact_facts(vis, xt, dur, tsum, terminal, n, what=""):
    """What holds without any tolerance, against the duration call on the same input."""
    assert vis[terminal] == 1.0, what
    assert np.all(vis[terminal + 1:] == 0.0) and np.all(xt[terminal + 1:] == 0.0), what
    assert np.all(vis[n == 0] == 0.0) and np.all(xt[n == 0] == 0.0), what
    assert np.all(vis >= 0.0) and np.all(vis <= dur) and np.all(xt <= tsum), (what, np.flatnonzero(~(vis <= dur))[:8])
    one = n == 1
    assert np.array_equal(_bits(vis[one]), _bits(dur[one])) and np.array_equal(_bits(xt[one]), _bits(tsum[one])), what


def test_the_cases_cover_both_forms_and_every_family():
    forms = {(k.split("_")[0], R.fast_form(*SHAPES[k][1:])) for k in NAMES}
    assert forms == {(f, x) for f in ("edge", "steep", "flat", "peaked", "geom") for x in (True, False)}


@pytest.mark.parametrize("name", NAMES)
def test_every_position_lies_within_the_model(env, name):
    _, _lib, eng = env
    lp, labels, terminal, beam, mm, v = _reference(name)
    vis, xt, z, dur, tsum = _kernel(env, name)
    rV, rX = _ratios(vis, xt, v, name)
    _, z_label, st, _ = label_call(eng, _lib, [lp], [labels], [terminal], beam, mm)
    assert st[0] == 0 and _same(z, z_label[0]), (name, z, z_label[0])
    record("visit", rV, VR.M_VISIT)
    record("exit_time", rX, VR.M_VISIT)
    record("z", R.z_ratio(z, v["ref"]), R.M_Z)


@pytest.mark.parametrize("name", NAMES)
def test_the_exact_facts_hold(env, name):
    terminal, v = _reference(name)[2], _reference(name)[5]
    vis, xt, _, dur, tsum = _kernel(env, name)
    _exact_facts(vis, xt, dur, tsum, terminal, v["n"], name)


def _gapped(V, mm, seed):
    """A lattice whose band (2 wide, 3 positions a frame; generic: 4 a frame under max_move 6) never holds every third
    position, nor the last three: L = 3 T + 1 (4 T + 1).  Every position a band holds is held by one frame."""
    step = 3 if mm <= 4 else 4
    T = 60
    S = step * T // 2
    lp, labels = R.sloped(T, S, 39, seed, alpha=1.0, zero_every=0)
    lp = R.pad_vocabulary(lp, V) if V != 39 else lp
    return lp, labels, R.live_terminals(lp, labels, 2, mm)[0], 2, mm


@pytest.mark.parametrize("V,mm", [(39, 4), (80, 4), (39, 6)], ids=["one_wavefront", "generic_V80", "generic_M6"])
def test_single_frame_positions_have_the_durations_bits(env, V, mm):
    _, _lib, eng = env
    # a steep case (398 of its 561 positions are held by one frame) in the form asked for, and a gapped one
    lp, labels, terminal, beam, _ = CASES["steep_T200_S280_V39_B2_M4"]()
    steep = (R.pad_vocabulary(lp, V) if V != 39 else lp, labels, R.live_terminals(lp, labels, beam, mm)[0], beam, mm)
    for lp, labels, terminal, beam, mm in (steep, _gapped(V, mm, seed=V + mm)):
        T, L = lp.shape[0], 2 * len(labels) + 1
        assert R.fast_form(len(labels), V, beam, mm) == (V <= 64 and mm <= 4)
        v = VR.visits(lp, labels, terminal, beam, mm)
        one = VR.single_frame_positions(T, L, beam)
        assert one.sum() >= L // 2 and np.sum(v["n"] == 0) >= (L // 4 if T == 60 else 0)
        for device in (False, True):
            (vis,), (xt,), z, st, rc = visit_call(eng, _lib, [lp], [labels], [terminal], beam, mm, device=device)
            (dur,), (tsum,), zd, _, rcd = duration_call(eng, _lib, [lp], [labels], [terminal], beam, mm, device=device)
            assert rc == 0 and rcd == 0 and np.all(vis[L:] == SENTINEL) and np.all(xt[L:] == SENTINEL) and _same(z[0], zd[0])
            assert not np.any(vis[:L] == SENTINEL) and not np.any(xt[:L] == SENTINEL)          # the sentinel is overwritten
            _exact_facts(vis[:L], xt[:L], dur[:L], tsum[:L], terminal, v["n"], (V, mm, T, device))
            assert np.sum(one & (vis[:L] > 0.0)) >= 20
            rV, rX = _ratios(vis[:L], xt[:L], v)
            record("visit", rV, VR.M_VISIT)
            record("exit_time", rX, VR.M_VISIT)


def _small(rng, V, T=None, S=None):
    T, S = T or int(rng.integers(30, 60)), S or int(rng.integers(3, 20))
    lp, labels = R.sloped(T, S, 39, int(rng.integers(1 << 30)), alpha=0.5, zero_every=5)
    lp = R.pad_vocabulary(lp, V) if V != 39 else lp
    return lp, labels, R.live_terminals(lp, labels, 64, 4)[0]


@pytest.mark.parametrize("V", [39, 80], ids=["one_wavefront", "generic"])
def test_frames_round_the_block_and_the_smallest_lattices(env, V):
    _, _lib, eng = env
    pad = lambda lp: R.pad_vocabulary(lp, V) if V != 39 else lp
    worst_V = worst_X = 0.0
    for T in (1, 31, 32, 33, 64, 65):
        for S, beam in ((7, 64), (40, 16)):
            lp, labels = R.sloped(T, S, 39, 900 + T + S, alpha=1.0, zero_every=5)
            live = R.live_terminals(lp, labels, beam, 4)
            if not live:                                  # (T = 1 under a 16-wide band of 81 positions reaches what max_move lets it)
                continue
            lp, terminal = pad(lp), live[0]
            L = 2 * S + 1
            v = VR.visits(lp, labels, terminal, beam, 4)
            vis, xt, z, rc = visit_call_one(eng, _lib, lp, labels, terminal, beam, 4)
            (dur,), (tsum,), zd, _, _ = duration_call(eng, _lib, [lp], [labels], [terminal], beam, 4)
            assert rc == 0 and np.all(vis[L:] == SENTINEL) and np.all(xt[L:] == SENTINEL) and _same(z, zd[0])
            _exact_facts(vis[:L], xt[:L], dur[:L], tsum[:L], terminal, v["n"], (T, S))
            rV, rX = _ratios(vis[:L], xt[:L], v, (T, S))
            worst_V, worst_X = max(worst_V, rV), max(worst_X, rX)
        # S = 0: one blank holds every frame, and is left at the last
        lp0 = pad(R.sloped(T, 1, 39, 5 + T)[0])
        vis, xt, z, rc = visit_call_one(eng, _lib, lp0, np.zeros(0, np.int32), 0, 64, 4)
        assert rc == 0 and vis[0] == 1.0 and xt[0] == T - 1 and np.all(vis[1:] == SENTINEL) and np.all(xt[1:] == SENTINEL)
    record("visit", worst_V, VR.M_VISIT)
    record("exit_time", worst_X, VR.M_VISIT)


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
    assert set(want) == {0, _lib.KA_ERR_BAD_LABEL, _lib.KA_ERR_NAN, _lib.KA_ERR_NONFINITE, _lib.KA_ERR_BAD_ARGS, _lib.KA_ERR_ZERO_MASS}
    lps, labs, terms = ([x[i] for x in lats] for i in range(3))
    vs, xs, z, st, rc = visit_call(eng, _lib, lps, labs, terms, 64, 4, device=device)
    assert rc == want[1] and list(st) == want
    for i, (lp, labels, term) in enumerate(lats):
        L = 2 * len(labels) + 1
        assert np.all(vs[i][L:] == SENTINEL) and np.all(xs[i][L:] == SENTINEL), i              # nothing written beyond [0, L)
        if want[i]:
            assert np.all(_bits(vs[i][:L]) == NAN64) and np.all(_bits(xs[i][:L]) == NAN64), i
            assert (z[i] == -np.inf) if want[i] == _lib.KA_ERR_ZERO_MASS else np.isnan(z[i]), i
    (alone,), (alone_x,), z1, _, _ = visit_call(eng, _lib, [good[0]], [good[1]], [good[2]], 64, 4)
    for i in (0, len(lats) - 1):
        assert np.array_equal(_bits(vs[i]), _bits(alone)) and np.array_equal(_bits(xs[i]), _bits(alone_x)) and z[i] == z1[0]
    v = VR.visits(*good, 64, 4)
    rV, rX = _ratios(alone[:-GUARD], alone_x[:-GUARD], v)
    record("visit", rV, VR.M_VISIT)
    record("exit_time", rX, VR.M_VISIT)


@pytest.mark.parametrize("V", [39, 80], ids=["one_wavefront", "generic"])
def test_null_exit_time_and_strided_rows(env, V):
    _, _lib, eng = env
    rng = np.random.default_rng(77 + V)
    lp, labels, term = _small(rng, V)
    L = 2 * len(labels) + 1
    vis, xt, z, rc = visit_call_one(eng, _lib, lp, labels, term, 64, 4)
    assert rc == 0 and np.all(vis[L:] == SENTINEL) and np.all(xt[L:] == SENTINEL)
    vis0, xt0, z0, rc = visit_call_one(eng, _lib, lp, labels, term, 64, 4, exit_time=False)
    assert rc == 0 and np.array_equal(_bits(vis0), _bits(vis)) and np.all(xt0 == SENTINEL) and z0 == z
    vis1, xt1, z1, rc = visit_call_one(eng, _lib, lp, labels, term, 64, 4, ld=V + 5)           # the other columns hold NaN
    assert rc == 0 and np.array_equal(_bits(vis1), _bits(vis)) and np.array_equal(_bits(xt1), _bits(xt)) and z1 == z
    # a batch with a NULL array, and one with a NULL entry, on both sides of the memory modes
    for device in (False, True):
        (d2, d3), none, zz, st, rc = visit_call(eng, _lib, [lp, lp], [labels, labels], [term, term], 64, 4, exit_time=False, device=device)
        assert rc == 0 and none is None and np.array_equal(_bits(d2), _bits(vis)) and np.array_equal(_bits(d3), _bits(vis))
        (d2, d3), (s2, s3), zz, st, rc = visit_call(eng, _lib, [lp, lp], [labels, labels], [term, term], 64, 4, exit_time=[False, True],
                                                    device=device)
        assert rc == 0 and np.all(s2 == SENTINEL) and np.array_equal(_bits(s3), _bits(xt)) and np.array_equal(_bits(d2), _bits(vis))
        assert zz[0] == zz[1] == z


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
    assert len(lats) == slots + pairs and all(R.fast_form(len(x[1]), V, 64, 4) == (V <= 64) for x in lats)
    lps, labs, terms = ([x[i] for x in lats] for i in range(3))
    vs, xs, z, st, rc = visit_call(eng, _lib, lps, labs, terms, 64, 4)
    assert all(st[i] == (_lib.KA_ERR_ZERO_MASS if i % 3 == 1 else _lib.KA_ERR_BAD_LABEL if i % 6 == 2 else 0) for i in range(pairs))
    assert np.all(st[pairs:] == 0)
    alone = {}
    worst_V = worst_X = 0.0
    for i in range(pairs, len(lats)):
        lp, labels, term = lats[i]
        if id(lp) not in alone:
            (d1,), (s1,), z1, st1, _ = visit_call(eng, _lib, [lp], [labels], [term], 64, 4)
            assert st1[0] == 0
            alone[id(lp)] = (d1, s1, z1[0])
        d1, s1, z1 = alone[id(lp)]
        assert np.array_equal(_bits(vs[i]), _bits(d1)) and np.array_equal(_bits(xs[i]), _bits(s1)), (i, "reused" if i >= slots else "filler")
        assert _same(z[i], z1), i
        if i >= len(lats) - 4:                            # a few of those on an inherited slot against the reference
            rV, rX = _ratios(vs[i][:-GUARD], xs[i][:-GUARD], VR.visits(lp, labels, term, 64, 4), i)
            worst_V, worst_X = max(worst_V, rV), max(worst_X, rX)
    record("visit", worst_V, VR.M_VISIT)
    record("exit_time", worst_X, VR.M_VISIT)


def test_no_side_effects_on_the_best_path_call(env):
    ka, _lib, eng = env
    rng = np.random.default_rng(9)
    lp, labels, term = _small(rng, 39, T=300, S=120)
    before = ka.ctc_best_path(lp, labels, 64, 4)
    for V in (39, 80):
        x = _small(rng, V, T=200, S=90)
        assert visit_call(eng, _lib, [x[0]], [x[1]], [x[2]], 64, 4)[4] == 0
    after = ka.ctc_best_path(lp, labels, 64, 4)
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def test_python_layer_gives_the_raw_calls_results(env):
    import torch
    ka, _lib, eng = env
    rng = np.random.default_rng(12)
    lats = [_small(rng, 39), _small(rng, 39, T=70, S=30), _small(rng, 39, T=1, S=2)]
    lps, labs, terms = ([x[i] for x in lats] for i in range(3))
    vs, xs, z, st, rc = visit_call(eng, _lib, lps, labs, terms, 64, 4)
    assert rc == 0
    batch = ka.ctc_state_visits_batch(lps, labs, terms, 64, 4)
    dev, dst = ka.ctc_state_visits_device([torch.from_numpy(x).cuda() for x in lps], [torch.from_numpy(x).cuda() for x in labs], terms, 64, 4,
                                          return_status=True)
    assert dst == [0, 0, 0]
    for i in range(3):
        for d, s, ll in (batch[i], ka.ctc_state_visits(lps[i], labs[i], terms[i], 64, 4)):
            assert d.dtype == s.dtype == np.float64 and isinstance(ll, float)
            assert np.array_equal(_bits(d), _bits(vs[i][:-GUARD])) and np.array_equal(_bits(s), _bits(xs[i][:-GUARD])) and ll == z[i]
        d, s, ll = dev[i]
        assert d.dtype == s.dtype == torch.float64 and d.is_cuda and s.is_cuda
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(vs[i][:-GUARD])) and np.array_equal(_bits(s.cpu().numpy()), _bits(xs[i][:-GUARD]))
        assert ll == z[i]
    # failures raise, or come back as statuses
    bad = lps[0].copy()
    bad[3, 3] = np.nan
    with pytest.raises(ValueError):
        ka.ctc_state_visits(bad, labs[0], terms[0], 64, 4)
    with pytest.raises(ValueError):
        ka.ctc_state_visits(lps[0], labs[0], 2 * len(labs[0]) + 1, 64, 4)
    res, status = ka.ctc_state_visits_batch([bad, lps[1]], [labs[0], labs[1]], [terms[0], terms[1]], 64, 4, return_status=True)
    assert status == [_lib.KA_ERR_NAN, 0] and np.all(np.isnan(res[0][0])) and np.isnan(res[0][2])
    assert np.array_equal(_bits(res[1][0]), _bits(vs[1][:-GUARD]))
    # the caller's tensors
    L0 = 2 * len(labs[0]) + 1
    out = [(torch.full((L0,), -7.0, dtype=torch.float64, device="cuda"), torch.full((L0,), -7.0, dtype=torch.float64, device="cuda"))]
    (d, s, ll), = ka.ctc_state_visits_device([torch.from_numpy(lps[0]).cuda()], [labs[0]], [terms[0]], 64, 4, out=out)
    assert d is out[0][0] and s is out[0][1]
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(vs[0][:-GUARD])) and np.array_equal(_bits(s.cpu().numpy()), _bits(xs[0][:-GUARD]))
    # the helpers on the call's own output, with the duration call beside it
    dur, _, _ = ka.ctc_state_durations(lps[1], labs[1], terms[1], 64, 4)
    vis, xt, _ = batch[1]
    first, last = ka.phoneme_spans(vis, xt, dur)
    seen = vis > 0
    assert np.all(first[seen] <= last[seen] + 1e-9) and np.all(np.isnan(last[~seen]))
    labels_v, blanks_v = ka.phoneme_visits(vis)
    assert len(labels_v) == len(labs[1]) and len(blanks_v) == len(labs[1]) + 1
