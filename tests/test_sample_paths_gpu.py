"""The path sampling kernels against tests/sample_ref.py, draw by draw, through the raw C ABI (tests/sample_harness.py), and
the Python front end against the raw call.

Every draw is checked conditionally: for every sample and every t >= 1 the reference is asked for the running sums of the draw
from the kernel's own s_t, and the kernel's s_{t-1} must be the reference's choice unless the draw is undecidable (U within
sample_ref.DELTA = 2^-26 of a threshold: then either neighbour of the threshold).  Undecidable draws are counted and held to
the caps of tests/test_sample_paths_cpu.py: at most 3 in a case, at most 1e-5 of all draws."""
import functools

import numpy as np
import pytest

import posterior_ref as R
import sample_ref as S
from fb_harness import engine, label_call, tiny
from sample_harness import SENTINEL, sample_call, sample_call_one

pytestmark = pytest.mark.gpu

SEED = 20240
KS = (1, 7, 64)


@pytest.fixture(scope="module")
def env():
    return engine()


@functools.lru_cache(maxsize=None)
def _case(name):
    lp, labels, term, beam, mm = R.edge_cases()[name]()
    return lp, labels, term, beam, mm, S.Lattice(lp, labels, beam, mm)


def _items():
    out = []
    for name, (T, Sn, V, beam, mm) in R.case_shapes().items():
        fast = R.fast_form(Sn, V, beam, mm)
        out.append((name, "one_wavefront" if fast else "generic", False))
        if fast:
            out.append((name, "generic", True))
    return out


def _check(lat, paths, seed, term, what):
    wrong, ties = S.check_draws(lat, paths, seed, term)
    assert wrong == [], (what, wrong[:5], len(wrong))
    for k, row in enumerate(paths):
        assert S.valid_path(lat, row, term) is None, (what, k, S.valid_path(lat, row, term))
    return ties


def _run_item(eng, _lib, name, form, pad):
    """One case in one form with K in KS: (draws, undecidable draws, None or what is wrong)."""
    lp, labels, term, beam, mm, lat = _case(name)
    lpk = R.pad_vocabulary(lp, 80) if pad else lp
    assert R.fast_form(len(labels), lpk.shape[1], beam, mm) == (form == "one_wavefront")
    bufs, ll, st, rc = sample_call(eng, _lib, [lpk] * len(KS), [labels] * len(KS), [term] * len(KS), KS, [SEED + K for K in KS], beam, mm)
    if rc != 0 or np.any(st != 0):
        return 0, 0, ("status", rc, st.tolist())
    draws = ties = 0
    for K, paths in zip(KS, bufs):
        if paths.shape != (K, lat.T):
            return draws, ties, ("shape", paths.shape)
        wrong, n = S.check_draws(lat, paths, SEED + K, term)
        bad = [(k, S.valid_path(lat, row, term)) for k, row in enumerate(paths) if S.valid_path(lat, row, term) is not None]
        if wrong or bad:
            return draws, ties, (K, wrong[:5], len(wrong), bad[:3])
        ties += n
        draws += K * (lat.T - 1)
    return draws, ties, None


@pytest.fixture(scope="module")
def every_item(env):
    """Every case in every form, run and checked once: (name, form) -> (draws, undecidable draws, None or what is wrong).
    The per-case tests and the suite's cap read it, so either can run alone and in any order."""
    ka, _lib, eng = env
    return {(name, form): _run_item(eng, _lib, name, form, pad) for name, form, pad in _items()}


@pytest.mark.parametrize("name,form,pad", _items(), ids=[f"{n}-{f}" for n, f, _ in _items()])
def test_every_draw_is_the_references_choice_from_the_kernels_own_state(every_item, name, form, pad):
    draws, ties, wrong = every_item[(name, form)]
    print("undecidable draws:", ties, "of", draws)
    assert wrong is None, (name, form, wrong)
    assert ties <= 3


def test_undecidable_draws_stay_under_the_suites_cap(every_item):
    draws = sum(v[0] for v in every_item.values())
    ties = sum(v[1] for v in every_item.values())
    print("undecidable draws:", ties, "of", draws)
    assert draws > 0 and ties <= 1e-5 * draws


@pytest.mark.parametrize("form", ["one_wavefront", "generic"])
@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 64, 65])
def test_block_edges_equal_the_reference_outright(env, T, form):
    ka, _lib, eng = env
    rng = np.random.default_rng(700 + T)
    for zero, ninf in ((False, False), (True, False), (False, True), (True, True)):
        lp, labels = tiny(rng, T, 4, 6, zero_label=zero, ninf=ninf)
        live = R.live_terminals(lp, labels, 1000, 4)
        assert live
        lat = S.Lattice(lp, labels, 1000, 4)
        lpk = R.pad_vocabulary(lp, 80) if form == "generic" else lp
        for term in {live[0], live[-1], min(live)}:             # the likeliest, the least likely, and the lowest: below the top
            want = S.sample_paths(lp, labels, term, 64, SEED + T, 1000, 4, lattice=lat)
            (got,), ll, st, rc = sample_call(eng, _lib, [lpk], [labels], [term], 64, SEED + T, 1000, 4)
            assert rc == 0 and st[0] == 0
            ties = _check(lat, got, SEED + T, term, (T, form, zero, ninf, term))
            if ties == 0 and S.undecidable_draws(lat, want, SEED + T) == 0:
                assert np.array_equal(got, want), (T, form, zero, ninf, term)


def test_fewer_samples_are_a_prefix_and_a_seed_changes_the_paths(env):
    ka, _lib, eng = env
    for name in ("steep_T200_S280_V39_B7_M4", "steep_T200_S280_V80_B7_M4"):
        lp, labels, term, beam, mm, lat = _case(name)
        (a, b, c), ll, st, rc = sample_call(eng, _lib, [lp] * 3, [labels] * 3, [term] * 3, [64, 8, 64], [SEED, SEED, SEED + 1], beam, mm)
        assert rc == 0
        assert np.array_equal(a[:8], b)
        assert np.any(a != c)
        one, z, rc = sample_call_one(eng, _lib, lp, labels, term, 64, SEED, beam, mm)
        assert rc == 0 and np.array_equal(one, a) and z == ll[0]          # alone or in a batch: the same bits


def test_pad_columns_and_rows_beyond_n_samples_keep_the_sentinel(env):
    ka, _lib, eng = env
    for name in ("geom_T65_S5_V39_B1000_M4", "edge_T400_S150_V80_B64_M4_back0"):
        lp, labels, term, beam, mm, lat = _case(name)
        T = lat.T
        (buf,), ll, st, rc = sample_call(eng, _lib, [lp], [labels], [term], 7, SEED, beam, mm, pad=5, extra_rows=3)
        assert rc == 0 and buf.shape == (10, T + 5)
        assert np.all(buf[:7, T:] == SENTINEL) and np.all(buf[7:] == SENTINEL) and np.all(buf[:7, :T] >= 0)
        one, z, rc = sample_call_one(eng, _lib, lp, labels, term, 7, SEED, beam, mm, ld_paths=T + 5, rows=9)
        assert rc == 0 and np.array_equal(one[:7, :T], buf[:7, :T]) and np.all(one[:7, T:] == SENTINEL) and np.all(one[7:] == SENTINEL)


@pytest.mark.parametrize("V", [39, 80], ids=["one_wavefront", "generic"])
def test_failed_lattices_read_minus_one_and_leave_the_others_alone(env, V):
    ka, _lib, eng = env
    lp, labels = R.sloped(70, 12, 39, 31, alpha=0.5, zero_every=5)
    lp = R.pad_vocabulary(lp, V) if V != 39 else lp
    term = R.live_terminals(lp, labels, 16, 4)[0]
    bad_label = labels.copy(); bad_label[3] = V
    nan = lp.copy(); nan[40, 2] = np.nan
    inf = lp.copy(); inf[5, 1] = np.inf
    dead = lp.copy(); dead[:, 0] = -np.inf
    lats = [(lp, labels, term), (lp, bad_label, term), (nan, labels, term), (inf, labels, term), (lp, labels, 2 * 12 + 1),
            (dead, labels, 2 * 12), (lp, labels, term)]
    want = [0, _lib.KA_ERR_BAD_LABEL, _lib.KA_ERR_NAN, _lib.KA_ERR_NONFINITE, _lib.KA_ERR_BAD_ARGS, _lib.KA_ERR_ZERO_MASS, 0]
    lps, labs, terms = ([x[i] for x in lats] for i in range(3))
    bufs, ll, st, rc = sample_call(eng, _lib, lps, labs, terms, 9, SEED, 16, 4, pad=2, extra_rows=1)
    occs, ll_l, st_l, rc_l = label_call(eng, _lib, lps, labs, terms, 16, 4)
    assert list(st) == want == list(st_l) and rc == rc_l == want[1]
    assert np.array_equal(ll.view(np.int64), ll_l.view(np.int64))
    good, z, rc1 = sample_call_one(eng, _lib, lp, labels, term, 9, SEED, 16, 4)
    assert rc1 == 0
    for i, buf in enumerate(bufs):
        assert np.all(buf[:9, 70:] == SENTINEL) and np.all(buf[9:] == SENTINEL)
        if want[i]:
            assert np.all(buf[:9, :70] == -1), i
        else:
            assert np.array_equal(buf[:9, :70], good) and ll[i] == z


def test_bad_call_arguments(env):
    ka, _lib, eng = env
    lp, labels, term, beam, mm, lat = _case("geom_T65_S5_V39_B1000_M4")
    for K in (0, 65):
        buf, z, rc = sample_call_one(eng, _lib, lp, labels, term, K, SEED, beam, mm, rows=2)
        assert rc == _lib.KA_ERR_BAD_ARGS and np.all(buf == SENTINEL)
    buf, z, rc = sample_call_one(eng, _lib, lp, labels, term, 2, SEED, beam, mm, ld_paths=lat.T - 1)
    assert rc == _lib.KA_ERR_BAD_ARGS and np.all(buf == SENTINEL)
    bufs, ll, st, rc = sample_call(eng, _lib, [lp, lp], [labels, labels], [term, term], [4, 65], SEED, beam, mm)
    assert rc == _lib.KA_ERR_BAD_ARGS and all(np.all(b == SENTINEL) for b in bufs)


@pytest.mark.parametrize("V,slots,pairs", [(39, 1024, 76), (80, 512, 28)], ids=["one_wavefront_1100", "generic_540"])
def test_a_reused_slot_gives_the_bits_of_a_lattice_sent_alone(env, V, slots, pairs):
    """Lattice slots + k runs on slot k after lattice k, which is longer and wider, and every third of which fails."""
    ka, _lib, eng = env
    rng = np.random.default_rng(V)

    def lattice(T, Sn):
        lp, labels = R.sloped(T, Sn, 39, int(rng.integers(1 << 30)), alpha=0.5, zero_every=5)
        lp = R.pad_vocabulary(lp, V) if V != 39 else lp
        return lp, labels, R.live_terminals(lp, labels, 64, 4)[0]

    first, second = [], []
    for k in range(pairs):
        T2, S2 = int(rng.integers(40, 100)), int(rng.integers(2, 12))
        lp, labels, term = lattice(T2 + int(rng.integers(33, 100)), int(rng.integers(40, 70)))
        if k % 3 == 0:
            lp = lp.copy()
            lp[lp.shape[0] // 2, 3] = np.nan
        first.append((lp, labels, term, int(rng.integers(1, 65))))
        second.append(lattice(T2, S2) + (int(rng.integers(1, 65)),))
    pool = [lattice(int(rng.integers(20, 60)), int(rng.integers(1, 12))) + (int(rng.integers(1, 65)),) for _ in range(16)]
    lats = first + [pool[i % 16] for i in range(slots - pairs)] + second
    assert len(lats) > slots and all(R.fast_form(len(x[1]), V, 64, 4) == (V <= 64) for x in lats)
    lps, labs, terms, Ks = ([x[i] for x in lats] for i in range(4))
    seeds = [SEED + i % 5 for i in range(len(lats))]
    bufs, ll, st, rc = sample_call(eng, _lib, lps, labs, terms, Ks, seeds, 64, 4)
    alone = {}
    for i, (lp, labels, term, K) in enumerate(lats):
        key = (id(lp), seeds[i])
        if key not in alone:
            alone[key] = sample_call(eng, _lib, [lp], [labels], [term], K, seeds[i], 64, 4)
        (b1,), l1, s1, _ = alone[key]
        assert st[i] == s1[0] == (_lib.KA_ERR_NAN if i < pairs and i % 3 == 0 else 0), i
        assert np.array_equal(bufs[i], b1) and ll[i:i + 1].view(np.int64)[0] == l1.view(np.int64)[0], i
    i = len(lats) - 1                                                   # one inherited slot against the reference
    lat = S.Lattice(lps[i][:, :39], labs[i], 64, 4)
    _check(lat, bufs[i], seeds[i], terms[i], "slot")


@pytest.mark.parametrize("name", ["edge_T400_S150_V39_B16_M4_back0", "edge_T400_S150_V80_B64_M4_back0", "geom_T1_S5_V39_B1000_M4"])
def test_log_likelihood_has_the_label_calls_bits(env, name):
    ka, _lib, eng = env
    lp, labels, term, beam, mm, lat = _case(name)
    bufs, ll, st, rc = sample_call(eng, _lib, [lp], [labels], [term], 3, SEED, beam, mm)
    occs, ll_l, st_l, rc_l = label_call(eng, _lib, [lp], [labels], [term], beam, mm)
    assert rc == rc_l == 0 and ll.view(np.int64)[0] == ll_l.view(np.int64)[0]


def test_python_front_end_equals_the_raw_call(env):
    import torch
    ka, _lib, eng = env
    names = ("steep_T200_S280_V39_B7_M4", "geom_T65_S5_V39_B1000_M4")
    cases = [_case(n) for n in names]
    beam, mm = 7, 4
    lps, labs, terms = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    terms[1] = R.live_terminals(lps[1], labs[1], beam, mm)[0]
    raw, ll, st, rc = sample_call(eng, _lib, lps, labs, terms, [64, 5], [SEED, SEED + 1], beam, mm)
    assert rc == 0
    res, status = ka.ctc_sample_paths_batch(lps, labs, terms, [64, 5], [SEED, SEED + 1], beam, mm, return_status=True)
    assert status == [0, 0]
    for (p, z), r, z0 in zip(res, raw, ll):
        assert p.dtype == np.int32 and np.array_equal(p, r) and z == z0
    d_lp = [torch.from_numpy(x).cuda() for x in lps]
    d_lab = [torch.from_numpy(x).cuda() for x in labs]
    res = ka.ctc_sample_paths_device(d_lp, d_lab, terms, [64, 5], [SEED, SEED + 1], beam, mm)
    for (p, z), r, z0 in zip(res, raw, ll):
        assert p.dtype == torch.int32 and np.array_equal(p.cpu().numpy(), r) and z == z0
    wide = [torch.full((K, x.shape[0] + 3), SENTINEL, dtype=torch.int32, device="cuda") for K, x in zip((64, 5), lps)]
    out = [w[:, :x.shape[0]] for w, x in zip(wide, lps)]
    res = ka.ctc_sample_paths_device(d_lp, d_lab, terms, [64, 5], [SEED, SEED + 1], beam, mm, out=out)
    for (p, z), w, r in zip(res, wide, raw):
        assert np.array_equal(w.cpu().numpy()[:, :r.shape[1]], r) and bool(torch.all(w[:, r.shape[1]:] == SENTINEL))
    p1, z1 = ka.ctc_sample_paths(lps[0], labs[0], terms[0], 64, SEED, beam, mm)
    assert np.array_equal(p1, raw[0]) and z1 == ll[0]
    with pytest.raises(ValueError):
        ka.ctc_sample_paths(lps[0], labs[0], terms[0], 65, SEED, beam, mm)


def test_segment_boundary_spread_end_to_end(env):
    ka, _lib, eng = env
    T, Sn = 240, 40
    lp, labels = R.sloped(T, Sn, 39, 77, alpha=0.3)
    best = np.asarray(ka.ctc_best_path(lp, labels, 64, 4)[0]).astype(np.int64)
    paths, z = ka.ctc_sample_paths(lp, labels, best, 64, SEED, 64, 4)
    seg_ends = [60, 130, 200, 260]
    sq, ss, eq, es = ka.segment_boundary_spread(paths, best, seg_ends, Sn)
    assert sq.shape == eq.shape == (4, 3) and np.all(np.diff(sq, axis=1) >= 0) and np.all(np.diff(eq, axis=1) >= 0)
    assert np.all(ss >= 0) and np.all(es >= 0) and np.all(eq[3] == T) and es[3] == 0.0
    dur, _, z2 = ka.ctc_state_durations(lp, labels, best, 64, 4)
    assert z == z2
    start, end = ka.segment_boundary_shift(dur, best, seg_ends, Sn)
    cuts = [2 * min(int(best[b]) // 2, Sn) for b in (60, 130, 200)]
    tau = ka.sampled_crossing_frames(paths, cuts).astype(np.float64)
    want = ka.expected_crossing_frames(dur, cuts)
    assert np.all(np.abs(tau.mean(axis=0) - want) <= 5.0 * np.maximum(tau.std(axis=0, ddof=1), 0.5) / 8.0)


def _unique_peaked(T, Sn, V, beam, mm, seed):
    """posterior_ref.peaked's construction with distinct labels of non-zero value: peaked's own label value 0 and repeated
    neighbours make several best paths tie exactly, and then the samples spread over them."""
    rng = np.random.default_rng(seed)
    labels = (1 + rng.permutation(V - 1)[:Sn]).astype(np.int32)
    lab = R.expand(labels)
    L = len(lab)
    lo, hi = R.windows(T, L, beam)
    s, states = 0, []
    for t in range(T):
        want = min(L - 1, (L * (t + 1)) // T + int(rng.integers(-1, 2)))
        ok = [j for j in range(mm) if lo[t] <= s + j < hi[t] and not (j >= 2 and j % 2 == 0 and lab[s + j] == 0)]
        s += min(ok, key=lambda j: abs(s + j - want))
        states.append(s)
    logits = -rng.uniform(30.0, 60.0, size=(T, V))
    logits[np.arange(T), lab[states]] = 0.0
    return R._normalise(logits), labels, np.array(states, np.int32)


@pytest.mark.parametrize("V", [39, 80], ids=["one_wavefront", "generic"])
def test_on_peaked_inputs_with_a_unique_best_path_every_sample_is_that_path(env, V):
    ka, _lib, eng = env
    lp, labels, states = _unique_peaked(150, 30, 39, 16, 4, 5)
    ref = R.ref_at(lp, labels, int(states[-1]), 16, 4)
    assert all(g[states[t] - lo] > 1.0 - 1e-9 for t, (lo, g) in enumerate(ref["gamma"]))      # the path holds all the mass
    lpk = R.pad_vocabulary(lp, V) if V != 39 else lp
    (got,), ll, st, rc = sample_call(eng, _lib, [lpk], [labels], [int(states[-1])], 64, SEED, 16, 4)
    assert rc == 0 and np.all(got == states[None, :])
