"""State posteriors at chosen frames on the MI355X, through the C ABI and the Python API, against the float64 reference
(tests/posterior_ref.forward_backward(..., full=True)): |d gamma| <= 1e-3, |row sum - 1| <= 1e-4, band_lo equal to the
reference's lo, Z within 1e-9 max(1, |Z|) of ka_ctc_label_posteriors' Z, gamma at (T-1, s*) exactly 1; cross-checked with
the label occupancy and the path posteriors of the same lattice, and end to end through the boundary confidence.  Beside
those, the per-cell check of DESIGN.md section 4.21: every cell within posterior_ref.state_tolerance (M_STATE x
state_error_model) where the reference is 2^-120 or more and below 2^-119 elsewhere (posterior_ref.state_ratio), and Z
within posterior_ref.z_tolerance."""
import numpy as np
import pytest

import posterior_ref as R
from fb_harness import band_width as _W, engine, label_call_one as _label_call, record, state_call as _call, state_call_one
from golden_util import g1_cases, g2_cases, g3_case
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    return engine()


def _ref(lp, labels, terminal, beam, mm):
    return R.forward_backward(lp, labels, np.full(lp.shape[0], int(terminal), np.int64), beam, mm, full=True)


def _check(g, lo, ll, frames, lp, labels, terminal, beam, mm, what, eng=None, _lib=None, ref=None):
    ref = ref or _ref(lp, labels, terminal, beam, mm)
    assert ref["status"] == R.OK, what
    T = lp.shape[0]
    W = _W(len(labels), beam)
    assert g.shape == (len(frames), W) and lo.shape == (len(frames),), what
    for k, f in enumerate(frames):
        rlo, rg = ref["gamma"][int(f)]
        assert lo[k] == rlo, (what, f, lo[k], rlo)
        n = len(rg)
        err = np.max(np.abs(g[k, :n].astype(np.float64) - rg)) if n else 0.0
        assert err <= 1e-3, (what, f, err)
        _WORST[0] = max(_WORST[0], err)
        assert np.all(g[k, n:] == 0.0), (what, f)
        assert abs(g[k].astype(np.float64).sum() - 1.0) <= 1e-4, (what, f)
        if f == T - 1:
            want = np.zeros(W, np.float32)
            want[int(terminal) - rlo] = 1.0
            assert np.array_equal(g[k], want), what
    assert abs(ll - ref["ll"]) <= 1e-3 + 1e-6 * T, (what, ll, ref["ll"])
    record("state", R.state_ratio(g, frames, ref, what), R.M_STATE)
    record("z", R.z_ratio(ll, ref), R.M_Z)
    if eng is not None:
        _, z = _label_call(eng, _lib, lp, labels, terminal, beam, mm)
        assert abs(ll - z) <= 1e-9 * max(1.0, abs(z)), (what, ll, z)
    return ref


_WORST = [0.0]   # the largest |d gamma| seen (printed by the last test with -s)


def _spread(T, K, rng=None):
    """K distinct frames spread over [0, T), T-1 among them."""
    f = np.unique(np.linspace(0, T - 1, K).astype(np.int64))
    return f


def test_g1_cases_with_their_stored_terminals(env):
    ka, _lib, eng = env
    n = 0
    for c in g1_cases():
        if c["status"] != 0:
            continue
        s = int(c["path"][-1])
        T = c["lp"].shape[0]
        frames = np.arange(T)
        gs, los, ll, st, rc = _call(eng, _lib, [c["lp"]], [c["labels"]], [s], [frames], c["beam"], c["max_move"])
        ref = _ref(c["lp"], c["labels"], s, c["beam"], c["max_move"])
        assert st[0] == ref["status"], c["idx"]
        if ref["status"] == R.ZERO_MASS:
            assert ll[0] == -np.inf and np.isnan(gs[0]).all() and (los[0] == -1).all()
            continue
        _check(gs[0], los[0], ll[0], frames, c["lp"], c["labels"], s, c["beam"], c["max_move"], c["idx"], eng, _lib, ref)
        n += 1
    assert n >= 100


def test_g2_cases(env):
    ka, _lib, eng = env
    for c in g2_cases():
        lp = O.hash_logprobs(c["T"], c["V"], c["seed"])
        labels = O.hash_labels(c["S"], c["V"], c["seed"])
        s = int(c["path"][-1])
        frames = _spread(c["T"], 100)
        gs, los, ll, st, rc = _call(eng, _lib, [lp], [labels], [s], [frames], c["beam"], c["max_move"])
        assert rc == 0 and st[0] == 0, c["idx"]
        _check(gs[0], los[0], ll[0], frames, lp, labels, s, c["beam"], c["max_move"], c["idx"], eng, _lib)


def test_g3_cfg2_one_lattice_and_cross_checks(env):
    ka, _lib, eng = env
    c = g3_case()
    lp = O.hash_logprobs(c["T"], c["V"], c["seed"])
    labels = O.hash_labels(c["S"], c["V"], c["seed"])
    path = c["path"]
    s = int(path[-1])
    frames = _spread(c["T"], 200)
    g, lo, ll = ka.ctc_state_posteriors(lp, labels, path, frames, beam_size=c["beam"], max_move=c["max_move"])
    assert g.dtype == np.float32 and lo.dtype == np.int64
    ref = _check(g, lo, ll, frames, lp, labels, s, c["beam"], c["max_move"], "g3", eng, _lib)
    _cross_check(ka, g, lo, ll, frames, lp, labels, path, c["beam"], c["max_move"], eng, _lib, ref)


def _cross_check(ka, g, lo, ll, frames, lp, labels, path, beam, mm, eng, _lib, ref):
    """gamma summed by label value vs the label occupancy; gamma at the best path's state vs its path posterior, which
    stores alpha at the path as a float: 1e-4 beyond that call's own distance from the float64
    reference."""
    occ, z = _label_call(eng, _lib, lp, labels, int(path[-1]), beam, mm)
    assert ll == z
    lab = R.expand(labels)
    for k, f in enumerate(frames):
        cols = np.arange(g.shape[1])
        ok = lo[k] + cols < len(lab)
        row = np.zeros(lp.shape[1])
        np.add.at(row, lab[lo[k] + cols[ok]], g[k, ok].astype(np.float64))
        assert np.max(np.abs(row - occ[f])) <= 1e-5, (f, np.max(np.abs(row - occ[f])))
    post, _ = ka.ctc_path_posteriors(lp, labels, path, beam_size=beam, max_move=mm)
    for k, f in enumerate(frames):
        j = int(path[f]) - lo[k]
        got = g[k, j] if 0 <= j < g.shape[1] else 0.0
        rlo, rg = ref["gamma"][int(f)]
        exact = rg[int(path[f]) - rlo] if 0 <= int(path[f]) - rlo < len(rg) else 0.0
        assert abs(float(got) - float(post[f])) <= 1e-4 + abs(float(post[f]) - exact), (f, got, post[f], exact)


# the shapes of test_label_posteriors_gpu.RANDOM: both forms, unbanded, V = 80
RANDOM = [(400, 150, 39, 1000, 1), (400, 150, 64, 64, 2), (500, 300, 39, 1000, 3), (500, 300, 64, 1000, 4),
          (400, 150, 80, 64, 4), (400, 150, 39, 64, 5), (300, 100, 64, 1000, 6), (400, 700, 39, 1500, 4),
          (600, 600, 64, 1100, 3), (300, 600, 39, 5000, 4), (250, 200, 80, 5000, 6), (200, 80, 80, 1000, 2)]


@pytest.mark.parametrize("shape", RANDOM, ids=[f"T{a}_S{b}_V{c}_B{d}_M{e}" for a, b, c, d, e in RANDOM])
def test_random_lattices_both_forms(env, shape):
    ka, _lib, eng = env
    T, S, V, beam, mm = shape
    rng = np.random.default_rng(T * 7 + S + V + beam + mm)
    lp = np.log(rng.dirichlet(np.full(V, 0.3), size=T)).astype(np.float32)
    labels = rng.integers(1, V, size=S).astype(np.int32)
    labels[::17] = 0                                   # label value 0: the veto of align.py:80-81
    lp[rng.integers(0, T, 5), rng.integers(0, V, 5)] = -np.inf
    path = O.ctc_best_path_c(lp, labels, beam, mm)[0]
    frames = np.sort(rng.choice(T, 40, replace=False))
    gs, los, ll, st, rc = _call(eng, _lib, [lp], [labels], [path[-1]], [frames], beam, mm)
    assert rc == 0 and st[0] == 0
    ref = _check(gs[0], los[0], ll[0], frames, lp, labels, int(path[-1]), beam, mm, shape, eng, _lib)
    _cross_check(ka, gs[0], los[0], ll[0], frames, lp, labels, path, beam, mm, eng, _lib, ref)


@pytest.mark.parametrize("V,beam", [(39, 40), (80, 40), (39, 5000)])
def test_hard_case_terminal_far_below_the_frame_best(env, V, beam):
    ka, _lib, eng = env
    T, S, mm = 600, 120, 4
    lp = O.hash_logprobs(T, V, 11)
    labels = O.hash_labels(S, V, 11)
    lp[T - 6:T - 1, 0] -= 40.0
    lp[T - 1, 0] = -260.0
    path = O.ctc_best_path_c(lp, labels, beam, mm)[0]
    ref = _ref(lp, labels, path[-1], beam, mm)
    assert ref["last_max"] - ref["ll"] > 200.0
    frames = np.concatenate([np.arange(0, T - 40, 37), np.arange(T - 40, T)])
    gs, los, ll, st, rc = _call(eng, _lib, [lp], [labels], [path[-1]], [frames], beam, mm)
    assert rc == 0 and st[0] == 0
    _check(gs[0], los[0], ll[0], frames, lp, labels, int(path[-1]), beam, mm, (V, beam), eng, _lib, ref)


@pytest.mark.parametrize("V,beam", [(39, 1000), (80, 1000)])
def test_query_patterns(env, V, beam):
    """K = 0, K = 1, every frame, frames only in the last block, only in the first block, only in a middle block."""
    ka, _lib, eng = env
    T, S, mm = 333, 90, 4                                # 11 blocks, the last one of 13 frames
    lp = O.hash_logprobs(T, V, 7)
    labels = O.hash_labels(S, V, 7)
    s = int(O.ctc_best_path_c(lp, labels, beam, mm)[0][-1])
    ref = _ref(lp, labels, s, beam, mm)
    patterns = [np.zeros(0, np.int64), np.array([150]), np.arange(T), np.arange(320, T), np.array([T - 1]),
                np.arange(0, 32), np.array([0]), np.array([161, 170, 191])]
    gs, los, ll, st, rc = _call(eng, _lib, [lp] * len(patterns), [labels] * len(patterns), [s] * len(patterns), patterns, beam, mm)
    assert rc == 0 and st.tolist() == [0] * len(patterns)
    assert len(set(ll.tolist())) == 1
    full = {int(f): (gs[2][f], los[2][f]) for f in range(T)}
    for p, (frames, g, lo) in enumerate(zip(patterns, gs, los)):
        _check(g, lo, ll[p], frames, lp, labels, s, beam, mm, ("pattern", p), ref=ref)
        for k, f in enumerate(frames):             # a row does not depend on which other frames are asked for
            assert np.array_equal(g[k].view(np.int32), full[int(f)][0].view(np.int32)) and lo[k] == full[int(f)][1], (p, f)
    # K = 0 through the single-lattice entry point and the Python API: Z only
    g0, lo0, z0 = ka.ctc_state_posteriors(lp, labels, s, [], beam_size=beam, max_move=mm)
    assert g0.shape == (0, _W(S, beam)) and lo0.shape == (0,) and z0 == ll[0]


@pytest.mark.parametrize("V,beam", [(39, 1000), (80, 1000), (39, 3000)])
def test_statuses(env, V, beam):
    ka, _lib, eng = env
    T, S, mm = 120, 30, 4
    lp = O.hash_logprobs(T, V, 5)
    labels = O.hash_labels(S, V, 5)
    s = int(O.ctc_best_path_c(lp, labels, beam, mm)[0][-1])
    nan = lp.copy()
    nan[40, 3] = np.nan
    pinf = lp.copy()
    pinf[70, 1] = np.inf
    dead = lp.copy()
    dead[:, 0] = -np.inf                                # the last blank is reached only through -inf emissions
    badlab = labels.copy()
    badlab[3] = V
    cases = [(lp, labels, s, 0), (nan, labels, s, _lib.KA_ERR_NAN), (pinf, labels, s, _lib.KA_ERR_NONFINITE),
             (lp, labels, 2 * S + 1, _lib.KA_ERR_BAD_ARGS), (dead, labels, 2 * S, _lib.KA_ERR_ZERO_MASS),
             (lp, badlab, s, _lib.KA_ERR_BAD_LABEL), (lp, labels, -1, _lib.KA_ERR_BAD_ARGS), (lp, labels, 1 << 40, _lib.KA_ERR_BAD_ARGS)]
    frames = [np.array([0, 17, 64, 100, T - 1])] * len(cases)
    gs, los, ll, st, rc = _call(eng, _lib, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], frames, beam, mm)
    assert st.tolist() == [c[3] for c in cases]
    assert rc == cases[1][3]                            # the first lattice that failed
    _check(gs[0], los[0], ll[0], frames[0], lp, labels, s, beam, mm, "ok lattice beside failures", eng, _lib)
    for k in range(1, len(cases)):
        assert np.isnan(gs[k]).all() and (los[k] == -1).all(), k
    assert ll[4] == -np.inf and np.isnan(ll[[1, 2, 3, 5, 6, 7]]).all()
    with pytest.raises(ValueError):
        ka.ctc_state_posteriors(dead, labels, 2 * S, [0, 5], beam_size=beam, max_move=mm)
    with pytest.raises(IndexError):
        ka.ctc_state_posteriors(lp, badlab, s, [0, 5], beam_size=beam, max_move=mm)
    res, sts = ka.ctc_state_posteriors_batch([lp, dead], [labels, labels], [s, 2 * S], [[3], [3]], beam_size=beam, max_move=mm,
                                             return_status=True)
    assert sts == [0, _lib.KA_ERR_ZERO_MASS] and res[1][2] == -np.inf and res[1][1].tolist() == [-1]


def test_bad_frames_and_ld_out_fail_the_call(env):
    ka, _lib, eng = env
    T, S, V, beam, mm = 120, 30, 39, 1000, 4
    lp = O.hash_logprobs(T, V, 5)
    labels = O.hash_labels(S, V, 5)
    s = int(O.ctc_best_path_c(lp, labels, beam, mm)[0][-1])
    good = np.array([0, 5, 9])
    for bad in ([5, 3], [4, 4], [0, T], [-1, 3]):
        gs, los, ll, st, rc = _call(eng, _lib, [lp, lp], [labels, labels], [s, s], [good, np.array(bad)], beam, mm)
        assert rc == _lib.KA_ERR_BAD_ARGS, bad
        assert "lattice 1" in _lib.last_error(), _lib.last_error()
        assert st.tolist() == [99, 99] and (gs[0] == -7.0).all()       # nothing ran
    W = _W(S, beam)
    gs, los, ll, st, rc = _call(eng, _lib, [lp, lp], [labels, labels], [s, s], [good, good], beam, mm, ld_out=[W, W - 1])
    assert rc == _lib.KA_ERR_BAD_ARGS and "lattice 1" in _lib.last_error()
    # a wider pitch is legal: the other columns are left alone
    gs, los, ll, st, rc = _call(eng, _lib, [lp], [labels], [s], [good], beam, mm)
    assert rc == 0
    wide, lo, z, rc = state_call_one(eng, _lib, lp, labels, s, good, beam, mm, ld_out=W + 5, fill=-3.5)
    assert rc == 0 and z == ll[0] and np.array_equal(lo, los[0])
    assert np.array_equal(wide[:, :W].view(np.int32), gs[0].view(np.int32)) and (wide[:, W:] == -3.5).all()


def test_bit_stability_single_batch_and_device(env):
    import torch
    ka, _lib, eng = env
    shapes = [(3000, 700, 1000, 4), (1200, 500, 64, 3), (1500, 600, 2500, 4), (900, 300, 1000, 2)]
    for V in (39, 80):
        lps = [O.hash_logprobs(T, V, 20 + i) for i, (T, S, B, M) in enumerate(shapes)]
        labs = [O.hash_labels(S, V, 20 + i) for i, (T, S, B, M) in enumerate(shapes)]
        frs = [_spread(T, 50) for T, S, B, M in shapes]
        for beam, mm in ((1000, 4), (3000, 4)):
            terms = [int(O.ctc_best_path_c(lp, lab, beam, mm)[0][-1]) for lp, lab in zip(lps, labs)]
            batch, lo_b, ll_b, st, rc = _call(eng, _lib, lps, labs, terms, frs, beam, mm)
            assert rc == 0
            for i in range(len(shapes)):
                g1, lo1, z1 = ka.ctc_state_posteriors(lps[i], labs[i], terms[i], frs[i], beam_size=beam, max_move=mm)
                assert np.array_equal(g1.view(np.int32), batch[i].view(np.int32)), (V, beam, i)
                assert np.array_equal(lo1, lo_b[i]) and z1 == ll_b[i]
            dev = ka.ctc_state_posteriors_device([torch.from_numpy(x).cuda() for x in lps], [torch.from_numpy(x).cuda() for x in labs],
                                                 terms, frs, beam_size=beam, max_move=mm)
            for i, (g, lo, z) in enumerate(dev):
                assert g.is_cuda and lo.is_cuda and lo.dtype == torch.int64
                assert np.array_equal(g.cpu().numpy().view(np.int32), batch[i].view(np.int32)), (V, beam, i)
                assert np.array_equal(lo.cpu().numpy(), lo_b[i]) and z == ll_b[i]
            if (V, beam) == (39, 1000):
                for i in range(len(shapes)):
                    _check(batch[i], lo_b[i], ll_b[i], frs[i], lps[i], labs[i], terms[i], beam, mm, (V, beam, i))


@pytest.mark.parametrize("V,beam", [(39, 1000), (80, 1000)])
def test_device_strides_in_and_out(env, V, beam):
    import torch
    ka, _lib, eng = env
    T, S, mm = 700, 200, 4
    lp = O.hash_logprobs(T, V, 31)
    labels = O.hash_labels(S, V, 31)
    s = int(O.ctc_best_path_c(lp, labels, beam, mm)[0][-1])
    frames = _spread(T, 60)
    W = _W(S, beam)
    wide_in = torch.full((T, V + 13), 5.0, dtype=torch.float32, device="cuda")
    wide_in[:, 7:7 + V] = torch.from_numpy(lp).cuda()
    wide_out = torch.full((len(frames), W + 9), -3.5, dtype=torch.float32, device="cuda")
    view = wide_out[:, 4:4 + W]
    (g, lo, z), = ka.ctc_state_posteriors_device([wide_in[:, 7:7 + V]], [labels], [s], [frames], beam_size=beam, max_move=mm, out=[view])
    assert g.data_ptr() == view.data_ptr()
    host, los, ll, _, _ = _call(eng, _lib, [lp], [labels], [s], [frames], beam, mm)
    assert np.array_equal(view.cpu().numpy().view(np.int32), host[0].view(np.int32)) and z == ll[0]
    assert np.array_equal(lo.cpu().numpy(), los[0])
    rest = torch.cat([wide_out[:, :4], wide_out[:, 4 + W:]], 1)
    assert bool((rest == -3.5).all())


def test_cfg2_batch_of_1024_both_forms(env):
    """1024 cfg2-length lattices in one call, beam 1100: S = 5000 lattices take the generic form (band 1100), S = 500 ones
    the fast form (band 1001)."""
    import torch
    ka, _lib, eng = env
    n, T, V, S, seed0, beam = 1024, 50000, 64, 5000, 9000, 1100
    lib = ka.load_library()
    lp = torch.empty((n, T, V), dtype=torch.float32, device="cuda")
    lab = torch.empty((n, S), dtype=torch.int32, device="cuda")
    assert lib.ka_hash_logprobs_batch_f32(lp.data_ptr(), n, T, V, V, T * V, seed0, None) == 0
    assert lib.ka_hash_labels_batch_i32(lab.data_ptr(), n, S, V, S, seed0, None) == 0
    torch.cuda.synchronize()
    lps = list(lp.unbind(0))
    labs = [lab[i] if i % 4 == 0 else lab[i, :500] for i in range(n)]     # a quarter generic, the rest fast
    from kokoro_align_amd.align import DeviceBatch
    batch = DeviceBatch(lps, labs, beam, 4)
    batch.run()
    terms = [int(v) for v in torch.stack([p[-1] for p in batch.path]).cpu().tolist()]
    frames = [_spread(T, 200)] * n
    res, st = ka.ctc_state_posteriors_device(lps, labs, terms, frames, beam_size=beam, max_move=4, return_status=True)
    assert st == [0] * n
    for i, (g, lo, z) in enumerate(res):
        assert g.shape == (200, _W(int(labs[i].shape[0]), beam))
    sums = torch.stack([g.sum(-1, dtype=torch.float64) for g, _, _ in res])
    assert float((sums - 1).abs().max()) <= 1e-4
    assert all(bool((g >= 0).all()) and bool((g <= 1).all()) for g, _, _ in res)
    for i in range(n):                                  # the last frame: exactly 1 at the terminal
        g, lo, _ = res[i]
        assert float(g[-1, terms[i] - int(lo[-1])]) == 1.0
    for i in (0, 1, 1023):
        lp_i = O.hash_logprobs(T, V, seed0 + i)
        g, lo, z = res[i]
        _check(g.cpu().numpy(), lo.cpu().numpy(), z, frames[i], lp_i, labs[i].cpu().numpy(), terms[i], beam, 4, i, eng, _lib)


def test_best_path_bits_unchanged_by_a_state_posterior_call(env):
    ka, _lib, eng = env
    for T, V, S, beam, mm, seed in [(3000, 39, 700, 1000, 4, 1), (1200, 64, 900, 1000, 4, 2), (900, 80, 600, 2500, 4, 4)]:
        lp = O.hash_logprobs(T, V, seed)
        labels = O.hash_labels(S, V, seed)
        before = ka.ctc_best_path(lp, labels, beam_size=beam, max_move=mm, verbose=False)
        ka.ctc_state_posteriors(lp, labels, before[0], _spread(T, 30), beam_size=beam, max_move=mm)
        after = ka.ctc_best_path(lp, labels, beam_size=beam, max_move=mm, verbose=False)
        for b, a in zip(before, after):
            assert np.array_equal(b.view(np.int32), a.view(np.int32))


# ---- end to end: best path -> boundary frames -> state posteriors -> boundary confidence ----
def _ref_confidence(ka, ref, frames, W, path, seg_ends, n_ph):
    g = np.zeros((len(frames), W))
    lo = np.zeros(len(frames), np.int64)
    for k, f in enumerate(frames):
        lo[k], rg = ref["gamma"][int(f)]
        g[k, :len(rg)] = rg
    return ka.segment_boundary_confidence(g, lo, frames, path, seg_ends, n_ph)


@pytest.mark.parametrize("T,S,V,beam", [(3000, 700, 39, 1000), (1500, 600, 39, 2500), (800, 200, 80, 64)])
def test_end_to_end_boundary_confidence(env, T, S, V, beam):
    ka, _lib, eng = env
    lp = O.hash_logprobs(T, V, 77)
    labels = O.hash_labels(S, V, 77)
    path, _, _ = ka.ctc_best_path(lp, labels, beam_size=beam, verbose=False)
    seg_ends = np.array(sorted(set(np.linspace(T // 13, T - 1, 12).astype(int).tolist())) + [T + 5])
    frames = ka.boundary_frames(seg_ends, T)
    g, lo, ll = ka.ctc_state_posteriors(lp, labels, path, frames, beam_size=beam)
    n_ph = S - 3                                        # some end states clip to n_phonemes
    p_start, p_end = ka.segment_boundary_confidence(g, lo, frames, path, seg_ends, n_ph)
    ref = _ref(lp, labels, path[-1], beam, 4)
    r_start, r_end = _ref_confidence(ka, ref, frames, g.shape[1], path, seg_ends, n_ph)
    assert np.max(np.abs(p_start - r_start)) <= 1e-3 and np.max(np.abs(p_end - r_end)) <= 1e-3
    assert p_end[-1] == 1.0
    assert np.all((p_start >= 0) & (p_start <= 1 + 1e-5)) and np.all((p_end >= 0) & (p_end <= 1 + 1e-5))


def test_end_to_end_confident_lattice(env):
    """Log-probs that strongly favour one path: every boundary is certain."""
    ka, _lib, eng = env
    rng = np.random.default_rng(3)
    S, V = 100, 39
    labels = np.empty(S, np.int32)
    labels[0] = rng.integers(1, V)
    for i in range(1, S):                               # no two neighbours alike, no blank
        labels[i] = (labels[i - 1] + rng.integers(1, V - 1) - 1) % (V - 1) + 1
    lab = R.expand(labels)
    T = 2 * len(lab)
    states = np.arange(T) // 2                          # every state for two frames
    logits = np.zeros((T, V))
    logits[np.arange(T), lab[states]] = 25.0
    lp = (logits - np.log(np.exp(logits).sum(1, keepdims=True))).astype(np.float32)
    path, _, _ = ka.ctc_best_path(lp, labels, verbose=False)
    assert np.array_equal(path, states)
    seg_ends = np.array([37, 90, 151, 260, T])
    frames = ka.boundary_frames(seg_ends, T)
    g, lo, ll = ka.ctc_state_posteriors(lp, labels, path, frames)
    p_start, p_end = ka.segment_boundary_confidence(g, lo, frames, path, seg_ends, S)
    assert np.all(p_start >= 0.999) and np.all(p_end >= 0.999), (p_start, p_end)
    print(f"largest |d gamma| against the float64 reference in this module: {_WORST[0]:.3g}")
