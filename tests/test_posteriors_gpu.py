"""Best-path posteriors and lattice log-likelihood on the MI355X, all through the C ABI, against the float64 reference
(tests/posterior_ref.py): |d posterior| <= 1e-3, |d log-likelihood| <= 1e-3 + 1e-6 T nats.  Beside those, the per-cell
check of DESIGN.md section 4.21: every frame's posterior within posterior_ref.path_tolerance (M_PATH x path_error_model)
where the reference is 2^-120 or more and below 2^-119 elsewhere (posterior_ref.path_ratio), and the log-likelihood within
posterior_ref.z_tolerance."""
import numpy as np
import pytest

import posterior_ref as R
from fb_harness import engine, path_call as _call, record, tiny
from golden_util import g1_cases, g2_cases, g3_case
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    return engine()


def _check(post, ll, lp, labels, path, beam, mm, what):
    ref = R.forward_backward(lp, labels, path, beam, mm)
    assert ref["status"] == R.OK, what
    T = lp.shape[0]
    assert np.all(np.isfinite(post)), what
    err = np.max(np.abs(post.astype(np.float64) - ref["post"]))
    assert err <= 1e-3, (what, err)
    assert abs(ll - ref["ll"]) <= 1e-3 + 1e-6 * T, (what, ll, ref["ll"])
    record("path", R.path_ratio(post, ref, what), R.M_PATH)
    record("z", R.z_ratio(ll, ref), R.M_Z)
    assert post[-1] == 1.0, what
    return ref


def test_g1_cases_with_their_stored_paths(env):
    ka, _lib, eng = env
    n = 0
    for c in g1_cases():
        if c["status"] != 0:
            continue
        posts, ll, st, rc = _call(eng, _lib, [c["lp"]], [c["labels"]], [c["path"]], c["beam"], c["max_move"])
        ref = R.forward_backward(c["lp"], c["labels"], c["path"], c["beam"], c["max_move"])
        assert st[0] == ref["status"], c["idx"]
        if ref["status"] == R.ZERO_MASS:
            assert ll[0] == -np.inf and np.isnan(posts[0]).all()
            continue
        _check(posts[0], ll[0], c["lp"], c["labels"], c["path"], c["beam"], c["max_move"], c["idx"])
        n += 1
    assert n >= 100


def test_g2_cases(env):
    ka, _lib, eng = env
    for c in g2_cases():
        lp = O.hash_logprobs(c["T"], c["V"], c["seed"])
        labels = O.hash_labels(c["S"], c["V"], c["seed"])
        posts, ll, st, rc = _call(eng, _lib, [lp], [labels], [c["path"]], c["beam"], c["max_move"])
        assert rc == 0 and st[0] == 0, c["idx"]
        _check(posts[0], ll[0], lp, labels, c["path"], c["beam"], c["max_move"], c["idx"])


def test_g3_cfg2_one_lattice(env):
    ka, _lib, eng = env
    c = g3_case()
    lp = O.hash_logprobs(c["T"], c["V"], c["seed"])
    labels = O.hash_labels(c["S"], c["V"], c["seed"])
    post, ll = ka.ctc_path_posteriors(lp, labels, c["path"], beam_size=c["beam"], max_move=c["max_move"])
    _check(post, ll, lp, labels, c["path"], c["beam"], c["max_move"], "g3")


# (T, S, V, beam, max_move): bands of 64, 1000 (fast form), > 1009 and unbanded (generic form), V = 80 (generic)
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
    posts, ll, st, rc = _call(eng, _lib, [lp], [labels], [path], beam, mm)
    assert rc == 0 and st[0] == 0
    ref = _check(posts[0], ll[0], lp, labels, path, beam, mm, shape)
    # the terminal's likelihood bounds the Viterbi score, up to the rounding of that float32 running sum (a lattice with one
    # dominant path has Z within a few ulp of it)
    total = O.ctc_best_path_c(lp, labels, beam, mm, return_total=True)[3]
    slack = 1e-3 + T * float(np.spacing(np.float32(abs(total))))
    assert ref["ll"] >= float(total) - slack and ll[0] >= float(total) - slack


@pytest.mark.parametrize("V,beam", [(39, 40), (80, 40), (39, 5000)])
def test_hard_case_terminal_far_below_the_frame_best(env, V, beam):
    """alpha_{T-1}(s*) more than 200 nats below the last frame's best cell: the chapters this feature exists to flag."""
    ka, _lib, eng = env
    T, S, mm = 600, 120, 4
    lp = O.hash_logprobs(T, V, 11)
    labels = O.hash_labels(S, V, 11)
    lp[T - 6:T - 1, 0] -= 40.0                          # blanks of the last frames are very unlikely ...
    lp[T - 1, 0] = -260.0                               # ... and the terminal (the last blank, the highest live state) is worse
    path = O.ctc_best_path_c(lp, labels, beam, mm)[0]
    ref = R.forward_backward(lp, labels, path, beam, mm)
    assert ref["last_max"] - ref["ll"] > 200.0
    posts, ll, st, rc = _call(eng, _lib, [lp], [labels], [path], beam, mm)
    assert rc == 0 and st[0] == 0
    _check(posts[0], ll[0], lp, labels, path, beam, mm, (V, beam))


@pytest.mark.parametrize("V,beam", [(39, 1000), (80, 1000), (39, 3000)])
def test_statuses(env, V, beam):
    ka, _lib, eng = env
    T, S, mm = 120, 30, 4
    lp = O.hash_logprobs(T, V, 5)
    labels = O.hash_labels(S, V, 5)
    path = O.ctc_best_path_c(lp, labels, beam, mm)[0]
    nan = lp.copy()
    nan[40, 3] = np.nan
    pinf = lp.copy()
    pinf[70, 1] = np.inf
    far = path.copy()
    far[50] = 2 * S + 1
    dead = lp.copy()
    dead[:, 0] = -np.inf                                # the last blank is reached only through -inf emissions
    dead_path = path.copy()
    dead_path[-1] = 2 * S
    badlab = labels.copy()
    badlab[3] = V
    cases = [(lp, labels, path, 0), (nan, labels, path, _lib.KA_ERR_NAN), (pinf, labels, path, _lib.KA_ERR_NONFINITE),
             (lp, labels, far, _lib.KA_ERR_BAD_ARGS), (dead, labels, dead_path, _lib.KA_ERR_ZERO_MASS),
             (lp, badlab, path, _lib.KA_ERR_BAD_LABEL)]
    posts, ll, st, rc = _call(eng, _lib, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], beam, mm)
    assert st.tolist() == [c[3] for c in cases]
    assert rc == cases[1][3]                            # the first lattice that failed
    _check(posts[0], ll[0], lp, labels, path, beam, mm, "ok lattice beside failures")
    for k in range(1, len(cases)):
        assert np.isnan(posts[k]).all(), k
    assert ll[4] == -np.inf and np.isnan(ll[[1, 2, 3, 5]]).all()
    with pytest.raises(ValueError):
        ka.ctc_path_posteriors(dead, labels, dead_path, beam_size=beam, max_move=mm)
    with pytest.raises(IndexError):
        ka.ctc_path_posteriors(lp, badlab, path, beam_size=beam, max_move=mm)


def test_host_and_device_memory_agree_and_batch_is_bit_stable(env):
    import torch
    ka, _lib, eng = env
    shapes = [(3000, 700, 1000, 4), (1200, 500, 64, 3), (1500, 600, 2500, 4), (900, 300, 1000, 2)]
    for V in (39, 80):
        lps = [O.hash_logprobs(T, V, 20 + i) for i, (T, S, B, M) in enumerate(shapes)]
        labs = [O.hash_labels(S, V, 20 + i) for i, (T, S, B, M) in enumerate(shapes)]
        for beam, mm in ((1000, 4), (64, 3), (3000, 4)):   # (3000: the unbanded DP; bands over 1009 run in the generic form)
            paths = [O.ctc_best_path_c(lp, lab, beam, mm)[0] for lp, lab in zip(lps, labs)]
            batch, ll_b, st, rc = _call(eng, _lib, lps, labs, paths, beam, mm)
            assert rc == 0
            again, ll_a, _, _ = _call(eng, _lib, lps, labs, paths, beam, mm)
            for i in range(len(shapes)):
                alone, ll_1, _, _ = _call(eng, _lib, [lps[i]], [labs[i]], [paths[i]], beam, mm)
                assert np.array_equal(alone[0].view(np.int32), batch[i].view(np.int32)), (V, beam, i)
                assert np.array_equal(again[i].view(np.int32), batch[i].view(np.int32)), (V, beam, i)
                assert ll_1[0] == ll_b[i] == ll_a[i]
            dev = ka.ctc_path_posteriors_device([torch.from_numpy(x).cuda() for x in lps], [torch.from_numpy(x).cuda() for x in labs],
                                                [torch.from_numpy(x).cuda() for x in paths], beam_size=beam, max_move=mm)
            for i, (p, z) in enumerate(dev):
                assert np.array_equal(p.cpu().numpy().view(np.int32), batch[i].view(np.int32)), (V, beam, i)
                assert z == ll_b[i]


def test_cfg2_batch_of_1024(env):
    import torch
    ka, _lib, eng = env
    n, T, V, S, seed0 = 1024, 50000, 64, 5000, 9000
    lib = ka.load_library()
    lp = torch.empty((n, T, V), dtype=torch.float32, device="cuda")
    lab = torch.empty((n, S), dtype=torch.int32, device="cuda")
    assert lib.ka_hash_logprobs_batch_f32(lp.data_ptr(), n, T, V, V, T * V, seed0, None) == 0
    assert lib.ka_hash_labels_batch_i32(lab.data_ptr(), n, S, V, S, seed0, None) == 0
    torch.cuda.synchronize()
    lps, labs = list(lp.unbind(0)), list(lab.unbind(0))
    from kokoro_align_amd.align import DeviceBatch
    batch = DeviceBatch(lps, labs, 1000, 4)
    batch.run()
    total = batch.total.copy()
    paths = batch.path
    res, st = ka.ctc_path_posteriors_device(lps, labs, paths, beam_size=1000, max_move=4, return_status=True)
    assert st == [0] * n
    for i, (p, z) in enumerate(res):
        assert z >= float(total[i]) - 1e-3, i
    post = torch.stack([p for p, _ in res])
    assert bool((post[:, -1] == 1.0).all())
    assert bool((post >= 0).all()) and bool((post <= 1 + 1e-6).all())
    for i in (0, 1, 137, 300, 511, 777, 1000, 1023):
        lp_i = O.hash_logprobs(T, V, seed0 + i)
        assert np.array_equal(lp_i, lps[i].cpu().numpy())
        _check(res[i][0].cpu().numpy(), res[i][1], lp_i, labs[i].cpu().numpy(), paths[i].cpu().numpy(), 1000, 4, i)


def test_best_path_bits_unchanged_by_a_posterior_call(env):
    ka, _lib, eng = env
    shapes = [(3000, 39, 700, 1000, 4, 1), (1200, 64, 900, 1000, 4, 2), (900, 64, 600, 2500, 4, 4)]
    for T, V, S, beam, mm, seed in shapes:
        lp = O.hash_logprobs(T, V, seed)
        labels = O.hash_labels(S, V, seed)
        before = ka.ctc_best_path(lp, labels, beam_size=beam, max_move=mm, verbose=False)
        ka.ctc_path_posteriors(lp, labels, before[0], beam_size=beam, max_move=mm)
        after = ka.ctc_best_path(lp, labels, beam_size=beam, max_move=mm, verbose=False)
        for b, a in zip(before, after):
            assert np.array_equal(b.view(np.int32), a.view(np.int32))


@pytest.mark.parametrize("V", [39, 80])
@pytest.mark.parametrize("beam", [64, 1009])
def test_band_that_jumps_past_the_label_ring_beside_neighbours(env, beam, V):
    """L = 1201 over T = 16: the band moves 75 positions a frame, more than the 64 labels a frame's request brings into the
    fast form's ring, so the ring's catch-up loop runs (V = 80 takes the generic form, which has no ring).  Such a band outruns
    every path (at most 3 positions a frame), so the lattice can only answer zero mass; its neighbours in the launch must be
    what they are alone."""
    ka, _lib, eng = env
    mm = 4
    rng = np.random.default_rng(1201)
    lats = [tiny(rng, 40, 12, 39), R.sloped(16, 600, 39, 1201), tiny(rng, 40, 12, 39)]
    paths = []
    for k, (lp, labels) in enumerate(lats):
        T, L = lp.shape[0], 2 * len(labels) + 1
        path = np.minimum(L - 1, (L * np.arange(T)) // T).astype(np.int32)
        if k != 1:
            path[-1] = R.live_terminals(lp, labels, beam, mm)[0]
        paths.append(path)
    assert R.forward_backward(*lats[1], paths[1], beam, mm)["status"] == R.ZERO_MASS == -9
    lps = [R.pad_vocabulary(lp, V) if V != 39 else lp for lp, _ in lats]
    posts, ll, st, rc = _call(eng, _lib, lps, [labels for _, labels in lats], paths, beam, mm)
    assert st.tolist() == [0, -9, 0] and rc == -9
    assert np.isnan(posts[1]).all() and ll[1] == -np.inf
    for k in (0, 2):
        ref = R.forward_backward(*lats[k], paths[k], beam, mm)
        assert ref["status"] == R.OK
        record("path", R.path_ratio(posts[k], ref, k), R.M_PATH)
        record("z", R.z_ratio(ll[k], ref), R.M_Z)
