"""Label occupancy posteriors and the differentiable lattice log-likelihood on the MI355X, through the C ABI and the Python
API, against the float64 reference (tests/occupancy_ref.py): |d occ| <= 1e-3, |row sum - 1| <= 1e-4, occ[T-1, lab'[s*]] = 1
exactly, Z within 1e-9 max(1, |Z|) of ka_ctc_path_posteriors' Z for a path that ends at s*.  Beside those, the per-cell
check of DESIGN.md section 4.21: every cell within posterior_ref.label_tolerance (M_LABEL x label_error_model) where the
reference is 2^-120 or more and below 2^-119 elsewhere (posterior_ref.label_ratio), and Z within posterior_ref.z_tolerance."""
import numpy as np
import pytest

import occupancy_ref as Q
import posterior_ref as R
from fb_harness import I, engine, label_call as _call, path_z_one as _path_z, record
from golden_util import g1_cases, g2_cases, g3_case
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    return engine()


def _check(occ, ll, lp, labels, terminal, beam, mm, what, eng=None, _lib=None, ref=None):
    ref = ref or Q.occupancy(lp, labels, terminal, beam, mm)
    assert ref["status"] == R.OK, what
    T = lp.shape[0]
    assert np.all(np.isfinite(occ)), what
    err = np.max(np.abs(occ.astype(np.float64) - ref["occ"]))
    assert err <= 1e-3, (what, err)
    assert np.max(np.abs(occ.astype(np.float64).sum(1) - 1.0)) <= 1e-4, what
    assert occ[T - 1, R.expand(labels)[terminal]] == 1.0, what
    assert abs(ll - ref["ll"]) <= 1e-3 + 1e-6 * T, (what, ll, ref["ll"])
    record("label", R.label_ratio(occ, ref["fb"], labels, what), R.M_LABEL)
    record("z", R.z_ratio(ll, ref["fb"]), R.M_Z)
    if eng is not None:
        z = _path_z(eng, _lib, lp, labels, terminal, beam, mm)
        assert abs(ll - z) <= 1e-9 * max(1.0, abs(z)), (what, ll, z)
    return ref


def test_g1_cases_with_their_stored_terminals(env):
    ka, _lib, eng = env
    n = 0
    for c in g1_cases():
        if c["status"] != 0:
            continue
        s = int(c["path"][-1])
        occs, ll, st, rc = _call(eng, _lib, [c["lp"]], [c["labels"]], [s], c["beam"], c["max_move"])
        ref = Q.occupancy(c["lp"], c["labels"], s, c["beam"], c["max_move"])
        assert st[0] == ref["status"], c["idx"]
        if ref["status"] == R.ZERO_MASS:
            assert ll[0] == -np.inf and np.isnan(occs[0]).all()
            continue
        _check(occs[0], ll[0], c["lp"], c["labels"], s, c["beam"], c["max_move"], c["idx"], eng, _lib, ref)
        n += 1
    assert n >= 100


def test_g2_cases(env):
    ka, _lib, eng = env
    for c in g2_cases():
        lp = O.hash_logprobs(c["T"], c["V"], c["seed"])
        labels = O.hash_labels(c["S"], c["V"], c["seed"])
        s = int(c["path"][-1])
        occs, ll, st, rc = _call(eng, _lib, [lp], [labels], [s], c["beam"], c["max_move"])
        assert rc == 0 and st[0] == 0, c["idx"]
        _check(occs[0], ll[0], lp, labels, s, c["beam"], c["max_move"], c["idx"], eng, _lib)


def test_g3_cfg2_one_lattice(env):
    ka, _lib, eng = env
    c = g3_case()
    lp = O.hash_logprobs(c["T"], c["V"], c["seed"])
    labels = O.hash_labels(c["S"], c["V"], c["seed"])
    occ, ll = ka.ctc_label_posteriors(lp, labels, c["path"], beam_size=c["beam"], max_move=c["max_move"])
    _check(occ, ll, lp, labels, int(c["path"][-1]), c["beam"], c["max_move"], "g3", eng, _lib)


# the shapes of test_posteriors_gpu.RANDOM: bands of 64, 1000 (fast form), > 1009 and unbanded (generic form), V = 80 (generic)
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
    occs, ll, st, rc = _call(eng, _lib, [lp], [labels], [path[-1]], beam, mm)
    assert rc == 0 and st[0] == 0
    _check(occs[0], ll[0], lp, labels, int(path[-1]), beam, mm, shape, eng, _lib)
    post = R.forward_backward(lp, labels, path, beam, mm)["post"]
    lab = R.expand(labels)
    assert np.all(occs[0][np.arange(T), lab[path]] >= post - 2e-3)


def test_many_labels_use_global_bins(env):
    """V above the generic form's LDS bins (2048): the fixed-point bins live in the workspace."""
    ka, _lib, eng = env
    T, S, V, beam, mm = 120, 40, 3000, 1000, 4
    lp = O.hash_logprobs(T, V, 3)
    labels = O.hash_labels(S, V, 3)
    path = O.ctc_best_path_c(lp, labels, beam, mm)[0]
    occs, ll, st, rc = _call(eng, _lib, [lp], [labels], [path[-1]], beam, mm)
    assert rc == 0 and st[0] == 0
    _check(occs[0], ll[0], lp, labels, int(path[-1]), beam, mm, "V3000", eng, _lib)
    again, ll2, _, _ = _call(eng, _lib, [lp], [labels], [path[-1]], beam, mm)
    assert np.array_equal(again[0].view(np.int32), occs[0].view(np.int32)) and ll2[0] == ll[0]


@pytest.mark.parametrize("V,beam", [(39, 40), (80, 40), (39, 5000)])
def test_hard_case_terminal_far_below_the_frame_best(env, V, beam):
    ka, _lib, eng = env
    T, S, mm = 600, 120, 4
    lp = O.hash_logprobs(T, V, 11)
    labels = O.hash_labels(S, V, 11)
    lp[T - 6:T - 1, 0] -= 40.0
    lp[T - 1, 0] = -260.0
    path = O.ctc_best_path_c(lp, labels, beam, mm)[0]
    ref = Q.occupancy(lp, labels, path[-1], beam, mm)
    assert ref["last_max"] - ref["ll"] > 200.0
    occs, ll, st, rc = _call(eng, _lib, [lp], [labels], [path[-1]], beam, mm)
    assert rc == 0 and st[0] == 0
    _check(occs[0], ll[0], lp, labels, int(path[-1]), beam, mm, (V, beam), eng, _lib, ref)


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
    occs, ll, st, rc = _call(eng, _lib, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], beam, mm)
    assert st.tolist() == [c[3] for c in cases]
    assert rc == cases[1][3]                            # the first lattice that failed
    _check(occs[0], ll[0], lp, labels, s, beam, mm, "ok lattice beside failures", eng, _lib)
    for k in range(1, len(cases)):
        assert np.isnan(occs[k]).all(), k
    assert ll[4] == -np.inf and np.isnan(ll[[1, 2, 3, 5, 6, 7]]).all()
    with pytest.raises(ValueError):
        ka.ctc_label_posteriors(dead, labels, 2 * S, beam_size=beam, max_move=mm)
    with pytest.raises(IndexError):
        ka.ctc_label_posteriors(lp, badlab, s, beam_size=beam, max_move=mm)
    res, sts = ka.ctc_label_posteriors_batch([lp, dead], [labels, labels], [s, 2 * S], beam_size=beam, max_move=mm, return_status=True)
    assert sts == [0, _lib.KA_ERR_ZERO_MASS] and res[1][1] == -np.inf


def test_bit_stability_batch_against_single_and_device(env):
    import torch
    ka, _lib, eng = env
    shapes = [(3000, 700, 1000, 4), (1200, 500, 64, 3), (1500, 600, 2500, 4), (900, 300, 1000, 2)]
    for V in (39, 80):
        lps = [O.hash_logprobs(T, V, 20 + i) for i, (T, S, B, M) in enumerate(shapes)]
        labs = [O.hash_labels(S, V, 20 + i) for i, (T, S, B, M) in enumerate(shapes)]
        for beam, mm in ((1000, 4), (64, 3), (3000, 4)):
            terms = [int(O.ctc_best_path_c(lp, lab, beam, mm)[0][-1]) for lp, lab in zip(lps, labs)]
            batch, ll_b, st, rc = _call(eng, _lib, lps, labs, terms, beam, mm)
            assert rc == 0
            again, ll_a, _, _ = _call(eng, _lib, lps, labs, terms, beam, mm)
            for i in range(len(shapes)):
                alone, ll_1, _, _ = _call(eng, _lib, [lps[i]], [labs[i]], [terms[i]], beam, mm)
                assert np.array_equal(alone[0].view(np.int32), batch[i].view(np.int32)), (V, beam, i)
                assert np.array_equal(again[i].view(np.int32), batch[i].view(np.int32)), (V, beam, i)
                assert ll_1[0] == ll_b[i] == ll_a[i]
            if (V, beam) == (39, 1000):
                for i in range(len(shapes)):
                    _check(batch[i], ll_b[i], lps[i], labs[i], terms[i], beam, mm, (V, beam, i), eng, _lib)
            dev = ka.ctc_label_posteriors_device([torch.from_numpy(x).cuda() for x in lps], [torch.from_numpy(x).cuda() for x in labs],
                                                 terms, beam_size=beam, max_move=mm)
            for i, (o, z) in enumerate(dev):
                assert np.array_equal(o.cpu().numpy().view(np.int32), batch[i].view(np.int32)), (V, beam, i)
                assert z == ll_b[i]


@pytest.mark.parametrize("V,beam", [(39, 1000), (80, 1000)])
def test_device_strides_in_and_out(env, V, beam):
    import torch
    ka, _lib, eng = env
    T, S, mm = 700, 200, 4
    lp = O.hash_logprobs(T, V, 31)
    labels = O.hash_labels(S, V, 31)
    s = int(O.ctc_best_path_c(lp, labels, beam, mm)[0][-1])
    wide_in = torch.full((T, V + 13), 5.0, dtype=torch.float32, device="cuda")
    wide_in[:, 7:7 + V] = torch.from_numpy(lp).cuda()
    wide_out = torch.full((T, V + 9), -3.5, dtype=torch.float32, device="cuda")
    view = wide_out[:, 4:4 + V]
    (o, z), = ka.ctc_label_posteriors_device([wide_in[:, 7:7 + V]], [labels], [s], beam_size=beam, max_move=mm, out=[view])
    assert o.data_ptr() == view.data_ptr()
    host, ll, _, _ = _call(eng, _lib, [lp], [labels], [s], beam, mm)
    assert np.array_equal(view.cpu().numpy().view(np.int32), host[0].view(np.int32)) and z == ll[0]
    rest = torch.cat([wide_out[:, :4], wide_out[:, 4 + V:]], 1)
    assert bool((rest == -3.5).all())


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
    paths = batch.path
    terms = [int(v) for v in torch.stack([p[-1] for p in paths]).cpu().tolist()]
    out = torch.empty((n, T, V), dtype=torch.float32, device="cuda")
    res, st = ka.ctc_label_posteriors_device(lps, labs, terms, beam_size=1000, max_move=4, out=list(out.unbind(0)), return_status=True)
    assert st == [0] * n
    sums = out.sum(-1, dtype=torch.float64)
    assert float((sums - 1).abs().max()) <= 1e-4
    assert bool((out >= 0).all()) and bool((out <= 1).all())
    lab_last = [int((labs[i][(terms[i] - 1) // 2] if terms[i] % 2 else 0)) for i in range(n)]
    assert bool((out[torch.arange(n), T - 1, torch.tensor(lab_last)] == 1.0).all())
    for i in (0, 511, 1023):
        lp_i = O.hash_logprobs(T, V, seed0 + i)
        _check(out[i].cpu().numpy(), res[i][1], lp_i, labs[i].cpu().numpy(), terms[i], 1000, 4, i, eng, _lib)


def test_workspace_bytes_for_8192_cfg2(env):
    ka, _lib, eng = env
    n = 8192
    assert 0 < eng.lib.ka_label_posterior_workspace_bytes(n, I([50000] * n), I([5000] * n), 64, 1000, 4, _lib.KA_MEM_DEVICE) <= 16 << 30


def test_best_path_bits_unchanged_by_a_label_posterior_call(env):
    ka, _lib, eng = env
    for T, V, S, beam, mm, seed in [(3000, 39, 700, 1000, 4, 1), (1200, 64, 900, 1000, 4, 2), (900, 80, 600, 2500, 4, 4)]:
        lp = O.hash_logprobs(T, V, seed)
        labels = O.hash_labels(S, V, seed)
        before = ka.ctc_best_path(lp, labels, beam_size=beam, max_move=mm, verbose=False)
        ka.ctc_label_posteriors(lp, labels, before[0], beam_size=beam, max_move=mm)
        after = ka.ctc_best_path(lp, labels, beam_size=beam, max_move=mm, verbose=False)
        for b, a in zip(before, after):
            assert np.array_equal(b.view(np.int32), a.view(np.int32))


# ---- autograd ----
def _small(seed, T=300, S=80, V=39):
    lp = O.hash_logprobs(T, V, seed)
    labels = O.hash_labels(S, V, seed)
    s = int(O.ctc_best_path_c(lp, labels, 1000, 4)[0][-1])
    return lp, labels, s


def test_autograd_value_and_gradient(env):
    import torch
    ka, _lib, eng = env
    lp, labels, s = _small(41)
    x = torch.from_numpy(lp).cuda().requires_grad_()
    z = ka.lattice_log_likelihood(x, labels, s)
    assert z.dim() == 0 and z.dtype == torch.float64 and z.device == x.device
    occ, ll = ka.ctc_label_posteriors(lp, labels, s)
    assert float(z.detach()) == ll
    z.backward()
    assert x.grad.dtype == torch.float32
    assert np.array_equal(x.grad.cpu().numpy().view(np.int32), occ.view(np.int32))


def test_autograd_through_log_softmax(env):
    import torch
    ka, _lib, eng = env
    T, V, S = 250, 39, 70
    rng = np.random.default_rng(5)
    logits = rng.normal(size=(T, V)) * 3
    labels = O.hash_labels(S, V, 5)
    lp64 = torch.log_softmax(torch.from_numpy(logits), -1).numpy()
    s = int(O.ctc_best_path_c(lp64.astype(np.float32), labels, 1000, 4)[0][-1])
    x = torch.tensor(logits, dtype=torch.float32, device="cuda", requires_grad=True)
    z = ka.lattice_log_likelihood(torch.log_softmax(x, -1), labels, s)
    z.backward()
    ref = Q.occupancy(torch.log_softmax(x.detach(), -1).cpu().numpy(), labels, s)["occ"]
    sm = torch.softmax(torch.from_numpy(logits), -1).numpy()
    want = ref - sm * ref.sum(-1, keepdims=True)
    assert np.max(np.abs(x.grad.cpu().numpy() - want)) <= 2e-3


def test_autograd_list_input_sums(env):
    import torch
    ka, _lib, eng = env
    items = [_small(50 + i, T=200 + 50 * i, S=50 + 10 * i) for i in range(3)]
    xs = [torch.from_numpy(lp).cuda().requires_grad_() for lp, _, _ in items]
    z = ka.lattice_log_likelihood(xs, [lab for _, lab, _ in items], [s for _, _, s in items])
    assert z.shape == (3,) and z.dtype == torch.float64
    (2.0 * z.sum()).backward()
    for x, (lp, lab, s), zi in zip(xs, items, z.detach().cpu().numpy()):
        occ, ll = ka.ctc_label_posteriors(lp, lab, s)
        assert zi == ll
        assert np.allclose(x.grad.cpu().numpy(), 2.0 * occ, atol=0, rtol=0)


def test_autograd_zero_infinity(env):
    import torch
    ka, _lib, eng = env
    lp, labels, s = _small(61)
    dead = lp.copy()
    dead[:, 0] = -np.inf
    S = len(labels)
    xs = [torch.from_numpy(lp).cuda().requires_grad_(), torch.from_numpy(dead).cuda().requires_grad_()]
    with pytest.raises(ValueError):
        ka.lattice_log_likelihood(xs, [labels, labels], [s, 2 * S])
    z = ka.lattice_log_likelihood(xs, [labels, labels], [s, 2 * S], zero_infinity=True)
    assert float(z[1].detach()) == 0.0 and np.isfinite(float(z[0].detach()))
    z.sum().backward()
    assert bool((xs[1].grad == 0).all()) and bool(torch.isfinite(xs[0].grad).all())
    with pytest.raises(ValueError):
        ka.lattice_log_likelihood(torch.from_numpy(lp).cuda(), labels, 2 * S + 1, zero_infinity=True)
