"""Label occupancy posteriors, CPU side: the float64 reference (tests/occupancy_ref.py) against brute-force path enumeration,
torch autograd of a dense banded alpha recursion and finite differences of Z, its invariants, and the C-ABI / Python boundary
of the feature (no compute: there is no GPU)."""
import ctypes
import re

import numpy as np
import pytest

import occupancy_ref as Q
import posterior_ref as R
from fb_harness import assert_declared_exported_bound, header_text, tiny as _tiny
from oracle import oracle as O

NEW_SYMBOLS = ("ka_ctc_label_posteriors_f32", "ka_ctc_label_posteriors_batch_f32", "ka_label_posterior_workspace_bytes")


@pytest.mark.parametrize("mm", [1, 2, 3, 4, 5])
def test_reference_matches_brute_force(mm):
    rng = np.random.default_rng(300 + mm)
    checked = 0
    for trial in range(40):
        T = int(rng.integers(1, 7 if mm <= 3 else 6))
        S = int(rng.integers(0, 5))
        V = int(rng.integers(2, 6))
        beam = int(rng.choice([2, 3, 5, 1000]))
        lp, labels = _tiny(rng, T, S, V, zero_label=trial % 3 == 0, ninf=trial % 4 == 1)
        terminal = int(rng.integers(0, 2 * S + 1))
        want, want_ll = Q.brute_force(lp, labels, terminal, beam, mm)
        got = Q.occupancy(lp, labels, terminal, beam, mm)
        if want_ll == -np.inf:
            assert got["status"] == R.ZERO_MASS and got["ll"] == -np.inf and np.isnan(got["occ"]).all()
            continue
        assert got["status"] == R.OK
        assert abs(got["ll"] - want_ll) < 1e-9
        np.testing.assert_allclose(got["occ"], want, atol=1e-12)
        checked += 1
    assert checked >= 10


@pytest.mark.parametrize("T,S,V,beam,mm,seed", [(30, 10, 7, 9, 4, 1), (24, 8, 6, 1000, 3, 2), (20, 7, 9, 6, 5, 3), (16, 5, 5, 1000, 1, 4)])
def test_reference_is_the_autograd_gradient_of_z(T, S, V, beam, mm, seed):
    import torch
    rng = np.random.default_rng(seed)
    lp, labels = _tiny(rng, T, S, V, zero_label=True, ninf=True)
    labels[0] = 0
    path = O.ctc_best_path_c(lp, labels, beam, mm)[0]
    terminal = int(path[-1])
    ref = Q.occupancy(lp, labels, terminal, beam, mm)
    assert ref["status"] == R.OK
    x = torch.tensor(lp, dtype=torch.float64, requires_grad=True)
    z = Q.torch_z(x, labels, terminal, beam, mm)
    assert abs(float(z.detach()) - ref["ll"]) < 1e-9
    z.backward()
    assert np.max(np.abs(x.grad.numpy() - ref["occ"])) < 1e-9


def test_reference_matches_central_finite_differences():
    rng = np.random.default_rng(11)
    T, S, V, beam, mm = 40, 12, 8, 11, 4
    lp, labels = _tiny(rng, T, S, V, zero_label=True)
    lp = lp.astype(np.float64)
    terminal = int(O.ctc_best_path_c(lp.astype(np.float32), labels, beam, mm)[0][-1])
    ref = Q.occupancy(lp, labels, terminal, beam, mm)
    h = 1e-5
    for _ in range(40):
        t, v = int(rng.integers(0, T)), int(rng.integers(0, V))
        up, dn = lp.copy(), lp.copy()
        up[t, v] += h
        dn[t, v] -= h
        fd = (R.forward_backward(up, labels, np.full(T, terminal), beam, mm)["ll"]
              - R.forward_backward(dn, labels, np.full(T, terminal), beam, mm)["ll"]) / (2 * h)
        assert abs(fd - ref["occ"][t, v]) < 1e-7, (t, v, fd, ref["occ"][t, v])


def test_rows_sum_to_one_and_dominate_the_path_posterior():
    rng = np.random.default_rng(5)
    for T, S, V, beam, mm in [(60, 20, 9, 12, 4), (50, 15, 6, 1000, 3), (45, 12, 12, 8, 6), (40, 10, 5, 1000, 2)]:
        lp, labels = _tiny(rng, T, S, V, zero_label=True, ninf=True)
        path = O.ctc_best_path_c(lp, labels, beam, mm)[0]
        ref = Q.occupancy(lp, labels, path[-1], beam, mm)
        assert ref["status"] == R.OK
        assert np.max(np.abs(ref["occ"].sum(1) - 1.0)) < 1e-9
        lab = R.expand(labels)
        assert ref["occ"][T - 1, lab[path[-1]]] == pytest.approx(1.0, abs=1e-12)
        post = R.forward_backward(lp, labels, path, beam, mm)["post"]
        assert np.all(ref["occ"][np.arange(T), lab[path]] >= post - 1e-12)


def test_reference_statuses():
    lp = np.log(np.full((5, 4), 0.25, np.float32))
    labels = np.array([1, 2], np.int32)
    assert Q.occupancy(lp, np.array([4], np.int32), 0)["status"] == R.BAD_LABEL
    assert Q.occupancy(lp, labels, 5)["status"] == R.BAD_ARGS
    assert Q.occupancy(lp, labels, -1)["status"] == R.BAD_ARGS
    dead = lp.copy()
    dead[:, 0] = -np.inf
    got = Q.occupancy(dead, labels, 4)
    assert got["status"] == R.ZERO_MASS and got["ll"] == -np.inf and np.isnan(got["occ"]).all()


def test_new_symbols_declared_exported_and_bound():
    lib = assert_declared_exported_bound(NEW_SYMBOLS)
    assert lib.ka_version() >= 102
    assert int(re.search(r"#define KA_VERSION (\d+)", header_text()).group(1)) >= 102


def test_workspace_is_bounded_by_resident_lattices():
    from kokoro_align_amd import _lib
    L = _lib.load_library()

    def ws(n, T, S, V=64, beam=1000, mm=4, mem=1):
        return L.ka_label_posterior_workspace_bytes(n, (ctypes.c_int64 * n)(*[T] * n), (ctypes.c_int64 * n)(*[S] * n), V, beam, mm, mem)

    big = ws(8192, 50000, 5000)
    assert 0 < big <= 16 << 30
    assert ws(2048, 50000, 5000) - ws(1024, 50000, 5000) < 1 << 20     # beyond the resident slots only descriptors grow
    one = ws(1, 50000, 5000)
    assert one >= (50000 // 32) * 1024 * 8                               # the checkpointed columns
    assert one < 64 << 20                                                # ... and no alpha lattice
    assert ws(1, 50000, 5000, mem=0) >= one + 2 * 50000 * 64 * 4        # host buffers are staged in and out
    assert ws(1, 3000, 700, V=5000) >= ws(1, 3000, 700, V=80) + 5000 * 8  # global bins above the LDS cap
    assert ws(2, 50000, 5000, mm=300) == 0


def test_public_api_exists():
    import kokoro_align_amd as ka
    for name in ("ctc_label_posteriors", "ctc_label_posteriors_batch", "ctc_label_posteriors_device", "lattice_log_likelihood",
                 "segment_agreement"):
        assert callable(getattr(ka, name)), name


def test_segment_agreement_uses_align_ranges():
    import kokoro_align_amd as ka
    labels = np.array([3, 1], np.int32)                 # lab' = [0, 3, 0, 1, 0]
    path = np.array([0, 1, 1, 2, 3, 4])
    occ = np.zeros((6, 4), np.float32)
    occ[:, 0] = 0.5
    occ[:, 3] = 0.25
    occ[:, 1] = 0.25
    got = ka.segment_agreement(occ, labels, path, np.array([2, 2, 5, 9]))
    np.testing.assert_allclose(got[[0, 2, 3]], [(0.5 + 0.25) / 2, (0.25 + 0.5 + 0.25) / 3, 0.5])
    assert np.isnan(got[1])


def test_label_posteriors_without_a_gpu_is_a_loud_error():
    """No device: the call raises, never a silent CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import kokoro_align_amd as ka
    lp = np.log(np.full((4, 3), 1 / 3, np.float32))
    with pytest.raises((ka.KAError, ValueError)):
        ka.ctc_label_posteriors(lp, np.array([1], np.int32), 2)
