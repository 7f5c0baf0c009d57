"""What an engine keeps between calls, through the raw C ABI (``eng.lib``): the one batch in flight, the settings, the timing
events of a profiled batch and the halo-clean range of the workspace.  A call that is refused, one that only plans and the
redo inside ka_batch_finish must leave the batch in flight as it was; a forward-backward call, which lays its own layout
over the shared workspace, must drop what the last tiled launch left clean there.

Reference of every best-path result: oracle.ctc_best_path_c, bit for bit.  Outputs start as sentinels (-9, -7.0, status 99,
as in fb_harness.py), so a call that wrote nothing shows."""
import ctypes

import numpy as np
import pytest

import fb_harness as H
from oracle import oracle as O
from test_books_gpu import _lattice_with_neg_inf

pytestmark = pytest.mark.gpu

MM = 4
SMALL = (40, 6, 8, 7)                # T, S, V, seed
LARGE = ([6000], [3000], 64, 2000)   # T, S, V, beam of the shape that is only planned
# the smallest S whose 2S+1 positions need two 128-position tiles (ka_debug_plan_tiles_width reports 2 from S = 64, 1 below)
TILED = [(96, 64, 8, 11), (120, 70, 8, 12)]


@pytest.fixture(scope="module")
def env():
    ka, _lib, eng = H.engine()
    yield _lib, eng
    eng.set_mode("auto")
    eng.set_backtrace("auto")
    eng.set_tile_width(0)
    eng.set_verify(0)
    eng.set_profiling(False)


_want = {}


def _lattice(T, S, V, seed):
    return O.hash_logprobs(T, V, seed), O.hash_labels(S, V, seed)


def _oracle(key, lp, lab, beam):
    """(path, labels, scores, total, end) of the C oracle, computed once per lattice."""
    if key not in _want:
        _want[key] = O.ctc_best_path_c(lp, lab, beam, MM, return_total=True)
    return _want[key]


def _dev_ptrs(tensors):
    return ctypes.cast((ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors]), ctypes.POINTER(ctypes.c_void_p))


class RawBatch:
    """Device copies of host lattices, sentinel-prefilled device outputs and the tables of one raw best-path call."""

    def __init__(self, lattices, beam):
        import torch
        self.n, self.beam = len(lattices), beam
        self.V = lattices[0][0].shape[1]
        self.lps = [torch.from_numpy(np.ascontiguousarray(lp, np.float32)).cuda() for lp, _ in lattices]
        self.labs = [torch.from_numpy(np.ascontiguousarray(lab, np.int32)).cuda() for _, lab in lattices]
        Ts = [int(x.shape[0]) for x in self.lps]
        self.path = [torch.full((t,), -9, dtype=torch.int32, device="cuda") for t in Ts]
        self.lab_out = [torch.full((t,), -9, dtype=torch.int32, device="cuda") for t in Ts]
        self.scores = [torch.full((t,), -7.0, dtype=torch.float32, device="cuda") for t in Ts]
        self.Ts, self.Ss, self.lds = H.I(Ts), H.I([int(x.shape[0]) for x in self.labs]), H.I([self.V] * self.n)
        self.total = np.full(self.n, -7.0, np.float32)
        self.status = np.full(self.n, 99, np.int32)
        torch.cuda.synchronize()

    def enqueue(self, eng):
        return eng.lib.ka_ctc_best_path_batch_enqueue_f32(eng.handle, self.n, _dev_ptrs(self.lps), self.Ts, self.V, self.lds, _dev_ptrs(self.labs),
                                                          self.Ss, self.beam, MM, _dev_ptrs(self.path), _dev_ptrs(self.lab_out),
                                                          _dev_ptrs(self.scores), None)

    def finish(self, eng):
        return eng.lib.ka_batch_finish(eng.handle, self.total.ctypes.data, self.status.ctypes.data)

    def check(self, k, want, tag):
        assert self.status[k] == 0, (tag, k, self.status[k])
        assert np.array_equal(self.path[k].cpu().numpy(), want[0]), f"{tag}: best_path differs"
        assert np.array_equal(self.lab_out[k].cpu().numpy(), want[1]), f"{tag}: best_labels differ"
        assert np.array_equal(self.scores[k].cpu().numpy().view(np.int32), want[2].view(np.int32)), f"{tag}: best_scores differ"
        assert self.total[k].view(np.int32) == np.float32(want[3]).view(np.int32), f"{tag}: total differs"


def _small():
    lp, lab = _lattice(*SMALL)
    return (lp, lab), _oracle("small", lp, lab, 1000)


def _plan_bytes(eng, _lib):
    Ts, Ss, V, beam = LARGE
    return int(eng.lib.ka_engine_workspace_bytes(eng.handle, 1, H.I(Ts), H.I(Ss), V, beam, MM, _lib.KA_MEM_DEVICE))


def _kernel_ms(eng):
    ms = (ctypes.c_float * 4)(*[-1.0] * 4)
    return eng.lib.ka_engine_last_kernel_ms(eng.handle, ms), list(ms)


def test_second_enqueue_is_refused_and_harms_nothing(env):
    _lib, eng = env
    lat, want = _small()
    b = RawBatch([lat], 1000)
    assert b.enqueue(eng) == _lib.KA_OK
    try:
        assert b.enqueue(eng) == _lib.KA_ERR_BAD_ARGS
        assert "already enqueued" in _lib.last_error()
        lp, lab, head = H._one(*lat)
        post = np.full(lp.shape[0], -7.0, np.float32)
        ll = np.full(1, -7.0, np.float64)
        rc = eng.lib.ka_ctc_path_posteriors_f32(eng.handle, *head, 1000, MM, want[0].ctypes.data, post.ctypes.data, ll.ctypes.data,
                                                _lib.KA_MEM_HOST, None)
        assert rc == _lib.KA_ERR_BAD_ARGS
        assert "already enqueued" in _lib.last_error()
        assert (post == -7.0).all() and ll[0] == -7.0
    finally:
        rc = b.finish(eng)
    assert rc == _lib.KA_OK
    b.check(0, want, "after two refused calls")


def test_planning_touches_nothing(env):
    _lib, eng = env
    idle_auto = _plan_bytes(eng, _lib)
    eng.set_mode("tiled")
    idle_tiled = _plan_bytes(eng, _lib)
    eng.set_mode("auto")
    assert idle_auto > 0 and idle_tiled > 0
    lat, want = _small()
    b = RawBatch([lat], 1000)
    assert b.enqueue(eng) == _lib.KA_OK
    try:
        assert _plan_bytes(eng, _lib) == idle_auto
        eng.set_mode("tiled")
        assert _plan_bytes(eng, _lib) == idle_tiled
        eng.set_mode("auto")
        assert _plan_bytes(eng, _lib) == idle_auto
    finally:
        eng.set_mode("auto")
        rc = b.finish(eng)
    assert rc == _lib.KA_OK
    b.check(0, want, "after planning another shape")


def test_redo_inside_a_profiled_batch(env):
    """The second wide lattice holds -inf: the tiled form declines it and ka_batch_finish redoes it through the generic kernels,
    a launch of its own inside the profiled batch.  The batch keeps its size, its statuses and its times."""
    _lib, eng = env
    wide = [_lattice_with_neg_inf(6000, 3000, 64, 41, 0.0), _lattice_with_neg_inf(6000, 3000, 64, 42, 0.10)]
    small = _lattice(SMALL[0], SMALL[1], 64, SMALL[3])      # (a batch has one V)
    want_small = _oracle("small, V = 64", *small, 2000)
    want = [_oracle(("wide", k), lp, lab, 2000) for k, (lp, lab) in enumerate(wide)] + [want_small]
    eng.set_profiling(True)
    try:
        b = RawBatch(wide + [small], 2000)
        assert b.enqueue(eng) == _lib.KA_OK
        assert b.finish(eng) == _lib.KA_OK, _lib.last_error()
        assert (b.status != 99).all()
        for k in range(3):
            b.check(k, want[k], f"profiled batch, lattice {k}")
        rc, ms = _kernel_ms(eng)
        assert rc == _lib.KA_OK and all(np.isfinite(x) and x >= 0 for x in ms), (rc, ms)
        one = RawBatch([small], 2000)
        assert one.enqueue(eng) == _lib.KA_OK and one.finish(eng) == _lib.KA_OK
        one.check(0, want_small, "profiled batch of the small lattice")
        rc, ms = _kernel_ms(eng)
        assert rc == _lib.KA_OK and all(np.isfinite(x) and x >= 0 for x in ms), (rc, ms)
        eng.set_profiling(False)
        one = RawBatch([small], 2000)
        assert one.enqueue(eng) == _lib.KA_OK and one.finish(eng) == _lib.KA_OK
        one.check(0, want_small, "unprofiled batch")
        rc, _ = _kernel_ms(eng)
        assert rc == _lib.KA_ERR_BAD_ARGS and "no profiled batch has been finished" in _lib.last_error()
    finally:
        eng.set_profiling(False)


def test_forward_backward_call_drops_the_halo_clean_range(env):
    """The second tiled launch has the shape of the first, so it would skip its halo fill - but the label posteriors in between
    have written over the region.  With verify on, a tile that reads a slot nobody wrote reports KA_ERR_INTERNAL."""
    _lib, eng = env
    lattices = [_lattice(*shape) for shape in TILED]
    want = [_oracle(("tiled", k), lp, lab, 1000) for k, (lp, lab) in enumerate(lattices)]
    for T, S, V, _ in TILED:
        assert eng.lib.ka_debug_plan_tiles_width(T, S, V, 1000, MM, 128, None, None, 0, None) >= 2
    eng.set_tile_width(128)
    eng.set_mode("tiled")
    eng.set_backtrace("serial")
    eng.set_verify(1)
    try:
        first = RawBatch(lattices, 1000)
        tiled_bytes = int(eng.lib.ka_engine_workspace_bytes(eng.handle, first.n, first.Ts, first.Ss, first.V, 1000, MM, _lib.KA_MEM_DEVICE))
        fb_bytes = int(eng.lib.ka_label_posterior_workspace_bytes(1, H.I([TILED[0][0]]), H.I([TILED[0][1]]), TILED[0][2], 1000, MM, _lib.KA_MEM_HOST))
        assert fb_bytes >= tiled_bytes > 0, "the forward-backward call must cover the tiled launch's halo region"
        assert first.enqueue(eng) == _lib.KA_OK and first.finish(eng) == _lib.KA_OK, _lib.last_error()
        occ, z = H.label_call_one(eng, _lib, *lattices[0], int(want[0][0][-1]), 1000, MM, fill=-7.0)
        assert np.isfinite(z) and (occ != -7.0).all()
        second = RawBatch(lattices, 1000)
        assert second.enqueue(eng) == _lib.KA_OK and second.finish(eng) == _lib.KA_OK, _lib.last_error()
        for k in range(len(lattices)):
            first.check(k, want[k], f"first tiled launch, lattice {k}")
            second.check(k, want[k], f"tiled launch after the label posteriors, lattice {k}")
    finally:
        eng.set_verify(0)
        eng.set_mode("auto")
        eng.set_backtrace("auto")
        eng.set_tile_width(0)
