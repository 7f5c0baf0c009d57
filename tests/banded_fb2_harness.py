"""Raw ctypes callers of the state-visit, boundary-quantile, sampled-path and MEA-path calls and of their ``_banded`` forms
for tests/test_banded_posteriors2_gpu.py, beside banded_fb_harness.py and with its ``Result``: they go to the C ABI through
``eng.lib`` and never through kokoro_align_amd/posteriors.py.  One function, ``run``, for all eight batch symbols in both memory
modes: with ``tables`` it calls ``ka_ctc_<kind>_banded_batch_f32``, without them the sibling, with otherwise the same arguments,
so the two can be compared bit for bit.

Every output lies in a buffer filled with a sentinel (-7, status 99) that is GUARD entries longer than the output, and
two-dimensional outputs have rows GUARD columns wider than what a call may write (``Result.guards_intact()``).  The MEA call's
expected accuracies are one host array per call, filled with the sentinel first: ``Result.ea``."""
import ctypes

import numpy as np

import banded_fb_harness as BH
from fb_harness import GUARD, SENTINEL, I, P, _addresses, _lattices

KINDS = ("state_visits", "boundary_quantiles", "sample_paths", "mea_path")
LEVELS = (0.05, 0.5, 0.95)


class Result(BH.Result):
    """outs[i]: visits: (visit [L], exit_time [L]); quantiles: (quantile [K, M],); samples: (paths [n_samples, T],); MEA:
    (path [T],), with ``ea`` [n] the expected accuracies."""

    def __init__(self, raw, shapes, ll, st, rc, ea=None):
        super().__init__(raw, shapes, ll, st, rc)
        self.ea = ea

    def same_bits(self, other):
        if (self.ea is None) != (other.ea is None) or (self.ea is not None and self.ea.tobytes() != other.ea.tobytes()):
            return False
        return super().same_bits(other)


def run(eng, _lib, kind, lps, labs, own, beam, mm, tables=None, device=False, null_table=None, levels=LEVELS):
    """``own``: visits and MEA: terminals; quantiles: (terminals, cut lists); samples: (terminals, n_samples list, seed list).
    ``tables``: a list of tables, or None for the sibling.  ``null_table``: "array" passes a NULL table array, an index passes a
    NULL entry there (banded calls only)."""
    assert kind in KINDS
    n = len(lps)
    lps, Ts, V, lds, labs, Ss = _lattices(lps, labs)
    T = [x.shape[0] for x in lps]
    L = [2 * x.shape[0] + 1 for x in labs]
    lv = np.ascontiguousarray(levels, np.float64)
    M = len(lv)
    if kind == "state_visits":
        terms = own
        shapes = [((l,), (l,)) for l in L]
        dtypes = (np.float64, np.float64)
    elif kind == "boundary_quantiles":
        terms, cuts = own
        cuts = [np.ascontiguousarray(np.asarray(c).reshape(-1), np.int64) for c in cuts]
        shapes = [((len(c), M),) for c in cuts]
        dtypes = (np.int32,)
    elif kind == "sample_paths":
        terms, Ks, seeds = own
        shapes = [((k, t),) for k, t in zip(Ks, T)]
        dtypes = (np.int32,)
    else:
        terms = own
        shapes = [((t,),) for t in T]
        dtypes = (np.int32,)
    raw = [tuple(BH._buffer(s, d) for s, d in zip(shp, dtypes)) for shp in shapes]
    tabs = None if tables is None else [np.ascontiguousarray(t, np.int32) for t in tables]
    ll = np.zeros(n, np.float64)
    st = np.full(n, 99, np.int32)
    ea = np.full(n, SENTINEL, np.float64) if kind == "mea_path" else None
    if device:
        import torch
        up = lambda xs: [torch.from_numpy(x).cuda() for x in xs]
        d_lps, d_labs = up(lps), up(labs)
        d_tabs = None if tabs is None else up(tabs)
        d_raw = [up(bufs) for bufs in raw]
        addr = lambda xs: [x.data_ptr() for x in xs]
        a_lp, a_lab = addr(d_lps), addr(d_labs)
        a_tab = None if tabs is None else addr(d_tabs)
        a_out = [addr(bufs) for bufs in d_raw]
        mem = _lib.KA_MEM_DEVICE
    else:
        addr = lambda xs: [x.ctypes.data for x in xs]
        a_lp, a_lab = addr(lps), addr(labs)
        a_tab = None if tabs is None else addr(tabs)
        a_out = [addr(bufs) for bufs in raw]
        mem = _lib.KA_MEM_HOST
    out_col = lambda k: _addresses([a[k] for a in a_out])
    if kind == "state_visits":
        tail = (I(terms), out_col(0), out_col(1))
    elif kind == "boundary_quantiles":
        tail = (I(terms), P(cuts), I([len(c) for c in cuts]), lv.ctypes.data, M, out_col(0), I([M + GUARD] * n))
    elif kind == "sample_paths":
        a_K = np.ascontiguousarray(Ks, np.int32)
        a_seed = np.ascontiguousarray([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], np.uint64)
        tail = (I(terms), a_K.ctypes.data, a_seed.ctypes.data, out_col(0), I([t + GUARD for t in T]))
    else:
        tail = (I(terms), out_col(0), ea.ctypes.data)
    head = (eng.handle, n, _addresses(a_lp), Ts, V, lds, _addresses(a_lab), Ss, beam, mm)
    if tables is None:
        rc = getattr(eng.lib, f"ka_ctc_{kind}_batch_f32")(*head, *tail, ll.ctypes.data, st.ctypes.data, mem, None)
    else:
        if null_table == "array":
            p_tab = None
        else:
            p_tab = _addresses([None if null_table == i else a for i, a in enumerate(a_tab)])
        rc = getattr(eng.lib, f"ka_ctc_{kind}_banded_batch_f32")(*head, p_tab, *tail, ll.ctypes.data, st.ctypes.data, mem, None)
    if device:
        import torch
        torch.cuda.synchronize()
        raw = [tuple(x.cpu().numpy() for x in bufs) for bufs in d_raw]
    return Result(raw, shapes, ll, st, rc, ea)


def single(eng, _lib, kind, lp, labels, own, beam, mm, table, levels=LEVELS):
    """The single-lattice symbol ``ka_ctc_<kind>_banded_f32`` on host buffers: (outputs as ``run`` shapes them, ll, rc[, ea])."""
    lp = np.ascontiguousarray(lp, np.float32)
    labels = np.ascontiguousarray(labels, np.int32)
    tab = np.ascontiguousarray(table, np.int32)
    T, V = lp.shape
    L = 2 * len(labels) + 1
    ll = np.zeros(1, np.float64)
    head = (eng.handle, lp.ctypes.data, T, V, V, labels.ctypes.data, len(labels), beam, mm, tab.ctypes.data)
    f = getattr(eng.lib, f"ka_ctc_{kind}_banded_f32")
    if kind == "state_visits":
        a, b = np.full(L, SENTINEL), np.full(L, SENTINEL)
        rc = f(*head, int(own), a.ctypes.data, b.ctypes.data, ll.ctypes.data, _lib.KA_MEM_HOST, None)
        return (a, b), ll[0], rc
    if kind == "boundary_quantiles":
        term, cuts = own
        cuts = np.ascontiguousarray(cuts, np.int64)
        lv = np.ascontiguousarray(levels, np.float64)
        q = np.full((len(cuts), len(lv)), -7, np.int32)
        rc = f(*head, int(term), cuts.ctypes.data, len(cuts), lv.ctypes.data, len(lv), q.ctypes.data, len(lv), ll.ctypes.data,
               _lib.KA_MEM_HOST, None)
        return (q,), ll[0], rc
    if kind == "sample_paths":
        term, K, seed = own
        paths = np.full((K, T), -7, np.int32)
        rc = f(*head, int(term), int(K), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), paths.ctypes.data, T, ll.ctypes.data,
               _lib.KA_MEM_HOST, None)
        return (paths,), ll[0], rc
    path = np.full(T, -7, np.int32)
    ea = np.full(1, SENTINEL)
    rc = f(*head, int(own), path.ctypes.data, ea.ctypes.data, ll.ctypes.data, _lib.KA_MEM_HOST, None)
    return (path,), ll[0], rc, ea[0]
