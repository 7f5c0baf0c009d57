"""Raw ctypes callers of the four forward-backward calls and of their ``_banded`` forms for tests/test_banded_posteriors_gpu.py,
beside fb_harness.py and with its engine set-up: they go to the C ABI through ``eng.lib`` and never through
kokoro_align_amd/posteriors.py.  One function, ``run``, for all eight batch symbols in both memory modes: with ``tables`` it
calls ``ka_ctc_<kind>_banded_batch_f32``, without them the sibling, with otherwise the same arguments, so the two can be compared
bit for bit.

Every output lies in a buffer filled with a sentinel (-7.0, band_lo -9, status 99) that is GUARD entries longer than the output,
and two-dimensional outputs have rows GUARD columns wider than what a call may write: ``Result.guards_intact()`` tells whether a
call wrote outside an output's extent."""
import numpy as np

from fb_harness import GUARD, SENTINEL, I, P, _addresses, _lattices, band_width

KINDS = ("path_posteriors", "label_posteriors", "state_posteriors", "state_durations")


class Result:
    """outs[i]: the lattice's outputs without their guards, in the order of the C signature (path: post [T]; label: occ [T, V];
    state: gamma [K, W], band_lo [K]; durations: duration [L], time_sum [L]); ll, st per lattice; rc of the call."""

    def __init__(self, raw, shapes, ll, st, rc):
        self.raw, self.shapes, self.ll, self.st, self.rc = raw, shapes, ll, st, rc
        self.outs = [tuple(self._payload(b, s) for b, s in zip(bufs, shp)) for bufs, shp in zip(raw, shapes)]

    @staticmethod
    def _payload(buf, shape):
        if len(shape) == 1:
            return buf[:shape[0]].copy()
        rows, cols = shape
        return buf[:rows * (cols + GUARD)].reshape(rows, cols + GUARD)[:, :cols].copy()

    def guards_intact(self):
        for bufs, shp in zip(self.raw, self.shapes):
            for buf, shape in zip(bufs, shp):
                fill = -9 if buf.dtype == np.int64 else SENTINEL
                if len(shape) == 1:
                    guard = buf[shape[0]:]
                else:
                    rows, cols = shape
                    guard = np.concatenate([buf[:rows * (cols + GUARD)].reshape(rows, cols + GUARD)[:, cols:].reshape(-1),
                                            buf[rows * (cols + GUARD):]])
                if not np.all(guard == fill):
                    return False
        return True

    def same_bits(self, other):
        """Outputs, log-likelihoods (as bits: NaN equals NaN), statuses and rc."""
        if self.rc != other.rc or not np.array_equal(self.st, other.st):
            return False
        if not np.array_equal(self.ll.view(np.uint64), other.ll.view(np.uint64)):
            return False
        return all(a.shape == b.shape and a.tobytes() == b.tobytes() for x, y in zip(self.outs, other.outs) for a, b in zip(x, y))


def _buffer(shape, dtype):
    n = shape[0] if len(shape) == 1 else shape[0] * (shape[1] + GUARD)
    return np.full(n + GUARD, -9 if dtype == np.int64 else SENTINEL, dtype)


def run(eng, _lib, kind, lps, labs, own, beam, mm, tables=None, device=False, null_table=None):
    """``own``: the call's own input - path posteriors: a list of paths; state posteriors: (terminals, frame lists); the others:
    terminals.  ``tables``: a list of tables (int32 as they go in), or None for the sibling.  ``null_table``: "array" passes a
    NULL table array, an index passes a NULL entry there (banded calls only)."""
    assert kind in KINDS
    n = len(lps)
    lps, Ts, V, lds, labs, Ss = _lattices(lps, labs)
    T = [x.shape[0] for x in lps]
    L = [2 * x.shape[0] + 1 for x in labs]
    W = [band_width(x.shape[0], beam) for x in labs]
    ins = []                                   # per-lattice input arrays that follow the memory mode
    if kind == "path_posteriors":
        ins = [np.ascontiguousarray(p, np.int32) for p in own]
        shapes = [((t,),) for t in T]
        dtypes = (np.float32,)
    elif kind == "label_posteriors":
        terms = own
        shapes = [((t, V),) for t in T]
        dtypes = (np.float32,)
    elif kind == "state_posteriors":
        terms, frames = own
        frs = [np.ascontiguousarray(np.asarray(f).reshape(-1), np.int64) for f in frames]
        shapes = [((len(f), w), (len(f),)) for f, w in zip(frs, W)]
        dtypes = (np.float32, np.int64)
    else:
        terms = own
        shapes = [((l,), (l,)) for l in L]
        dtypes = (np.float64, np.float64)
    raw = [tuple(_buffer(s, d) for s, d in zip(shp, dtypes)) for shp in shapes]
    tabs = None if tables is None else [np.ascontiguousarray(t, np.int32) for t in tables]
    ll = np.zeros(n, np.float64)
    st = np.full(n, 99, np.int32)
    if device:
        import torch
        up = lambda xs: [torch.from_numpy(x).cuda() for x in xs]
        d_lps, d_labs, d_ins = up(lps), up(labs), up(ins)
        d_tabs = None if tabs is None else up(tabs)
        d_raw = [up(bufs) for bufs in raw]
        addr = lambda xs: [x.data_ptr() for x in xs]
        a_lp, a_lab, a_in = addr(d_lps), addr(d_labs), addr(d_ins)
        a_tab = None if tabs is None else addr(d_tabs)
        a_out = [addr(bufs) for bufs in d_raw]
        mem = _lib.KA_MEM_DEVICE
    else:
        addr = lambda xs: [x.ctypes.data for x in xs]
        a_lp, a_lab, a_in = addr(lps), addr(labs), addr(ins)
        a_tab = None if tabs is None else addr(tabs)
        a_out = [addr(bufs) for bufs in raw]
        mem = _lib.KA_MEM_HOST
    out_col = lambda k: _addresses([a[k] for a in a_out])
    if kind == "path_posteriors":
        tail = (_addresses(a_in), out_col(0))
    elif kind == "label_posteriors":
        tail = (I(terms), out_col(0), I([V + GUARD] * n))
    elif kind == "state_posteriors":
        tail = (I(terms), P(frs), I([len(f) for f in frs]), out_col(0), I([w + GUARD for w in W]), out_col(1))
    else:
        tail = (I(terms), out_col(0), out_col(1))
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
    return Result(raw, shapes, ll, st, rc)
