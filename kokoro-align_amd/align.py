"""Drop-in for kokoro_align/align.py: same functions, keyword names, defaults, file formats.

    ctc_best_path(log_probs, labels, beam_size=1000, max_move=4)      <- align.py:43-109
    best_path(input_file, voca_file, output_file)                     <- align.py:112-124
    align(best_path_file, mfcc_file, voca_file, align_file, remove_wordsep)  <- align.py:127-169
    pandas_read_align(files)                                          <- align.py:172-190

plus what the reference has no name for: many lattices in one launch (ctc_best_path_batch, DeviceBatch,
ctc_best_path_device), the log-softmax of align.py:116-117 on the device (log_softmax_device) and the best path over a band
the caller gives (ctc_best_path_banded[_batch|_device] with the tables diagonal_band, anchored_band, band_around_path and the
diagnostic band_edge_contact), over a band that steers itself (ctc_best_path_tracking[_batch|_device]), the banded best path
with the caller's boundary conditions (ctc_best_path_resume[_batch|_device], free_start_scores, ctc_best_path_chunked) and the
two together (ctc_best_path_tracking_resume[_batch|_device], ctc_best_path_tracking_chunked), and how much of a resumed
chunk's path is final (ctc_best_path_determined[_batch|_device], ctc_best_path_tracking_determined[_batch|_device]) with the
aligner that commits frames while it is fed (StreamingAligner).

The DP + backtrace (the reference's per-frame NumPy loop) run in the HIP library through the C
ABI of include/kokoro_align_amd.h.  NumPy arrays are handed over as host buffers; torch tensors
on a ROCm device are handed over by pointer and the results stay on the device.  The batch calls take their
lattices through _lattices.py, as the forward-backward calls over the same band (posteriors.py) do.
"""
import os

import numpy as np

from . import _lib
from ._lattices import (_band_tables, _current_device, _device_lattices, _host_lattices, _i64_array, _is_tensor,  # noqa: F401
                        _ptr_array, _stream_ptr)
from .encoder import decode_text, merge_repeated


# ------------------------------------------------------------------------------------------
# ctc_best_path
# ------------------------------------------------------------------------------------------
def ctc_best_path(log_probs, labels, beam_size=1000, max_move=4, verbose=True):
    """CTC best path of ``labels`` through ``log_probs`` (reference: align.py:43-109).

    log_probs [T, V] float32, labels [S] integer ids (blanks are inserted here).  Returns
    (best_path int32 [T] in blank-expanded positions, best_labels int32 [T], best_scores
    float32 [T]).  NumPy in -> NumPy out; ROCm torch tensors in -> torch tensors out (same
    device).  Raises ValueError where the reference does (no live state in the last frame).

    Differences from the reference, by design: float64 ``log_probs`` are cast to float32 first;
    NaN / +inf log-probs are not supported (the reference's np.argmax treats NaN as a maximum).
    """
    if _is_tensor(log_probs):
        out = ctc_best_path_device([log_probs], [labels], beam_size, max_move, verbose=verbose)
        return out[0]
    lp = np.ascontiguousarray(log_probs, dtype=np.float32)
    lab = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)
    if lp.ndim != 2:
        raise ValueError("log_probs must be [T, V]")
    T, V = lp.shape
    S = lab.shape[0]
    if verbose:  # the reference prints these two lines (align.py:53-54)
        print(f"Label length: {2 * S + 1}")
        print(f"Time length: {T}")
    if T == 0:
        raise IndexError("list index out of range")  # reference: beams[-1] on an empty list, align.py:101
    path = np.empty(T, np.int32)
    lout = np.empty(T, np.int32)
    sout = np.empty(T, np.float32)
    eng = _lib.default_engine(_current_device())
    rc = eng.lib.ka_ctc_best_path_f32(eng.handle, lp.ctypes.data, T, V, V, lab.ctypes.data, S, int(beam_size),
                                      int(max_move), path.ctypes.data, lout.ctypes.data, sout.ctypes.data,
                                      None, _lib.KA_MEM_HOST, None)
    _lib.check(rc, "ctc_best_path")
    return path, lout, sout


# ------------------------------------------------------------------------------------------
# the batch calls: plain, over a caller-given band, over a self-steering band
# ------------------------------------------------------------------------------------------
END_RULES = {"highest": 0, "best": 1}

# per call: the dtypes of its outputs, and the statuses that ``return_status`` lets through without raising
_BEST_PATH_CALLS = {
    "": ((np.int32, np.int32, np.float32), (_lib.KA_OK, _lib.KA_ERR_EMPTY_BEAM, _lib.KA_ERR_BAD_LABEL, _lib.KA_ERR_NAN, _lib.KA_ERR_NONFINITE)),
    "_banded": ((np.int32, np.int32, np.float32), (_lib.KA_OK, _lib.KA_ERR_EMPTY_BEAM, _lib.KA_ERR_BAD_LABEL, _lib.KA_ERR_NAN, _lib.KA_ERR_BAD_ARGS)),
    "_tracking": ((np.int32, np.int32, np.float32, np.int32), (_lib.KA_OK, _lib.KA_ERR_EMPTY_BEAM, _lib.KA_ERR_BAD_LABEL, _lib.KA_ERR_NAN)),
    "_resume": ((np.int32, np.int32, np.float32), (_lib.KA_OK, _lib.KA_ERR_EMPTY_BEAM, _lib.KA_ERR_BAD_LABEL, _lib.KA_ERR_NAN, _lib.KA_ERR_BAD_ARGS)),
    "_tracking_resume": ((np.int32, np.int32, np.float32, np.int32),
                         (_lib.KA_OK, _lib.KA_ERR_EMPTY_BEAM, _lib.KA_ERR_BAD_LABEL, _lib.KA_ERR_NAN, _lib.KA_ERR_BAD_ARGS)),
}
_BEST_PATH_CALLS["_determined"] = _BEST_PATH_CALLS["_resume"]
_BEST_PATH_CALLS["_tracking_determined"] = _BEST_PATH_CALLS["_tracking_resume"]


def _run_best_path(lat, call, beam_size, max_move, own_args, outputs, return_status, more_outputs=()):
    """The call ``ka_ctc_best_path<call>_batch_f32`` ("", "_banded", "_tracking", "_resume", "_tracking_resume", "_determined",
    "_tracking_determined"): the arguments all take, ``own_args``
    behind ``max_move`` (the band tables; period and end rule; start rows and ends), then the outputs (paths, labels, scores and,
    for tracking, the tables walked: allocated here, or the caller's ``outputs`` after a check), ``more_outputs`` as they are
    (the resumed call's last rows and entries), totals and statuses, and the status handling of ``return_status``.
    KA_ERR_BAD_ARGS is let through only as a lattice's own status (a bad table), not as the call's."""
    dtypes, let_through = _BEST_PATH_CALLS[call]
    if outputs is None:
        outputs = [[lat.empty(T, dt) for T in lat.T] for dt in dtypes]
    elif len(outputs) != len(dtypes) or any(len(arrs) != lat.n or not all(lat.is_out(a, (T,), dt) for a, T in zip(arrs, lat.T))
                                            for arrs, dt in zip(outputs, dtypes)):
        raise ValueError(f"outputs must be {len(dtypes)} lists of contiguous {' / '.join(np.dtype(dt).name for dt in dtypes)} "
                         "arrays of T_i elements where the inputs are")
    name = f"ctc_best_path{call}_{lat.form}"
    status = np.zeros(lat.n, np.int32)
    total = np.zeros(lat.n, np.float32)
    eng = lat.engine()
    p_lp, _k1 = _ptr_array([lat.ptr(x) for x in lat.lps])
    p_lab, _k2 = _ptr_array([lat.ptr(x) for x in lat.labs])
    p_T, _k3 = _i64_array(lat.T)
    p_S, _k4 = _i64_array(lat.S)
    p_ld, _k5 = _i64_array([lat.ld(x) for x in lat.lps])
    p_outs = [_ptr_array([lat.ptr(x) for x in arrs]) for arrs in outputs]
    with lat.guard():
        rc = getattr(eng.lib, f"ka_ctc_best_path{call}_batch_f32")(
            eng.handle, lat.n, p_lp, p_T, lat.V, p_ld, p_lab, p_S, int(beam_size), int(max_move), *own_args,
            *[p for p, _ in p_outs], *more_outputs, total.ctypes.data, status.ctypes.data, lat.mem, lat.stream())
    results = list(zip(*outputs))
    if return_status:
        if rc not in let_through or (rc == _lib.KA_ERR_BAD_ARGS and not np.any(status == _lib.KA_ERR_BAD_ARGS)):
            _lib.check(rc, name)
        return results, status.tolist(), total
    _lib.check(rc, name)
    return results


def _best_path_banded(lat, band_lo, beam_size, max_move, outputs, return_status):
    tables = _band_tables(lat, band_lo)         # (held until the call has returned: the addresses below are theirs)
    p_band, _k = _ptr_array([lat.ptr(x) for x in tables])
    return _run_best_path(lat, "_banded", beam_size, max_move, (p_band,), outputs, return_status)


def _best_path_tracking(lat, beam_size, max_move, period, end_rule, outputs, return_status):
    end_rule = END_RULES[end_rule] if isinstance(end_rule, str) else int(end_rule)
    return _run_best_path(lat, "_tracking", beam_size, max_move, (int(period), end_rule), outputs, return_status)


def ctc_best_path_batch(log_probs_list, labels_list, beam_size=1000, max_move=4, device=None,
                        return_status=False):
    """Independent lattices (one per audio file) in ONE launch; host NumPy buffers in and out.

    Returns a list of (best_path, best_labels, best_scores); with ``return_status`` also the
    per-lattice status list (0 ok, -1 empty beam = the reference's ValueError) and total scores,
    in which case failures do not raise.
    """
    lat = _host_lattices(log_probs_list, labels_list, None, None, device)
    if lat is None:
        return ([], [], []) if return_status else []
    return _run_best_path(lat, "", beam_size, max_move, (), None, return_status)


class DeviceBatch:
    """A batch of device-resident lattices with its pointer tables prebuilt, so that a
    launch is one C call.  Tensors are torch ROCm tensors (float32 log-probs [T_i, V] with
    unit column stride, int32 labels [S_i]); outputs are allocated here and reused."""

    def __init__(self, log_probs, labels, beam_size=1000, max_move=4, outputs=None):
        import torch
        assert len(log_probs) == len(labels) and len(log_probs) > 0
        dev = log_probs[0].device
        self.device_index = dev.index if dev.index is not None else torch.cuda.current_device()
        self.n = len(log_probs)
        self.V = int(log_probs[0].shape[1])
        self.log_probs, self.labels = [], []
        for lp, lab in zip(log_probs, labels):
            if lp.dtype != torch.float32:
                lp = lp.float()
            if lp.dim() != 2 or lp.shape[1] != self.V or lp.shape[0] == 0:
                raise ValueError("log_probs must be non-empty [T_i, V] tensors with one V")
            if lp.stride(1) != 1:
                lp = lp.contiguous()
            lab = lab.reshape(-1)
            if lab.dtype != torch.int32 or not lab.is_contiguous() or lab.device != dev:
                lab = lab.to(device=dev, dtype=torch.int32).contiguous()
            self.log_probs.append(lp)
            self.labels.append(lab)
        self.T = [int(x.shape[0]) for x in self.log_probs]
        self.S = [int(x.shape[0]) for x in self.labels]
        if outputs is None:
            self.path = [torch.empty(t, dtype=torch.int32, device=dev) for t in self.T]
            self.best_labels = [torch.empty(t, dtype=torch.int32, device=dev) for t in self.T]
            self.best_scores = [torch.empty(t, dtype=torch.float32, device=dev) for t in self.T]
        else:
            self.path, self.best_labels, self.best_scores = outputs
        self.beam_size, self.max_move = int(beam_size), int(max_move)
        self.engine = _lib.default_engine(self.device_index)
        self._p_lp, self._k1 = _ptr_array([x.data_ptr() for x in self.log_probs])
        self._p_lab, self._k2 = _ptr_array([x.data_ptr() for x in self.labels])
        self._p_path, self._k3 = _ptr_array([x.data_ptr() for x in self.path])
        self._p_lout, self._k4 = _ptr_array([x.data_ptr() for x in self.best_labels])
        self._p_sout, self._k5 = _ptr_array([x.data_ptr() for x in self.best_scores])
        self._p_T, self._k6 = _i64_array(self.T)
        self._p_S, self._k7 = _i64_array(self.S)
        self._p_ld, self._k8 = _i64_array([x.stride(0) for x in self.log_probs])
        self.status = np.zeros(self.n, np.int32)
        self.total = np.zeros(self.n, np.float32)

    def workspace_bytes(self):
        """device workspace this batch's engine will carve for it, with the engine's current mode settings"""
        e = self.engine
        return int(e.lib.ka_engine_workspace_bytes(e.handle, self.n, self._p_T, self._p_S, self.V, self.beam_size,
                                                   self.max_move, _lib.KA_MEM_DEVICE))

    def enqueue(self):
        """Launch prep + forward DP + backtrace on torch's current stream; no host sync."""
        e = self.engine
        rc = e.lib.ka_ctc_best_path_batch_enqueue_f32(
            e.handle, self.n, self._p_lp, self._p_T, self.V, self._p_ld, self._p_lab, self._p_S,
            self.beam_size, self.max_move, self._p_path, self._p_lout, self._p_sout,
            _stream_ptr(self.device_index))
        _lib.check(rc, "ctc_best_path_batch_enqueue")

    def finish(self, raise_on_error=True):
        """Synchronise the stream and fetch per-lattice status / total scores."""
        e = self.engine
        rc = e.lib.ka_batch_finish(e.handle, self.total.ctypes.data, self.status.ctypes.data)
        if raise_on_error:
            _lib.check(rc, "ctc_best_path_batch")
        elif rc not in (_lib.KA_OK, _lib.KA_ERR_EMPTY_BEAM, _lib.KA_ERR_BAD_LABEL, _lib.KA_ERR_NAN, _lib.KA_ERR_NONFINITE):
            _lib.check(rc, "ctc_best_path_batch")
        return self.status

    def run(self, raise_on_error=True):
        self.enqueue()
        return self.finish(raise_on_error)

    def results(self):
        return list(zip(self.path, self.best_labels, self.best_scores))


def ctc_best_path_device(log_probs, labels, beam_size=1000, max_move=4, verbose=False):
    """Lists of ROCm torch tensors in, list of (best_path, best_labels, best_scores) tensors out.
    One launch for the whole list; nothing leaves the device except 16 B of status per lattice."""
    import torch
    dev = log_probs[0].device
    labels = [x if _is_tensor(x) else torch.as_tensor(np.asarray(x).reshape(-1).astype(np.int32)) for x in labels]
    for lp, lab in zip(log_probs, labels):
        if verbose:
            print(f"Label length: {2 * int(lab.numel()) + 1}")
            print(f"Time length: {int(lp.shape[0])}")
        if lp.shape[0] == 0:
            raise IndexError("list index out of range")
    with torch.cuda.device(dev):
        batch = DeviceBatch(log_probs, labels, beam_size, max_move)
        batch.run()
    return batch.results()


# ------------------------------------------------------------------------------------------
# best path over a caller-given band
# ------------------------------------------------------------------------------------------
def diagonal_band(T, L, beam_size):
    """The reference's band as a table: lo_t = max(0, L t // T - beam_size // 2) (align.py:64), int64 [T]."""
    t = np.arange(int(T), dtype=np.int64)
    return np.maximum(0, np.int64(L) * t // np.int64(T) - np.int64(int(beam_size) // 2))


def anchored_band(T, L, anchors, beam_size):
    """A band of width ``beam_size`` centred on the broken line through ``anchors``: (frame, position) pairs, strictly increasing
    in frame and non-decreasing in position, between the implied (0, 0) and (T, L).  The centre is interpolated with floor
    division between neighbours; lo = clip(centre - beam_size // 2, 0, L - 1).  Without anchors it is ``diagonal_band``."""
    T, L = int(T), int(L)
    pts = [(0, 0)] + [(int(f), int(p)) for f, p in anchors] + [(T, L)]
    for (f0, p0), (f1, p1) in zip(pts[:-1], pts[1:]):
        if f1 <= f0 or p1 < p0:
            raise ValueError("anchors must be strictly increasing in frame within (0, T) and non-decreasing in position within [0, L]")
    lo = np.zeros(T, np.int64)
    for (f0, p0), (f1, p1) in zip(pts[:-1], pts[1:]):
        t = np.arange(f0, f1, dtype=np.int64)
        lo[f0:f1] = np.int64(p0) + np.int64(p1 - p0) * (t - f0) // np.int64(f1 - f0) - np.int64(int(beam_size) // 2)
    return np.clip(lo, 0, L - 1)


def band_around_path(path, L, beam_size):
    """lo_t = clip(path[t] - beam_size // 2, 0, L - 1): the band of a second pass around a first pass's path (monotone because
    paths only move up)."""
    return np.clip(np.asarray(path, dtype=np.int64) - np.int64(int(beam_size) // 2), 0, int(L) - 1)


def band_edge_contact(best_path, band_lo, beam_size, L, max_move=4):
    """Frames at which ``best_path`` lies within ``max_move - 1`` positions of the band's low edge lo_t (where lo_t > 0) or of
    its high edge hi_t - 1 (where hi_t < L): where the band, not the log-probs, may have decided the path.  An edge clamped to
    the lattice's own end does not count.  Works on any table, ``diagonal_band`` included."""
    p = np.asarray(best_path, dtype=np.int64)
    lo = np.asarray(band_lo, dtype=np.int64)
    hi = np.minimum(lo + np.int64(int(beam_size)), np.int64(int(L)))
    reach = int(max_move) - 1
    low = (lo > 0) & (p - lo <= reach)
    high = (hi < int(L)) & (hi - 1 - p <= reach)
    return np.nonzero(low | high)[0]


def ctc_best_path_banded_batch(log_probs_list, labels_list, band_lo_list, beam_size=1000, max_move=4, device=None,
                               return_status=False, outputs=None):
    """``ctc_best_path_batch`` over caller-given bands: frame t of lattice i searches positions [band_lo[t], min(band_lo[t] +
    beam_size, 2S+1)).  Host NumPy buffers in and out.  A table must be non-decreasing with entries in [0, 2S+1) (status -2,
    ValueError); a band that loses every live state raises ValueError like the reference's empty beam (status -1).  With
    ``return_status`` failures do not raise and (results, statuses, totals) are returned; a failed lattice's arrays are not written.
    ``outputs``: (paths, labels, scores), lists of contiguous int32 / int32 / float32 arrays of T_i elements to write into."""
    lat = _host_lattices(log_probs_list, labels_list, band_lo_list, "band_lo", device)
    if lat is None:
        return ([], [], []) if return_status else []
    return _best_path_banded(lat, band_lo_list, beam_size, max_move, outputs, return_status)


def ctc_best_path_banded_device(log_probs, labels, band_lo, beam_size=1000, max_move=4, return_status=False, outputs=None):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V], integer labels [S_i], integer tables [T_i]; labels and tables
    may also be NumPy arrays), list of (best_path, best_labels, best_scores) tensors out.  One launch for the whole list; a table
    built on the device from a device-resident path needs no round trip.  ``outputs``: (paths, labels, scores), lists of contiguous
    int32 / int32 / float32 tensors of T_i elements on the same device to write into."""
    lat = _device_lattices(log_probs, labels, band_lo, "band_lo")
    return _best_path_banded(lat, band_lo, beam_size, max_move, outputs, return_status)


def ctc_best_path_banded(log_probs, labels, band_lo, beam_size=1000, max_move=4):
    """``ctc_best_path`` over a caller-given band: frame t searches positions [band_lo[t], min(band_lo[t] + beam_size, 2S+1))
    instead of the reference's diagonal (align.py:64-65); everything else is the reference's.  ``band_lo`` [T] integers,
    non-decreasing, in [0, 2S+1): ``diagonal_band`` (the reference's, and then the result is ``ctc_best_path``'s bit for bit),
    ``anchored_band``, ``band_around_path`` or any table of the caller's.  NumPy in -> NumPy out; ROCm torch tensors in ->
    torch tensors out.  Raises ValueError where ``ctc_best_path`` does (no live state in the last frame) and for an invalid
    table; ``band_edge_contact`` says whether the path it returns leant on the band."""
    if _is_tensor(log_probs):
        return ctc_best_path_banded_device([log_probs], [labels], [band_lo], beam_size, max_move)[0]
    lp = np.asarray(log_probs)
    if lp.ndim != 2:
        raise ValueError("log_probs must be [T, V]")
    return ctc_best_path_banded_batch([lp], [labels], [band_lo], beam_size, max_move)[0]


# ------------------------------------------------------------------------------------------
# best path over a self-steering band
# ------------------------------------------------------------------------------------------
def ctc_best_path_tracking_batch(log_probs_list, labels_list, beam_size=1000, max_move=4, period=16, end_rule="highest", device=None,
                                 return_status=False, outputs=None):
    """``ctc_best_path_tracking`` for a list of lattices in one call.  Host NumPy buffers in and out: a list of (best_path,
    best_labels, best_scores, band_lo).  With ``return_status`` failures of single lattices do not raise and (results, statuses,
    totals) are returned; a failed lattice's path arrays are not written.  ``outputs``: (paths, labels, scores, tables), lists
    of contiguous int32 / int32 / float32 / int32 arrays of T_i elements to write into."""
    lat = _host_lattices(log_probs_list, labels_list, None, None, device)
    if lat is None:
        return ([], [], []) if return_status else []
    return _best_path_tracking(lat, beam_size, max_move, period, end_rule, outputs, return_status)


def ctc_best_path_tracking_device(log_probs, labels, beam_size=1000, max_move=4, period=16, end_rule="highest", return_status=False,
                                  outputs=None):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V], integer labels [S_i], which may also be NumPy arrays), list of
    (best_path, best_labels, best_scores, band_lo) tensors out.  One launch for the whole list; the tables stay on the device
    for the banded posterior calls (``band_lo=``).  ``outputs``: (paths, labels, scores, tables), lists of contiguous int32 /
    int32 / float32 / int32 tensors of T_i elements on the same device to write into."""
    lat = _device_lattices(log_probs, labels, None, None)
    return _best_path_tracking(lat, beam_size, max_move, period, end_rule, outputs, return_status)


def ctc_best_path_tracking(log_probs, labels, beam_size=1000, max_move=4, period=16, end_rule="highest"):
    """``ctc_best_path_banded`` with a band that steers itself: every ``period`` frames (a multiple of 4 in [4, 65536]) the band
    is re-centred on the best-scoring live cell of two frames before, lo_t = min(max(lo_{t-1}, c - beam_size // 2), 2S), and
    never moves back.  It waits while the reader pauses and follows as fast as they read, where the reference's diagonal assumes
    a uniform rate.  Returns (best_path, best_labels, best_scores, band_lo): ``band_lo`` is the table that was walked, valid for
    ``ctc_best_path_banded`` (which returns the same path under it) and for every posterior call's ``band_lo=``.
    ``end_rule``: "highest" ends the path at the highest live position of the last frame (the reference's rule), "best" at the
    best-scoring one (audio that ends before the text does).  The path is kept while period x (positions advanced per frame) <
    beam_size / 2; the steering is greedy, and ``band_edge_contact`` on the returned table shows where the band may have
    decided the path.  NumPy in -> NumPy out; ROCm torch tensors in -> torch tensors out."""
    if _is_tensor(log_probs):
        return ctc_best_path_tracking_device([log_probs], [labels], beam_size, max_move, period, end_rule)[0]
    lp = np.asarray(log_probs)
    if lp.ndim != 2:
        raise ValueError("log_probs must be [T, V]")
    return ctc_best_path_tracking_batch([lp], [labels], beam_size, max_move, period, end_rule)[0]


# ------------------------------------------------------------------------------------------
# resumable best path: the banded best path under the caller's boundary conditions
# ------------------------------------------------------------------------------------------
END_CELLS = {"highest": -1, "best": -2}


def free_start_scores(L, lo=0, hi=None):
    """A start row for ``ctc_best_path_resume`` that lets the path begin anywhere in [lo, hi) at no cost: float32 [L], 0.0 there
    and NaN (a dead cell) elsewhere.  ``hi`` None is L."""
    row = np.full(int(L), np.nan, np.float32)
    row[int(lo):int(L) if hi is None else int(hi)] = 0.0
    return row


def _score_rows(lat, rows):
    """The start rows of a resumed call as the call wants them: per lattice None or float32 [2S+1] where the lattices are."""
    if rows is None:
        return [None] * lat.n
    if len(rows) != lat.n:
        raise ValueError("init_scores must hold one row (or None) per lattice")
    out = []
    for r, S in zip(rows, lat.S):
        if r is not None:
            if lat.form == "batch":
                r = np.ascontiguousarray(np.asarray(r.detach().cpu() if _is_tensor(r) else r, dtype=np.float32).reshape(-1))
            else:
                import torch
                r = (r if _is_tensor(r) else torch.as_tensor(np.asarray(r, dtype=np.float32))).reshape(-1)
                r = r.to(device=lat.dev, dtype=torch.float32).contiguous()
            if r.shape[0] != 2 * S + 1:
                raise ValueError("a start row must have 2S+1 entries")
        out.append(r)
    return out


def _end_cells(lat, end):
    """The ends of a resumed call: one value for all lattices or one per lattice, rule names or positions -> int32 [n]."""
    ends = [end] * lat.n if isinstance(end, (str, int, np.integer)) else list(end)
    if len(ends) != lat.n:
        raise ValueError("end must be one value or one per lattice")
    return np.array([END_CELLS[x] if isinstance(x, str) else int(x) for x in ends], np.int32)


def _best_path_resume(lat, band_lo, init_scores, end, beam_size, max_move, final_scores, return_status, determined=False):
    tables = _band_tables(lat, band_lo)         # (held until the call has returned, like the rows: the addresses below are theirs)
    rows = _score_rows(lat, init_scores)
    ends = _end_cells(lat, end)
    last = [lat.empty((2 * S + 1,), np.float32) for S in lat.S] if final_scores else None
    entry = np.full(lat.n, -1, np.int32)
    p_band, _k1 = _ptr_array([lat.ptr(x) for x in tables])
    p_init, _k2 = _ptr_array([None if x is None else lat.ptr(x) for x in rows])
    p_last, _k3 = _ptr_array([lat.ptr(x) for x in last]) if final_scores else (None, None)
    det = np.full(lat.n, -1, np.int32)           # (the determined call: one more cell per lattice, one more entry per result)
    out = _run_best_path(lat, "_determined" if determined else "_resume", beam_size, max_move, (p_band, p_init, ends.ctypes.data), None,
                         return_status, (p_last, entry.ctypes.data) + ((det.ctypes.data,) if determined else ()))
    results = out[0] if return_status else out
    results = [r + (int(entry[i]), last[i] if final_scores else None) + ((int(det[i]),) if determined else ()) for i, r in enumerate(results)]
    return (results,) + tuple(out[1:]) if return_status else results


def ctc_best_path_resume_batch(log_probs_list, labels_list, band_lo_list, init_scores_list=None, end="highest", beam_size=1000,
                               max_move=4, device=None, return_status=False, final_scores=True):
    """``ctc_best_path_resume`` for a list of lattices in one call.  Host NumPy buffers in and out: a list of (best_path,
    best_labels, best_scores, entry, final_scores).  ``init_scores_list``: None, or per lattice None or a row; ``end``: one value
    for all or one per lattice.  With ``return_status`` failures of single lattices do not raise and (results, statuses, totals)
    are returned; a failed lattice's path arrays are not written, its entry is -1 and its last row is written (all NaN unless
    its forward pass ran).  ``final_scores=False`` asks for no last rows (None in the results)."""
    lat = _host_lattices(log_probs_list, labels_list, band_lo_list, "band_lo", device)
    if lat is None:
        return ([], [], []) if return_status else []
    return _best_path_resume(lat, band_lo_list, init_scores_list, end, beam_size, max_move, final_scores, return_status)


def ctc_best_path_resume_device(log_probs, labels, band_lo, init_scores=None, end="highest", beam_size=1000, max_move=4,
                                return_status=False, final_scores=True):
    """``ctc_best_path_resume_batch`` on lists of ROCm torch tensors (labels, tables and rows may also be NumPy arrays): paths,
    labels, scores and last rows stay on the device, so a chunk resumes from the row the chunk before it left there; the entries
    are Python integers."""
    lat = _device_lattices(log_probs, labels, band_lo, "band_lo")
    return _best_path_resume(lat, band_lo, init_scores, end, beam_size, max_move, final_scores, return_status)


def ctc_best_path_resume(log_probs, labels, band_lo, init_scores=None, end="highest", beam_size=1000, max_move=4):
    """``ctc_best_path_banded`` under the caller's boundary conditions: started from a score row, ended at a cell or by a rule,
    returning the row after its last frame and the cell of the start row its path left from.

    ``init_scores`` [2S+1] float32: the scores before frame 0; NaN is a dead cell, -inf a live cell of score -inf, +inf a
    ValueError.  No band applies to the row (only the cells frame 0 can reach matter).  None is the reference's start, position
    0 at score 0.0; ``free_start_scores`` lets the path begin anywhere (a recording that holds a part of its text).
    ``end``: "highest" ends the path at the highest live position of the last frame (the reference's rule), "best" at the
    best-scoring one (the first maximum in ascending position), an integer at that position (ValueError if it is not live).
    Returns (best_path, best_labels, best_scores, entry, final_scores): ``entry`` is the cell of the start row the path left
    from (0 for None), ``final_scores`` [2S+1] the live cells' scores after the last frame and NaN elsewhere, which is the
    ``init_scores`` of a call on the frames that follow.  With None, "highest" every array is ``ctc_best_path_banded``'s bit for
    bit, and a lattice cut into chunks that resume from each other (``ctc_best_path_chunked``) gives the uncut call's bits.
    NumPy in -> NumPy out; ROCm torch tensors in -> torch tensors out."""
    if _is_tensor(log_probs):
        return ctc_best_path_resume_device([log_probs], [labels], [band_lo], [init_scores], end, beam_size, max_move)[0]
    lp = np.asarray(log_probs)
    if lp.ndim != 2:
        raise ValueError("log_probs must be [T, V]")
    return ctc_best_path_resume_batch([lp], [labels], [band_lo], [init_scores], end, beam_size, max_move)[0]


def ctc_best_path_chunked(log_probs, labels, band_lo, chunk_frames, beam_size=1000, max_move=4):
    """``ctc_best_path_banded`` in chunks of ``chunk_frames`` frames: the same (best_path, best_labels, best_scores), bit for bit.
    A forward sweep runs the chunks in order, each from the row the one before it ended with, and keeps every chunk's start
    row; the last chunk's path is taken at once; the earlier chunks are then run again, last to first, from their kept rows
    with ``end`` = the next chunk's ``entry``.  Cost: (2 - 1/chunks) forward passes instead of one.  What it buys: the kernels
    hold move codes for ``chunk_frames`` frames instead of T (256 bytes per frame in the one-wavefront form), so a long
    recording's workspace is bounded by the chunk, and the first sweep can run while the log-probs still arrive."""
    chunk_frames = int(chunk_frames)
    if chunk_frames < 1:
        raise ValueError("chunk_frames must be at least 1")
    tensor = _is_tensor(log_probs)
    if not tensor:
        log_probs = np.asarray(log_probs)
    if log_probs.ndim != 2:
        raise ValueError("log_probs must be [T, V]")
    T = int(log_probs.shape[0])
    if not tensor or not _is_tensor(band_lo):
        band_lo = np.asarray(band_lo.detach().cpu() if _is_tensor(band_lo) else band_lo).reshape(-1)
    if band_lo.shape[0] != T:
        raise ValueError("a band table must have one entry per frame")
    cuts = list(range(0, T, chunk_frames))
    if not cuts:
        raise IndexError("list index out of range")

    def run(a, init, end):
        b = min(a + chunk_frames, T)
        return ctc_best_path_resume(log_probs[a:b], labels, band_lo[a:b], init, end, beam_size, max_move)

    starts, init = [], None
    for a in cuts[:-1]:
        starts.append(init)
        init = run(a, init, "highest")[4]
    parts = [run(cuts[-1], init, "highest")]
    for a, init in zip(reversed(cuts[:-1]), reversed(starts)):
        parts.append(run(a, init, parts[-1][3]))
    parts.reverse()
    if tensor:
        import torch
        return tuple(torch.cat([p[i] for p in parts]) for i in range(3))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


# ------------------------------------------------------------------------------------------
# resumable tracking best path: the self-steering band under the caller's boundary conditions
# ------------------------------------------------------------------------------------------
def _best_path_tracking_resume(lat, first_lo, init_scores, end, beam_size, max_move, period, final_scores, return_status, determined=False):
    rows = _score_rows(lat, init_scores)        # (held until the call has returned: the addresses below are theirs)
    ends = _end_cells(lat, end)
    first = [first_lo] * lat.n if isinstance(first_lo, (int, np.integer)) else list(first_lo)
    if len(first) != lat.n:
        raise ValueError("first_lo must be one value or one per lattice")
    first = np.array([int(x) for x in first], np.int32)
    last = [lat.empty((2 * S + 1,), np.float32) for S in lat.S] if final_scores else None
    entry = np.full(lat.n, -1, np.int32)
    next_lo = np.full(lat.n, -1, np.int32)
    p_init, _k1 = _ptr_array([None if x is None else lat.ptr(x) for x in rows])
    p_last, _k2 = _ptr_array([lat.ptr(x) for x in last]) if final_scores else (None, None)
    det = np.full(lat.n, -1, np.int32)           # (the determined call: one more cell per lattice, one more entry per result)
    out = _run_best_path(lat, "_tracking_determined" if determined else "_tracking_resume", beam_size, max_move,
                         (int(period), first.ctypes.data, p_init, ends.ctypes.data), None, return_status,
                         (p_last, entry.ctypes.data, next_lo.ctypes.data) + ((det.ctypes.data,) if determined else ()))
    results = out[0] if return_status else out
    results = [r + (int(entry[i]), last[i] if final_scores else None, int(next_lo[i])) + ((int(det[i]),) if determined else ())
               for i, r in enumerate(results)]
    return (results,) + tuple(out[1:]) if return_status else results


def ctc_best_path_tracking_resume_batch(log_probs_list, labels_list, first_lo=0, init_scores_list=None, end="highest", beam_size=1000,
                                        max_move=4, period=16, device=None, return_status=False, final_scores=True):
    """``ctc_best_path_tracking_resume`` for a list of lattices in one call.  Host NumPy buffers in and out: a list of (best_path,
    best_labels, best_scores, band_lo, entry, final_scores, next_lo).  ``first_lo`` and ``end``: one value for all or one per
    lattice; ``init_scores_list``: None, or per lattice None or a row.  With ``return_status`` failures of single lattices do not
    raise and (results, statuses, totals) are returned; a failed lattice's path arrays are not written, its entry is -1, its last
    row is written (all NaN unless its forward pass ran) and its next_lo is -1 unless its forward pass ran (status -1: then its
    table is written too).  ``final_scores=False`` asks for no last rows (None in the results)."""
    lat = _host_lattices(log_probs_list, labels_list, None, None, device)
    if lat is None:
        return ([], [], []) if return_status else []
    return _best_path_tracking_resume(lat, first_lo, init_scores_list, end, beam_size, max_move, period, final_scores, return_status)


def ctc_best_path_tracking_resume_device(log_probs, labels, first_lo=0, init_scores=None, end="highest", beam_size=1000, max_move=4,
                                         period=16, return_status=False, final_scores=True):
    """``ctc_best_path_tracking_resume_batch`` on lists of ROCm torch tensors (labels and rows may also be NumPy arrays): paths,
    labels, scores, tables and last rows stay on the device; the entries and next_lo are Python integers."""
    lat = _device_lattices(log_probs, labels, None, None)
    return _best_path_tracking_resume(lat, first_lo, init_scores, end, beam_size, max_move, period, final_scores, return_status)


def ctc_best_path_tracking_resume(log_probs, labels, first_lo=0, init_scores=None, end="highest", beam_size=1000, max_move=4, period=16):
    """``ctc_best_path_tracking`` under ``ctc_best_path_resume``'s boundary conditions, so that the self-steering band crosses a
    cut: started from the score row ``init_scores`` with the band of frame 0 at ``first_lo``, ended by ``end`` ("highest", "best"
    or a position), returning (best_path, best_labels, best_scores, band_lo, entry, final_scores, next_lo).  ``next_lo`` is the
    low end the frame behind the last would get: with ``final_scores`` it is what a call on the frames that follow starts from
    (``first_lo=``, ``init_scores=``), and if this chunk's length is a multiple of ``period`` that call continues the uncut one bit
    for bit (``ctc_best_path_tracking_chunked``).  The retargets fall on the chunk's own frames t > 0 with t % period == 0; frame 0
    never retargets.  With 0, None every array is ``ctc_best_path_tracking``'s.  Unlike that call this one can raise ValueError
    for an empty beam: a start row out of the first band's reach, or an end cell that is not live.
    NumPy in -> NumPy out; ROCm torch tensors in -> torch tensors out."""
    if _is_tensor(log_probs):
        return ctc_best_path_tracking_resume_device([log_probs], [labels], first_lo, [init_scores], end, beam_size, max_move, period)[0]
    lp = np.asarray(log_probs)
    if lp.ndim != 2:
        raise ValueError("log_probs must be [T, V]")
    return ctc_best_path_tracking_resume_batch([lp], [labels], first_lo, [init_scores], end, beam_size, max_move, period)[0]


def ctc_best_path_tracking_chunked(log_probs, labels, chunk_frames, beam_size=1000, max_move=4, period=16, end_rule="highest"):
    """``ctc_best_path_tracking`` in chunks of ``chunk_frames`` frames, a positive multiple of ``period`` (ValueError otherwise: a
    chunk's retargets fall on its own multiples of the period, so any other cut steers another band): the same (best_path,
    best_labels, best_scores, band_lo), bit for bit.  A forward sweep of ``ctc_best_path_tracking_resume`` runs the chunks in
    order, each from the row and the low end the one before it ended with, and keeps every chunk's start row and table; the last
    chunk's path is taken at once; the earlier chunks are then run again, last to first, with ``ctc_best_path_resume`` over
    their kept tables and ``end`` = the next chunk's ``entry``.  Cost: (2 - 1/chunks) forward passes instead of one.  What it
    buys: move codes for ``chunk_frames`` frames instead of T, with no table known in advance."""
    chunk_frames, period = int(chunk_frames), int(period)
    if period < 4 or period % 4 != 0:
        raise ValueError("period must be a multiple of 4 in [4, 65536]")
    if chunk_frames < 1 or chunk_frames % period != 0:
        raise ValueError("chunk_frames must be a positive multiple of period")
    tensor = _is_tensor(log_probs)
    if not tensor:
        log_probs = np.asarray(log_probs)
    if log_probs.ndim != 2:
        raise ValueError("log_probs must be [T, V]")
    T = int(log_probs.shape[0])
    cuts = list(range(0, T, chunk_frames))
    if not cuts:
        raise IndexError("list index out of range")
    end = END_RULES[end_rule] if isinstance(end_rule, str) else int(end_rule)
    end = {0: "highest", 1: "best"}[end]

    starts, tables, init, lo = [], [], None, 0
    for a in cuts[:-1]:
        starts.append(init)
        r = ctc_best_path_tracking_resume(log_probs[a:a + chunk_frames], labels, lo, init, "highest", beam_size, max_move, period)
        tables.append(r[3])
        init, lo = r[5], r[6]
    last = ctc_best_path_tracking_resume(log_probs[cuts[-1]:], labels, lo, init, end, beam_size, max_move, period)
    parts, entry = [last[:4]], last[4]
    for a, init, table in zip(reversed(cuts[:-1]), reversed(starts), reversed(tables)):
        r = ctc_best_path_resume(log_probs[a:a + chunk_frames], labels, table, init, entry, beam_size, max_move)
        parts.append(r[:3] + (table,))
        entry = r[3]
    parts.reverse()
    if tensor:
        import torch
        return tuple(torch.cat([p[i] for p in parts]) for i in range(4))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


# ------------------------------------------------------------------------------------------
# determined prefixes: how much of a resumed chunk's path is final, and the aligner that commits frames while it is fed
# ------------------------------------------------------------------------------------------
def ctc_best_path_determined_batch(log_probs_list, labels_list, band_lo_list, init_scores_list=None, end="highest", beam_size=1000,
                                   max_move=4, device=None, return_status=False, final_scores=True):
    """``ctc_best_path_determined`` for a list of lattices in one call: ``ctc_best_path_resume_batch``'s arguments and results,
    each result with ``determined`` appended.  A failed lattice's ``determined`` is -1 unless its forward pass ran to its end
    with live cells (a given end that is dead)."""
    lat = _host_lattices(log_probs_list, labels_list, band_lo_list, "band_lo", device)
    if lat is None:
        return ([], [], []) if return_status else []
    return _best_path_resume(lat, band_lo_list, init_scores_list, end, beam_size, max_move, final_scores, return_status, True)


def ctc_best_path_determined_device(log_probs, labels, band_lo, init_scores=None, end="highest", beam_size=1000, max_move=4,
                                    return_status=False, final_scores=True):
    """``ctc_best_path_determined_batch`` on lists of ROCm torch tensors, as ``ctc_best_path_resume_device``; ``determined`` is a
    Python integer."""
    lat = _device_lattices(log_probs, labels, band_lo, "band_lo")
    return _best_path_resume(lat, band_lo, init_scores, end, beam_size, max_move, final_scores, return_status, True)


def ctc_best_path_determined(log_probs, labels, band_lo, init_scores=None, end="highest", beam_size=1000, max_move=4):
    """``ctc_best_path_resume`` that also says how much of its path is final: (best_path, best_labels, best_scores, entry,
    final_scores, determined).  The live cells after the last frame are all followed back along their chosen moves until they
    meet in one cell (the reference's flush_determined_path, kokoro_align/align.py:21-40); ``determined`` is the number of
    frames before that: frames [0, determined) are the same whichever live cell the path later ends at and whatever audio
    follows.  0: no frame of this chunk is final, but every line leaves the start row at ``entry``, which closes the chunk
    before this one.  -1: the lines reach more than one start cell, or no cell is live.  It depends on the live cells, not on
    ``end``.  Every other value is ``ctc_best_path_resume``'s, bit for bit."""
    if _is_tensor(log_probs):
        return ctc_best_path_determined_device([log_probs], [labels], [band_lo], [init_scores], end, beam_size, max_move)[0]
    lp = np.asarray(log_probs)
    if lp.ndim != 2:
        raise ValueError("log_probs must be [T, V]")
    return ctc_best_path_determined_batch([lp], [labels], [band_lo], [init_scores], end, beam_size, max_move)[0]


def ctc_best_path_tracking_determined_batch(log_probs_list, labels_list, first_lo=0, init_scores_list=None, end="highest", beam_size=1000,
                                            max_move=4, period=16, device=None, return_status=False, final_scores=True):
    """``ctc_best_path_tracking_determined`` for a list of lattices in one call: ``ctc_best_path_tracking_resume_batch``'s
    arguments and results, each result with ``determined`` appended."""
    lat = _host_lattices(log_probs_list, labels_list, None, None, device)
    if lat is None:
        return ([], [], []) if return_status else []
    return _best_path_tracking_resume(lat, first_lo, init_scores_list, end, beam_size, max_move, period, final_scores, return_status, True)


def ctc_best_path_tracking_determined_device(log_probs, labels, first_lo=0, init_scores=None, end="highest", beam_size=1000, max_move=4,
                                             period=16, return_status=False, final_scores=True):
    """``ctc_best_path_tracking_determined_batch`` on lists of ROCm torch tensors, as ``ctc_best_path_tracking_resume_device``;
    ``determined`` is a Python integer."""
    lat = _device_lattices(log_probs, labels, None, None)
    return _best_path_tracking_resume(lat, first_lo, init_scores, end, beam_size, max_move, period, final_scores, return_status, True)


def ctc_best_path_tracking_determined(log_probs, labels, first_lo=0, init_scores=None, end="highest", beam_size=1000, max_move=4, period=16):
    """``ctc_best_path_tracking_resume`` that also says how much of its path is final: (best_path, best_labels, best_scores,
    band_lo, entry, final_scores, next_lo, determined), ``determined`` as in ``ctc_best_path_determined``.  Every other value is
    ``ctc_best_path_tracking_resume``'s, bit for bit."""
    if _is_tensor(log_probs):
        return ctc_best_path_tracking_determined_device([log_probs], [labels], first_lo, [init_scores], end, beam_size, max_move, period)[0]
    lp = np.asarray(log_probs)
    if lp.ndim != 2:
        raise ValueError("log_probs must be [T, V]")
    return ctc_best_path_tracking_determined_batch([lp], [labels], first_lo, [init_scores], end, beam_size, max_move, period)[0]


class StreamingAligner:
    """The self-steering band fed chunk by chunk, committing frames as soon as they are final.

    ``push(log_probs_chunk)`` takes the next ``[frames, V]`` log-prob rows (NumPy, or ROCm torch tensors throughout) and returns
    the frames that have become final since the last call as (best_path, best_labels, best_scores, band_lo) arrays, possibly
    empty; ``finish()`` returns the rest under the aligner's ``end`` rule ("highest" or "best").  The commits concatenated are
    ``ctc_best_path_tracking`` of the whole input, bit for bit, and a committed frame never changes.  A chunk's length must be
    a multiple of ``period``; only the last may be ragged, and a push after a ragged one raises ValueError.

    Per push the chunk runs once through ``ctc_best_path_tracking_determined`` from the row and low end the chunk before it
    left.  If its lines merge (``determined >= 0``), every pending earlier chunk is closed, newest first, by
    ``ctc_best_path_resume`` over its own table with ``end`` = the entry of the chunk after it, and those frames are emitted
    followed by this chunk's determined frames; the chunk stays pending from there on.  At most two forward passes per chunk,
    as ``ctc_best_path_tracking_chunked``; the pending chunks are the only state held.  (A separate class from ``streams.py``'s
    ``StreamedAligner``, which runs whole lattices on several streams.)

    ``confidence=True``: ``push()`` and ``finish()`` return a fifth array, float32, one value per committed frame: the posterior
    of the committed state given all audio pushed so far, under the tracked band (``ctc_posteriors_resume``).  Every push runs its
    chunk forward-only from the alpha row the chunk before it left.  On a commit the pending chunks are visited newest first: the
    newest ends anywhere (``free_end_scores``; at ``finish()`` it ends at the final path's last state), every older one at the
    ``beta_out`` of the chunk after it; only the newly committed frames' values are returned.  Cost: at most two full
    forward-backward passes and one forward-only pass per chunk, and one more row of 2S+1 doubles per pending chunk.  With
    ``False`` nothing changes.

    ``confidence="margin"``: the fifth array is float64, the best-path margin of every committed state (``ctc_margins_resume``,
    ``unit="state"``): how much the best alignment of all audio pushed so far would lose if it had to be at another state in
    that frame, >= 0 for a committed frame, +inf where no other state has a path.  The same visits as ``confidence=True`` with
    max-plus passes in its place (no exp or log; a third of the cost), and exact: at every commit the values are those of the
    whole prefix under the concatenated table with a free end, bit for bit, and at ``finish()`` those of
    ``ctc_path_margins(..., band_lo=table)`` of the whole input.  Any other value of ``confidence`` raises ValueError."""

    def __init__(self, labels, beam_size=1000, max_move=4, period=16, end="highest", confidence=False):
        self.labels = labels
        self.beam_size, self.max_move, self.period = int(beam_size), int(max_move), int(period)
        if self.period < 4 or self.period % 4 != 0:
            raise ValueError("period must be a multiple of 4 in [4, 65536]")
        if end not in END_CELLS:
            raise ValueError('end must be "highest" or "best"')
        self.end = end
        if confidence != "margin" if isinstance(confidence, str) else confidence not in (True, False):
            raise ValueError('confidence must be False, True or "margin"')
        self.confidence = "margin" if isinstance(confidence, str) else bool(confidence)
        self._row, self._lo = None, 0      # what the next chunk starts from
        self._alpha = None                 # confidence: ln alpha of the last pushed frame, the next chunk's start row
        self._pending = []                 # oldest first: dicts of a chunk's rows, start row, table, path parts, emitted frames
        self._ragged = False
        self._finished = False
        self.frames_pushed = 0
        self.frames_committed = 0

    @staticmethod
    def _cat(parts):
        if _is_tensor(parts[0][0]):
            import torch
            return tuple(torch.cat([p[i] for p in parts]) for i in range(4))
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))

    def _close_pending(self, entry):
        """Close every pending chunk but the newest, newest first, from the entry of the chunk after it."""
        for c in reversed(self._pending[:-1]):
            r = ctc_best_path_resume(c["lp"], self.labels, c["table"], c["init"], entry, self.beam_size, self.max_move)
            c["out"] = r[:3] + (c["table"],)
            entry = r[3]

    def _emit(self, upto_last):
        """The not-yet-emitted frames of the closed chunks in order, then frames [emitted, upto_last) of the newest chunk."""
        parts = [tuple(x[c["emitted"]:] for x in c["out"]) for c in self._pending[:-1]]
        last = self._pending[-1]
        parts.append(tuple(x[last["emitted"]:upto_last] for x in last["out"]))
        last["emitted"] = max(last["emitted"], upto_last)
        self._pending = [last]
        out = self._cat(parts)
        self.frames_committed += int(out[0].shape[0])
        return out

    def _confidence(self, upto_last, terminal=None):
        """The posterior of the committed state at every frame ``_emit(upto_last)`` is about to return: the pending chunks newest
        first, the newest to a free end (or ``terminal``), each older one to the row the chunk after it handed back."""
        from .posteriors import ctc_margins_resume, ctc_posteriors_resume, free_end_scores
        L = 2 * int(self._pending[-1]["S"]) + 1
        end = free_end_scores(L) if terminal is None else int(terminal)
        posts = []
        for k in range(len(self._pending) - 1, -1, -1):
            c = self._pending[k]
            if self.confidence == "margin":     # (the same visit in max-plus: the start row is D, the row handed back E)
                post, _r, _s, _l, _d, end, _z = ctc_margins_resume(c["lp"], self.labels, c["table"], c["out"][0], c["alpha_in"], end, "state",
                                                                   None, "e" if k > 0 else False, self.beam_size, self.max_move)
            else:
                _o, post, _a, end, _z = ctc_posteriors_resume(c["lp"], self.labels, c["table"], c["alpha_in"], end, c["out"][0], False,
                                                              "beta" if k > 0 else False, self.beam_size, self.max_move)
            posts.append(post[c["emitted"]:upto_last] if k == len(self._pending) - 1 else post[c["emitted"]:])
        posts.reverse()
        if _is_tensor(posts[0]):
            import torch
            return torch.cat(posts)
        return np.concatenate(posts)

    def _forward(self, lp, table):
        """confidence: the chunk forward-only from the kept alpha row; what it adds to the chunk's pending entry"""
        from .posteriors import ctc_margins_resume, ctc_posteriors_resume, free_end_scores
        S = int(self.labels.shape[0]) if _is_tensor(self.labels) else int(np.asarray(self.labels).reshape(-1).shape[0])
        alpha_in = self._alpha
        if self.confidence == "margin":
            self._alpha = ctc_margins_resume(lp, self.labels, table, None, alpha_in, free_end_scores(2 * S + 1), "state", None, "d",
                                             self.beam_size, self.max_move)[4]
        else:
            self._alpha = ctc_posteriors_resume(lp, self.labels, table, alpha_in, free_end_scores(2 * S + 1), None, False, "alpha",
                                                self.beam_size, self.max_move)[2]
        return {"alpha_in": alpha_in, "S": S}

    def push(self, log_probs_chunk):
        if self._finished:
            raise ValueError("the aligner is finished")
        if self._ragged:
            raise ValueError("a chunk whose length is no multiple of period must be the last")
        lp = log_probs_chunk if _is_tensor(log_probs_chunk) else np.asarray(log_probs_chunk)
        if lp.ndim != 2 or lp.shape[0] == 0:
            raise ValueError("a chunk must be non-empty [frames, V] log-probs")
        self._ragged = int(lp.shape[0]) % self.period != 0
        r = ctc_best_path_tracking_determined(lp, self.labels, self._lo, self._row, self.end, self.beam_size, self.max_move, self.period)
        path, lab, sc, table, entry, row, next_lo, det = r
        forward = self._forward(lp, table) if self.confidence else {}      # (before the chunk is registered: it may raise)
        self._pending.append({"lp": lp, "init": self._row, "table": table, "out": (path, lab, sc, table), "emitted": 0, "entry": entry, **forward})
        self._row, self._lo = row, next_lo
        self.frames_pushed += int(lp.shape[0])
        if det >= 0:
            self._close_pending(entry)
            conf = (self._confidence(det),) if self.confidence else ()
            return self._emit(det) + conf
        empty = self._pending[-1]["out"]
        conf = ()
        if self.confidence:
            dtype = np.float64 if self.confidence == "margin" else np.float32
            conf = ((sc[:0].double() if dtype is np.float64 else sc[:0]) if _is_tensor(sc) else np.zeros(0, dtype),)
        return tuple(x[:0] for x in empty) + conf

    def finish(self):
        """Close what is pending with the last chunk's own entry and return the remaining frames."""
        if self._finished:
            raise ValueError("the aligner is finished")
        self._finished = True
        if not self._pending:
            raise IndexError("list index out of range")   # (no frame was pushed: ctc_best_path's error for T = 0)
        last = self._pending[-1]
        self._close_pending(last["entry"])
        n = int(last["out"][0].shape[0])
        conf = (self._confidence(n, int(last["out"][0][-1])),) if self.confidence else ()
        out = self._emit(n) + conf
        self._pending = []
        return out


def log_softmax_device(logits, out=None):
    """Mean-subtracted log-softmax of align.py:116-117 on the device (HIP kernel), float32."""
    import torch
    x = logits if logits.dtype == torch.float32 else logits.float()
    if x.stride(1) != 1:
        x = x.contiguous()
    if out is None:
        out = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    lib = _lib.load_library()
    idx = x.device.index if x.device.index is not None else torch.cuda.current_device()
    with torch.cuda.device(x.device):
        rc = lib.ka_log_softmax_f32(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], x.stride(0),
                                    out.stride(0), _stream_ptr(idx))
    _lib.check(rc, "log_softmax_device")
    return out


# ------------------------------------------------------------------------------------------
# file-level wrappers (same file names, npz keys, dtypes and text format as the reference)
# ------------------------------------------------------------------------------------------
def _host_log_softmax(logits):
    """align.py:116-117 verbatim in behaviour: float32 NumPy, mean-subtracted, NOT max-subtracted."""
    centred = logits - np.mean(logits, axis=-1, keepdims=True)
    return centred - np.log(np.sum(np.exp(centred), axis=-1, keepdims=True))


def best_path(input_file, voca_file, output_file, device_softmax=False, track_period=None, track_chunk=None):
    """``*.logits.npz`` + ``*.voca.txt`` -> ``*.best_path.npz`` (reference: align.py:112-124).

    Keys/dtypes of the output: best_path int32, best_labels int32, best_scores float32.
    ``device_softmax=True`` computes the log-softmax with the HIP kernel (1e-6 of the NumPy
    formula) and keeps the log-probs on the device; the default reproduces the reference's
    host NumPy arithmetic bit for bit and hands the DP a host buffer.
    ``track_period``: a period for ``ctc_best_path_tracking`` instead of the reference's diagonal band; the table it walked is
    stored as a fourth key, band_lo int32 (``align`` reads its three keys as before).  None changes nothing.
    ``track_chunk``: with ``track_period``, a chunk length (a multiple of the period) for ``ctc_best_path_tracking_chunked``: the
    same file, bit for bit, from kernels that hold one chunk's move codes.
    """
    from .transcript import read_transcript
    with np.load(input_file) as f:
        logits = f['data']
    labels = read_transcript(voca_file)
    if track_period is not None:
        if device_softmax:
            import torch
            dev = torch.device("cuda", _current_device())
            lp = log_softmax_device(torch.from_numpy(np.ascontiguousarray(logits, np.float32)).to(dev))
        else:
            lp = _host_log_softmax(logits)
        if track_chunk is not None:
            out = ctc_best_path_tracking_chunked(lp, labels, track_chunk, period=track_period)
        else:
            out = ctc_best_path_tracking(lp, labels, period=track_period)
        p, l, s, b = (x.cpu().numpy() if _is_tensor(x) else x for x in out)
        np.savez(output_file, best_path=p, best_labels=l, best_scores=s, band_lo=b)
        return
    if device_softmax:
        import torch
        dev = torch.device("cuda", _current_device())
        lp = log_softmax_device(torch.from_numpy(np.ascontiguousarray(logits, np.float32)).to(dev))
        (p, l, s), = ctc_best_path_device([lp], [labels], verbose=True)
        p, l, s = p.cpu().numpy(), l.cpu().numpy(), s.cpu().numpy()
    else:
        p, l, s = ctc_best_path(_host_log_softmax(logits), labels)
    np.savez(output_file, best_path=p, best_labels=l, best_scores=s)


def align(best_path_file, mfcc_file, voca_file, align_file, remove_wordsep):
    """Best path -> one line per silence-delimited audio segment (reference: align.py:127-169).

    Line format: audio_end|text|voca|decoded|non_blanks|non_blanks_score|all_score, floats
    printed as Python repr of float(np.float32 sum).  A partially written file is removed
    on any error, like the reference.
    """
    from .transcript import VocaAligner
    with np.load(best_path_file) as f:
        path = f['best_path'] // 2          # expanded position -> phoneme index (align.py:135)
        best_labels = f['best_labels']
        best_scores = f['best_scores']
    with np.load(mfcc_file) as f:
        seg_ends = f['indices']
    aligner = VocaAligner(voca_file)
    n_phonemes = len(aligner)
    n_frames = len(path)
    try:
        with open(align_file, 'wt') as out:
            for i in range(len(seg_ends)):
                a = seg_ends[i - 1] if i > 0 else 0
                b = seg_ends[i]
                text_start = min(path[a], n_phonemes)
                text_end = min(path[b], n_phonemes) if b < n_frames else n_phonemes
                seg_labels = best_labels[a:b]
                seg_scores = best_scores[a:b]
                voiced = seg_labels != 0
                decoded = merge_repeated(decode_text(seg_labels))
                non_blanks = np.sum(voiced).item()
                non_blanks_score = np.sum(seg_scores[voiced]).item()
                all_score = np.sum(seg_scores).item()
                text, voca = aligner.get_token(text_start, text_end, remove_wordsep=remove_wordsep)
                out.write(f'{b}|{text}|{voca}|{decoded}|{non_blanks}|{non_blanks_score}|{all_score}\n')
    except BaseException:
        os.unlink(align_file)
        raise


def pandas_read_align(files):
    """Read ``*.align.txt`` files into one DataFrame (reference: align.py:172-190)."""
    import pandas as pd
    rows = []
    for file in files:
        prev_end = '0'
        with open(file) as f:
            for line in f:
                fields = line.rstrip().split('|')
                rows.append([prev_end] + fields)
                prev_end = fields[0]
    cols = ['audio_start', 'audio_end', 'text', 'voca', 'decoded', 'non_blanks', 'non_blanks_score', 'all_score']
    df = pd.DataFrame(rows, columns=cols)
    for c in ('audio_start', 'audio_end', 'non_blanks'):
        df[c] = df[c].astype(int)
    for c in ('non_blanks_score', 'all_score'):
        df[c] = df[c].astype(float)
    df['audio_len'] = df['audio_end'] - df['audio_start']
    return df
