"""Drop-in for kokoro_align/align.py: same functions, keyword names, defaults, file formats.

    ctc_best_path(log_probs, labels, beam_size=1000, max_move=4)      <- align.py:43-109
    best_path(input_file, voca_file, output_file)                     <- align.py:112-124
    align(best_path_file, mfcc_file, voca_file, align_file, remove_wordsep)  <- align.py:127-169
    pandas_read_align(files)                                          <- align.py:172-190

The DP + backtrace (the reference's per-frame NumPy loop) run in the HIP library through the C
ABI of include/kokoro_align_amd.h.  NumPy arrays are handed over as host buffers; torch tensors
on a ROCm device are handed over by pointer and the results stay on the device.
"""
import ctypes
import os

import numpy as np

from . import _lib
from .encoder import decode_text, merge_repeated


# ------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------
def _is_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "device")


def _stream_ptr(device_index):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device_index).cuda_stream)


def _ptr_array(ptrs):
    arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)), arr


def _i64_array(vals):
    arr = (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])
    return ctypes.cast(arr, ctypes.POINTER(ctypes.c_int64)), arr


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


def _current_device():
    dev = os.environ.get("KA_DEVICE")
    if dev is not None:
        return int(dev)
    try:
        import torch
        if torch.cuda.is_available():
            return torch.cuda.current_device()
    except ImportError:
        pass
    return 0


def ctc_best_path_batch(log_probs_list, labels_list, beam_size=1000, max_move=4, device=None,
                        return_status=False):
    """Independent lattices (one per audio file) in ONE launch; host NumPy buffers in and out.

    Returns a list of (best_path, best_labels, best_scores); with ``return_status`` also the
    per-lattice status list (0 ok, -1 empty beam = the reference's ValueError) and total scores,
    in which case failures do not raise.
    """
    n = len(log_probs_list)
    assert n == len(labels_list)
    if n == 0:
        return ([], [], []) if return_status else []
    lps = [np.ascontiguousarray(x, dtype=np.float32) for x in log_probs_list]
    labs = [np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int32) for x in labels_list]
    V = lps[0].shape[1]
    for x in lps:
        if x.ndim != 2 or x.shape[1] != V:
            raise ValueError("all log_probs must be [T_i, V] with one V")
        if x.shape[0] == 0:
            raise IndexError("list index out of range")
    Ts = [x.shape[0] for x in lps]
    Ss = [x.shape[0] for x in labs]
    paths = [np.empty(t, np.int32) for t in Ts]
    louts = [np.empty(t, np.int32) for t in Ts]
    souts = [np.empty(t, np.float32) for t in Ts]
    status = np.zeros(n, np.int32)
    total = np.zeros(n, np.float32)
    eng = _lib.default_engine(_current_device() if device is None else device)
    p_lp, _k1 = _ptr_array([x.ctypes.data for x in lps])
    p_lab, _k2 = _ptr_array([x.ctypes.data for x in labs])
    p_path, _k3 = _ptr_array([x.ctypes.data for x in paths])
    p_lout, _k4 = _ptr_array([x.ctypes.data for x in louts])
    p_sout, _k5 = _ptr_array([x.ctypes.data for x in souts])
    p_T, _k6 = _i64_array(Ts)
    p_S, _k7 = _i64_array(Ss)
    p_ld, _k8 = _i64_array([V] * n)
    rc = eng.lib.ka_ctc_best_path_batch_f32(eng.handle, n, p_lp, p_T, V, p_ld, p_lab, p_S, int(beam_size),
                                            int(max_move), p_path, p_lout, p_sout, total.ctypes.data,
                                            status.ctypes.data, _lib.KA_MEM_HOST, None)
    results = list(zip(paths, louts, souts))
    if return_status:
        if rc not in (_lib.KA_OK, _lib.KA_ERR_EMPTY_BEAM, _lib.KA_ERR_BAD_LABEL, _lib.KA_ERR_NAN, _lib.KA_ERR_NONFINITE):
            _lib.check(rc, "ctc_best_path_batch")
        return results, status.tolist(), total
    _lib.check(rc, "ctc_best_path_batch")
    return results


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
# best-path posteriors and lattice log-likelihood (forward-backward over the same band)
# ------------------------------------------------------------------------------------------
_POSTERIOR_LATTICE_STATUSES = (_lib.KA_OK, _lib.KA_ERR_BAD_LABEL, _lib.KA_ERR_NAN, _lib.KA_ERR_NONFINITE, _lib.KA_ERR_BAD_ARGS,
                               _lib.KA_ERR_ZERO_MASS)


def ctc_path_posteriors(log_probs, labels, best_path, beam_size=1000, max_move=4):
    """How sure the model is of a best path, frame by frame: (posteriors float32 [T], log_likelihood float).

    posteriors[t] is the probability, over every path of the band of ``ctc_best_path`` that ends where ``best_path`` ends,
    that frame t sits at ``best_path[t]``; log_likelihood is the log of the total probability of those paths (nats).
    NumPy in -> NumPy out; ROCm torch tensors are handed to ``ctc_path_posteriors_device``.  Raises IndexError for a label
    outside [0, V), ValueError for NaN / +inf log-probs, a path value outside [0, 2S+1) or a terminal no finite path reaches.
    """
    if _is_tensor(log_probs):
        (post, ll), = ctc_path_posteriors_device([log_probs], [labels], [best_path], beam_size, max_move)
        return post, ll
    (post, ll), = ctc_path_posteriors_batch([log_probs], [labels], [best_path], beam_size, max_move)
    return post, ll


def _host_lattices(log_probs_list, labels_list, others, what, paths=False):
    """The input handling of the two ``*_batch`` calls: (log-probs, labels, best paths or None, V) as contiguous NumPy arrays,
    or None for an empty batch.  ``others`` holds one best path (``paths``) or terminal per lattice."""
    n = len(log_probs_list)
    if n != len(labels_list) or n != len(others):
        raise ValueError(f"log_probs, labels and {what} must be lists of one length")
    if n == 0:
        return None
    lps = [np.ascontiguousarray(x, dtype=np.float32) for x in log_probs_list]
    labs = [np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int32) for x in labels_list]
    bps = [np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int32) for x in others] if paths else None
    V = lps[0].shape[1] if lps[0].ndim == 2 else 0
    for i, x in enumerate(lps):
        if x.ndim != 2 or x.shape[1] != V:
            raise ValueError("all log_probs must be [T_i, V] with one V")
        if x.shape[0] == 0:
            raise IndexError("list index out of range")
        if paths and bps[i].shape[0] != x.shape[0]:
            raise ValueError("a best path must have one position per frame")
    return lps, labs, bps, V


def _device_lattices(log_probs, labels, others, what, paths=False):
    """The input handling of the two ``*_device`` calls: (log-probs, labels, best paths or None, V, device, device index) as
    tensors on the first log-prob's device, log-probs float32 with unit column stride, labels and paths int32 contiguous."""
    import torch
    n = len(log_probs)
    if n != len(labels) or n != len(others) or n == 0:
        raise ValueError(f"log_probs, labels and {what} must be non-empty lists of one length")
    dev = log_probs[0].device
    V = int(log_probs[0].shape[1])

    def int32_on_dev(x):
        x = x if _is_tensor(x) else torch.as_tensor(np.asarray(x).reshape(-1).astype(np.int32))
        return x.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()

    lps, labs, bps = [], [], ([] if paths else None)
    for i, (lp, lab) in enumerate(zip(log_probs, labels)):
        if lp.dtype != torch.float32:
            lp = lp.float()
        if lp.dim() != 2 or lp.shape[1] != V:
            raise ValueError("all log_probs must be [T_i, V] tensors with one V")
        if lp.shape[0] == 0:
            raise IndexError("list index out of range")
        if lp.stride(1) != 1:
            lp = lp.contiguous()
        labs.append(int32_on_dev(lab))
        if paths:
            bp = int32_on_dev(others[i])
            if bp.shape[0] != lp.shape[0]:
                raise ValueError("a best path must have one position per frame")
            bps.append(bp)
        lps.append(lp)
    dev_index = dev.index if dev.index is not None else torch.cuda.current_device()
    return lps, labs, bps, V, dev, dev_index


def _run_lattices(eng, fn, name, lp_ptrs, Ts, V, lds, lab_ptrs, Ss, beam_size, max_move, own_args, outs, mem, stream, return_status):
    """One ``ka_ctc_{path,label}_posteriors_batch_f32`` call: the arguments both take around ``own_args`` (the call's own
    pointer arrays), then the results (outs[i], log_likelihood[i]) and the status handling of ``return_status``."""
    n = len(lp_ptrs)
    status = np.zeros(n, np.int32)
    ll = np.zeros(n, np.float64)
    p_lp, _k1 = _ptr_array(lp_ptrs)
    p_lab, _k2 = _ptr_array(lab_ptrs)
    p_T, _k3 = _i64_array(Ts)
    p_S, _k4 = _i64_array(Ss)
    p_ld, _k5 = _i64_array(lds)
    rc = getattr(eng.lib, fn)(eng.handle, n, p_lp, p_T, V, p_ld, p_lab, p_S, int(beam_size), int(max_move), *own_args,
                              ll.ctypes.data, status.ctypes.data, mem, stream)
    results = [(o, float(z)) for o, z in zip(outs, ll)]
    if return_status:
        if rc not in _POSTERIOR_LATTICE_STATUSES:
            _lib.check(rc, name)
        return results, status.tolist()
    _lib.check(rc, name)
    return results


def ctc_path_posteriors_batch(log_probs_list, labels_list, best_path_list, beam_size=1000, max_move=4, device=None,
                              return_status=False):
    """Posteriors of many lattices in ONE launch; host NumPy buffers in and out.

    Returns a list of (posteriors, log_likelihood); with ``return_status`` also the per-lattice status list, in which case
    failures do not raise (their posteriors are NaN, their log-likelihood NaN, or -inf for KA_ERR_ZERO_MASS).
    """
    got = _host_lattices(log_probs_list, labels_list, best_path_list, "best paths", paths=True)
    if got is None:
        return ([], []) if return_status else []
    lps, labs, paths, V = got
    posts = [np.empty(x.shape[0], np.float32) for x in lps]
    eng = _lib.default_engine(_current_device() if device is None else device)
    p_path, _k1 = _ptr_array([x.ctypes.data for x in paths])
    p_post, _k2 = _ptr_array([x.ctypes.data for x in posts])
    return _run_lattices(eng, "ka_ctc_path_posteriors_batch_f32", "ctc_path_posteriors_batch", [x.ctypes.data for x in lps],
                         [x.shape[0] for x in lps], V, [V] * len(lps), [x.ctypes.data for x in labs], [x.shape[0] for x in labs],
                         beam_size, max_move, (p_path, p_post), posts, _lib.KA_MEM_HOST, None, return_status)


def ctc_path_posteriors_device(log_probs, labels, best_paths, beam_size=1000, max_move=4, return_status=False):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V], labels [S_i], best paths [T_i] - e.g. the outputs of
    ``ctc_best_path_device``), list of (posteriors tensor [T_i] on the device, log_likelihood float) out.  One launch on
    torch's current stream."""
    import torch
    lps, labs, paths, V, dev, dev_index = _device_lattices(log_probs, labels, best_paths, "best paths", paths=True)
    posts = [torch.empty(int(x.shape[0]), dtype=torch.float32, device=dev) for x in lps]
    eng = _lib.default_engine(dev_index)
    p_path, _k1 = _ptr_array([x.data_ptr() for x in paths])
    p_post, _k2 = _ptr_array([x.data_ptr() for x in posts])
    with torch.cuda.device(dev):
        return _run_lattices(eng, "ka_ctc_path_posteriors_batch_f32", "ctc_path_posteriors_device", [x.data_ptr() for x in lps],
                             [x.shape[0] for x in lps], V, [x.stride(0) for x in lps], [x.data_ptr() for x in labs],
                             [x.shape[0] for x in labs], beam_size, max_move, (p_path, p_post), posts, _lib.KA_MEM_DEVICE,
                             _stream_ptr(dev_index), return_status)


def segment_confidence(posteriors, seg_ends):
    """Mean and minimum posterior of every segment that ``align()`` writes a line for: frames [a, b) with
    a = seg_ends[i-1] (0 for the first), b = seg_ends[i], clipped to the posteriors' length.  Returns two float64 arrays
    (NaN for a segment without frames)."""
    post = np.asarray(posteriors, dtype=np.float64).reshape(-1)
    ends = np.asarray(seg_ends).reshape(-1)
    mean = np.full(len(ends), np.nan)
    low = np.full(len(ends), np.nan)
    for i in range(len(ends)):
        a = int(ends[i - 1]) if i > 0 else 0
        b = min(int(ends[i]), len(post))
        if b > a:
            mean[i] = post[a:b].mean()
            low[i] = post[a:b].min()
    return mean, low


# ------------------------------------------------------------------------------------------
# label occupancy posteriors and a differentiable lattice log-likelihood (same band, same forward-backward)
# ------------------------------------------------------------------------------------------
def _terminal_of(terminal):
    """An int, or a best path whose last value is the terminal."""
    if _is_tensor(terminal):
        terminal = terminal.detach().reshape(-1)[-1].item() if terminal.dim() > 0 else terminal.item()
    a = np.asarray(terminal)
    return int(a.reshape(-1)[-1]) if a.ndim > 0 else int(a)


def ctc_label_posteriors(log_probs, labels, terminal, beam_size=1000, max_move=4):
    """Per-frame label posteriors of the band's paths that end at ``terminal``: (occ float32 [T, V], log_likelihood float).

    occ[t, v] is the probability that frame t emits label value v (blank = 0), over every path of the band of
    ``ctc_best_path`` that ends at state ``terminal`` (an int, or a best path whose last value is used); each row sums to 1 and
    occ equals d log_likelihood / d log_probs.  log_likelihood is the value ``ctc_path_posteriors`` returns for a path that
    ends there.  NumPy in -> NumPy out; ROCm torch tensors go to ``ctc_label_posteriors_device``.  Raises IndexError for a
    label outside [0, V), ValueError for NaN / +inf log-probs, a terminal outside [0, 2S+1) or one no finite path reaches.
    """
    if _is_tensor(log_probs):
        (occ, ll), = ctc_label_posteriors_device([log_probs], [labels], [terminal], beam_size, max_move)
        return occ, ll
    (occ, ll), = ctc_label_posteriors_batch([log_probs], [labels], [terminal], beam_size, max_move)
    return occ, ll


def ctc_label_posteriors_batch(log_probs_list, labels_list, terminals, beam_size=1000, max_move=4, device=None, return_status=False):
    """Label posteriors of many lattices in ONE launch; host NumPy buffers in and out.

    Returns a list of (occ [T_i, V], log_likelihood); with ``return_status`` also the per-lattice status list, in which case
    failures do not raise (their rows are NaN, their log-likelihood NaN, or -inf for KA_ERR_ZERO_MASS).
    """
    got = _host_lattices(log_probs_list, labels_list, terminals, "terminals")
    if got is None:
        return ([], []) if return_status else []
    lps, labs, _, V = got
    occs = [np.empty((x.shape[0], V), np.float32) for x in lps]
    eng = _lib.default_engine(_current_device() if device is None else device)
    p_occ, _k1 = _ptr_array([x.ctypes.data for x in occs])
    p_ldo, _k2 = _i64_array([V] * len(lps))
    p_term, _k3 = _i64_array([_terminal_of(s) for s in terminals])
    return _run_lattices(eng, "ka_ctc_label_posteriors_batch_f32", "ctc_label_posteriors_batch", [x.ctypes.data for x in lps],
                         [x.shape[0] for x in lps], V, [V] * len(lps), [x.ctypes.data for x in labs], [x.shape[0] for x in labs],
                         beam_size, max_move, (p_term, p_occ, p_ldo), occs, _lib.KA_MEM_HOST, None, return_status)


def ctc_label_posteriors_device(log_probs, labels, terminals, beam_size=1000, max_move=4, out=None, return_status=False):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V] with unit column stride, labels [S_i]) and terminals (ints
    or best paths), list of (occ tensor [T_i, V] on the device, log_likelihood float) out.  ``out``: optional list of float32
    [T_i, V] tensors with unit column stride to write into (views into wider tensors keep their other columns).  One launch
    on torch's current stream."""
    import torch
    lps, labs, _, V, dev, dev_index = _device_lattices(log_probs, labels, terminals, "terminals")
    n = len(lps)
    if out is None:
        out = [torch.empty((int(x.shape[0]), V), dtype=torch.float32, device=dev) for x in lps]
    else:
        if len(out) != n:
            raise ValueError("out must hold one tensor per lattice")
        for o, x in zip(out, lps):
            if o.dtype != torch.float32 or o.dim() != 2 or tuple(o.shape) != (int(x.shape[0]), V) or o.stride(1) != 1 or o.device != dev:
                raise ValueError("out tensors must be float32 [T_i, V] on the input's device with unit column stride")
    eng = _lib.default_engine(dev_index)
    p_occ, _k1 = _ptr_array([x.data_ptr() for x in out])
    p_ldo, _k2 = _i64_array([x.stride(0) for x in out])
    p_term, _k3 = _i64_array([_terminal_of(s) for s in terminals])
    with torch.cuda.device(dev):
        return _run_lattices(eng, "ka_ctc_label_posteriors_batch_f32", "ctc_label_posteriors_device", [x.data_ptr() for x in lps],
                             [x.shape[0] for x in lps], V, [x.stride(0) for x in lps], [x.data_ptr() for x in labs],
                             [x.shape[0] for x in labs], beam_size, max_move, (p_term, p_occ, p_ldo), out, _lib.KA_MEM_DEVICE,
                             _stream_ptr(dev_index), return_status)


def _lattice_ll_function():
    import torch

    class LatticeLogLikelihood(torch.autograd.Function):
        """Z of every lattice (float64 [n]); backward: grad_out[i] * occ_i, the occupancy saved by forward."""

        @staticmethod
        def forward(ctx, labels, terminals, beam_size, max_move, zero_infinity, *lps):
            n = len(lps)
            if lps[0].is_cuda:
                res, st = ctc_label_posteriors_device([x.detach() for x in lps], labels, terminals, beam_size, max_move,
                                                      return_status=True)
            else:
                res, st = ctc_label_posteriors_batch([x.detach().float().numpy() for x in lps], labels, terminals, beam_size,
                                                     max_move, return_status=True)
                res = [(torch.from_numpy(o), z) for o, z in res]
            for i, s in enumerate(st):
                if s == _lib.KA_ERR_ZERO_MASS and zero_infinity:
                    continue
                if s != _lib.KA_OK:
                    _raise_lattice_status(s, i)
            occs, zs = [], []
            for (o, z), s in zip(res, st):
                if s == _lib.KA_ERR_ZERO_MASS:
                    o = torch.zeros_like(o)
                    z = 0.0
                occs.append(o)
                zs.append(z)
            ctx.occs = occs
            ctx.dtypes = [x.dtype for x in lps]
            return torch.tensor(zs, dtype=torch.float64, device=lps[0].device).reshape(n)

        @staticmethod
        def backward(ctx, grad_out):
            grads = [(g * o.to(torch.float64)).to(dt) for g, o, dt in zip(grad_out.unbind(0), ctx.occs, ctx.dtypes)]
            ctx.occs = None
            return (None, None, None, None, None, *grads)

    return LatticeLogLikelihood


_LATTICE_LL = None


def _raise_lattice_status(st, i):
    what = f"lattice_log_likelihood: lattice {i}"
    if st == _lib.KA_ERR_BAD_LABEL:
        raise IndexError(f"{what}: label outside [0, V)")
    if st == _lib.KA_ERR_NAN:
        raise ValueError(f"{what}: log_probs contain NaN")
    if st == _lib.KA_ERR_NONFINITE:
        raise ValueError(f"{what}: a log-prob is +inf")
    if st == _lib.KA_ERR_BAD_ARGS:
        raise ValueError(f"{what}: terminal outside [0, 2S+1)")
    if st == _lib.KA_ERR_ZERO_MASS:
        raise ValueError(f"{what}: no path of finite score reaches the terminal")
    raise _lib.KAError(f"{what}: status {st}")


def lattice_log_likelihood(log_probs, labels, terminal, beam_size=1000, max_move=4, zero_infinity=False):
    """Differentiable log-likelihood Z of the band's paths that end at ``terminal`` (this engine's topology: band, moves,
    label-0 veto), float64 on the input's device.  One [T, V] tensor (labels, terminal for it) -> 0-d; a list of them (lists
    of labels and terminals) -> [n].  The gradient with respect to the log-probs is the label occupancy (``ctc_label_posteriors``)
    times the incoming gradient; the forward pass saves it, so backward launches nothing.  With ``zero_infinity``, a lattice
    whose terminal no finite path reaches gives 0 and a zero gradient (as ``torch.nn.CTCLoss``); otherwise, and for every
    other failure, this raises as ``ctc_label_posteriors`` does."""
    global _LATTICE_LL
    if _LATTICE_LL is None:
        _LATTICE_LL = _lattice_ll_function()
    single = _is_tensor(log_probs)
    lps = [log_probs] if single else list(log_probs)
    labs = [labels] if single else list(labels)
    terms = [terminal] if single else list(terminal)
    if len(lps) == 0 or len(labs) != len(lps) or len(terms) != len(lps):
        raise ValueError("log_probs, labels and terminals must be non-empty lists of one length")
    z = _LATTICE_LL.apply(labs, [_terminal_of(s) for s in terms], int(beam_size), int(max_move), bool(zero_infinity), *lps)
    return z[0] if single else z


def segment_agreement(occ, labels, best_path, seg_ends):
    """Soft transcript agreement of every segment that ``align()`` writes a line for: the mean over its frames [a, b)
    (a = seg_ends[i-1], 0 for the first, b = seg_ends[i], clipped to the frames) of occ[t, lab'[best_path[t]]], the
    occupancy of the label the best path emits.  float64 array, NaN for a segment without frames."""
    occ = np.asarray(occ.detach().cpu() if _is_tensor(occ) else occ, dtype=np.float64)
    lab = np.zeros(2 * len(np.asarray(labels).reshape(-1)) + 1, np.int64)
    lab[1::2] = np.asarray(labels).reshape(-1)
    path = np.asarray(best_path).reshape(-1).astype(np.int64)
    T = min(len(path), occ.shape[0])
    agree = occ[np.arange(T), lab[path[:T]]]
    ends = np.asarray(seg_ends).reshape(-1)
    mean = np.full(len(ends), np.nan)
    for i in range(len(ends)):
        a = int(ends[i - 1]) if i > 0 else 0
        b = min(int(ends[i]), T)
        if b > a:
            mean[i] = agree[a:b].mean()
    return mean


# ------------------------------------------------------------------------------------------
# state posteriors at chosen frames and the confidence of align()'s text boundaries (same band, same forward-backward)
# ------------------------------------------------------------------------------------------
def _frames_of(frames, T):
    """A query frame list as int64 NumPy, checked: strictly increasing in [0, T)."""
    if _is_tensor(frames):
        frames = frames.detach().cpu().numpy()
    f = np.ascontiguousarray(np.asarray(frames).reshape(-1), dtype=np.int64)
    if len(f) and (f[0] < 0 or f[-1] >= T or np.any(np.diff(f) <= 0)):
        raise ValueError(f"frames must be strictly increasing in [0, {T})")
    return f


def _band_width(S, beam_size):
    """W = max(1, min(beam_size, 2S+1)): the widest band, the row length of a state posterior."""
    return max(1, min(int(beam_size), 2 * int(S) + 1))


def ctc_state_posteriors(log_probs, labels, terminal, frames, beam_size=1000, max_move=4):
    """Posterior of every band position at chosen frames: (gamma float32 [K, W], band_lo int64 [K], log_likelihood float).

    gamma[k, j] is the probability that frame ``frames[k]`` sits at state band_lo[k] + j, over every path of the band of
    ``ctc_best_path`` that ends at state ``terminal`` (an int, or a best path whose last value is used); columns past the
    band's width are 0, each row sums to 1.  W = min(beam_size, 2S+1).  ``frames``: strictly increasing in [0, T).
    NumPy in -> NumPy out; ROCm torch tensors go to ``ctc_state_posteriors_device``.  Raises as ``ctc_label_posteriors``,
    and ValueError for bad frames.
    """
    if _is_tensor(log_probs):
        (g, lo, ll), = ctc_state_posteriors_device([log_probs], [labels], [terminal], [frames], beam_size, max_move)
        return g, lo, ll
    (g, lo, ll), = ctc_state_posteriors_batch([log_probs], [labels], [terminal], [frames], beam_size, max_move)
    return g, lo, ll


def ctc_state_posteriors_batch(log_probs_list, labels_list, terminals, frames_list, beam_size=1000, max_move=4, device=None,
                               return_status=False):
    """State posteriors of many lattices in ONE launch; host NumPy buffers in and out.

    Returns a list of (gamma [K_i, W_i], band_lo [K_i], log_likelihood); with ``return_status`` also the per-lattice status
    list, in which case failures do not raise (their rows are NaN, band_lo -1, their log-likelihood NaN, or -inf for
    KA_ERR_ZERO_MASS).
    """
    got = _host_lattices(log_probs_list, labels_list, terminals, "terminals")
    if got is None:
        return ([], []) if return_status else []
    if len(frames_list) != len(log_probs_list):
        raise ValueError("frames must hold one list per lattice")
    lps, labs, _, V = got
    frames = [_frames_of(f, x.shape[0]) for f, x in zip(frames_list, lps)]
    Ws = [_band_width(len(lab), beam_size) for lab in labs]
    gammas = [np.empty((len(f), W), np.float32) for f, W in zip(frames, Ws)]
    los = [np.empty(len(f), np.int64) for f in frames]
    eng = _lib.default_engine(_current_device() if device is None else device)
    p_term, _k1 = _i64_array([_terminal_of(s) for s in terminals])
    p_fr, _k2 = _ptr_array([f.ctypes.data for f in frames])
    p_K, _k3 = _i64_array([len(f) for f in frames])
    p_g, _k4 = _ptr_array([g.ctypes.data for g in gammas])
    p_ldo, _k5 = _i64_array(Ws)
    p_lo, _k6 = _ptr_array([x.ctypes.data for x in los])
    got = _run_lattices(eng, "ka_ctc_state_posteriors_batch_f32", "ctc_state_posteriors_batch", [x.ctypes.data for x in lps],
                        [x.shape[0] for x in lps], V, [V] * len(lps), [x.ctypes.data for x in labs], [x.shape[0] for x in labs],
                        beam_size, max_move, (p_term, p_fr, p_K, p_g, p_ldo, p_lo), list(zip(gammas, los)), _lib.KA_MEM_HOST, None,
                        return_status)
    return _state_results(got, return_status)


def _state_results(got, return_status):
    """_run_lattices' ((gamma, band_lo), z) pairs as (gamma, band_lo, z) triples."""
    res, st = got if return_status else (got, None)
    res = [(g, lo, z) for (g, lo), z in res]
    return (res, st) if return_status else res


def ctc_state_posteriors_device(log_probs, labels, terminals, frames, beam_size=1000, max_move=4, out=None, return_status=False):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V] with unit column stride, labels [S_i]), terminals (ints or
    best paths) and host frame lists (strictly increasing in [0, T_i)); list of (gamma tensor [K_i, W_i], band_lo int64 tensor
    [K_i], both on the device, log_likelihood float) out, W_i = min(beam_size, 2 S_i + 1).  ``out``: optional list of float32
    [K_i, W_i] tensors with unit column stride to write gamma into (views into wider tensors keep their other columns).  One
    launch on torch's current stream."""
    import torch
    lps, labs, _, V, dev, dev_index = _device_lattices(log_probs, labels, terminals, "terminals")
    n = len(lps)
    if len(frames) != n:
        raise ValueError("frames must hold one list per lattice")
    frames = [_frames_of(f, int(x.shape[0])) for f, x in zip(frames, lps)]
    Ws = [_band_width(x.shape[0], beam_size) for x in labs]
    if out is None:
        out = [torch.empty((len(f), W), dtype=torch.float32, device=dev) for f, W in zip(frames, Ws)]
    else:
        if len(out) != n:
            raise ValueError("out must hold one tensor per lattice")
        for o, f, W in zip(out, frames, Ws):
            if o.dtype != torch.float32 or o.dim() != 2 or tuple(o.shape) != (len(f), W) or o.stride(1) != 1 or o.device != dev:
                raise ValueError("out tensors must be float32 [K_i, W_i] on the input's device with unit column stride")
    los = [torch.empty(len(f), dtype=torch.int64, device=dev) for f in frames]
    eng = _lib.default_engine(dev_index)
    p_term, _k1 = _i64_array([_terminal_of(s) for s in terminals])
    p_fr, _k2 = _ptr_array([f.ctypes.data for f in frames])
    p_K, _k3 = _i64_array([len(f) for f in frames])
    p_g, _k4 = _ptr_array([o.data_ptr() for o in out])
    p_ldo, _k5 = _i64_array([max(o.stride(0), W) for o, W in zip(out, Ws)])   # (a tensor with no rows may report any stride)
    p_lo, _k6 = _ptr_array([x.data_ptr() for x in los])
    with torch.cuda.device(dev):
        got = _run_lattices(eng, "ka_ctc_state_posteriors_batch_f32", "ctc_state_posteriors_device", [x.data_ptr() for x in lps],
                            [x.shape[0] for x in lps], V, [x.stride(0) for x in lps], [x.data_ptr() for x in labs],
                            [x.shape[0] for x in labs], beam_size, max_move, (p_term, p_fr, p_K, p_g, p_ldo, p_lo),
                            list(zip(out, los)), _lib.KA_MEM_DEVICE, _stream_ptr(dev_index), return_status)
    return _state_results(got, return_status)


def boundary_frames(seg_ends, T):
    """The frames ``align()`` reads the best path at, sorted and unique: 0 (the first segment's start) and every
    seg_ends[i] < T (a segment's end, which is also the next one's start).  int64 array."""
    ends = np.asarray(seg_ends, dtype=np.int64).reshape(-1)
    return np.unique(np.concatenate([np.zeros(1, np.int64), ends[ends < int(T)]]))


def segment_boundary_confidence(gamma, band_lo, frames, best_path, seg_ends, n_phonemes):
    """How likely each text boundary ``align()`` writes is right, from state posteriors at ``boundary_frames`` (host only).

    For segment i (frames [a, b), a = seg_ends[i-1], 0 for the first, b = seg_ends[i]) ``align()`` writes text_start =
    min(best_path[a] // 2, n_phonemes) and text_end = min(best_path[b] // 2, n_phonemes), or n_phonemes where b >= T.  With
    state s read as text index min(s // 2, n_phonemes), p_start[i] is the posterior probability of text_start at frame a and
    p_end[i] that of text_end at frame b (1.0 where b >= T).  Returns two float64 arrays.  Raises ValueError if a frame it
    needs is not in ``frames``."""
    g = np.asarray(gamma.detach().cpu() if _is_tensor(gamma) else gamma, dtype=np.float64)
    lo = np.asarray(band_lo.detach().cpu() if _is_tensor(band_lo) else band_lo, dtype=np.int64).reshape(-1)
    fr = np.asarray(frames.detach().cpu() if _is_tensor(frames) else frames, dtype=np.int64).reshape(-1)
    path = np.asarray(best_path.detach().cpu() if _is_tensor(best_path) else best_path, dtype=np.int64).reshape(-1)
    ends = np.asarray(seg_ends, dtype=np.int64).reshape(-1)
    T, n_ph = len(path), int(n_phonemes)
    row_of = {int(f): k for k, f in enumerate(fr)}
    cols = np.arange(g.shape[1] if g.ndim == 2 else 0, dtype=np.int64)

    def p_at(t):
        k = row_of.get(int(t))
        if k is None:
            raise ValueError(f"segment_boundary_confidence: frame {int(t)} is not among the query frames")
        want = min(int(path[t]) // 2, n_ph)
        text = np.minimum((lo[k] + cols) // 2, n_ph)
        return float(np.sum(g[k][text == want]))

    p_start = np.empty(len(ends))
    p_end = np.empty(len(ends))
    for i in range(len(ends)):
        a = int(ends[i - 1]) if i > 0 else 0
        b = int(ends[i])
        p_start[i] = p_at(a)
        p_end[i] = p_at(b) if b < T else 1.0
    return p_start, p_end


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


def best_path(input_file, voca_file, output_file, device_softmax=False):
    """``*.logits.npz`` + ``*.voca.txt`` -> ``*.best_path.npz`` (reference: align.py:112-124).

    Keys/dtypes of the output: best_path int32, best_labels int32, best_scores float32.
    ``device_softmax=True`` computes the log-softmax with the HIP kernel (1e-6 of the NumPy
    formula) and keeps the log-probs on the device; the default reproduces the reference's
    host NumPy arithmetic bit for bit and hands the DP a host buffer.
    """
    from .transcript import read_transcript
    with np.load(input_file) as f:
        logits = f['data']
    labels = read_transcript(voca_file)
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
