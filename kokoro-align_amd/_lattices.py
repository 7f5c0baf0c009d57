"""The lattices of one batched call, as every ``ka_ctc_<call>_batch_f32`` takes them: the input layer of the best-path batch
calls (align.py) and of the forward-backward calls (posteriors.py).

``_Lattices`` is that input (log-probs, labels), normalised once and aware of its memory mode; ``_host_lattices`` builds it from
NumPy buffers, ``_device_lattices`` from ROCm torch tensors, and ``_band_tables`` checks the band tables that go with it.  The
ctypes table helpers are here too.
"""
import contextlib
import ctypes
import operator
import os

import numpy as np

from . import _lib


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


def _host_rows(x):
    """float32 [T, V] rows as they lie if their columns are adjacent (a view with a row stride is handed over with its ld),
    else a contiguous copy"""
    x = np.asarray(x)
    if x.dtype == np.float32 and x.ndim == 2 and x.shape[1] > 0 and x.strides[1] == 4 and x.strides[0] % 4 == 0 and \
            x.strides[0] >= 4 * x.shape[1]:
        return x
    return np.ascontiguousarray(x, dtype=np.float32)


# ------------------------------------------------------------------------------------------
# the lattices of one call
# ------------------------------------------------------------------------------------------
class _Lattices:
    """n lattices as one ``ka_ctc_<call>_batch_f32`` call takes them: ``lps`` float32 [T_i, V] with unit column
    stride, ``labs`` int32 [S_i].  What differs between host and device memory is in the attributes ``mode`` brings:
    form, mem, dev, ptr(x), ld(x) (row pitch), int32(x) (a per-position input as the call wants it), empty(shape, dtype),
    is_out(x, shape, dtype) (a contiguous output of the caller's, where the lattices are), engine(), stream(), guard()."""

    def __init__(self, lps, labels, V, **mode):
        self.__dict__.update(mode)
        self.lps, self.V, self.n = lps, V, len(lps)
        self.labs = [self.int32(x) for x in labels]
        self.T = [int(x.shape[0]) for x in lps]
        self.S = [int(x.shape[0]) for x in self.labs]


def _count(log_probs, labels, others, what):
    """The number of lattices.  ``others`` holds the call's own input (one best path, terminal or table per lattice; None if
    it has none) and is only counted."""
    n = len(log_probs)
    if n != len(labels) or n != len(labels if others is None else others):
        raise ValueError(f"{'log_probs and labels' if others is None else 'log_probs, labels and ' + what} must be lists of one length")
    return n


def _host_lattices(log_probs_list, labels_list, others, what, device):
    """The input handling of the ``*_batch`` calls: NumPy arrays in (``_host_rows``), NumPy results; None for an empty batch.
    ``others``, ``what``: ``_count``."""
    if _count(log_probs_list, labels_list, others, what) == 0:
        return None
    lps = [_host_rows(x) for x in log_probs_list]
    V = lps[0].shape[1] if lps[0].ndim == 2 else 0
    for x in lps:
        if x.ndim != 2 or x.shape[1] != V:
            raise ValueError("all log_probs must be [T_i, V] with one V")
        if x.shape[0] == 0:
            raise IndexError("list index out of range")
    return _Lattices(lps, labels_list, V, form="batch", mem=_lib.KA_MEM_HOST, dev=None, ptr=operator.attrgetter("ctypes.data"),
                     ld=lambda x: max(x.shape[1], x.strides[0] // x.itemsize),
                     int32=lambda x: np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int32), empty=np.empty,
                     is_out=lambda x, shape, dtype: x.dtype == dtype and x.shape == shape and x.flags.c_contiguous,
                     engine=lambda: _lib.default_engine(_current_device() if device is None else device),
                     stream=lambda: None, guard=contextlib.nullcontext)


def _device_lattices(log_probs, labels, others, what):
    """The input handling of the ``*_device`` calls: tensors on the first log-prob's device in, results there, the call on
    torch's current stream; ``others`` as in ``_host_lattices``."""
    import torch
    if _count(log_probs, labels, others, what) == 0:
        raise ValueError("the device forms take no empty batch")
    dev = log_probs[0].device
    V = int(log_probs[0].shape[1])
    lps = []
    for lp in log_probs:
        if lp.dtype != torch.float32:
            lp = lp.float()
        if lp.dim() != 2 or lp.shape[1] != V:
            raise ValueError("all log_probs must be [T_i, V] tensors with one V")
        if lp.shape[0] == 0:
            raise IndexError("list index out of range")
        if lp.stride(1) != 1:
            lp = lp.contiguous()
        lps.append(lp)
    dev_index = dev.index if dev.index is not None else torch.cuda.current_device()
    dtypes = {np.float32: torch.float32, np.float64: torch.float64, np.int64: torch.int64, np.int32: torch.int32}

    def int32(x):
        x = x if _is_tensor(x) else torch.as_tensor(np.asarray(x).reshape(-1).astype(np.int32))
        return x.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()

    return _Lattices(lps, labels, V, form="device", mem=_lib.KA_MEM_DEVICE, dev=dev, ptr=operator.methodcaller("data_ptr"),
                     ld=lambda x: x.stride(0), int32=int32, empty=lambda shape, dtype: torch.empty(shape, dtype=dtypes[dtype], device=dev),
                     is_out=lambda x, shape, dtype: x.dtype == dtypes[dtype] and tuple(x.shape) == shape and x.is_contiguous() and x.device == dev,
                     engine=lambda: _lib.default_engine(dev_index), stream=lambda: _stream_ptr(dev_index),
                     guard=lambda: torch.cuda.device(dev))


def _band_tables(lat, band_lo):
    """The tables of a banded call as the call wants them: one per lattice, int32 where the lattices are, T_i entries.  They
    may come as int64 (as ``diagonal_band`` and the other table builders return them) or as tensors.  A host table's entries
    must fit int32 (a wrapped entry would name another band); a device tensor is checked for its length only, without a sync."""
    if len(band_lo) != lat.n:
        raise ValueError("band_lo must hold one table per lattice")
    tables = []
    for b, T in zip(band_lo, lat.T):
        if _is_tensor(b) and lat.form == "batch":
            b = b.detach().cpu().numpy()
        if not _is_tensor(b):
            b = np.asarray(b).reshape(-1)
            if b.size and (b.min() < -2 ** 31 or b.max() >= 2 ** 31):
                raise ValueError("band_lo: entries must fit int32")
        b = lat.int32(b)
        if b.shape[0] != T:
            raise ValueError("a band table must have one entry per frame")
        tables.append(b)
    return tables
