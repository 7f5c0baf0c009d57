"""Raw callers of the banded and the tracking best-path batch symbols for the GPU tests that choose their engine (a private one
with a reserved workspace) and pass raw addresses, a NULL table or sentinel-filled outputs.  Like the callers of fb_harness.py
they go to the C ABI through ``eng.lib`` and never through the Python API of kokoro_align_amd/align.py: being independent of it
is their point.  ``lps`` and ``labs`` are (address, length) pairs, everything else lists of addresses; (rc, status, total)."""
import ctypes

import numpy as np


def _addresses(xs):
    return ctypes.cast((ctypes.c_void_p * len(xs))(*xs), ctypes.POINTER(ctypes.c_void_p))


def _i64(xs):
    return (ctypes.c_int64 * len(xs))(*[int(v) for v in xs])


def _head(eng, lps, labs, lds, V, beam_size, max_move):
    """the arguments every best-path batch call starts with"""
    return (eng.handle, len(lps), _addresses([x[0] for x in lps]), _i64([x[1] for x in lps]), V, _i64(lds),
            _addresses([x[0] for x in labs]), _i64([x[1] for x in labs]), int(beam_size), int(max_move))


def banded_call(eng, lps, labs, bands, lds, V, beam_size, max_move, paths, louts, souts, mem, stream):
    """ka_ctc_best_path_banded_batch_f32: the tables sit behind max_move"""
    status = np.zeros(len(lps), np.int32)
    total = np.zeros(len(lps), np.float32)
    rc = eng.lib.ka_ctc_best_path_banded_batch_f32(*_head(eng, lps, labs, lds, V, beam_size, max_move), _addresses(bands), _addresses(paths),
                                                   _addresses(louts), _addresses(souts), total.ctypes.data, status.ctypes.data, mem, stream)
    return rc, status, total


def tracking_call(eng, lps, labs, lds, V, beam_size, max_move, period, end_rule, paths, louts, souts, bands, mem, stream):
    """ka_ctc_best_path_tracking_batch_f32: period and end rule (an integer) sit behind max_move, the tables are the fourth output"""
    status = np.zeros(len(lps), np.int32)
    total = np.zeros(len(lps), np.float32)
    rc = eng.lib.ka_ctc_best_path_tracking_batch_f32(*_head(eng, lps, labs, lds, V, beam_size, max_move), int(period), int(end_rule),
                                                     _addresses(paths), _addresses(louts), _addresses(souts), _addresses(bands),
                                                     total.ctypes.data, status.ctypes.data, mem, stream)
    return rc, status, total
