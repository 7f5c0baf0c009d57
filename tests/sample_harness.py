"""Raw ctypes callers of the path sampling symbols for tests/test_sample_paths_gpu.py, beside fb_harness.py's callers of the
posterior calls: they go to the C ABI through ``eng.lib`` and never through kokoro_align_amd/posteriors.py.  Outputs are int32
buffers of ``rows`` x ``ld_paths`` values filled with the sentinel -77 (status 99), so a test can tell what a call wrote."""
import ctypes

import numpy as np

from fb_harness import I, P, _lattices, _one

SENTINEL = -77


def sample_call(eng, _lib, lps, labs, terms, Ks, seeds, beam, mm, pad=0, extra_rows=0):
    """ka_ctc_sample_paths_batch_f32 on host buffers: (paths list, log-likelihoods, statuses, rc); lattice i's buffer is
    [Ks[i] + extra_rows, T_i + pad] with ld_paths = T_i + pad."""
    n = len(lps)
    lps, Ts, V, lds, labs, Ss = _lattices(lps, labs)
    Ks = [int(Ks)] * n if np.ndim(Ks) == 0 else [int(k) for k in Ks]
    seeds = [int(seeds)] * n if np.ndim(seeds) == 0 else [int(s) for s in seeds]
    bufs = [np.full((max(K, 0) + extra_rows, x.shape[0] + pad), SENTINEL, np.int32) for K, x in zip(Ks, lps)]
    a_K = np.asarray(Ks, np.int32)
    a_seed = np.asarray(seeds, np.uint64)
    ll = np.zeros(n, np.float64)
    st = np.full(n, 99, np.int32)
    rc = eng.lib.ka_ctc_sample_paths_batch_f32(eng.handle, n, P(lps), Ts, V, lds, P(labs), Ss, beam, mm, I(terms), a_K.ctypes.data,
                                               a_seed.ctypes.data, P(bufs), I([x.shape[0] + pad for x in lps]), ll.ctypes.data,
                                               st.ctypes.data, _lib.KA_MEM_HOST, None)
    return bufs, ll, st, rc


def sample_call_one(eng, _lib, lp, labels, terminal, K, seed, beam, mm, ld_paths=None, rows=None):
    """ka_ctc_sample_paths_f32 for one lattice on host buffers: (paths [rows or K, ld_paths or T], Z, rc)."""
    lp, labels, head = _one(lp, labels)
    T = lp.shape[0]
    ld = T if ld_paths is None else ld_paths
    buf = np.full((max(K, 1) if rows is None else rows, max(ld, 1)), SENTINEL, np.int32)
    z = np.zeros(1, np.float64)
    rc = eng.lib.ka_ctc_sample_paths_f32(eng.handle, *head, beam, mm, int(terminal), int(K), ctypes.c_uint64(int(seed)), buf.ctypes.data,
                                         int(ld), z.ctypes.data, _lib.KA_MEM_HOST, None)
    return buf, z[0], rc
