"""Raw ctypes callers of the boundary-quantile symbols for tests/test_boundary_quantiles_gpu.py, beside fb_harness.py's callers
of the posterior calls and with its engine set-up: they go to the C ABI through ``eng.lib`` and never through
kokoro_align_amd/posteriors.py.  Outputs are int32 buffers of K_i + GUARD rows of M + ``pad`` values (row pitch ld_q = M + pad)
filled with the sentinel -77 (status 99), so a test can tell what a call wrote, and that it wrote nothing beside [K, M]."""
import numpy as np

from fb_harness import I, P, _addresses, _lattices, _one

GUARD = 2
SENTINEL = -77


def quant_call(eng, _lib, lps, labs, terms, cuts, levels, beam, mm, pad=0, device=False, ld_q=None, M=None):
    """ka_ctc_boundary_quantiles_batch_f32 on host buffers, or (``device``) on device copies of them (the cuts and levels stay
    on the host): (quantile list, log-likelihoods, statuses, rc); lattice i's buffer is [K_i + GUARD, M + pad].  ``ld_q`` and
    ``M`` override what is passed for the pitch and the number of levels (for the argument checks)."""
    n = len(lps)
    lps, Ts, V, lds, labs, Ss = _lattices(lps, labs)
    cuts = [np.ascontiguousarray(np.asarray(c).reshape(-1), np.int64) for c in cuts]
    lv = np.ascontiguousarray(np.asarray(levels, np.float64).reshape(-1))
    m = len(lv)
    bufs = [np.full((len(c) + GUARD, m + pad), SENTINEL, np.int32) for c in cuts]
    ll = np.zeros(n, np.float64)
    st = np.full(n, 99, np.int32)
    if device:
        import torch
        keep = [[torch.from_numpy(x).cuda() for x in xs] for xs in (lps, labs, bufs)]
        ptr = lambda k: [x.data_ptr() for x in keep[k]]
        p_lp, p_lab, p_out = _addresses(ptr(0)), _addresses(ptr(1)), _addresses(ptr(2))
        mem = _lib.KA_MEM_DEVICE
    else:
        p_lp, p_lab, p_out = P(lps), P(labs), P(bufs)
        mem = _lib.KA_MEM_HOST
    rc = eng.lib.ka_ctc_boundary_quantiles_batch_f32(eng.handle, n, p_lp, Ts, V, lds, p_lab, Ss, beam, mm, I(terms), P(cuts),
                                                     I([len(c) for c in cuts]), lv.ctypes.data, m if M is None else M, p_out,
                                                     I([m + pad if ld_q is None else ld_q] * n), ll.ctypes.data, st.ctypes.data, mem, None)
    if device:
        import torch
        torch.cuda.synchronize()
        bufs = [x.cpu().numpy() for x in keep[2]]
    return bufs, ll, st, rc


def quant_call_one(eng, _lib, lp, labels, terminal, cuts, levels, beam, mm, pad=0):
    """ka_ctc_boundary_quantiles_f32 for one lattice on host buffers: (quantile [K + GUARD, M + pad], Z, rc)."""
    lp, labels, head = _one(lp, labels)
    c = np.ascontiguousarray(np.asarray(cuts).reshape(-1), np.int64)
    lv = np.ascontiguousarray(np.asarray(levels, np.float64).reshape(-1))
    buf = np.full((len(c) + GUARD, len(lv) + pad), SENTINEL, np.int32)
    z = np.zeros(1, np.float64)
    rc = eng.lib.ka_ctc_boundary_quantiles_f32(eng.handle, *head, beam, mm, int(terminal), c.ctypes.data, len(c), lv.ctypes.data, len(lv),
                                               buf.ctypes.data, len(lv) + pad, z.ctypes.data, _lib.KA_MEM_HOST, None)
    return buf, z[0], rc


def written(buf, K, M):
    """The [K, M] block of a buffer, after a check that nothing beside it was written."""
    assert np.all(buf[K:] == SENTINEL) and np.all(buf[:, M:] == SENTINEL)
    return buf[:K, :M]
