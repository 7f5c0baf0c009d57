"""Raw ctypes callers of the maximum-expected-accuracy symbols for tests/test_mea_path_gpu.py, beside fb_harness.py's callers of
the posterior calls: they go to the C ABI through ``eng.lib`` and never through kokoro_align_amd/posteriors.py.  A path buffer
holds T + GUARD int32 values filled with the sentinel -77, the expected accuracies are filled with -7.0 and the statuses with
99, so a test can tell what a call wrote, and that it wrote nothing past T."""
import numpy as np

from fb_harness import GUARD, I, P, _addresses, _lattices, _one

SENTINEL = -77
EA_SENTINEL = -7.0


def mea_call(eng, _lib, lps, labs, terms, beam, mm, device=False):
    """ka_ctc_mea_path_batch_f32 on host buffers, or (``device``) on device copies of them: (path list, expected accuracies,
    log-likelihoods, statuses, rc); every path array has T_i + GUARD entries."""
    n = len(lps)
    lps, Ts, V, lds, labs, Ss = _lattices(lps, labs)
    paths = [np.full(x.shape[0] + GUARD, SENTINEL, np.int32) for x in lps]
    ea = np.full(n, EA_SENTINEL, np.float64)
    ll = np.zeros(n, np.float64)
    st = np.full(n, 99, np.int32)
    if device:
        import torch
        keep = [[torch.from_numpy(x).cuda() for x in xs] for xs in (lps, labs, paths)]
        ptr = lambda k: _addresses([x.data_ptr() for x in keep[k]])
        p_lp, p_lab, p_path, mem = ptr(0), ptr(1), ptr(2), _lib.KA_MEM_DEVICE
    else:
        p_lp, p_lab, p_path, mem = P(lps), P(labs), P(paths), _lib.KA_MEM_HOST
    rc = eng.lib.ka_ctc_mea_path_batch_f32(eng.handle, n, p_lp, Ts, V, lds, p_lab, Ss, beam, mm, I(terms), p_path, ea.ctypes.data,
                                           ll.ctypes.data, st.ctypes.data, mem, None)
    if device:
        import torch
        torch.cuda.synchronize()
        paths = [x.cpu().numpy() for x in keep[2]]
    return paths, ea, ll, st, rc


def mea_call_one(eng, _lib, lp, labels, terminal, beam, mm, ld=None):
    """ka_ctc_mea_path_f32 for one lattice on host buffers, its log-probs in rows of pitch ``ld`` (V if None) whose other
    columns hold NaN: (path [T + GUARD], expected accuracy, Z, rc)."""
    lp, labels, head = _one(lp, labels)
    T, V = lp.shape
    if ld is not None:
        wide = np.full((T, max(ld, 1)), np.nan, np.float32)
        wide[:, :min(V, ld)] = lp[:, :min(V, ld)]
        lp = wide
        head = (lp.ctypes.data, T, V, ld) + head[4:]
    path = np.full(T + GUARD, SENTINEL, np.int32)
    ea = np.full(1, EA_SENTINEL, np.float64)
    z = np.zeros(1, np.float64)
    rc = eng.lib.ka_ctc_mea_path_f32(eng.handle, *head, beam, mm, int(terminal), path.ctypes.data, ea.ctypes.data, z.ctypes.data,
                                     _lib.KA_MEM_HOST, None)
    return path, ea[0], z[0], rc
