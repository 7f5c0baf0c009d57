"""Raw ctypes callers of the state visit symbols for tests/test_state_visits_gpu.py, beside fb_harness.py's callers of the
posterior calls and with its engine set-up: they go to the C ABI through ``eng.lib`` and never through
kokoro_align_amd/posteriors.py.  Outputs are float64 buffers of L + GUARD values filled with the sentinel -7.0 (status 99), so
a test can tell what a call wrote, and that it wrote nothing past L."""
import ctypes

import numpy as np

from fb_harness import I, P, _lattices, _one

GUARD = 4
SENTINEL = -7.0


def _addresses(xs):
    return ctypes.cast((ctypes.c_void_p * len(xs))(*xs), ctypes.POINTER(ctypes.c_void_p))


def visit_call(eng, _lib, lps, labs, terms, beam, mm, exit_time=True, device=False):
    """ka_ctc_state_visits_batch_f32 on host buffers, or (``device``) on device copies of them: (visit list, exit_time
    list or None, log-likelihoods, statuses, rc); every output array has L_i + GUARD entries.  ``exit_time``: True, False (a
    NULL array) or a list of booleans (NULL entries)."""
    n = len(lps)
    lps, Ts, V, lds, labs, Ss = _lattices(lps, labs)
    Ls = [2 * x.shape[0] + 1 for x in labs]
    want = [bool(exit_time)] * n if isinstance(exit_time, bool) else [bool(x) for x in exit_time]
    visits = [np.full(L + GUARD, SENTINEL, np.float64) for L in Ls]
    exits = [np.full(L + GUARD, SENTINEL, np.float64) for L in Ls]
    ll = np.zeros(n, np.float64)
    st = np.full(n, 99, np.int32)
    if device:
        import torch
        keep = [[torch.from_numpy(x).cuda() for x in xs] for xs in (lps, labs, visits, exits)]
        ptr = lambda k: [x.data_ptr() for x in keep[k]]
        p_lp, p_lab, a_vis, a_exit = _addresses(ptr(0)), _addresses(ptr(1)), ptr(2), ptr(3)
        mem = _lib.KA_MEM_DEVICE
    else:
        p_lp, p_lab, a_vis, a_exit = P(lps), P(labs), [x.ctypes.data for x in visits], [x.ctypes.data for x in exits]
        mem = _lib.KA_MEM_HOST
    p_exit = _addresses([a if w else None for a, w in zip(a_exit, want)]) if any(want) else None
    rc = eng.lib.ka_ctc_state_visits_batch_f32(eng.handle, n, p_lp, Ts, V, lds, p_lab, Ss, beam, mm, I(terms), _addresses(a_vis),
                                               p_exit, ll.ctypes.data, st.ctypes.data, mem, None)
    if device:
        import torch
        torch.cuda.synchronize()
        visits = [x.cpu().numpy() for x in keep[2]]
        exits = [x.cpu().numpy() for x in keep[3]]
    return visits, (exits if any(want) else None), ll, st, rc


def visit_call_one(eng, _lib, lp, labels, terminal, beam, mm, exit_time=True, ld=None):
    """ka_ctc_state_visits_f32 for one lattice on host buffers, its log-probs in rows of pitch ``ld`` (V if None) whose other
    columns hold NaN: (visit [L + GUARD], exit_time [L + GUARD] - untouched if ``exit_time`` is False -, Z, rc)."""
    lp, labels, head = _one(lp, labels)
    T, V = lp.shape
    if ld is not None:
        wide = np.full((T, ld), np.nan, np.float32)
        wide[:, :V] = lp
        lp = wide
        head = (lp.ctypes.data, T, V, ld) + head[4:]
    L = 2 * labels.shape[0] + 1
    vis = np.full(L + GUARD, SENTINEL, np.float64)
    xtime = np.full(L + GUARD, SENTINEL, np.float64)
    z = np.zeros(1, np.float64)
    rc = eng.lib.ka_ctc_state_visits_f32(eng.handle, *head, beam, mm, int(terminal), vis.ctypes.data,
                                         xtime.ctypes.data if exit_time else None, z.ctypes.data, _lib.KA_MEM_HOST, None)
    return vis, xtime, z[0], rc
