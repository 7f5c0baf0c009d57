"""Raw ctypes callers of the state duration symbols for tests/test_durations_gpu.py, beside fb_harness.py's callers of the
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


def duration_call(eng, _lib, lps, labs, terms, beam, mm, time_sum=True, device=False):
    """ka_ctc_state_durations_batch_f32 on host buffers, or (``device``) on device copies of them: (duration list, time_sum
    list or None, log-likelihoods, statuses, rc); every output array has L_i + GUARD entries.  ``time_sum``: True, False (a
    NULL array) or a list of booleans (NULL entries)."""
    n = len(lps)
    lps, Ts, V, lds, labs, Ss = _lattices(lps, labs)
    Ls = [2 * x.shape[0] + 1 for x in labs]
    want = [bool(time_sum)] * n if isinstance(time_sum, bool) else [bool(x) for x in time_sum]
    durs = [np.full(L + GUARD, SENTINEL, np.float64) for L in Ls]
    sums = [np.full(L + GUARD, SENTINEL, np.float64) for L in Ls]
    ll = np.zeros(n, np.float64)
    st = np.full(n, 99, np.int32)
    if device:
        import torch
        keep = [[torch.from_numpy(x).cuda() for x in xs] for xs in (lps, labs, durs, sums)]
        ptr = lambda k: [x.data_ptr() for x in keep[k]]
        p_lp, p_lab, a_dur, a_sum = _addresses(ptr(0)), _addresses(ptr(1)), ptr(2), ptr(3)
        mem = _lib.KA_MEM_DEVICE
    else:
        p_lp, p_lab, a_dur, a_sum = P(lps), P(labs), [x.ctypes.data for x in durs], [x.ctypes.data for x in sums]
        mem = _lib.KA_MEM_HOST
    p_sum = _addresses([a if w else None for a, w in zip(a_sum, want)]) if any(want) else None
    rc = eng.lib.ka_ctc_state_durations_batch_f32(eng.handle, n, p_lp, Ts, V, lds, p_lab, Ss, beam, mm, I(terms), _addresses(a_dur),
                                                  p_sum, ll.ctypes.data, st.ctypes.data, mem, None)
    if device:
        import torch
        torch.cuda.synchronize()
        durs = [x.cpu().numpy() for x in keep[2]]
        sums = [x.cpu().numpy() for x in keep[3]]
    return durs, (sums if any(want) else None), ll, st, rc


def duration_call_one(eng, _lib, lp, labels, terminal, beam, mm, time_sum=True, ld=None):
    """ka_ctc_state_durations_f32 for one lattice on host buffers, its log-probs in rows of pitch ``ld`` (V if None) whose other
    columns hold NaN: (duration [L + GUARD], time_sum [L + GUARD] - untouched if ``time_sum`` is False -, Z, rc)."""
    lp, labels, head = _one(lp, labels)
    T, V = lp.shape
    if ld is not None:
        wide = np.full((T, ld), np.nan, np.float32)
        wide[:, :V] = lp
        lp = wide
        head = (lp.ctypes.data, T, V, ld) + head[4:]
    L = 2 * labels.shape[0] + 1
    dur = np.full(L + GUARD, SENTINEL, np.float64)
    tsum = np.full(L + GUARD, SENTINEL, np.float64)
    z = np.zeros(1, np.float64)
    rc = eng.lib.ka_ctc_state_durations_f32(eng.handle, *head, beam, mm, int(terminal), dur.ctypes.data,
                                            tsum.ctypes.data if time_sum else None, z.ctypes.data, _lib.KA_MEM_HOST, None)
    return dur, tsum, z[0], rc
