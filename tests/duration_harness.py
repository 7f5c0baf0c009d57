"""Raw ctypes callers of the state duration and state visit symbols for tests/test_durations_gpu.py and
tests/test_state_visits_gpu.py, beside fb_harness.py's callers of the posterior calls and with its engine set-up: they go to the
C ABI through ``eng.lib`` and never through kokoro_align_amd/posteriors.py.  The two calls have one signature - a terminal, an
output and an optional second output of 2S+1 doubles - so one caller, ``pair_call`` / ``pair_call_one``, serves both by symbol.
Outputs are float64 buffers of L + GUARD values filled with the sentinel -7.0 (status 99), so a test can tell what a call wrote,
and that it wrote nothing past L."""
import numpy as np

from fb_harness import GUARD, SENTINEL, I, P, _addresses, _lattices, _one


def pair_call(call, eng, _lib, lps, labs, terms, beam, mm, second=True, device=False):
    """ka_ctc_<call>_batch_f32 (``call``: "state_durations" or "state_visits") on host buffers, or (``device``) on device copies
    of them: (first output list, second output list or None, log-likelihoods, statuses, rc); every output array has L_i + GUARD
    entries.  ``second``: True, False (a NULL array) or a list of booleans (NULL entries)."""
    n = len(lps)
    lps, Ts, V, lds, labs, Ss = _lattices(lps, labs)
    Ls = [2 * x.shape[0] + 1 for x in labs]
    want = [bool(second)] * n if isinstance(second, bool) else [bool(x) for x in second]
    firsts = [np.full(L + GUARD, SENTINEL, np.float64) for L in Ls]
    seconds = [np.full(L + GUARD, SENTINEL, np.float64) for L in Ls]
    ll = np.zeros(n, np.float64)
    st = np.full(n, 99, np.int32)
    if device:
        import torch
        keep = [[torch.from_numpy(x).cuda() for x in xs] for xs in (lps, labs, firsts, seconds)]
        ptr = lambda k: [x.data_ptr() for x in keep[k]]
        p_lp, p_lab, a_first, a_second = _addresses(ptr(0)), _addresses(ptr(1)), ptr(2), ptr(3)
        mem = _lib.KA_MEM_DEVICE
    else:
        p_lp, p_lab, a_first, a_second = P(lps), P(labs), [x.ctypes.data for x in firsts], [x.ctypes.data for x in seconds]
        mem = _lib.KA_MEM_HOST
    p_second = _addresses([a if w else None for a, w in zip(a_second, want)]) if any(want) else None
    rc = getattr(eng.lib, f"ka_ctc_{call}_batch_f32")(eng.handle, n, p_lp, Ts, V, lds, p_lab, Ss, beam, mm, I(terms), _addresses(a_first),
                                                      p_second, ll.ctypes.data, st.ctypes.data, mem, None)
    if device:
        import torch
        torch.cuda.synchronize()
        firsts = [x.cpu().numpy() for x in keep[2]]
        seconds = [x.cpu().numpy() for x in keep[3]]
    return firsts, (seconds if any(want) else None), ll, st, rc


def pair_call_one(call, eng, _lib, lp, labels, terminal, beam, mm, second=True, ld=None):
    """ka_ctc_<call>_f32 for one lattice on host buffers, its log-probs in rows of pitch ``ld`` (V if None) whose other columns
    hold NaN: (first output [L + GUARD], second output [L + GUARD] - untouched if ``second`` is False -, Z, rc)."""
    lp, labels, head = _one(lp, labels)
    T, V = lp.shape
    if ld is not None:
        wide = np.full((T, ld), np.nan, np.float32)
        wide[:, :V] = lp
        lp = wide
        head = (lp.ctypes.data, T, V, ld) + head[4:]
    L = 2 * labels.shape[0] + 1
    first = np.full(L + GUARD, SENTINEL, np.float64)
    moment = np.full(L + GUARD, SENTINEL, np.float64)
    z = np.zeros(1, np.float64)
    rc = getattr(eng.lib, f"ka_ctc_{call}_f32")(eng.handle, *head, beam, mm, int(terminal), first.ctypes.data,
                                                moment.ctypes.data if second else None, z.ctypes.data, _lib.KA_MEM_HOST, None)
    return first, moment, z[0], rc


def duration_call(eng, _lib, lps, labs, terms, beam, mm, time_sum=True, device=False):
    return pair_call("state_durations", eng, _lib, lps, labs, terms, beam, mm, time_sum, device)


def duration_call_one(eng, _lib, lp, labels, terminal, beam, mm, time_sum=True, ld=None):
    return pair_call_one("state_durations", eng, _lib, lp, labels, terminal, beam, mm, time_sum, ld)
