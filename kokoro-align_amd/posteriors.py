"""Forward-backward over the band of ``ctc_best_path``: path posteriors, label occupancy, state posteriors at chosen frames,
expected state durations, state visit probabilities, exact boundary-time quantiles, alignments sampled from the posterior, the
maximum-expected-accuracy alignment; and, from the best path's own recurrence instead of the sum over paths, the per-frame margin
of a path over the best alignment that disagrees with it (``ctc_path_margins``).

The calls take the same lattices (log-probs, labels, beam_size, max_move) in host or device memory and answer with one
log-likelihood and one status per lattice.  ``_Lattices`` (_lattices.py, shared with the best-path batch calls of align.py) is
that common input, normalised once and aware of its memory mode; ``_run_lattices`` is the one C call and the one status
handling.  What is a call's own (its extra inputs, its outputs, its argument tables) is in its private function; ``X_batch``
and ``X_device`` only choose the memory mode.
"""
import numpy as np

from . import _lib
from ._lattices import _band_tables, _device_lattices, _host_lattices, _i64_array, _is_tensor, _ptr_array

_POSTERIOR_LATTICE_STATUSES = (_lib.KA_OK, _lib.KA_ERR_BAD_LABEL, _lib.KA_ERR_NAN, _lib.KA_ERR_NONFINITE, _lib.KA_ERR_BAD_ARGS,
                               _lib.KA_ERR_ZERO_MASS)


# ------------------------------------------------------------------------------------------
# the call itself
# ------------------------------------------------------------------------------------------
def _run_lattices(lat, call, beam_size, max_move, own_args, outs, return_status, band_lo=None):
    """The call ``ka_ctc_<call>_batch_f32`` (path_posteriors, label_posteriors, state_posteriors, state_durations, state_visits, boundary_quantiles,
    sample_paths, mea_path): the
    arguments all of them take around ``own_args`` (the call's own tables), then the results (*outs[i], log_likelihood[i]),
    ``outs`` a list of tuples, and the status handling of ``return_status``.  With ``band_lo`` (a table per lattice) the call is
    ``ka_ctc_<call>_banded_batch_f32``, which takes the tables behind ``max_move``; without, today's symbol and arguments."""
    if band_lo is not None:
        tables = _band_tables(lat, band_lo)
        p_band, _k0 = _ptr_array([lat.ptr(x) for x in tables])
        call, own_args = f"{call}_banded", (p_band, *own_args)
    name = f"ctc_{call}_{lat.form}"
    status = np.zeros(lat.n, np.int32)
    ll = np.zeros(lat.n, np.float64)
    eng = lat.engine()
    p_lp, _k1 = _ptr_array([lat.ptr(x) for x in lat.lps])
    p_lab, _k2 = _ptr_array([lat.ptr(x) for x in lat.labs])
    p_T, _k3 = _i64_array(lat.T)
    p_S, _k4 = _i64_array(lat.S)
    p_ld, _k5 = _i64_array([lat.ld(x) for x in lat.lps])
    with lat.guard():
        rc = getattr(eng.lib, f"ka_ctc_{call}_batch_f32")(
            eng.handle, lat.n, p_lp, p_T, lat.V, p_ld, p_lab, p_S, int(beam_size), int(max_move), *own_args,
            ll.ctypes.data, status.ctypes.data, lat.mem, lat.stream())
    results = [(*o, float(z)) for o, z in zip(outs, ll)]
    if return_status:
        if rc not in _POSTERIOR_LATTICE_STATUSES:
            _lib.check(rc, name)
        return results, status.tolist()
    _lib.check(rc, name)
    return results


def _outputs(lat, out, shapes, shape_text, dtype=np.float32):
    """The [rows, columns] outputs of a call (float32, or ``dtype``): allocated here, or the caller's ``out`` tensors (only the
    device forms take any) after a check."""
    if out is None:
        return [lat.empty(s, dtype) for s in shapes]
    import torch
    if len(out) != lat.n:
        raise ValueError("out must hold one tensor per lattice")
    name = np.dtype(dtype).name
    for o, s in zip(out, shapes):
        if o.dtype != getattr(torch, name) or o.dim() != 2 or tuple(o.shape) != s or o.stride(1) != 1 or o.device != lat.dev:
            raise ValueError(f"out tensors must be {name} {shape_text} on the input's device with unit column stride")
    return out


def _terminal_of(terminal):
    """An int, or a best path whose last value is the terminal."""
    if _is_tensor(terminal):
        terminal = terminal.detach().reshape(-1)[-1].item() if terminal.dim() > 0 else terminal.item()
    a = np.asarray(terminal)
    return int(a.reshape(-1)[-1]) if a.ndim > 0 else int(a)


def _segments(seg_ends, T):
    """(i, a, b) for every segment that ``align()`` writes a line for: frames [a, b) with a = seg_ends[i-1] (0 for the
    first) and b = seg_ends[i], clipped to the T frames there are."""
    ends = np.asarray(seg_ends).reshape(-1)
    return [(i, int(ends[i - 1]) if i > 0 else 0, min(int(ends[i]), T)) for i in range(len(ends))]


# ------------------------------------------------------------------------------------------
# best-path posteriors and lattice log-likelihood
# ------------------------------------------------------------------------------------------
def ctc_path_posteriors(log_probs, labels, best_path, beam_size=1000, max_move=4, band_lo=None):
    """How sure the model is of a best path, frame by frame: (posteriors float32 [T], log_likelihood float).

    posteriors[t] is the probability, over every path of the band of ``ctc_best_path`` that ends where ``best_path`` ends,
    that frame t sits at ``best_path[t]``; log_likelihood is the log of the total probability of those paths (nats).
    NumPy in -> NumPy out; ROCm torch tensors are handed to ``ctc_path_posteriors_device``.  Raises IndexError for a label
    outside [0, V), ValueError for NaN / +inf log-probs, a path value outside [0, 2S+1) or a terminal no finite path reaches.
    ``band_lo``: a table [T] as ``ctc_best_path_banded`` takes it (``diagonal_band``, ``anchored_band``, ``band_around_path``):
    the band is then [band_lo[t], min(band_lo[t] + beam_size, 2S+1)) - the band to judge a path found under that table with;
    an invalid table raises ValueError.
    """
    call = ctc_path_posteriors_device if _is_tensor(log_probs) else ctc_path_posteriors_batch
    (result,) = call([log_probs], [labels], [best_path], beam_size, max_move, band_lo=_one_table(band_lo))
    return result


def _one_table(band_lo):
    """The ``band_lo`` of a single-lattice call as the list its batch form takes."""
    return None if band_lo is None else [band_lo]


def _path_posteriors(lat, best_paths, beam_size, max_move, return_status, band_lo=None):
    if lat is None:
        return ([], []) if return_status else []
    paths = [lat.int32(x) for x in best_paths]
    if any(p.shape[0] != T for p, T in zip(paths, lat.T)):
        raise ValueError("a best path must have one position per frame")
    posts = [lat.empty(T, np.float32) for T in lat.T]
    p_path, _k1 = _ptr_array([lat.ptr(x) for x in paths])
    p_post, _k2 = _ptr_array([lat.ptr(x) for x in posts])
    return _run_lattices(lat, "path_posteriors", beam_size, max_move, (p_path, p_post), list(zip(posts)), return_status, band_lo)


def ctc_path_posteriors_batch(log_probs_list, labels_list, best_path_list, beam_size=1000, max_move=4, device=None,
                              return_status=False, band_lo=None):
    """Posteriors of many lattices in ONE launch; host NumPy buffers in and out.

    Returns a list of (posteriors, log_likelihood); with ``return_status`` also the per-lattice status list, in which case
    failures do not raise (their posteriors are NaN, their log-likelihood NaN, or -inf for KA_ERR_ZERO_MASS).
    ``band_lo``: a list of tables, one per lattice (``ctc_path_posteriors``).
    """
    lat = _host_lattices(log_probs_list, labels_list, best_path_list, "best paths", device)
    return _path_posteriors(lat, best_path_list, beam_size, max_move, return_status, band_lo)


def ctc_path_posteriors_device(log_probs, labels, best_paths, beam_size=1000, max_move=4, return_status=False, band_lo=None):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V], labels [S_i], best paths [T_i] - e.g. the outputs of
    ``ctc_best_path_device``), list of (posteriors tensor [T_i] on the device, log_likelihood float) out.  One launch on
    torch's current stream.  ``band_lo``: a list of tables, one per lattice, tensors on the device or host arrays."""
    lat = _device_lattices(log_probs, labels, best_paths, "best paths")
    return _path_posteriors(lat, best_paths, beam_size, max_move, return_status, band_lo)


def segment_confidence(posteriors, seg_ends):
    """Mean and minimum posterior of every segment that ``align()`` writes a line for: frames [a, b) with
    a = seg_ends[i-1] (0 for the first), b = seg_ends[i], clipped to the posteriors' length.  Returns two float64 arrays
    (NaN for a segment without frames)."""
    post = np.asarray(posteriors, dtype=np.float64).reshape(-1)
    segs = _segments(seg_ends, len(post))
    mean = np.full(len(segs), np.nan)
    low = np.full(len(segs), np.nan)
    for i, a, b in segs:
        if b > a:
            mean[i] = post[a:b].mean()
            low[i] = post[a:b].min()
    return mean, low


# ------------------------------------------------------------------------------------------
# label occupancy posteriors and a differentiable lattice log-likelihood
# ------------------------------------------------------------------------------------------
def ctc_label_posteriors(log_probs, labels, terminal, beam_size=1000, max_move=4, band_lo=None):
    """Per-frame label posteriors of the band's paths that end at ``terminal``: (occ float32 [T, V], log_likelihood float).

    occ[t, v] is the probability that frame t emits label value v (blank = 0), over every path of the band of
    ``ctc_best_path`` that ends at state ``terminal`` (an int, or a best path whose last value is used); each row sums to 1 and
    occ equals d log_likelihood / d log_probs.  log_likelihood is the value ``ctc_path_posteriors`` returns for a path that
    ends there.  NumPy in -> NumPy out; ROCm torch tensors go to ``ctc_label_posteriors_device``.  Raises IndexError for a
    label outside [0, V), ValueError for NaN / +inf log-probs, a terminal outside [0, 2S+1) or one no finite path reaches.
    ``band_lo``: the band as a table [T], as ``ctc_path_posteriors`` takes it.
    """
    call = ctc_label_posteriors_device if _is_tensor(log_probs) else ctc_label_posteriors_batch
    (result,) = call([log_probs], [labels], [terminal], beam_size, max_move, band_lo=_one_table(band_lo))
    return result


def _label_posteriors(lat, terminals, beam_size, max_move, out, return_status, band_lo=None):
    if lat is None:
        return ([], []) if return_status else []
    occs = _outputs(lat, out, [(T, lat.V) for T in lat.T], "[T_i, V]")
    p_term, _k1 = _i64_array([_terminal_of(s) for s in terminals])
    p_occ, _k2 = _ptr_array([lat.ptr(x) for x in occs])
    p_ldo, _k3 = _i64_array([lat.ld(x) for x in occs])
    return _run_lattices(lat, "label_posteriors", beam_size, max_move, (p_term, p_occ, p_ldo), list(zip(occs)), return_status,
                         band_lo)


def ctc_label_posteriors_batch(log_probs_list, labels_list, terminals, beam_size=1000, max_move=4, device=None, return_status=False,
                               band_lo=None):
    """Label posteriors of many lattices in ONE launch; host NumPy buffers in and out.

    Returns a list of (occ [T_i, V], log_likelihood); with ``return_status`` also the per-lattice status list, in which case
    failures do not raise (their rows are NaN, their log-likelihood NaN, or -inf for KA_ERR_ZERO_MASS).
    ``band_lo``: a list of tables, one per lattice (``ctc_path_posteriors``).
    """
    lat = _host_lattices(log_probs_list, labels_list, terminals, "terminals", device)
    return _label_posteriors(lat, terminals, beam_size, max_move, None, return_status, band_lo)


def ctc_label_posteriors_device(log_probs, labels, terminals, beam_size=1000, max_move=4, out=None, return_status=False, band_lo=None):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V] with unit column stride, labels [S_i]) and terminals (ints
    or best paths), list of (occ tensor [T_i, V] on the device, log_likelihood float) out.  ``out``: optional list of float32
    [T_i, V] tensors with unit column stride to write into (views into wider tensors keep their other columns).  One launch
    on torch's current stream.  ``band_lo``: a list of tables, one per lattice, tensors on the device or host arrays."""
    lat = _device_lattices(log_probs, labels, terminals, "terminals")
    return _label_posteriors(lat, terminals, beam_size, max_move, out, return_status, band_lo)


def _lattice_ll_function():
    import torch

    class LatticeLogLikelihood(torch.autograd.Function):
        """Z of every lattice (float64 [n]); backward: grad_out[i] * occ_i, the occupancy saved by forward."""

        @staticmethod
        def forward(ctx, labels, terminals, beam_size, max_move, zero_infinity, band_lo, *lps):
            n = len(lps)
            if lps[0].is_cuda:
                res, st = ctc_label_posteriors_device([x.detach() for x in lps], labels, terminals, beam_size, max_move,
                                                      return_status=True, band_lo=band_lo)
            else:
                res, st = ctc_label_posteriors_batch([x.detach().float().numpy() for x in lps], labels, terminals, beam_size,
                                                     max_move, return_status=True, band_lo=band_lo)
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
            return (None, None, None, None, None, None, *grads)

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
        raise ValueError(f"{what}: terminal outside [0, 2S+1), or band_lo not non-decreasing in [0, 2S+1)")
    if st == _lib.KA_ERR_ZERO_MASS:
        raise ValueError(f"{what}: no path of finite score reaches the terminal")
    raise _lib.KAError(f"{what}: status {st}")


def lattice_log_likelihood(log_probs, labels, terminal, beam_size=1000, max_move=4, zero_infinity=False, band_lo=None):
    """Differentiable log-likelihood Z of the band's paths that end at ``terminal`` (this engine's topology: band, moves,
    label-0 veto), float64 on the input's device.  One [T, V] tensor (labels, terminal for it) -> 0-d; a list of them (lists
    of labels and terminals) -> [n].  The gradient with respect to the log-probs is the label occupancy (``ctc_label_posteriors``)
    times the incoming gradient; the forward pass saves it, so backward launches nothing.  With ``zero_infinity``, a lattice
    whose terminal no finite path reaches gives 0 and a zero gradient (as ``torch.nn.CTCLoss``); otherwise, and for every
    other failure, this raises as ``ctc_label_posteriors`` does.  ``band_lo``: the band as a table (one for one tensor, a list
    for a list), as ``ctc_label_posteriors`` takes it; value and gradient are then those of that band."""
    global _LATTICE_LL
    if _LATTICE_LL is None:
        _LATTICE_LL = _lattice_ll_function()
    single = _is_tensor(log_probs)
    lps = [log_probs] if single else list(log_probs)
    labs = [labels] if single else list(labels)
    terms = [terminal] if single else list(terminal)
    if len(lps) == 0 or len(labs) != len(lps) or len(terms) != len(lps):
        raise ValueError("log_probs, labels and terminals must be non-empty lists of one length")
    bands = None if band_lo is None else ([band_lo] if single else list(band_lo))
    z = _LATTICE_LL.apply(labs, [_terminal_of(s) for s in terms], int(beam_size), int(max_move), bool(zero_infinity), bands, *lps)
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
    segs = _segments(seg_ends, T)
    mean = np.full(len(segs), np.nan)
    for i, a, b in segs:
        if b > a:
            mean[i] = agree[a:b].mean()
    return mean


# ------------------------------------------------------------------------------------------
# state posteriors at chosen frames and the confidence of align()'s text boundaries
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


def ctc_state_posteriors(log_probs, labels, terminal, frames, beam_size=1000, max_move=4, band_lo=None):
    """Posterior of every band position at chosen frames: (gamma float32 [K, W], band_lo int64 [K], log_likelihood float).

    gamma[k, j] is the probability that frame ``frames[k]`` sits at state band_lo[k] + j, over every path of the band of
    ``ctc_best_path`` that ends at state ``terminal`` (an int, or a best path whose last value is used); columns past the
    band's width are 0, each row sums to 1.  W = min(beam_size, 2S+1).  ``frames``: strictly increasing in [0, T).
    NumPy in -> NumPy out; ROCm torch tensors go to ``ctc_state_posteriors_device``.  Raises as ``ctc_label_posteriors``,
    and ValueError for bad frames.  ``band_lo``: the band as a table [T], as ``ctc_path_posteriors`` takes it; the band_lo
    returned then holds the table's values at ``frames``.
    """
    call = ctc_state_posteriors_device if _is_tensor(log_probs) else ctc_state_posteriors_batch
    (result,) = call([log_probs], [labels], [terminal], [frames], beam_size, max_move, band_lo=_one_table(band_lo))
    return result


def _state_posteriors(lat, terminals, frames, beam_size, max_move, out, return_status, band_lo=None):
    if lat is None:
        return ([], []) if return_status else []
    if len(frames) != lat.n:
        raise ValueError("frames must hold one list per lattice")
    frames = [_frames_of(f, T) for f, T in zip(frames, lat.T)]      # (host memory in both forms)
    Ws = [_band_width(S, beam_size) for S in lat.S]
    gammas = _outputs(lat, out, [(len(f), W) for f, W in zip(frames, Ws)], "[K_i, W_i]")
    los = [lat.empty(len(f), np.int64) for f in frames]
    p_term, _k1 = _i64_array([_terminal_of(s) for s in terminals])
    p_fr, _k2 = _ptr_array([f.ctypes.data for f in frames])
    p_K, _k3 = _i64_array([len(f) for f in frames])
    p_g, _k4 = _ptr_array([lat.ptr(g) for g in gammas])
    p_ldo, _k5 = _i64_array([max(lat.ld(g), W) for g, W in zip(gammas, Ws)])   # (a tensor with no rows may report any stride)
    p_lo, _k6 = _ptr_array([lat.ptr(x) for x in los])
    return _run_lattices(lat, "state_posteriors", beam_size, max_move, (p_term, p_fr, p_K, p_g, p_ldo, p_lo), list(zip(gammas, los)),
                         return_status, band_lo)


def ctc_state_posteriors_batch(log_probs_list, labels_list, terminals, frames_list, beam_size=1000, max_move=4, device=None,
                               return_status=False, band_lo=None):
    """State posteriors of many lattices in ONE launch; host NumPy buffers in and out.

    Returns a list of (gamma [K_i, W_i], band_lo [K_i], log_likelihood); with ``return_status`` also the per-lattice status
    list, in which case failures do not raise (their rows are NaN, band_lo -1, their log-likelihood NaN, or -inf for
    KA_ERR_ZERO_MASS).  ``band_lo``: a list of tables, one per lattice (``ctc_path_posteriors``).
    """
    lat = _host_lattices(log_probs_list, labels_list, terminals, "terminals", device)
    return _state_posteriors(lat, terminals, frames_list, beam_size, max_move, None, return_status, band_lo)


def ctc_state_posteriors_device(log_probs, labels, terminals, frames, beam_size=1000, max_move=4, out=None, return_status=False,
                                band_lo=None):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V] with unit column stride, labels [S_i]), terminals (ints or
    best paths) and host frame lists (strictly increasing in [0, T_i)); list of (gamma tensor [K_i, W_i], band_lo int64 tensor
    [K_i], both on the device, log_likelihood float) out, W_i = min(beam_size, 2 S_i + 1).  ``out``: optional list of float32
    [K_i, W_i] tensors with unit column stride to write gamma into (views into wider tensors keep their other columns).  One
    launch on torch's current stream.  ``band_lo``: a list of tables, one per lattice, tensors on the device or host arrays."""
    lat = _device_lattices(log_probs, labels, terminals, "terminals")
    return _state_posteriors(lat, terminals, frames, beam_size, max_move, out, return_status, band_lo)


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

    segs = _segments(np.asarray(seg_ends, dtype=np.int64), T)
    p_start = np.empty(len(segs))
    p_end = np.empty(len(segs))
    for i, a, b in segs:                                # (b is clipped to T: b < T is seg_ends[i] < T)
        p_start[i] = p_at(a)
        p_end[i] = p_at(b) if b < T else 1.0
    return p_start, p_end


# ------------------------------------------------------------------------------------------
# expected state durations and the expected frame of every text boundary
# ------------------------------------------------------------------------------------------
def ctc_state_durations(log_probs, labels, terminal, beam_size=1000, max_move=4, band_lo=None):
    """How long the model expects every state to last: (duration float64 [L], time_sum float64 [L], log_likelihood float),
    L = 2S+1 positions of the blank-expanded labels (odd position 2i+1: phoneme i, even positions: the blanks around them).

    duration[s] is the expected number of frames spent in state s and time_sum[s] the expected sum of those frames' indices
    (time_sum / duration: the state's expected centre frame), over every path of the band of ``ctc_best_path`` that ends at
    state ``terminal`` (an int, or a best path whose last value is used): the state posteriors of ``ctc_state_posteriors``
    summed over all T frames, without the [T, W] matrix.  duration sums to T.  NumPy in -> NumPy out; ROCm torch tensors go
    to ``ctc_state_durations_device``.  Raises as ``ctc_label_posteriors``.  ``band_lo``: the band as a table [T], as
    ``ctc_path_posteriors`` takes it; a position no frame's band holds has duration 0.
    """
    call = ctc_state_durations_device if _is_tensor(log_probs) else ctc_state_durations_batch
    (result,) = call([log_probs], [labels], [terminal], beam_size, max_move, band_lo=_one_table(band_lo))
    return result


def _state_pairs(call, pair, lat, terminals, beam_size, max_move, out, return_status, band_lo=None):
    """The calls that write two float64 [2S+1] arrays per lattice, ``pair`` their names: "state_durations" and "state_visits"."""
    if lat is None:
        return ([], []) if return_status else []
    Ls = [2 * S + 1 for S in lat.S]
    if out is None:
        sums = [lat.empty(L, np.float64) for L in Ls]
        moments = [lat.empty(L, np.float64) for L in Ls]
    else:
        import torch
        if len(out) != lat.n or any(len(o) != 2 for o in out):
            raise ValueError(f"out must hold one ({pair[0]}, {pair[1]}) pair of tensors per lattice")
        for o, L in zip(out, Ls):
            if any(x.dtype != torch.float64 or tuple(x.shape) != (L,) or not x.is_contiguous() or x.device != lat.dev for x in o):
                raise ValueError("out tensors must be contiguous float64 [2 S_i + 1] on the input's device")
        sums, moments = [o[0] for o in out], [o[1] for o in out]
    p_term, _k1 = _i64_array([_terminal_of(s) for s in terminals])
    p_sum, _k2 = _ptr_array([lat.ptr(x) for x in sums])
    p_mom, _k3 = _ptr_array([lat.ptr(x) for x in moments])
    return _run_lattices(lat, call, beam_size, max_move, (p_term, p_sum, p_mom), list(zip(sums, moments)), return_status, band_lo)


def ctc_state_durations_batch(log_probs_list, labels_list, terminals, beam_size=1000, max_move=4, device=None, return_status=False,
                              band_lo=None):
    """State durations of many lattices in ONE launch; host NumPy buffers in and out.

    Returns a list of (duration [L_i], time_sum [L_i], log_likelihood); with ``return_status`` also the per-lattice status
    list, in which case failures do not raise (their arrays are NaN, their log-likelihood NaN, or -inf for KA_ERR_ZERO_MASS).
    ``band_lo``: a list of tables, one per lattice (``ctc_path_posteriors``).
    """
    lat = _host_lattices(log_probs_list, labels_list, terminals, "terminals", device)
    return _state_pairs("state_durations", ("duration", "time_sum"), lat, terminals, beam_size, max_move, None, return_status, band_lo)


def ctc_state_durations_device(log_probs, labels, terminals, beam_size=1000, max_move=4, out=None, return_status=False, band_lo=None):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V] with unit column stride, labels [S_i]) and terminals (ints
    or best paths), list of (duration, time_sum: float64 tensors [2 S_i + 1] on the device, log_likelihood float) out.
    ``out``: optional list of (duration, time_sum) pairs of contiguous float64 tensors to write into.  One launch on torch's
    current stream.  ``band_lo``: a list of tables, one per lattice, tensors on the device or host arrays."""
    lat = _device_lattices(log_probs, labels, terminals, "terminals")
    return _state_pairs("state_durations", ("duration", "time_sum"), lat, terminals, beam_size, max_move, out, return_status, band_lo)


def _host_f64(x):
    return np.asarray(x.detach().cpu() if _is_tensor(x) else x, dtype=np.float64).reshape(-1)


def phoneme_durations(duration):
    """(labels [S], blanks [S+1]) from ``ctc_state_durations``' duration [2S+1]: the expected frames of every phoneme (the odd
    positions) and of the blanks before, between and after them (the even ones).  float64 arrays (host)."""
    d = _host_f64(duration)
    if len(d) % 2 == 0:
        raise ValueError("duration must have 2S+1 entries")
    return d[1::2].copy(), d[0::2].copy()


def expected_crossing_frames(duration, cuts):
    """E[tau_c] for every cut position c in ``cuts`` (each in [0, L]), tau_c the first frame whose state is >= c.  Paths only
    move up, so state_t < c exactly for t < tau_c and E[tau_c] = sum_t P(state_t < c) = sum of duration[s] over s < c: the
    prefix sum of ``duration`` read at c (0 for c = 0, T for c = L).  float64 array (host)."""
    d = _host_f64(duration)
    c = np.asarray(cuts.detach().cpu() if _is_tensor(cuts) else cuts, dtype=np.int64).reshape(-1)
    if len(c) and (c.min() < 0 or c.max() > len(d)):
        raise ValueError(f"cuts must lie in [0, {len(d)}]")
    return np.concatenate([np.zeros(1), np.cumsum(d)])[c]


def segment_boundary_shift(duration, best_path, seg_ends, n_phonemes):
    """How far, in frames, the lattice expects each text boundary of ``align()`` from where the best path puts it (host only).

    For every boundary frame b that ``align()`` reads the best path at - ``boundary_frames(seg_ends, T)``: 0 and every
    seg_ends[i] < T - the text index is i = min(best_path[b] // 2, n_phonemes) and the cut position c = 2 i.  The best
    path's crossing frame is the first t with best_path[t] >= c; the expected one is E[tau_c] of
    ``expected_crossing_frames``.  shift = E[tau_c] - that frame: positive where the lattice expects the boundary later than
    the best path crosses it.  Returns (start_shift, end_shift), float64 per segment that ``align()`` writes a line for
    (frames [a, b), a = seg_ends[i-1], 0 for the first, b = seg_ends[i]): the shift of the boundary read at a and of the one
    read at b, the latter 0 where b >= T - there ``align()`` runs the text to its end whatever the path does."""
    d = _host_f64(duration)
    path = np.asarray(best_path.detach().cpu() if _is_tensor(best_path) else best_path, dtype=np.int64).reshape(-1)
    T, n_ph = len(path), int(n_phonemes)
    prefix = np.concatenate([np.zeros(1), np.cumsum(d)])
    reached = np.maximum.accumulate(path) if T else path      # (a best path never moves down; any other path: its running maximum)
    shift = {}
    for b in boundary_frames(seg_ends, T):
        c = 2 * min(int(path[b]) // 2, n_ph)
        if c > len(d):
            raise ValueError("segment_boundary_shift: a best-path position outside the duration's positions")
        shift[int(b)] = float(prefix[c]) - float(np.searchsorted(reached, c, side="left"))
    segs = _segments(np.asarray(seg_ends, dtype=np.int64), T)
    start = np.array([shift[a] if a < T else 0.0 for _, a, _ in segs], dtype=np.float64)
    end = np.array([shift[b] if b < T else 0.0 for _, _, b in segs], dtype=np.float64)   # (b is clipped to T: b < T is seg_ends[i] < T)
    return start, end


# ------------------------------------------------------------------------------------------
# state visit probabilities: which phonemes the path passes through at all
# ------------------------------------------------------------------------------------------
def ctc_state_visits(log_probs, labels, terminal, beam_size=1000, max_move=4, band_lo=None):
    """Which states the audio really holds: (visit float64 [L], exit_time float64 [L], log_likelihood float), L = 2S+1
    positions of the blank-expanded labels (odd position 2i+1: phoneme i, even positions: the blanks around them).

    visit[s] = V(s) = sum_t exit_t(s) is the probability that a path passes through state s at all, exit_t(s) the posterior
    probability of being in s at frame t and not at t+1, and exit_time[s] = X(s) = sum_t t exit_t(s) is its unnormalised first
    time moment (exit_time / visit: the state's expected last frame, given that it is visited), over every path of the band of ``ctc_best_path`` that ends at state ``terminal`` (an int, or a best path whose last value is
    used).  With ``max_move`` > 2 a path may jump over a phoneme; a phoneme the reader did not say shows as a low visit[2i+1].
    visit <= duration of ``ctc_state_durations`` position by position, and visit[terminal] is 1.  NumPy in -> NumPy out;
    ROCm torch tensors go to ``ctc_state_visits_device``.  Raises as ``ctc_label_posteriors``.  ``band_lo``: the band as a
    table [T], as ``ctc_path_posteriors`` takes it; a position no band holds, or below band_lo[0], has visit 0.
    """
    call = ctc_state_visits_device if _is_tensor(log_probs) else ctc_state_visits_batch
    (result,) = call([log_probs], [labels], [terminal], beam_size, max_move, band_lo=_one_table(band_lo))
    return result


def ctc_state_visits_batch(log_probs_list, labels_list, terminals, beam_size=1000, max_move=4, device=None, return_status=False,
                           band_lo=None):
    """State visit probabilities of many lattices in ONE launch; host NumPy buffers in and out.

    Returns a list of (visit [L_i], exit_time [L_i], log_likelihood); with ``return_status`` also the per-lattice status
    list, in which case failures do not raise (their arrays are NaN, their log-likelihood NaN, or -inf for KA_ERR_ZERO_MASS).
    ``band_lo``: a list of tables, one per lattice (``ctc_path_posteriors``).
    """
    lat = _host_lattices(log_probs_list, labels_list, terminals, "terminals", device)
    return _state_pairs("state_visits", ("visit", "exit_time"), lat, terminals, beam_size, max_move, None, return_status, band_lo)


def ctc_state_visits_device(log_probs, labels, terminals, beam_size=1000, max_move=4, out=None, return_status=False, band_lo=None):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V] with unit column stride, labels [S_i]) and terminals (ints
    or best paths), list of (visit, exit_time: float64 tensors [2 S_i + 1] on the device, log_likelihood float) out.
    ``out``: optional list of (visit, exit_time) pairs of contiguous float64 tensors to write into.  One launch on torch's
    current stream.  ``band_lo``: a list of tables, one per lattice, tensors on the device or host arrays."""
    lat = _device_lattices(log_probs, labels, terminals, "terminals")
    return _state_pairs("state_visits", ("visit", "exit_time"), lat, terminals, beam_size, max_move, out, return_status, band_lo)


def phoneme_visits(visit):
    """(labels [S], blanks [S+1]) from ``ctc_state_visits``' visit [2S+1]: the probability that the path passes through every
    phoneme (the odd positions) and through the blanks before, between and after them (the even ones).  float64 arrays (host)."""
    v = _host_f64(visit)
    if len(v) % 2 == 0:
        raise ValueError("visit must have 2S+1 entries")
    return v[1::2].copy(), v[0::2].copy()


def phoneme_spans(visit, exit_time, duration):
    """(first, last), float64 [2S+1] (host): the expected first and last frame of every state, given that the path visits it.

    last = X / V with X = ``exit_time`` and V = ``visit`` of ``ctc_state_visits``.  On a path the frames spent in a state
    number last - first + 1, so with D = ``duration`` of ``ctc_state_durations`` on the same input E[first; visited] =
    X - D + V and first = (X - D + V) / V.  NaN where V == 0."""
    v, x, d = _host_f64(visit), _host_f64(exit_time), _host_f64(duration)
    if not (len(v) == len(x) == len(d)) or len(v) % 2 == 0:
        raise ValueError("visit, exit_time and duration must have the same 2S+1 entries")
    seen = v > 0
    first, last = np.full(len(v), np.nan), np.full(len(v), np.nan)
    last[seen] = x[seen] / v[seen]
    first[seen] = (x[seen] - d[seen] + v[seen]) / v[seen]
    return first, last


def segment_expected_match(visit, labels, best_path, seg_ends):
    """The soft form of the reference's keep-or-drop test of a segment (host only): (expected float64, count int64) per segment
    that ``align()`` writes a line for.

    For segment i (frames [a, b), a = seg_ends[i-1], 0 for the first, b = seg_ends[i]) ``align()`` writes the transcript's
    phonemes [text_start, text_end), text_start = min(best_path[a] // 2, S) and text_end = min(best_path[b] // 2, S), or S
    where b >= T.  count[i] is the number of k in that range with labels[k] != 0 and expected[i] the sum of visit[2k+1] over
    them, so expected / count stands where the reference asks whether the phonemes decoded from the segment's best path are
    more than 70 % of the transcript's.  visit[2k+1] is the probability of passing through phoneme k ANYWHERE in the audio,
    not within the segment's frames: a phoneme said, but outside [a, b), still counts."""
    v = _host_f64(visit)
    lab = np.asarray(labels.detach().cpu() if _is_tensor(labels) else labels, dtype=np.int64).reshape(-1)
    S = len(lab)
    if len(v) != 2 * S + 1:
        raise ValueError("visit must have 2S+1 entries for the S labels")
    path = np.asarray(best_path.detach().cpu() if _is_tensor(best_path) else best_path, dtype=np.int64).reshape(-1)
    T = len(path)
    segs = _segments(np.asarray(seg_ends, dtype=np.int64), T)
    expected, count = np.zeros(len(segs), np.float64), np.zeros(len(segs), np.int64)
    for i, a, b in segs:
        start = min(int(path[a]) // 2, S) if a < T else S
        end = min(int(path[b]) // 2, S) if b < T else S
        k = np.arange(start, max(start, end))
        k = k[lab[k] != 0]
        count[i] = len(k)
        expected[i] = v[2 * k + 1].sum()
    return expected, count


# ------------------------------------------------------------------------------------------
# exact boundary-time quantiles: the interval a text boundary lies in
# ------------------------------------------------------------------------------------------
MAX_LEVELS = 8
_LEVEL_MIN = 2.0 ** -10


def _levels_of(q):
    """The levels of a quantile call as float64, checked: 1 to 8 of them, strictly increasing in [2^-10, 1 - 2^-10]."""
    lv = np.ascontiguousarray(np.asarray(q, dtype=np.float64).reshape(-1))
    if not 1 <= len(lv) <= MAX_LEVELS:
        raise ValueError(f"q must hold 1 to {MAX_LEVELS} levels")
    if not np.all((lv >= _LEVEL_MIN) & (lv <= 1.0 - _LEVEL_MIN)) or np.any(np.diff(lv) <= 0):      # (a NaN fails the first test)
        raise ValueError("q must be strictly increasing in [2^-10, 1 - 2^-10]")
    return lv


def _cuts_of(cuts, S):
    """A cut list as int64 NumPy, checked: strictly increasing in [0, 2S+1]."""
    if _is_tensor(cuts):
        cuts = cuts.detach().cpu().numpy()
    c = np.ascontiguousarray(np.asarray(cuts).reshape(-1), dtype=np.int64)
    if len(c) and (c[0] < 0 or c[-1] > 2 * S + 1 or np.any(np.diff(c) <= 0)):
        raise ValueError(f"cuts must be strictly increasing in [0, {2 * S + 1}]")
    return c


def ctc_boundary_quantiles(log_probs, labels, terminal, cuts, q=(0.05, 0.5, 0.95), beam_size=1000, max_move=4, band_lo=None):
    """The interval every boundary lies in: (quantile int32 [K, M], log_likelihood float) for K cut positions and M levels.

    tau_c is the first frame whose state is >= c (``expected_crossing_frames``), over every path of the band of
    ``ctc_best_path`` that ends at state ``terminal`` (an int, or a best path whose last value is used).  quantile[k, m] is
    the q[m]-quantile of tau at ``cuts[k]``: the first frame t at which P(tau_c <= t) = sum of the state posteriors at
    positions >= c reaches q[m], and T if none does - so the cut lies in [quantile[k, 0], quantile[k, -1]] with probability
    about q[-1] - q[0].  This is the exact form of what ``segment_boundary_spread`` estimates from 64 sampled paths: the sum is
    taken in 32.32 fixed point over the rows ``ctc_state_posteriors`` would write, so it is reproducible bit for bit, and no
    [T, W] or [64, T] matrix exists.  ``cuts``: strictly increasing in [0, 2S+1] (``boundary_cuts``); ``q``: 1 to 8 levels,
    strictly increasing in [2^-10, 1 - 2^-10].  Rows and columns ascend.  NumPy in -> NumPy out; ROCm torch tensors go to
    ``ctc_boundary_quantiles_device``.  Raises as ``ctc_label_posteriors``, and ValueError for bad cuts or levels.
    ``band_lo``: the band as a table [T], as ``ctc_path_posteriors`` takes it; a cut at or below band_lo[0] then reads 0.
    """
    call = ctc_boundary_quantiles_device if _is_tensor(log_probs) else ctc_boundary_quantiles_batch
    (result,) = call([log_probs], [labels], [terminal], [cuts], q, beam_size, max_move, band_lo=_one_table(band_lo))
    return result


def _boundary_quantiles(lat, terminals, cuts, q, beam_size, max_move, out, return_status, band_lo=None):
    levels = _levels_of(q)
    if lat is None:
        return ([], []) if return_status else []
    if len(cuts) != lat.n:
        raise ValueError("cuts must hold one list per lattice")
    cuts = [_cuts_of(c, S) for c, S in zip(cuts, lat.S)]      # (host memory in both forms)
    M = len(levels)
    quants = _outputs(lat, out, [(len(c), M) for c in cuts], "[K_i, M]", np.int32)
    p_term, _k1 = _i64_array([_terminal_of(s) for s in terminals])
    p_cut, _k2 = _ptr_array([c.ctypes.data for c in cuts])
    p_K, _k3 = _i64_array([len(c) for c in cuts])
    p_q, _k4 = _ptr_array([lat.ptr(x) for x in quants])
    p_ld, _k5 = _i64_array([max(lat.ld(x), M) for x in quants])   # (a tensor with at most one row may report any stride)
    return _run_lattices(lat, "boundary_quantiles", beam_size, max_move, (p_term, p_cut, p_K, levels.ctypes.data, M, p_q, p_ld),
                         list(zip(quants)), return_status, band_lo)


def ctc_boundary_quantiles_batch(log_probs_list, labels_list, terminals, cuts_list, q=(0.05, 0.5, 0.95), beam_size=1000, max_move=4,
                                 device=None, return_status=False, band_lo=None):
    """Boundary quantiles of many lattices in ONE launch; host NumPy buffers in and out.  ``q`` is one list of levels for
    every lattice.

    Returns a list of (quantile [K_i, M], log_likelihood); with ``return_status`` also the per-lattice status list, in which
    case failures do not raise (their quantiles are -1, their log-likelihood NaN, or -inf for KA_ERR_ZERO_MASS).
    ``band_lo``: a list of tables, one per lattice (``ctc_path_posteriors``).
    """
    lat = _host_lattices(log_probs_list, labels_list, terminals, "terminals", device)
    return _boundary_quantiles(lat, terminals, cuts_list, q, beam_size, max_move, None, return_status, band_lo)


def ctc_boundary_quantiles_device(log_probs, labels, terminals, cuts, q=(0.05, 0.5, 0.95), beam_size=1000, max_move=4, out=None,
                                  return_status=False, band_lo=None):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V] with unit column stride, labels [S_i]), terminals (ints or
    best paths) and host cut lists (strictly increasing in [0, 2 S_i + 1]); list of (quantile int32 tensor [K_i, M] on the
    device, log_likelihood float) out.  ``out``: optional list of int32 [K_i, M] tensors with unit column stride to write into
    (views into wider tensors keep their other columns).  One launch on torch's current stream.  ``band_lo``: a list of tables,
    one per lattice, tensors on the device or host arrays."""
    lat = _device_lattices(log_probs, labels, terminals, "terminals")
    return _boundary_quantiles(lat, terminals, cuts, q, beam_size, max_move, out, return_status, band_lo)


def _boundary_cut(path, b, n_ph):
    return 2 * min(int(path[b]) // 2, n_ph)


def boundary_cuts(best_path, seg_ends, n_phonemes):
    """The cut positions of ``align()``'s text boundaries, sorted and unique (int64): for every boundary frame b of
    ``boundary_frames(seg_ends, T)`` the text index is i = min(best_path[b] // 2, n_phonemes) and the cut c = 2 i - the cuts
    of ``segment_boundary_shift``, as ``ctc_boundary_quantiles`` takes them."""
    path = np.asarray(best_path.detach().cpu() if _is_tensor(best_path) else best_path, dtype=np.int64).reshape(-1)
    n_ph = int(n_phonemes)
    return np.unique(np.array([_boundary_cut(path, b, n_ph) for b in boundary_frames(seg_ends, len(path))], dtype=np.int64))


def segment_boundary_interval(quantile, cuts, best_path, seg_ends, n_phonemes):
    """The quantile frames of every text boundary of ``align()`` (host only): (start_q [n_seg, M], end_q [n_seg, M]), int64 per
    segment that ``align()`` writes a line for (frames [a, b), a = seg_ends[i-1], 0 for the first, b = seg_ends[i]): the
    quantiles of the boundary read at a and of the one read at b, laid out as ``segment_boundary_spread``'s.  ``quantile`` and
    ``cuts`` are those of ``ctc_boundary_quantiles`` (``boundary_cuts``, or any list that holds them).  Where b >= T
    ``align()`` runs the text to its end whatever the path does: the quantiles are T.  Raises ValueError if a cut it needs is
    not in ``cuts``."""
    qt = np.asarray(quantile.detach().cpu() if _is_tensor(quantile) else quantile, dtype=np.int64)
    c = np.asarray(cuts.detach().cpu() if _is_tensor(cuts) else cuts, dtype=np.int64).reshape(-1)
    if qt.ndim != 2 or qt.shape[0] != len(c):
        raise ValueError("quantile must be [len(cuts), M]")
    path = np.asarray(best_path.detach().cpu() if _is_tensor(best_path) else best_path, dtype=np.int64).reshape(-1)
    T, n_ph = len(path), int(n_phonemes)
    row_of = {int(v): k for k, v in enumerate(c)}
    at_end = np.full(qt.shape[1], T, dtype=np.int64)

    def rows(b):
        if b >= T:
            return at_end
        k = row_of.get(_boundary_cut(path, b, n_ph))
        if k is None:
            raise ValueError(f"segment_boundary_interval: cut {_boundary_cut(path, b, n_ph)} (frame {int(b)}) is not among the cuts")
        return qt[k]

    segs = _segments(np.asarray(seg_ends, dtype=np.int64), T)
    stack = lambda r: np.array(r, dtype=np.int64).reshape(len(r), qt.shape[1])
    return stack([rows(a) for _, a, _ in segs]), stack([rows(b) for _, _, b in segs])


# ------------------------------------------------------------------------------------------
# alignments sampled from the band posterior, and the spread of every text boundary
# ------------------------------------------------------------------------------------------
MAX_SAMPLES = 64


def ctc_sample_paths(log_probs, labels, terminal, n_samples=64, seed=0, beam_size=1000, max_move=4, band_lo=None):
    """Whole alignments drawn from the posterior over the band's paths: (paths int32 [n_samples, T], log_likelihood float).

    Row k is one path of the band of ``ctc_best_path`` that ends at state ``terminal`` (an int, or a best path whose last
    value is used), drawn with probability proportional to its score - its share of the lattice likelihood - by forward
    filtering and backward sampling; paths[k, t] is its position in the blank-expanded labels at frame t.  Any statistic of a
    path (a boundary's spread, a segment's duration, whether two cuts move together) is a sample statistic of the rows.
    Sample k depends on ``seed`` and k alone: it has the same bits whatever ``n_samples`` is, and whether the lattice is sent
    alone or in a batch.  One call draws at most 64 samples; more are the caller's loop over seeds (each seed gives 64 fresh,
    independent paths).  NumPy in -> NumPy out; ROCm torch tensors go to ``ctc_sample_paths_device``.  Raises as
    ``ctc_label_posteriors``, and ValueError for ``n_samples`` outside [1, 64].  ``band_lo``: the band as a table [T], as
    ``ctc_path_posteriors`` takes it: every row is then a path of that band.
    """
    call = ctc_sample_paths_device if _is_tensor(log_probs) else ctc_sample_paths_batch
    (result,) = call([log_probs], [labels], [terminal], n_samples, seed, beam_size, max_move, band_lo=_one_table(band_lo))
    return result


def _per_lattice(x, n, what):
    """An int for every lattice, or one per lattice."""
    xs = [int(x)] * n if np.ndim(x) == 0 else [int(v) for v in x]
    if len(xs) != n:
        raise ValueError(f"{what} must be an int or hold one per lattice")
    return xs


def _sample_paths(lat, terminals, n_samples, seed, beam_size, max_move, out, return_status, band_lo=None):
    if lat is None:
        return ([], []) if return_status else []
    Ks = _per_lattice(n_samples, lat.n, "n_samples")
    seeds = [v & 0xFFFFFFFFFFFFFFFF for v in _per_lattice(seed, lat.n, "seed")]
    if any(K < 1 or K > MAX_SAMPLES for K in Ks):
        raise ValueError(f"n_samples must lie in [1, {MAX_SAMPLES}]: draw more with further seeds")
    paths = _outputs(lat, out, [(K, T) for K, T in zip(Ks, lat.T)], "[n_samples_i, T_i]", np.int32)
    p_term, _k1 = _i64_array([_terminal_of(s) for s in terminals])
    a_K = np.asarray(Ks, np.int32)
    a_seed = np.asarray(seeds, np.uint64)
    p_paths, _k2 = _ptr_array([lat.ptr(x) for x in paths])
    p_ld, _k3 = _i64_array([max(lat.ld(x), T) for x, T in zip(paths, lat.T)])   # (a tensor with one row may report any stride)
    return _run_lattices(lat, "sample_paths", beam_size, max_move, (p_term, a_K.ctypes.data, a_seed.ctypes.data, p_paths, p_ld),
                         list(zip(paths)), return_status, band_lo)


def ctc_sample_paths_batch(log_probs_list, labels_list, terminals, n_samples=64, seed=0, beam_size=1000, max_move=4, device=None,
                           return_status=False, band_lo=None):
    """Sampled paths of many lattices in ONE launch; host NumPy buffers in and out.  ``n_samples`` and ``seed``: an int for
    every lattice, or one per lattice.

    Returns a list of (paths [n_samples_i, T_i], log_likelihood); with ``return_status`` also the per-lattice status list, in
    which case failures do not raise (their paths are -1, their log-likelihood NaN, or -inf for KA_ERR_ZERO_MASS).
    ``band_lo``: a list of tables, one per lattice (``ctc_path_posteriors``).
    """
    lat = _host_lattices(log_probs_list, labels_list, terminals, "terminals", device)
    return _sample_paths(lat, terminals, n_samples, seed, beam_size, max_move, None, return_status, band_lo)


def ctc_sample_paths_device(log_probs, labels, terminals, n_samples=64, seed=0, beam_size=1000, max_move=4, out=None, return_status=False,
                            band_lo=None):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V] with unit column stride, labels [S_i]) and terminals (ints
    or best paths), list of (paths int32 tensor [n_samples_i, T_i] on the device, log_likelihood float) out.  ``n_samples``
    and ``seed``: an int for every lattice, or one per lattice.  ``out``: optional list of int32 [n_samples_i, T_i] tensors
    with unit column stride to write into (views into wider tensors keep their other columns).  One launch on torch's current
    stream.  ``band_lo``: a list of tables, one per lattice, tensors on the device or host arrays."""
    lat = _device_lattices(log_probs, labels, terminals, "terminals")
    return _sample_paths(lat, terminals, n_samples, seed, beam_size, max_move, out, return_status, band_lo)


def _host_paths(paths):
    p = np.asarray(paths.detach().cpu() if _is_tensor(paths) else paths, dtype=np.int64)
    if p.ndim != 2:
        raise ValueError("paths must be [n_samples, T]")
    return p


def sampled_crossing_frames(paths, cuts):
    """tau_c of every sampled path for every cut position c in ``cuts``: the first frame whose state is >= c, and T if there
    is none - the tau_c of ``expected_crossing_frames``, whose value is the mean of a column here.  int64 [K, len(cuts)]
    (host)."""
    p = _host_paths(paths)
    c = np.asarray(cuts.detach().cpu() if _is_tensor(cuts) else cuts, dtype=np.int64).reshape(-1)
    reached = np.maximum.accumulate(p, axis=1) if p.shape[1] else p      # (a path never moves down: state_t < c exactly for t < tau_c)
    return np.sum(reached[:, :, None] < c[None, None, :], axis=1, dtype=np.int64)


def segment_boundary_spread(paths, best_path, seg_ends, n_phonemes, q=(0.05, 0.5, 0.95)):
    """How widely the lattice spreads each text boundary of ``align()``, from sampled paths (host only): the sample quantiles
    and the standard deviation of tau_c, the number the closed form of ``segment_boundary_shift`` cannot give.

    The cuts are those of ``segment_boundary_shift``: for every boundary frame b of ``boundary_frames(seg_ends, T)`` the text
    index is i = min(best_path[b] // 2, n_phonemes) and the cut c = 2 i; tau_c of a sample is ``sampled_crossing_frames``.
    Returns (start_quantiles [n_seg, len(q)], start_std [n_seg], end_quantiles [n_seg, len(q)], end_std [n_seg]), float64 per
    segment that ``align()`` writes a line for (frames [a, b), a = seg_ends[i-1], 0 for the first, b = seg_ends[i]): the
    boundary read at a and the one read at b.  Where b >= T ``align()`` runs the text to its end whatever the path does: the
    quantiles are T and the deviation 0."""
    p = _host_paths(paths)
    path = np.asarray(best_path.detach().cpu() if _is_tensor(best_path) else best_path, dtype=np.int64).reshape(-1)
    T, n_ph = len(path), int(n_phonemes)
    if p.shape[1] != T:
        raise ValueError("segment_boundary_spread: paths and best_path must have one position per frame")
    qs = np.asarray(q, dtype=np.float64).reshape(-1)
    frames = boundary_frames(seg_ends, T)
    cuts = np.array([2 * min(int(path[b]) // 2, n_ph) for b in frames], dtype=np.int64)
    tau = sampled_crossing_frames(p, cuts).astype(np.float64)          # [K, boundaries]
    col = {int(b): k for k, b in enumerate(frames)}
    at_end = (np.full(len(qs), float(T)), 0.0)

    def spread(b):
        if b >= T:
            return at_end
        x = tau[:, col[int(b)]]
        return np.quantile(x, qs), float(np.std(x))

    segs = _segments(np.asarray(seg_ends, dtype=np.int64), T)
    start = [spread(a) for _, a, _ in segs]
    end = [spread(b) for _, _, b in segs]
    stack = lambda rows: np.array([r[0] for r in rows], dtype=np.float64).reshape(len(rows), len(qs))
    return (stack(start), np.array([r[1] for r in start], dtype=np.float64), stack(end), np.array([r[1] for r in end], dtype=np.float64))


# ------------------------------------------------------------------------------------------
# the maximum-expected-accuracy alignment (posterior-decoded path), and where it leaves the best path
# ------------------------------------------------------------------------------------------
def ctc_mea_path(log_probs, labels, terminal, beam_size=1000, max_move=4, band_lo=None):
    """The alignment with the most frames at the right state in expectation: (path int32 [T], expected_accuracy float,
    log_likelihood float).

    Among the paths of the band of ``ctc_best_path`` that end at state ``terminal`` (an int, or a best path whose last value is
    used), ``path`` maximises the sum over the frames of the state posterior gamma_t(path[t]) of ``ctc_state_posteriors``,
    where the best path maximises the probability of the whole path; path[t] is its position in the blank-expanded labels.
    ``expected_accuracy`` is that sum - divided by T, the expected fraction of correctly placed frames, a one-number quality
    score of the lattice.  Ties go to the smallest move.  Equals the recursion run on ``ctc_state_posteriors`` at every frame
    bit for bit, without the [T, W] matrix.  NumPy in -> NumPy out; ROCm torch tensors go to ``ctc_mea_path_device``.  Raises
    as ``ctc_label_posteriors``.  ``band_lo``: the band as a table [T], as ``ctc_path_posteriors`` takes it: the path is then
    a path of that band (path[0] may lie above 0), decoded from that band's posteriors.
    """
    call = ctc_mea_path_device if _is_tensor(log_probs) else ctc_mea_path_batch
    (result,) = call([log_probs], [labels], [terminal], beam_size, max_move, band_lo=_one_table(band_lo))
    return result


def _mea_path(lat, terminals, beam_size, max_move, out, return_status, band_lo=None):
    if lat is None:
        return ([], []) if return_status else []
    if out is None:
        paths = [lat.empty(T, np.int32) for T in lat.T]
    else:
        import torch
        if len(out) != lat.n:
            raise ValueError("out must hold one tensor per lattice")
        for o, T in zip(out, lat.T):
            if o.dtype != torch.int32 or tuple(o.shape) != (T,) or not o.is_contiguous() or o.device != lat.dev:
                raise ValueError("out tensors must be contiguous int32 [T_i] on the input's device")
        paths = out
    ea = np.zeros(lat.n, np.float64)
    p_term, _k1 = _i64_array([_terminal_of(s) for s in terminals])
    p_path, _k2 = _ptr_array([lat.ptr(x) for x in paths])
    # (the expected accuracies are a host array the call fills: zipped as 0-d views, made floats once it has returned)
    got = _run_lattices(lat, "mea_path", beam_size, max_move, (p_term, p_path, ea.ctypes.data), list(zip(paths, ea.reshape(-1, 1))),
                        return_status, band_lo)
    results = [(p, float(v[0]), z) for p, v, z in (got[0] if return_status else got)]
    return (results, got[1]) if return_status else results


def ctc_mea_path_batch(log_probs_list, labels_list, terminals, beam_size=1000, max_move=4, device=None, return_status=False,
                       band_lo=None):
    """Maximum-expected-accuracy paths of many lattices in ONE launch; host NumPy buffers in and out.

    Returns a list of (path [T_i], expected_accuracy, log_likelihood); with ``return_status`` also the per-lattice status list,
    in which case failures do not raise (their paths are -1, their expected accuracy NaN, their log-likelihood NaN, or -inf for
    KA_ERR_ZERO_MASS).  ``band_lo``: a list of tables, one per lattice (``ctc_path_posteriors``).
    """
    lat = _host_lattices(log_probs_list, labels_list, terminals, "terminals", device)
    return _mea_path(lat, terminals, beam_size, max_move, None, return_status, band_lo)


def ctc_mea_path_device(log_probs, labels, terminals, beam_size=1000, max_move=4, out=None, return_status=False, band_lo=None):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V] with unit column stride, labels [S_i]) and terminals (ints
    or best paths), list of (path int32 tensor [T_i] on the device, expected_accuracy float, log_likelihood float) out.
    ``out``: optional list of contiguous int32 [T_i] tensors to write the paths into.  One launch on torch's current stream.
    ``band_lo``: a list of tables, one per lattice, tensors on the device or host arrays."""
    lat = _device_lattices(log_probs, labels, terminals, "terminals")
    return _mea_path(lat, terminals, beam_size, max_move, out, return_status, band_lo)


def path_outputs(log_probs, labels, path):
    """The (path, labels, scores) triple of ``ctc_best_path`` for any path over the blank-expanded labels (host only): path
    int32 [T], labels[t] = lab'[path[t]] int32, scores[t] = log_probs[t, labels[t]] float32.  Saved as
    ``np.savez(file, best_path=..., best_labels=..., best_scores=...)`` it is a ``best_path.npz`` that ``align()`` takes
    unchanged - e.g. for the path of ``ctc_mea_path``."""
    lp = np.asarray(log_probs.detach().cpu() if _is_tensor(log_probs) else log_probs, dtype=np.float32)
    lab = np.asarray(labels.detach().cpu() if _is_tensor(labels) else labels).reshape(-1)
    p = np.ascontiguousarray(np.asarray(path.detach().cpu() if _is_tensor(path) else path).reshape(-1), dtype=np.int32)
    expanded = np.zeros(2 * len(lab) + 1, np.int32)
    expanded[1::2] = lab
    if lp.ndim != 2 or len(p) != lp.shape[0]:
        raise ValueError("path_outputs: path must have one position per frame of log_probs [T, V]")
    if len(p) and (p.min() < 0 or p.max() >= len(expanded)):
        raise ValueError("path_outputs: a path position outside [0, 2S+1)")
    out_labels = expanded[p]
    return p, out_labels, np.ascontiguousarray(lp[np.arange(len(p)), out_labels], dtype=np.float32)


def segment_path_disagreement(best_path, mea_path, seg_ends, n_phonemes):
    """Where two alignments of one lattice - the best path and the path of ``ctc_mea_path`` - differ, per segment that
    ``align()`` writes a line for (host only): (boundary_shift int64 [boundaries], differing float64 [n_seg]).

    boundary_shift[k] belongs to frame b = ``boundary_frames(seg_ends, T)``[k]: with the cut of ``segment_boundary_shift``,
    c = 2 min(best_path[b] // 2, n_phonemes), it is the first frame at which ``mea_path`` reaches c minus the first frame at
    which ``best_path`` does (T for a path that never reaches it): positive where the posterior-decoded path crosses the text
    boundary later.  differing[i] is the share of the segment's frames [a, b) (a = seg_ends[i-1], 0 for the first,
    b = seg_ends[i], clipped to T) whose text index min(state // 2, n_phonemes) differs between the two paths; NaN for a
    segment without frames."""
    bp = np.asarray(best_path.detach().cpu() if _is_tensor(best_path) else best_path, dtype=np.int64).reshape(-1)
    mp = np.asarray(mea_path.detach().cpu() if _is_tensor(mea_path) else mea_path, dtype=np.int64).reshape(-1)
    T, n_ph = len(bp), int(n_phonemes)
    if len(mp) != T:
        raise ValueError("segment_path_disagreement: the two paths must have one position per frame")
    frames = boundary_frames(seg_ends, T)
    cuts = np.array([2 * min(int(bp[b]) // 2, n_ph) for b in frames], dtype=np.int64)
    both = sampled_crossing_frames(np.stack([bp, mp]), cuts) if T else np.zeros((2, len(cuts)), np.int64)
    differs = np.minimum(bp // 2, n_ph) != np.minimum(mp // 2, n_ph)
    segs = _segments(np.asarray(seg_ends, dtype=np.int64), T)
    share = np.full(len(segs), np.nan)
    for i, a, b in segs:
        if b > a:
            share[i] = differs[a:b].mean()
    return (both[1] - both[0]).astype(np.int64), share


# ------------------------------------------------------------------------------------------
# best-path margins from max-marginals: what the best alignment would lose if it had to be elsewhere
# ------------------------------------------------------------------------------------------
_MARGIN_UNITS = {"state": 0, "text": 1, 0: 0, 1: 1}


def ctc_path_margins(log_probs, labels, path, beam_size=1000, max_move=4, unit="state", band_lo=None, raw=False):
    """How far a path is ahead of the best alignment that disagrees with it, frame by frame: (margin float64 [T], runner_up
    int32 [T], score float).

    With m_t(s) the score of the best complete path of the band of ``ctc_best_path`` that is at state s in frame t and ends where
    ``path`` ends (the best path's own recurrence run forwards and backwards: adds and maxima only, float64, exact),
    margin[t] = m_t(path[t]) - max of m_t over the states of another group, runner_up[t] the lowest state attaining that maximum
    (-1 if there is none) and score the best path's score to path[T-1].  ``unit``: "state" - any other state - or "text" -
    another text index s // 2, which is what ``align()`` reads off the path at a segment's ends.  For a best path the margin
    is >= 0: the score it would lose if it had to be elsewhere at frame t.  Any path with values in [0, 2S+1) is legal; the
    margin is then signed.  It is +inf where no alternative exists and NaN where neither side has a path.  ``raw``: return
    (through, alt, runner_up, score), the two sides of the difference.  NumPy in -> NumPy out; ROCm torch tensors go to
    ``ctc_path_margins_device``.  Raises as ``ctc_path_posteriors``.  ``band_lo``: the band as a table [T], as
    ``ctc_best_path_banded`` takes it; None is the diagonal band of ``ctc_best_path``.
    """
    call = ctc_path_margins_device if _is_tensor(log_probs) else ctc_path_margins_batch
    (result,) = call([log_probs], [labels], [path], beam_size, max_move, unit, band_lo=_one_table(band_lo), raw=raw)
    return result


def _path_margins(lat, paths, beam_size, max_move, unit, return_status, band_lo, raw):
    if unit not in _MARGIN_UNITS:
        raise ValueError('unit must be "state" or "text"')
    if lat is None:
        return ([], []) if return_status else []
    paths = [lat.int32(x) for x in paths]
    if any(p.shape[0] != T for p, T in zip(paths, lat.T)):
        raise ValueError("a path must have one position per frame")
    p_band, _k0 = None, None
    if band_lo is not None:      # (an entry may be None: that lattice runs on the diagonal)
        if len(band_lo) != lat.n:
            raise ValueError("band_lo must hold one table (or None) per lattice")
        given = [i for i, b in enumerate(band_lo) if b is not None]
        sub = _Sub(lat, given)
        tables = dict(zip(given, _band_tables(sub, [band_lo[i] for i in given]))) if given else {}
        p_band, _k0 = _ptr_array([lat.ptr(tables[i]) if i in tables else None for i in range(lat.n)])
    through = [lat.empty(T, np.float64) for T in lat.T]
    alt = [lat.empty(T, np.float64) for T in lat.T]
    runner = [lat.empty(T, np.int32) for T in lat.T]
    p_path, _k1 = _ptr_array([lat.ptr(x) for x in paths])
    p_thr, _k2 = _ptr_array([lat.ptr(x) for x in through])
    p_alt, _k3 = _ptr_array([lat.ptr(x) for x in alt])
    p_run, _k4 = _ptr_array([lat.ptr(x) for x in runner])
    got = _run_lattices(lat, "path_margins", beam_size, max_move, (p_band, p_path, _MARGIN_UNITS[unit], p_thr, p_alt, p_run),
                        list(zip(through, alt, runner)), return_status)
    if not raw:     # through - alt: +inf where alt is -inf, NaN where both are (and for a failed lattice)
        def margin(th, al):
            if _is_tensor(th):
                return th - al
            with np.errstate(invalid="ignore"):
                return th - al
        results = [(margin(th, al), r, z) for th, al, r, z in (got[0] if return_status else got)]
        return (results, got[1]) if return_status else results
    return got


class _Sub:
    """The lattices ``given`` of a ``_Lattices``, as ``_band_tables`` reads them."""

    def __init__(self, lat, given):
        self.n, self.T, self.form, self.int32 = len(given), [lat.T[i] for i in given], lat.form, lat.int32


def ctc_path_margins_batch(log_probs_list, labels_list, path_list, beam_size=1000, max_move=4, unit="state", device=None,
                           return_status=False, band_lo=None, raw=False):
    """Margins of many lattices in ONE launch; host NumPy buffers in and out.

    Returns a list of (margin, runner_up, score), or of (through, alt, runner_up, score) with ``raw``; with ``return_status``
    also the per-lattice status list, in which case failures do not raise (their margins are NaN, their runner_up -1, their
    score NaN, or -inf for KA_ERR_ZERO_MASS).  ``band_lo``: a list with one table or None per lattice.
    """
    lat = _host_lattices(log_probs_list, labels_list, path_list, "paths", device)
    return _path_margins(lat, path_list, beam_size, max_move, unit, return_status, band_lo, raw)


def ctc_path_margins_device(log_probs, labels, paths, beam_size=1000, max_move=4, unit="state", return_status=False, band_lo=None,
                            raw=False):
    """Lists of ROCm torch tensors in (float32 log-probs [T_i, V], labels [S_i], paths [T_i] - e.g. the outputs of
    ``ctc_best_path_device``), list of (margin float64 tensor [T_i], runner_up int32 tensor [T_i], score float) out, on the
    device.  One launch on torch's current stream.  ``band_lo``: a list with one table (a tensor on the device or a host
    array) or None per lattice."""
    lat = _device_lattices(log_probs, labels, paths, "paths")
    return _path_margins(lat, paths, beam_size, max_move, unit, return_status, band_lo, raw)


def segment_boundary_margin(margin_text, seg_ends):
    """Per segment that ``align()`` writes a line for, how safe its two text boundaries are (host only): the smaller of the
    ``unit="text"`` margins at its first frame a (seg_ends[i-1], 0 for the first) and at the frame after its last, b =
    seg_ends[i]; a frame b >= T counts +inf, the convention of ``segment_boundary_confidence``.  float64 array."""
    m = np.asarray(margin_text.detach().cpu() if _is_tensor(margin_text) else margin_text, dtype=np.float64).reshape(-1)
    T = len(m)
    ends = np.asarray(seg_ends, dtype=np.int64).reshape(-1)
    out = np.empty(len(ends))
    for i in range(len(ends)):
        a, b = (int(ends[i - 1]) if i > 0 else 0), int(ends[i])
        at = [m[t] if t < T else np.inf for t in (a, b)]
        out[i] = np.nan if np.isnan(at).any() else min(at)
    return out


def segment_min_margin(margin, seg_ends):
    """Per segment that ``align()`` writes a line for, the smallest margin over its frames [a, b) (``_segments``); +inf for
    a segment without frames, NaN if one of its frames has none (host only).  float64 array."""
    m = np.asarray(margin.detach().cpu() if _is_tensor(margin) else margin, dtype=np.float64).reshape(-1)
    segs = _segments(np.asarray(seg_ends, dtype=np.int64), len(m))
    out = np.full(len(segs), np.inf)
    for i, a, b in segs:
        if b > a:
            out[i] = np.nan if np.isnan(m[a:b]).any() else m[a:b].min()
    return out


# ------------------------------------------------------------------------------------------
# forward-backward under the caller's boundary conditions: posteriors of a recording cut into chunks
# ------------------------------------------------------------------------------------------
_RESUME_ROWS = {True: (True, True), False: (False, False), "alpha": (True, False), "beta": (False, True)}


def free_end_scores(L):
    """The end row under which a path may end anywhere: ``L`` = 2S+1 zeros (float64).  Z is then the mass of the audio so far."""
    return np.zeros(int(L), np.float64)


def ctc_posteriors_resume(log_probs, labels, band_lo, alpha_in=None, end=None, path=None, occupancy=True, rows=True, beam_size=1000,
                          max_move=4):
    """Forward-backward over one chunk of a recording: (occ, path_post, alpha_out, beta_out, log_likelihood).

    The chunk's frames ``log_probs`` [T, V] run over the table ``band_lo`` [T] (required) from the row ``alpha_in`` (float64
    [2S+1], ln alpha of the row before the chunk's first frame, -inf = no mass; None: the virtual start state) to ``end``: an int,
    the terminal state, or a float64 row [2S+1], ln beta of the chunk's last frame (``free_end_scores``: the path may end
    anywhere).  ``alpha_out`` (ln alpha of the last frame over its band, -inf elsewhere) is the next chunk's ``alpha_in``;
    ``beta_out`` (ln beta of the row before the first frame) is the previous chunk's ``end``.  With both exchanged, occ and
    path_post of the chunks, concatenated, are the uncut recording's and every chunk's log_likelihood is the recording's.
    occ float32 [T, V] as ``ctc_label_posteriors`` (``occupancy=False``: None, and not computed); path_post float32 [T], the
    posterior of ``path[t]`` at frame t (None without ``path``); ``rows``: True, False, "alpha" or "beta" - which rows are
    returned (alpha_out and log_likelihood alone cost one forward pass).  NumPy in -> NumPy out; ROCm torch tensors go to
    ``ctc_posteriors_resume_device``.  Raises as ``ctc_label_posteriors``; a NaN or +inf in a row raises ValueError.
    """
    call = ctc_posteriors_resume_device if _is_tensor(log_probs) else ctc_posteriors_resume_batch
    (result,) = call([log_probs], [labels], [band_lo], None if alpha_in is None else [alpha_in], [end], None if path is None else [path],
                     occupancy, rows, beam_size, max_move)
    return result


def _row_f64(lat, x, L, what):
    """A row of a resumed call as the call wants it: float64 [L] where the lattices are."""
    if lat.form == "batch":
        if _is_tensor(x):
            x = x.detach().cpu().numpy()
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    else:
        import torch
        x = x if _is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float64).reshape(-1))
        x = x.reshape(-1).to(device=lat.dev, dtype=torch.float64).contiguous()
    if x.shape[0] != L:
        raise ValueError(f"{what} must have 2S+1 = {L} entries")
    return x


def _is_end_row(end):
    return _is_tensor(end) and end.dim() > 0 or not _is_tensor(end) and np.ndim(end) > 0


def _posteriors_resume(lat, band_lo, alpha_in, end, path, occupancy, rows, beam_size, max_move, return_status):
    if rows not in _RESUME_ROWS:
        raise ValueError('rows must be True, False, "alpha" or "beta"')
    want_a, want_b = _RESUME_ROWS[rows]
    n, Ls = lat.n, [2 * S + 1 for S in lat.S]
    for name, x in (("alpha_in", alpha_in), ("path", path)):
        if x is not None and len(x) != n:
            raise ValueError(f"{name} must hold one entry (or None) per lattice")
    if end is None or len(end) != n or any(e is None for e in end):
        raise ValueError("end must hold a terminal or an end row per lattice")
    tables = _band_tables(lat, band_lo)
    a_in = [None if alpha_in is None or alpha_in[i] is None else _row_f64(lat, alpha_in[i], Ls[i], "alpha_in") for i in range(n)]
    b_in = [_row_f64(lat, end[i], Ls[i], "an end row") if _is_end_row(end[i]) else None for i in range(n)]
    terms = [-1 if b_in[i] is not None else _terminal_of(end[i]) for i in range(n)]
    paths = [None if path is None or path[i] is None else lat.int32(path[i]) for i in range(n)]
    if any(p is not None and p.shape[0] != T for p, T in zip(paths, lat.T)):
        raise ValueError("a path must have one position per frame")
    occs = [lat.empty((T, lat.V), np.float32) if occupancy else None for T in lat.T]
    posts = [None if p is None else lat.empty(T, np.float32) for p, T in zip(paths, lat.T)]
    a_out = [lat.empty(L, np.float64) if want_a else None for L in Ls]
    b_out = [lat.empty(L, np.float64) if want_b else None for L in Ls]

    def ptrs(xs):
        return _ptr_array([None if x is None else lat.ptr(x) for x in xs])
    p_band, _k0 = ptrs(tables)
    p_ain, _k1 = ptrs(a_in)
    p_bin, _k2 = ptrs(b_in)
    p_term, _k3 = _i64_array(terms)
    p_path, _k4 = ptrs(paths)
    p_occ, _k5 = ptrs(occs)
    p_ldo, _k6 = _i64_array([lat.V if o is None else lat.ld(o) for o in occs])
    p_post, _k7 = ptrs(posts)
    p_aout, _k8 = ptrs(a_out)
    p_bout, _k9 = ptrs(b_out)
    return _run_lattices(lat, "posteriors_resume", beam_size, max_move,
                         (p_band, p_ain, p_bin, p_term, p_path, p_occ, p_ldo, p_post, p_aout, p_bout),
                         list(zip(occs, posts, a_out, b_out)), return_status)


def ctc_posteriors_resume_batch(log_probs_list, labels_list, band_lo, alpha_in=None, end=None, path=None, occupancy=True, rows=True,
                                beam_size=1000, max_move=4, device=None, return_status=False):
    """``ctc_posteriors_resume`` of many chunks in ONE launch; host NumPy buffers in and out.  ``band_lo`` and ``end`` hold one
    entry per lattice; ``alpha_in`` and ``path`` are None or lists in which any entry may be None.  Returns a list of (occ,
    path_post, alpha_out, beta_out, log_likelihood); with ``return_status`` also the per-lattice status list, in which case
    failures do not raise (every output of a failed lattice is NaN, rows included)."""
    lat = _host_lattices(log_probs_list, labels_list, band_lo, "tables", device)
    if lat is None:
        return ([], []) if return_status else []
    return _posteriors_resume(lat, band_lo, alpha_in, end, path, occupancy, rows, beam_size, max_move, return_status)


def ctc_posteriors_resume_device(log_probs, labels, band_lo, alpha_in=None, end=None, path=None, occupancy=True, rows=True,
                                 beam_size=1000, max_move=4, return_status=False):
    """``ctc_posteriors_resume_batch`` on lists of ROCm torch tensors: results and rows stay on the device (float64 rows), so
    that a chunk's rows reach its neighbour without a copy.  One launch on torch's current stream."""
    lat = _device_lattices(log_probs, labels, band_lo, "tables")
    return _posteriors_resume(lat, band_lo, alpha_in, end, path, occupancy, rows, beam_size, max_move, return_status)


def ctc_label_posteriors_chunked(log_probs, labels, band_lo, chunk_frames, terminal, path=None, beam_size=1000, max_move=4):
    """``ctc_label_posteriors(..., band_lo=)`` of a recording in the checkpoint workspace of one chunk: (occ float32 [T, V],
    path_post float32 [T] or None, log_likelihood).

    A forward-only sweep over chunks of ``chunk_frames`` frames keeps every chunk's start row (2S+1 doubles per chunk); the
    chunks are then visited newest first, each from its start row to the end row its successor handed back (the last one to
    ``terminal``).  By pass count that is one forward pass more than the uncut call.  NumPy in, NumPy out.
    """
    lp = np.asarray(log_probs)
    T = lp.shape[0]
    chunk = int(chunk_frames)
    if chunk < 1:
        raise ValueError("chunk_frames must be at least 1")
    band = np.asarray(band_lo).reshape(-1)
    if band.shape[0] != T:
        raise ValueError("a band table must have one entry per frame")
    pth = None if path is None else np.asarray(path).reshape(-1)
    if pth is not None and pth.shape[0] != T:
        raise ValueError("a path must have one position per frame")
    cuts = list(range(0, T, chunk)) + [T]
    starts, row = [], None
    for a, b in zip(cuts[:-2], cuts[1:-1]):      # forward only: the start row of every chunk but the first
        starts.append(row)
        _o, _p, row, _b, _z = ctc_posteriors_resume(lp[a:b], labels, band[a:b], row, free_end_scores(2 * len(np.asarray(labels).reshape(-1)) + 1),
                                                    None, False, "alpha", beam_size, max_move)
    starts.append(row)
    occ = np.empty((T, lp.shape[1]), np.float32)
    post = None if pth is None else np.empty(T, np.float32)
    end, z = _terminal_of(terminal), None
    for k in range(len(starts) - 1, -1, -1):     # newest first, with both rows
        a, b = cuts[k], cuts[k + 1]
        o, p, _a, end, zk = ctc_posteriors_resume(lp[a:b], labels, band[a:b], starts[k], end, None if pth is None else pth[a:b], True,
                                                  "beta" if k > 0 else False, beam_size, max_move)
        occ[a:b] = o
        if post is not None:
            post[a:b] = p
        z = zk if z is None else z
    return occ, post, z


# ------------------------------------------------------------------------------------------
# best-path margins under the caller's boundary conditions: margins of a recording cut into chunks, and rows of
# max-marginals at chosen frames
# ------------------------------------------------------------------------------------------
_MARGIN_ROWS = {True: (True, True), False: (False, False), "d": (True, False), "e": (False, True)}


def ctc_margins_resume(log_probs, labels, band_lo, path=None, d_in=None, end=None, unit="state", frames=None, rows=True, beam_size=1000,
                       max_move=4):
    """``ctc_path_margins`` over one chunk of a recording: (margin, runner_up, state_rows, rows_lo, d_out, e_out, score).

    The chunk's frames ``log_probs`` [T, V] run over the table ``band_lo`` [T] (None: the diagonal band) from the row ``d_in``
    (float64 [2S+1], the best score of every state of the row before the chunk's first frame, -inf = no path; None: the
    virtual start state) to ``end``: None (the last state of ``path``), an int, the terminal state, or a float64 row [2S+1],
    what a path that is at a state in the last frame still gains (``free_end_scores``: it may end anywhere).  ``d_out`` (the
    last frame's scores over its band, -inf elsewhere) is the next chunk's ``d_in``; ``e_out`` (the gain from the row before the
    first frame) is the previous chunk's ``end``.  With both exchanged the margins of the chunks, concatenated, are the uncut
    recording's bit for bit, and the last chunk's score is the recording's.  margin float64 [T] and runner_up int32 [T] as
    ``ctc_path_margins`` returns them (None without ``path``); ``frames`` (strictly increasing in [0, T)): state_rows float64
    [K, W] holds m at state rows_lo[k] + j of frame frames[k] (absolute: subtract ``score``), -inf past the band's width, W =
    min(beam_size, 2S+1); both None without ``frames``.  ``rows``: True, False, "d" or "e" - which rows are returned (d_out and
    score alone cost one forward pass).  All arithmetic is float64 adds and maxima: no tolerance applies anywhere.  NumPy in ->
    NumPy out; ROCm torch tensors go to ``ctc_margins_resume_device``.  Raises as ``ctc_path_margins``; a NaN or +inf in a row
    raises ValueError.
    """
    call = ctc_margins_resume_device if _is_tensor(log_probs) else ctc_margins_resume_batch
    (result,) = call([log_probs], [labels], [band_lo], None if path is None else [path], None if d_in is None else [d_in], [end], unit,
                     None if frames is None else [frames], rows, beam_size, max_move)
    return result


def _margins_resume(lat, band_lo, path, d_in, end, unit, frames, rows, beam_size, max_move, return_status, raw):
    if unit not in _MARGIN_UNITS:
        raise ValueError('unit must be "state" or "text"')
    if rows not in _MARGIN_ROWS:
        raise ValueError('rows must be True, False, "d" or "e"')
    want_d, want_e = _MARGIN_ROWS[rows]
    n, Ls = lat.n, [2 * S + 1 for S in lat.S]
    for name, x in (("band_lo", band_lo), ("path", path), ("d_in", d_in), ("end", end), ("frames", frames)):
        if x is not None and len(x) != n:
            raise ValueError(f"{name} must hold one entry (or None) per lattice")
    entry = lambda xs, i: None if xs is None else xs[i]
    given = [i for i in range(n) if entry(band_lo, i) is not None]
    tabs = dict(zip(given, _band_tables(_Sub(lat, given), [band_lo[i] for i in given]))) if given else {}
    tables = [tabs.get(i) for i in range(n)]
    paths = [None if entry(path, i) is None else lat.int32(path[i]) for i in range(n)]
    if any(p is not None and p.shape[0] != T for p, T in zip(paths, lat.T)):
        raise ValueError("a path must have one position per frame")
    a_in = [None if entry(d_in, i) is None else _row_f64(lat, d_in[i], Ls[i], "d_in") for i in range(n)]
    ends = [entry(end, i) for i in range(n)]
    b_in = [_row_f64(lat, e, L, "an end row") if e is not None and _is_end_row(e) else None for e, L in zip(ends, Ls)]
    terms = [-1 if e is None or b is not None else _terminal_of(e) for e, b in zip(ends, b_in)]
    if any(e is None and p is None for e, p in zip(ends, paths)):
        raise ValueError("end=None is the last state of path: a lattice needs one of the two")
    fr = [None if entry(frames, i) is None else _frames_of(frames[i], lat.T[i]) for i in range(n)]     # (host memory in both forms)
    Ws = [_band_width(S, beam_size) for S in lat.S]
    thr = [None if p is None else lat.empty(T, np.float64) for p, T in zip(paths, lat.T)]
    alt = [None if p is None else lat.empty(T, np.float64) for p, T in zip(paths, lat.T)]
    run = [None if p is None else lat.empty(T, np.int32) for p, T in zip(paths, lat.T)]
    srows = [None if f is None else lat.empty((len(f), W), np.float64) for f, W in zip(fr, Ws)]
    slo = [None if f is None else lat.empty(len(f), np.int64) for f in fr]
    a_out = [lat.empty(L, np.float64) if want_d else None for L in Ls]
    b_out = [lat.empty(L, np.float64) if want_e else None for L in Ls]

    def ptrs(xs):
        return _ptr_array([None if x is None else lat.ptr(x) for x in xs])
    p_band, _k0 = ptrs(tables)
    p_din, _k1 = ptrs(a_in)
    p_ein, _k2 = ptrs(b_in)
    p_term, _k3 = _i64_array(terms)
    p_path, _k4 = ptrs(paths)
    p_thr, _k5 = ptrs(thr)
    p_alt, _k6 = ptrs(alt)
    p_run, _k7 = ptrs(run)
    p_fr, _k8 = _ptr_array([None if f is None or not len(f) else f.ctypes.data for f in fr])
    p_K, _k9 = _i64_array([0 if f is None else len(f) for f in fr])
    p_rows, _k10 = ptrs([None if f is None or not len(f) else r for f, r in zip(fr, srows)])
    p_ld, _k11 = _i64_array(Ws)
    p_lo, _k12 = ptrs([None if f is None or not len(f) else x for f, x in zip(fr, slo)])
    p_dout, _k13 = ptrs(a_out)
    p_eout, _k14 = ptrs(b_out)
    got = _run_lattices(lat, "margins_resume", beam_size, max_move,
                        (p_band, p_din, p_ein, p_term, p_path, _MARGIN_UNITS[unit], p_thr, p_alt, p_run, p_fr, p_K, p_rows, p_ld, p_lo,
                         p_dout, p_eout), list(zip(thr, alt, run, srows, slo, a_out, b_out)), return_status)
    if raw:
        return got

    def margin(th, al):
        if th is None or _is_tensor(th):
            return None if th is None else th - al
        with np.errstate(invalid="ignore"):
            return th - al
    results = [(margin(th, al), *rest) for th, al, *rest in (got[0] if return_status else got)]
    return (results, got[1]) if return_status else results


def ctc_margins_resume_batch(log_probs_list, labels_list, band_lo, path=None, d_in=None, end=None, unit="state", frames=None, rows=True,
                             beam_size=1000, max_move=4, device=None, return_status=False, raw=False):
    """``ctc_margins_resume`` of many chunks in ONE launch; host NumPy buffers in and out.  ``band_lo``, ``path``, ``d_in``,
    ``end`` and ``frames`` are None or lists in which any entry may be None.  Returns a list of (margin, runner_up, state_rows,
    rows_lo, d_out, e_out, score), with ``raw`` of (through, alt, runner_up, ...); with ``return_status`` also the per-lattice
    status list, in which case failures do not raise (every float output of a failed lattice is NaN, rows included)."""
    lat = _host_lattices(log_probs_list, labels_list, log_probs_list, "log-probs", device)
    if lat is None:
        return ([], []) if return_status else []
    return _margins_resume(lat, band_lo, path, d_in, end, unit, frames, rows, beam_size, max_move, return_status, raw)


def ctc_margins_resume_device(log_probs, labels, band_lo, path=None, d_in=None, end=None, unit="state", frames=None, rows=True,
                              beam_size=1000, max_move=4, return_status=False, raw=False):
    """``ctc_margins_resume_batch`` on lists of ROCm torch tensors: results and rows stay on the device (float64 tensors), so
    that a chunk's rows reach its neighbour without a copy; ``frames`` are host lists.  One launch on torch's current stream."""
    lat = _device_lattices(log_probs, labels, log_probs, "log-probs")
    if lat is None:
        return ([], []) if return_status else []
    return _margins_resume(lat, band_lo, path, d_in, end, unit, frames, rows, beam_size, max_move, return_status, raw)


def ctc_state_margins(log_probs, labels, terminal, frames, beam_size=1000, max_move=4, band_lo=None):
    """How far every band position of chosen frames lies behind the best alignment: (rows float64 [K, W], band_lo int64 [K],
    score float).

    rows[k, j] = m - score, with m the score of the best complete path of the band of ``ctc_best_path`` that is at state
    band_lo[k] + j in frame ``frames[k]`` and ends at ``terminal`` (an int, or a best path whose last value is used), and score
    the best path's: every entry is <= 0, 0 on a best path's state, -inf where no path passes or past the band's width.  W =
    min(beam_size, 2S+1).  The best-path counterpart of ``ctc_state_posteriors``: adds and maxima only, float64, exact.
    ``band_lo``: the band as a table [T]; None is the diagonal band.  NumPy in -> NumPy out, tensors in -> tensors out.
    """
    _m, _r, srows, lo, _d, _e, score = ctc_margins_resume(log_probs, labels, band_lo, None, None, _terminal_of(terminal), "state", frames, False,
                                                          beam_size, max_move)
    if _is_tensor(srows):
        return srows - score, lo, score
    with np.errstate(invalid="ignore"):
        return srows - score, lo, score


def ctc_path_margins_chunked(log_probs, labels, path, band_lo, chunk_frames, unit="state", beam_size=1000, max_move=4, raw=False):
    """``ctc_path_margins(..., band_lo=)`` of a recording in the checkpoint workspace of one chunk, bit for bit: (margin float64
    [T], runner_up int32 [T], score float), or (through, alt, runner_up, score) with ``raw``.

    A forward-only sweep over chunks of ``chunk_frames`` frames keeps every chunk's start row (2S+1 doubles per chunk); the
    chunks are then visited newest first, each from its start row to the row its successor handed back (the last one to the
    path's last state).  By pass count that is one forward pass more than the uncut call.  NumPy in, NumPy out.
    """
    lp = np.asarray(log_probs)
    T = lp.shape[0]
    chunk = int(chunk_frames)
    if chunk < 1:
        raise ValueError("chunk_frames must be at least 1")
    band = np.asarray(band_lo).reshape(-1)
    if band.shape[0] != T:
        raise ValueError("a band table must have one entry per frame")
    pth = np.asarray(path).reshape(-1)
    if pth.shape[0] != T:
        raise ValueError("a path must have one position per frame")
    L = 2 * len(np.asarray(labels).reshape(-1)) + 1
    cuts = list(range(0, T, chunk)) + [T]
    starts, row = [], None
    for a, b in zip(cuts[:-2], cuts[1:-1]):      # forward only: the start row of every chunk but the first
        starts.append(row)
        row = ctc_margins_resume(lp[a:b], labels, band[a:b], None, row, free_end_scores(L), unit, None, "d", beam_size, max_move)[4]
    starts.append(row)
    through, alt, runner = np.empty(T, np.float64), np.empty(T, np.float64), np.empty(T, np.int32)
    end, score = None, None
    for k in range(len(starts) - 1, -1, -1):     # newest first, with both rows
        a, b = cuts[k], cuts[k + 1]
        ((th, al, ru, _s, _l, _d, end, z),) = ctc_margins_resume_batch([lp[a:b]], [labels], [band[a:b]], [pth[a:b]],
                                                                       None if starts[k] is None else [starts[k]], [end], unit, None,
                                                                       "e" if k > 0 else False, beam_size, max_move, raw=True)
        through[a:b], alt[a:b], runner[a:b] = th, al, ru
        score = z if score is None else score
    if raw:
        return through, alt, runner, score
    with np.errstate(invalid="ignore"):
        return through - alt, runner, score
