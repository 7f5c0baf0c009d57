"""Raw ctypes caller of ka_ctc_posteriors_resume_batch_f32 for tests/test_fb_resume_gpu.py, beside banded_fb_harness.py and with
its sentinel buffers and guards: it goes to the C ABI through ``eng.lib`` and never through kokoro_align_amd/posteriors.py.

Every lattice has all four output buffers (occ [T, V], path_post [T], alpha_out [L], beta_out [L]), filled with the sentinel and
GUARD entries longer (rows GUARD columns wider) than the output; ``want`` says which of them the call is handed, the others go in
as NULL and must come back untouched.  ``Result.outs[i]`` holds the four payloads in that order."""
import numpy as np

from banded_fb_harness import Result, _buffer
from fb_harness import GUARD, SENTINEL, I, _addresses, _lattices

OUTS = ("occ", "path_post", "alpha_out", "beta_out")
ALL = dict(occ=True, path_post=True, alpha_out=True, beta_out=True)


def run(eng, _lib, lps, labs, tables, beam, mm, alpha_in=None, beta_in=None, terms=None, paths=None, want=None, device=False,
        null_arrays=()):
    """``alpha_in``, ``beta_in``, ``paths``: None or lists in which an entry may be None.  ``terms``: terminals (-1 where a lattice
    brings an end row).  ``want``: a dict over OUTS (for all lattices) or a list of such dicts; a path_post without a path is
    what the caller asks for.  ``null_arrays``: names among OUTS + ("alpha_in", "beta_in", "path", "terminal") whose whole array
    goes in as NULL."""
    n = len(lps)
    lps, Ts, V, lds, labs, Ss = _lattices(lps, labs)
    T = [x.shape[0] for x in lps]
    L = [2 * x.shape[0] + 1 for x in labs]
    wants = [dict(ALL, **(want or {}))] * n if not isinstance(want, list) else [dict(ALL, **w) for w in want]
    opt = lambda xs, dt: [None] * n if xs is None else [None if x is None else np.ascontiguousarray(x, dt) for x in xs]
    a_in, b_in, pth = opt(alpha_in, np.float64), opt(beta_in, np.float64), opt(paths, np.int32)
    tabs = [np.ascontiguousarray(t, np.int32) for t in tables]
    terms = [-1] * n if terms is None else [int(t) for t in terms]
    shapes = [((t, V), (t,), (l,), (l,)) for t, l in zip(T, L)]
    dtypes = (np.float32, np.float32, np.float64, np.float64)
    raw = [tuple(_buffer(s, d) for s, d in zip(shp, dtypes)) for shp in shapes]
    ll = np.zeros(n, np.float64)
    st = np.full(n, 99, np.int32)
    if device:
        import torch
        up = lambda xs: [None if x is None else torch.from_numpy(x).cuda() for x in xs]
        addr = lambda xs: [None if x is None else x.data_ptr() for x in xs]
        mem = _lib.KA_MEM_DEVICE
    else:
        up = lambda xs: xs
        addr = lambda xs: [None if x is None else x.ctypes.data for x in xs]
        mem = _lib.KA_MEM_HOST
    d_lps, d_labs, d_tabs, d_ain, d_bin, d_pth = up(lps), up(labs), up(tabs), up(a_in), up(b_in), up(pth)
    d_raw = [up(list(bufs)) for bufs in raw]
    a_out = [addr(bufs) for bufs in d_raw]
    col = lambda k: _addresses([a[k] if w[OUTS[k]] else None for a, w in zip(a_out, wants)])
    arg = lambda name, value: None if name in null_arrays else value
    rc = eng.lib.ka_ctc_posteriors_resume_batch_f32(
        eng.handle, n, _addresses(addr(d_lps)), Ts, V, lds, _addresses(addr(d_labs)), Ss, beam, mm, _addresses(addr(d_tabs)),
        arg("alpha_in", _addresses(addr(d_ain))), arg("beta_in", _addresses(addr(d_bin))), arg("terminal", I(terms)),
        arg("path", _addresses(addr(d_pth))), arg("occ", col(0)), I([V + GUARD] * n), arg("path_post", col(1)), arg("alpha_out", col(2)),
        arg("beta_out", col(3)), ll.ctypes.data, st.ctypes.data, mem, None)
    if device:
        import torch
        torch.cuda.synchronize()
        raw = [tuple(x.cpu().numpy() for x in bufs) for bufs in d_raw]
    return Result(raw, shapes, ll, st, rc)


def untouched(res, i, name):
    """Is lattice i's buffer of output ``name`` still all sentinel?"""
    return bool(np.all(res.raw[i][OUTS.index(name)] == SENTINEL))


def all_nan(x):
    return bool(np.all(np.isnan(x)))
