"""What the six posterior test files share.  The raw callers go to the C ABI through ``eng.lib`` on host buffers and never
through the Python API of kokoro_align_amd/posteriors.py: being independent of it is their point.  Outputs are filled with
sentinels first (-7.0, -9, status 99), so a test can tell that a call wrote nothing."""
import ctypes
import json
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P = lambda xs: ctypes.cast((ctypes.c_void_p * len(xs))(*[x.ctypes.data for x in xs]), ctypes.POINTER(ctypes.c_void_p))
I = lambda xs: (ctypes.c_int64 * len(xs))(*[int(v) for v in xs])
GUARD = 4          # what a float output's buffer is longer than the output, filled with ...
SENTINEL = -7.0    # ... the value no call writes (statuses: 99), so a test can tell what a call wrote and that it stayed inside


def _addresses(xs):
    return ctypes.cast((ctypes.c_void_p * len(xs))(*xs), ctypes.POINTER(ctypes.c_void_p))


def record(call, ratio, m):
    """Prints one figure of the per-cell check (posterior_ref.*_ratio: the worst |kernel - float64| / E of a call's output) and,
    with KA_ACCURACY_OUT=<file>, appends it to that file as a JSON line (the source of profiles/posterior_accuracy.json);
    then holds it against m.  The figure is out before the assertion, so a run that fails still measures."""
    rec = dict(test=os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], call=call, ratio=float(ratio), m=m)
    print(json.dumps(rec))
    path = os.environ.get("KA_ACCURACY_OUT")
    if path:
        with open(path, "at") as f:
            f.write(json.dumps(rec) + "\n")
    assert ratio <= m, rec


def engine():
    """(package, binding, default engine in its automatic modes) for a module-scoped ``env`` fixture of the GPU tests."""
    import torch
    assert torch.cuda.is_available(), "the GPU tests need a device"
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    eng = _lib.default_engine(torch.cuda.current_device())
    eng.set_mode("auto")
    eng.set_backtrace("auto")
    return ka, _lib, eng


def band_width(S, beam):
    return max(1, min(beam, 2 * S + 1))


def _lattices(lps, labs):
    """(log-probs, T table, V, ld table, labels, S table): the arguments every batch call starts with."""
    lps = [np.ascontiguousarray(x, np.float32) for x in lps]
    labs = [np.ascontiguousarray(x, np.int32) for x in labs]
    V = lps[0].shape[1]
    return lps, I([x.shape[0] for x in lps]), V, I([V] * len(lps)), labs, I([x.shape[0] for x in labs])


def path_call(eng, _lib, lps, labs, paths, beam, mm):
    """ka_ctc_path_posteriors_batch_f32: (posteriors list, log-likelihoods, statuses, rc)."""
    n = len(lps)
    lps, Ts, V, lds, labs, Ss = _lattices(lps, labs)
    paths = [np.ascontiguousarray(x, np.int32) for x in paths]
    posts = [np.full(x.shape[0], -7.0, np.float32) for x in lps]
    ll = np.zeros(n, np.float64)
    st = np.full(n, 99, np.int32)
    rc = eng.lib.ka_ctc_path_posteriors_batch_f32(eng.handle, n, P(lps), Ts, V, lds, P(labs), Ss, beam, mm, P(paths), P(posts),
                                                  ll.ctypes.data, st.ctypes.data, _lib.KA_MEM_HOST, None)
    return posts, ll, st, rc


def label_call(eng, _lib, lps, labs, terms, beam, mm):
    """ka_ctc_label_posteriors_batch_f32: (occ list, log-likelihoods, statuses, rc)."""
    n = len(lps)
    lps, Ts, V, lds, labs, Ss = _lattices(lps, labs)
    occs = [np.full((x.shape[0], V), -7.0, np.float32) for x in lps]
    ll = np.zeros(n, np.float64)
    st = np.full(n, 99, np.int32)
    rc = eng.lib.ka_ctc_label_posteriors_batch_f32(eng.handle, n, P(lps), Ts, V, lds, P(labs), Ss, beam, mm, I(terms), P(occs),
                                                   I([V] * n), ll.ctypes.data, st.ctypes.data, _lib.KA_MEM_HOST, None)
    return occs, ll, st, rc


def state_call(eng, _lib, lps, labs, terms, frames, beam, mm, ld_out=None):
    """ka_ctc_state_posteriors_batch_f32: (gamma list, band_lo list, log-likelihoods, statuses, rc)."""
    n = len(lps)
    lps, Ts, V, lds, labs, Ss = _lattices(lps, labs)
    frs = [np.ascontiguousarray(np.asarray(f).reshape(-1), np.int64) for f in frames]
    Ws = [band_width(len(x), beam) for x in labs]
    gs = [np.full((len(f), w), -7.0, np.float32) for f, w in zip(frs, Ws)]
    los = [np.full(len(f), -9, np.int64) for f in frs]
    ll = np.zeros(n, np.float64)
    st = np.full(n, 99, np.int32)
    rc = eng.lib.ka_ctc_state_posteriors_batch_f32(eng.handle, n, P(lps), Ts, V, lds, P(labs), Ss, beam, mm, I(terms), P(frs),
                                                   I([len(f) for f in frs]), P(gs), I(ld_out or Ws), P(los), ll.ctypes.data,
                                                   st.ctypes.data, _lib.KA_MEM_HOST, None)
    return gs, los, ll, st, rc


def _one(lp, labels):
    """(log-probs, labels, the leading arguments after the engine) of a single-lattice call."""
    lp = np.ascontiguousarray(lp, np.float32)
    labels = np.ascontiguousarray(labels, np.int32)
    T, V = lp.shape
    return lp, labels, (lp.ctypes.data, T, V, V, labels.ctypes.data, labels.shape[0])


def path_z_one(eng, _lib, lp, labels, terminal, beam, mm):
    """ka_ctc_path_posteriors_f32's Z for a path that ends at the terminal."""
    lp, labels, head = _one(lp, labels)
    path = np.full(lp.shape[0], terminal, np.int32)
    post = np.zeros(lp.shape[0], np.float32)
    ll = np.zeros(1, np.float64)
    eng.lib.ka_ctc_path_posteriors_f32(eng.handle, *head, beam, mm, path.ctypes.data, post.ctypes.data, ll.ctypes.data,
                                       _lib.KA_MEM_HOST, None)
    return ll[0]


def label_call_one(eng, _lib, lp, labels, terminal, beam, mm, ld_out=None, fill=0.0):
    """ka_ctc_label_posteriors_f32 for one lattice into rows of pitch ``ld_out`` (V if None) prefilled with ``fill``:
    (occ [T, ld_out], Z)."""
    lp, labels, head = _one(lp, labels)
    ld_out = ld_out or lp.shape[1]
    occ = np.full((lp.shape[0], ld_out), fill, np.float32)
    ll = np.zeros(1, np.float64)
    rc = eng.lib.ka_ctc_label_posteriors_f32(eng.handle, *head, beam, mm, int(terminal), occ.ctypes.data, ld_out, ll.ctypes.data,
                                             _lib.KA_MEM_HOST, None)
    assert rc == 0
    return occ, ll[0]


def state_call_one(eng, _lib, lp, labels, terminal, frames, beam, mm, ld_out, fill):
    """ka_ctc_state_posteriors_f32 for one lattice into rows of pitch ``ld_out`` prefilled with ``fill``:
    (rows [K, ld_out], band_lo, Z, rc)."""
    lp, labels, head = _one(lp, labels)
    fr = np.ascontiguousarray(frames, np.int64)
    rows = np.full((len(fr), ld_out), fill, np.float32)
    lo = np.zeros(len(fr), np.int64)
    z = np.zeros(1, np.float64)
    rc = eng.lib.ka_ctc_state_posteriors_f32(eng.handle, *head, beam, mm, int(terminal), fr.ctypes.data, len(fr), rows.ctypes.data,
                                             ld_out, lo.ctypes.data, z.ctypes.data, _lib.KA_MEM_HOST, None)
    return rows, lo, z[0], rc


def tiny(rng, T, S, V, zero_label=False, ninf=False):
    """A small random lattice: Dirichlet log-probs [T, V], labels in [1, V), optionally one label 0 and one -inf."""
    lp = np.log(rng.dirichlet(np.ones(V), size=T)).astype(np.float32)
    labels = rng.integers(1, V, size=S).astype(np.int32)
    if zero_label and S:
        labels[rng.integers(0, S)] = 0
    if ninf:
        lp[rng.integers(0, T), rng.integers(0, V)] = -np.inf
    return lp, labels


def header_text():
    with open(os.path.join(ROOT, "include", "kokoro_align_amd.h")) as f:
        return f.read()


def declared():
    """The function names the public header declares (comments stripped)."""
    return set(re.findall(r"\b(ka_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)))


def assert_declared_exported_bound(names):
    """Each name is in the header, in the built library and in the ctypes binding; returns the raw library."""
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    header = declared()
    lib = ctypes.CDLL(ka.build_library())
    L = _lib.load_library()
    for name in names:
        assert name in header, name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None, name
    return lib
