#!/usr/bin/env python3
"""One SHA-256 per (case, call) over what the eight forward-backward calls and the eight calls over a caller-given band write:
the output bytes, then the log-likelihood and status bytes; behind it the number of lattices with status 0, and what the call's
*_workspace_bytes function answers for host and for device memory (a banded call: its sibling's plus
ka_band_table_workspace_bytes, or ka_boundary_quantile_band_table_workspace_bytes for the quantiles).  For a change of the kernels that must not move a bit: run it on the library before and after
and diff.

    python tools/fb_output_digest.py [--library path/to/libkokoro_align_amd.so] > digest.txt
    python tools/fb_output_digest.py --fold digest.txt      (needs no GPU)

``--fold`` condenses a listing for keeping: one line per case, and per call the first 12 hex digits of the SHA-256 of that call's
whole line (hash, status count and byte counts), under a header that names the calls.  Two listings are equal where their folds
are; a fold that differs names the case and the call, and the full listings tell the rest.

The calls go through the raw ctypes callers of tests/fb_harness.py, tests/duration_harness.py, tests/sample_harness.py and
tests/mea_harness.py: path posteriors, label occupancy, state posteriors at posterior_ref.query_frames(T), durations with
time_sum, 64 sampled paths with a fixed seed, the maximum-expected-accuracy path with its expected accuracy, and (tests/visit_harness.py)
the state visits with exit_time, (tests/quantile_harness.py) the boundary quantiles at cuts spread over [0, L] and the levels
0.05, 0.5 and 0.95, and (tests/banded_fb_harness.py, tests/banded_fb2_harness.py) the eight banded calls, each once with the diagonal as a table and once with a
stepping table of banded_fb_ref.random_table whose first low end lies above 0, so that the zeros below it are hashed.  The cases
are the smallest at which a slot mapping, a checkpoint extent or a block boundary can go wrong: every case of posterior_ref.edge_cases(), the one-wavefront ones once more in the generic form (V padded to 80), tiny
lattices round the 32-frame block, every max_move with a label 0 and a -inf, a band that jumps (L > T), one that jumps more
than 64 positions a frame (L > 64 T: past the label ring's request; every call answers zero mass), the bands on either side of
the form boundary, and one batch per form with more lattices than the form has slots."""
import argparse
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

SEED, SAMPLES = 20240229, 64
LEVELS = (0.05, 0.5, 0.95)


def terminal_of(R, lp, labels, beam, mm):
    live = R.live_terminals(lp, labels, beam, mm)
    return live[0] if live else 2 * len(labels)         # (without one the calls fail with zero mass: their fill is hashed)


def cases(R, H):
    """[(name, [(lp, labels, terminal)], beam, max_move)]"""
    out = []
    for name, build in R.edge_cases().items():
        lp, labels, term, beam, mm = build()
        out.append((name, [(lp, labels, term)], beam, mm))
        if R.fast_form(len(labels), lp.shape[1], beam, mm):
            out.append((name + "_as_V80", [(R.pad_vocabulary(lp, 80), labels, term)], beam, mm))
    rng = np.random.default_rng(SEED)

    def one(name, lp, labels, beam, mm):
        out.append((name, [(lp, labels, terminal_of(R, lp, labels, beam, mm))], beam, mm))
    for T in (1, 2, 31, 32, 33, 64, 65):
        for S in (0, 1, 7):
            one("tiny_T%d_S%d" % (T, S), *H.tiny(rng, T, S, 39), 1000, 4)
    for mm in (1, 2, 3, 4, 6):
        one("moves_M%d" % mm, *H.tiny(rng, 70, 20, 39, zero_label=True, ninf=True), 1000, mm)
    lp, labels = R.sloped(60, 70, 39, SEED)
    one("jumping_band", lp, labels, 16, 4)
    one("jumping_band_as_V80", R.pad_vocabulary(lp, 80), labels, 16, 4)
    lp, labels = R.sloped(16, 600, 39, 1201)
    one("ring_jump", lp, labels, 64, 4)
    one("ring_jump_as_V80", R.pad_vocabulary(lp, 80), labels, 64, 4)
    lp, labels = R.sloped(400, 520, 39, SEED + 1)
    for beam in (1009, 1010):
        one("band_%d" % beam, lp, labels, beam, 4)
    for name, n, V in (("batch_1030_one_wavefront", 1030, 39), ("batch_520_generic", 520, 80)):
        lats = []
        for _ in range(n):
            lp, labels = H.tiny(rng, 40, int(rng.integers(1, 20)), 39)
            lats.append((R.pad_vocabulary(lp, V) if V != 39 else lp, labels, terminal_of(R, lp, labels, 64, 4)))
        out.append((name, lats, 64, 4))
    return out


def path_of(lp, labels, term):
    T, L = lp.shape[0], 2 * len(labels) + 1
    p = np.minimum(L - 1, (L * np.arange(T)) // T).astype(np.int32)
    p[-1] = term
    return p


def tables_of(R, B, rng, lats, beam):
    """{name: one table per lattice}: the diagonal, and a random walk from 1 (0 where L = 1) with steps of L / T on average."""
    diag, step = [], []
    for lp, labels, _ in lats:
        T, L = lp.shape[0], 2 * len(labels) + 1
        diag.append(R.windows(T, L, beam)[0])
        step.append(B.random_table(rng, T, L, max(1, -(-2 * L // T)), lo0=min(1, L - 1)))
    return {"diagonal": diag, "stepping": step}


def workspace(L, _lib, fn, n, T, S, own, V, beam, mm, table=None):
    """"host=... device=..." of the *_workspace_bytes function ``fn`` (``own``: its arguments between S and V); ``table``: the
    function that answers a banded call's add-on"""
    arr = lambda xs: (ctypes.c_int64 * n)(*[int(x) for x in xs])
    got = []
    for mem in (_lib.KA_MEM_HOST, _lib.KA_MEM_DEVICE):
        b = getattr(L, fn)(n, arr(T), arr(S), *own, V, beam, mm, mem)
        got.append(b + (getattr(L, table)(n, arr(T), mem) if table else 0))
    return "host=%d device=%d" % tuple(got)


def fold(path):
    cases, calls = {}, None
    for ln in open(path):
        name, call, rest = ln.rstrip("\n").split(" ", 2)
        cases.setdefault(name, []).append((call, hashlib.sha256((call + " " + rest).encode()).hexdigest()[:12]))
    for name, row in cases.items():
        if calls is None:
            calls = [c for c, _ in row]
            print("# case", *calls)
        assert [c for c, _ in row] == calls, name
        print(name, *[h for _, h in row])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=None, help="the library to load instead of the tree's own")
    ap.add_argument("--fold", default=None, metavar="LISTING", help="condense a listing of this tool: one line per case")
    a = ap.parse_args()
    if a.fold:
        return fold(a.fold)
    if a.library:
        os.environ["KA_LIBRARY"] = os.path.abspath(a.library)      # (read when the package is imported)
    import banded_fb2_harness as BH2
    import banded_fb_harness as BH
    import banded_fb_ref as B
    import duration_harness as D
    import fb_harness as H
    import mea_harness as M
    import posterior_ref as R
    import quantile_harness as Q
    import sample_harness as S
    import visit_harness as VH
    _, _lib, eng = H.engine()
    rng_tab = np.random.default_rng(SEED + 2)
    for name, lats, beam, mm in cases(R, H):
        lps, labs, terms = ([x[i] for x in lats] for i in range(3))
        n, V = len(lats), lps[0].shape[1]
        Ts, Ss = [lp.shape[0] for lp in lps], [len(x) for x in labs]
        frames = [R.query_frames(lp.shape[0]) for lp in lps]
        cuts = [np.arange(0, 2 * s + 2, max(1, (2 * s + 1) // 16)) for s in Ss]
        paths_in = [path_of(*x) for x in lats]
        i64 = lambda xs: (ctypes.c_int64 * n)(*[int(x) for x in xs])
        ws = lambda fn, *own, **kw: workspace(eng.lib, _lib, fn, n, Ts, Ss, own, V, beam, mm, **kw)
        results = {}
        posts, ll, st, _ = H.path_call(eng, _lib, lps, labs, paths_in, beam, mm)
        results["path"] = (posts, ll, st, ws("ka_posterior_workspace_bytes"))
        occs, ll, st, _ = H.label_call(eng, _lib, lps, labs, terms, beam, mm)
        results["label"] = (occs, ll, st, ws("ka_label_posterior_workspace_bytes"))
        gs, los, ll, st, _ = H.state_call(eng, _lib, lps, labs, terms, frames, beam, mm)
        results["state"] = (gs + los, ll, st, ws("ka_state_posterior_workspace_bytes", i64(len(f) for f in frames)))
        durs, sums, ll, st, _ = D.duration_call(eng, _lib, lps, labs, terms, beam, mm, time_sum=True)
        results["durations"] = (durs + sums, ll, st, ws("ka_state_duration_workspace_bytes"))
        paths, ll, st, _ = S.sample_call(eng, _lib, lps, labs, terms, SAMPLES, SEED, beam, mm)
        results["samples"] = (paths, ll, st, ws("ka_sample_paths_workspace_bytes", (ctypes.c_int32 * n)(*[SAMPLES] * n)))
        paths, ea, ll, st, _ = M.mea_call(eng, _lib, lps, labs, terms, beam, mm)
        results["mea"] = (paths + [ea], ll, st, ws("ka_mea_path_workspace_bytes"))
        visits, exits, ll, st, _ = VH.visit_call(eng, _lib, lps, labs, terms, beam, mm, exit_time=True)
        results["visits"] = (visits + exits, ll, st, ws("ka_state_visit_workspace_bytes"))
        quants, ll, st, _ = Q.quant_call(eng, _lib, lps, labs, terms, cuts, LEVELS, beam, mm)
        results["quantiles"] = (quants, ll, st, ws("ka_boundary_quantile_workspace_bytes", i64(len(c) for c in cuts), len(LEVELS)))
        for tname, tabs in tables_of(R, B, rng_tab, lats, beam).items():
            for kind, own, fn, extra in (("path_posteriors", paths_in, "ka_posterior_workspace_bytes", ()),
                                         ("label_posteriors", terms, "ka_label_posterior_workspace_bytes", ()),
                                         ("state_posteriors", (terms, frames), "ka_state_posterior_workspace_bytes", (i64(len(f) for f in frames),)),
                                         ("state_durations", terms, "ka_state_duration_workspace_bytes", ())):
                r = BH.run(eng, _lib, kind, lps, labs, own, beam, mm, tables=tabs)
                results["%s_banded_%s" % (kind, tname)] = ([x for bufs in r.raw for x in bufs], r.ll, r.st,
                                                           ws(fn, *extra, table="ka_band_table_workspace_bytes"))
            k_samples = (ctypes.c_int32 * n)(*[SAMPLES] * n)
            for kind, own, fn, extra, add_on in (
                    ("state_visits", terms, "ka_state_visit_workspace_bytes", (), "ka_band_table_workspace_bytes"),
                    ("boundary_quantiles", (terms, cuts), "ka_boundary_quantile_workspace_bytes", (i64(len(c) for c in cuts), len(LEVELS)),
                     "ka_boundary_quantile_band_table_workspace_bytes"),
                    ("sample_paths", (terms, [SAMPLES] * n, [SEED] * n), "ka_sample_paths_workspace_bytes", (k_samples,), "ka_band_table_workspace_bytes"),
                    ("mea_path", terms, "ka_mea_path_workspace_bytes", (), "ka_band_table_workspace_bytes")):
                r = BH2.run(eng, _lib, kind, lps, labs, own, beam, mm, tables=tabs, levels=LEVELS)
                outs = [x for bufs in r.raw for x in bufs] + ([r.ea] if r.ea is not None else [])
                results["%s_banded_%s" % (kind, tname)] = (outs, r.ll, r.st, ws(fn, *extra, table=add_on))
        for call, (outs, ll, st, bytes_) in results.items():
            h = hashlib.sha256()
            for x in list(outs) + [ll, st]:
                h.update(np.ascontiguousarray(x).tobytes())
            print(name, call, h.hexdigest(), "ok=%d/%d" % (int(np.sum(np.asarray(st) == 0)), n), bytes_, flush=True)


if __name__ == "__main__":
    main()
