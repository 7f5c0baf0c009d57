#!/usr/bin/env python3
"""One SHA-256 per (case, call) over what the seven forward-backward calls write: the output bytes, then the log-likelihood and
status bytes.  For a change of the kernels that must not move a bit: run it on the library before and after and diff.

    python tools/fb_output_digest.py [--library path/to/libkokoro_align_amd.so] > digest.txt

The calls go through the raw ctypes callers of tests/fb_harness.py, tests/duration_harness.py, tests/sample_harness.py and
tests/mea_harness.py: path posteriors, label occupancy, state posteriors at posterior_ref.query_frames(T), durations with
time_sum, 64 sampled paths with a fixed seed, the maximum-expected-accuracy path with its expected accuracy, and (tests/visit_harness.py)
the state visits with exit_time.  The cases
are the smallest at which a slot mapping, a checkpoint extent or a block boundary can go wrong: every case of posterior_ref.edge_cases(), the one-wavefront ones once more in the generic form (V padded to 80), tiny
lattices round the 32-frame block, every max_move with a label 0 and a -inf, a band that jumps (L > T), one that jumps more
than 64 positions a frame (L > 64 T: past the label ring's request; every call answers zero mass), the bands on either side of
the form boundary, and one batch per form with more lattices than the form has slots."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

SEED, SAMPLES = 20240229, 64


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=None, help="the library to load instead of the tree's own")
    a = ap.parse_args()
    if a.library:
        os.environ["KA_LIBRARY"] = os.path.abspath(a.library)      # (read when the package is imported)
    import duration_harness as D
    import fb_harness as H
    import mea_harness as M
    import posterior_ref as R
    import sample_harness as S
    import visit_harness as VH
    _, _lib, eng = H.engine()
    for name, lats, beam, mm in cases(R, H):
        lps, labs, terms = ([x[i] for x in lats] for i in range(3))
        frames = [R.query_frames(lp.shape[0]) for lp in lps]
        results = {}
        posts, ll, st, _ = H.path_call(eng, _lib, lps, labs, [path_of(*x) for x in lats], beam, mm)
        results["path"] = (posts, ll, st)
        occs, ll, st, _ = H.label_call(eng, _lib, lps, labs, terms, beam, mm)
        results["label"] = (occs, ll, st)
        gs, los, ll, st, _ = H.state_call(eng, _lib, lps, labs, terms, frames, beam, mm)
        results["state"] = (gs + los, ll, st)
        durs, sums, ll, st, _ = D.duration_call(eng, _lib, lps, labs, terms, beam, mm, time_sum=True)
        results["durations"] = (durs + sums, ll, st)
        paths, ll, st, _ = S.sample_call(eng, _lib, lps, labs, terms, SAMPLES, SEED, beam, mm)
        results["samples"] = (paths, ll, st)
        paths, ea, ll, st, _ = M.mea_call(eng, _lib, lps, labs, terms, beam, mm)
        results["mea"] = (paths + [ea], ll, st)
        visits, exits, ll, st, _ = VH.visit_call(eng, _lib, lps, labs, terms, beam, mm, exit_time=True)
        results["visits"] = (visits + exits, ll, st)
        for call, (outs, ll, st) in results.items():
            h = hashlib.sha256()
            for x in list(outs) + [ll, st]:
                h.update(np.ascontiguousarray(x).tobytes())
            print(name, call, h.hexdigest(), flush=True)


if __name__ == "__main__":
    main()
