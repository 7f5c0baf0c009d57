#!/usr/bin/env python3
"""The answer of every ka_*_workspace_bytes export of the library over a grid of arguments, one JSON object per line:
{"fn": name, "args": {...}, "bytes": n}.  No GPU is needed: the byte counts are host arithmetic.

    python tools/workspace_bytes.py > listing.jsonl          # print
    python tools/workspace_bytes.py --golden                 # rewrite tests/golden/workspace_bytes.json

tests/test_workspace_bytes_cpu.py replays the golden file through call() below, so a change of a planner that moves a byte
shows on a CPU.  (ka_engine_workspace_bytes takes an engine, which takes a GPU: it is not listed.)"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")

# the arguments of every export, in the order of include/kokoro_align_amd.h
PLAIN = ("n", "T", "S", "V", "beam_size", "max_move", "mem")
WITH_K = ("n", "T", "S", "K", "V", "beam_size", "max_move", "mem")
SIGNATURES = {
    "ka_workspace_bytes": ("n", "T", "S", "V", "beam_size", "max_move"),
    "ka_posterior_workspace_bytes": PLAIN,
    "ka_label_posterior_workspace_bytes": PLAIN,
    "ka_state_duration_workspace_bytes": PLAIN,
    "ka_state_visit_workspace_bytes": PLAIN,
    "ka_mea_path_workspace_bytes": PLAIN,
    "ka_path_margin_workspace_bytes": PLAIN,
    "ka_posteriors_resume_workspace_bytes": PLAIN,
    "ka_banded_workspace_bytes": PLAIN,
    "ka_tracking_workspace_bytes": PLAIN,
    "ka_resume_workspace_bytes": PLAIN,
    "ka_tracking_resume_workspace_bytes": PLAIN,
    "ka_determined_workspace_bytes": PLAIN + ("tracking",),
    "ka_state_posterior_workspace_bytes": WITH_K,
    "ka_margins_resume_workspace_bytes": WITH_K,
    "ka_boundary_quantile_workspace_bytes": ("n", "T", "S", "K", "M", "V", "beam_size", "max_move", "mem"),
    "ka_sample_paths_workspace_bytes": ("n", "T", "S", "n_samples", "V", "beam_size", "max_move", "mem"),
    "ka_band_table_workspace_bytes": ("n", "T", "mem"),
    "ka_boundary_quantile_band_table_workspace_bytes": ("n", "T", "mem"),
}
ARRAYS = {"T": ctypes.c_int64, "S": ctypes.c_int64, "K": ctypes.c_int64, "n_samples": ctypes.c_int32}   # a list, or None: NULL

HOST, DEVICE = 0, 1
# (T, S): the first two have T no multiple of 4 (the shifted table's length), the last two are a short and a long recording
SINGLE = [(1, 0), (5, 3), (4001, 700), (50000, 5000)]
# a batch of three in (V, beam_size, max_move): all one-wavefront; V above 64, max_move above 4 (all generic); a band above the
# one-wavefront form's widest on the two long lattices and below it on the short one (mixed forms)
BATCH_T, BATCH_S = [4001, 50000, 5], [700, 5000, 3]
BATCH_FORMS = [(39, 300, 4), (80, 300, 4), (39, 300, 5), (39, 1100, 4)]
# the per-lattice extras of the calls that take them: one small value each, and 0 where the call allows it
EXTRA_ONE = {"K": [[2], [0]], "n_samples": [[2]]}
EXTRA_BATCH = {"K": [[2, 0, 4]], "n_samples": [[2, 1, 3]]}


def grid():
    """The argument sets, as a list of (fn, args)."""
    out = []
    for fn, sig in SIGNATURES.items():
        extra = next((a for a in ("K", "n_samples") if a in sig), None)
        scalars = [{}]
        if "tracking" in sig:
            scalars = [{"tracking": 0}, {"tracking": 1}]
        if "M" in sig:
            scalars = [{"M": 3}, {"M": 1}, {"M": 0}, {"M": 9}]      # (0 and 9: refused)
        mems = [HOST, DEVICE] if "mem" in sig else [None]

        def add(n, T, S, V=39, beam=300, mm=4, mem=HOST, ex=None, **more):
            a = {"n": n, "T": T, "S": S, "V": V, "beam_size": beam, "max_move": mm, "mem": mem, "tracking": 0, "M": 3, "K": ex, "n_samples": ex}
            a.update(more)
            out.append((fn, {k: a[k] for k in sig}))

        for mem in mems:
            for sc in scalars:
                for T, S in SINGLE:
                    for ex in EXTRA_ONE.get(extra, [None]):
                        add(1, [T], [S], mem=mem, ex=ex, **sc)
                for V, beam, mm in BATCH_FORMS:
                    for ex in EXTRA_BATCH.get(extra, [None]):
                        add(3, BATCH_T, BATCH_S, V, beam, mm, mem=mem, ex=ex, **sc)
                add(0, [], [], mem=mem, ex=[], **sc)
            # refusals: an unsupported shape, a negative count, a NULL T
            one = EXTRA_ONE.get(extra, [None])[0]
            add(1, [5], [3], mm=300, mem=mem, ex=one)
            add(-1, [5], [3], mem=mem, ex=one)
            add(1, None, [3], mem=mem, ex=one)
        if "mem" in sig:
            add(1, [5], [3], mem=7, ex=EXTRA_ONE.get(extra, [None])[0])
        if extra == "K":
            add(1, [5], [3], ex=[99])                       # more query frames, or cuts, than the lattice has
            if fn == "ka_margins_resume_workspace_bytes":
                add(3, BATCH_T, BATCH_S, ex=None)           # K may be NULL here: no query frames
        if extra == "n_samples":
            add(1, [5], [3], ex=[0])                        # not allowed
    return out


def call(lib, fn, args):
    """One export called with `args` (a dict by argument name; an array argument is a list, or None for NULL)."""
    keep, argv = [], []
    for name in SIGNATURES[fn]:
        v = args[name]
        if name in ARRAYS:
            if v is None:
                argv.append(None)
                continue
            buf = (ARRAYS[name] * max(len(v), 1))(*v)
            keep.append(buf)
            argv.append(ctypes.cast(buf, ctypes.c_void_p) if name == "n_samples" else buf)
        else:
            argv.append(int(v))
    return int(getattr(lib, fn)(*argv))


def listing(lib):
    return [{"fn": fn, "args": args, "bytes": call(lib, fn, args)} for fn, args in grid()]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from kokoro_align_amd import _lib
    rows = listing(_lib.load_library())
    if "--golden" in sys.argv[1:]:
        with open(GOLDEN, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
        print(f"wrote {len(rows)} entries to {GOLDEN}")
    else:
        for r in rows:
            print(json.dumps(r))
