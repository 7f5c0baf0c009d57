"""Wall time of every forward-backward call against ITSELF IN THE PARENT COMMIT's library, loaded beside this tree's (--parent
<path to the parent's libkokoro_align_amd.so>), for a change to the core all of them share (ka_posterior_common.hpp: the running
maxima taken with fmax on doubles, DESIGN.md section 4.21, "magnitude").  1024 cfg2 lattices (T = 50 000, S = 5000, beam 1000,
V = 64), device-resident hash-generated inputs.  The two libraries alternate in one process after a warm-up round, every round in
a shuffled order of its own, `reps` repetitions, the minimum counts; a call's time is a host clock around a call that
synchronises.  The parent runs twice per round (parent_a, parent_b): the difference of its own two minima is the noise the
ratio is read against.  The outputs of the two libraries are compared bit for bit while they are there.

    python tools/bench_fb_maxima.py --parent PATH [--n 1024] [--V 64] [--reps 3] [--calls path,label,...] [--out profiles/fb_maxima_bench.jsonl]
    python tools/bench_fb_maxima.py --parent PATH --n 256 --V 80 --append        (the generic form: 256-thread workgroups)
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import kokoro_align_amd as ka  # noqa: E402
from bench_banded import BEAM, MAX_MOVE, cfg2  # noqa: E402
from kokoro_align_amd import _lib  # noqa: E402
from kokoro_align_amd._lattices import _i64_array, _ptr_array  # noqa: E402

CALLS = ("path", "label", "state", "durations", "visits", "quantiles", "samples", "mea", "resume")
SYMBOLS = dict(path="ka_ctc_path_posteriors_batch_f32", label="ka_ctc_label_posteriors_batch_f32", state="ka_ctc_state_posteriors_batch_f32",
               durations="ka_ctc_state_durations_batch_f32", visits="ka_ctc_state_visits_batch_f32",
               quantiles="ka_ctc_boundary_quantiles_batch_f32", samples="ka_ctc_sample_paths_batch_f32", mea="ka_ctc_mea_path_batch_f32",
               resume="ka_ctc_posteriors_resume_batch_f32")


_alive = []          # every pointer table handed to a call, with the array it was cast from


def pa(ptrs):
    _alive.append(_ptr_array(ptrs))
    return _alive[-1][0]


def ia(vals):
    _alive.append(_i64_array(vals))
    return _alive[-1][0]


def parent_library(path):
    """The parent commit's library beside this tree's, with this tree's prototypes, and an engine of its own."""
    lib, own = ctypes.CDLL(path), _lib.load_library()
    for name in ("ka_engine_create", "ka_engine_destroy") + tuple(SYMBOLS.values()):
        getattr(lib, name).restype = getattr(own, name).restype
        getattr(lib, name).argtypes = getattr(own, name).argtypes
    h = ctypes.c_void_p()
    _lib.check(lib.ka_engine_create(torch.cuda.current_device(), ctypes.byref(h)), "parent engine")
    return lib, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--V", type=int, default=64, help="64: the one-wavefront form; above it (80) the generic form")
    ap.add_argument("--append", action="store_true", help="add the lines to --out")
    ap.add_argument("--calls", default=",".join(CALLS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fb_maxima_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fb_maxima.py needs a GPU"
    eng = _lib.default_engine(torch.cuda.current_device())
    plib, peng = parent_library(args.parent)
    n = args.n
    lps, labs = cfg2(n, V=args.V)
    T, S, V = int(lps[0].shape[0]), int(labs[0].shape[0]), int(lps[0].shape[1])
    L, W = 2 * S + 1, min(BEAM, 2 * S + 1)
    ptrs = lambda xs: pa([x.data_ptr() for x in xs])
    dev = lambda shape, dt: [torch.empty(shape, dtype=dt, device="cuda") for _ in range(n)]
    p_lp, p_lab = ptrs(lps), ptrs(labs)
    p_T, p_S, p_ld, p_term = ia([T] * n), ia([S] * n), ia([V] * n), ia([L - 1] * n)
    head = (n, p_lp, p_T, V, p_ld, p_lab, p_S, BEAM, MAX_MOVE)
    st, z = np.zeros(n, np.int32), np.zeros(n, np.float64)
    tail = (z.ctypes.data, st.ctypes.data, _lib.KA_MEM_DEVICE, None)
    lines = []
    for call in args.calls.split(","):
        keep = []                                              # what the call's pointers point at
        if call == "path":
            path = torch.from_numpy(np.minimum(L - 1, (L * np.arange(T)) // T).astype(np.int32)).cuda()
            path[-1] = L - 1
            outs = dev(T, torch.float32)
            mid = (ptrs([path] * n), ptrs(outs))
            keep = [path]
        elif call == "label":
            outs = dev((T, V), torch.float32)
            mid = (p_term, ptrs(outs), ia([V] * n))
        elif call == "state":
            frames = np.ascontiguousarray(np.linspace(0, T - 1, 100).astype(np.int64))
            outs, los = dev((100, W), torch.float32), dev(100, torch.int64)
            mid = (p_term, pa([frames.ctypes.data] * n), ia([100] * n), ptrs(outs), ia([W] * n), ptrs(los))
            keep = [frames, los]
        elif call in ("durations", "visits"):
            outs, second = dev(L, torch.float64), dev(L, torch.float64)
            mid = (p_term, ptrs(outs), ptrs(second))
            keep = [second]
        elif call == "quantiles":
            cuts = np.ascontiguousarray(np.arange(2, L, 200, dtype=np.int64))
            levels = np.ascontiguousarray([0.05, 0.5, 0.95], np.float64)
            outs = dev((len(cuts), 3), torch.int32)
            mid = (p_term, pa([cuts.ctypes.data] * n), ia([len(cuts)] * n), levels.ctypes.data, 3, ptrs(outs),
                   ia([3] * n))
            keep = [cuts, levels]
        elif call == "samples":
            K, seeds = np.full(n, 4, np.int32), np.arange(n, dtype=np.uint64)
            outs = dev((4, T), torch.int32)
            mid = (p_term, K.ctypes.data, seeds.ctypes.data, ptrs(outs), ia([T] * n))
            keep = [K, seeds]
        elif call == "mea":
            outs, ea = dev(T, torch.int32), np.zeros(n, np.float64)
            mid = (p_term, ptrs(outs), ea.ctypes.data)
            keep = [ea]
        else:
            assert call == "resume", call
            table = torch.from_numpy(ka.diagonal_band(T, L, BEAM).astype(np.int32)).cuda()
            start, end = np.full(L, -np.inf), np.full(L, -np.inf)
            start[0] = end[L - 1] = 0.0
            start, end = torch.from_numpy(start).cuda(), torch.from_numpy(end).cuda()
            outs, a_out, b_out = dev((T, V), torch.float32), dev(L, torch.float64), dev(L, torch.float64)
            mid = (ptrs([table] * n), ptrs([start] * n), ptrs([end] * n), None, None, ptrs(outs), ia([V] * n), None,
                   ptrs(a_out), ptrs(b_out))
            keep = [table, start, end, a_out, b_out]
        fn = lambda l, h: (lambda: getattr(l, SYMBOLS[call])(h, *head, *mid, *tail))
        calls = [("this", fn(eng.lib, eng.handle)), ("parent_a", fn(plib, peng)), ("parent_b", fn(plib, peng))]
        times, bits, zs = {name: [] for name, _ in calls}, {}, {}
        for rep in range(-1, args.reps):
            order = list(calls)
            random.Random(rep).shuffle(order)
            for name, f in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = f()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                _lib.check(rc, call + " " + name)
                assert not st.any(), (call, name, st[:8])
                if rep >= 0:
                    times[name].append(dt)
                elif name != "parent_b":                       # the warm-up round also compares the two libraries' outputs
                    bits[name] = [x.clone() for x in outs[:8]]
                    zs[name] = z.copy()
        best = {name: min(v) for name, v in times.items()}
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(bits["this"], bits["parent_a"])) \
            and np.array_equal(zs["this"].view(np.int64), zs["parent_a"].view(np.int64))
        parent = min(best["parent_a"], best["parent_b"])
        rec = dict(call=call, symbol=SYMBOLS[call], n=n, T=T, S=S, V=V, beam=BEAM, ms_this=round(best["this"], 3), ms_parent=round(parent, 3),
                   ratio_to_parent=round(best["this"] / parent, 4), parent_spread_ms=round(abs(best["parent_a"] - best["parent_b"]), 3),
                   all_ms={k: [round(x, 3) for x in v] for k, v in times.items()}, same_bits_as_parent=bool(same))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del outs, keep, mid, calls, bits
        torch.cuda.empty_cache()
    plib.ka_engine_destroy(peng)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "at" if args.append else "wt") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
