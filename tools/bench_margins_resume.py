"""Wall time of the resumed margin call (ka_ctc_margins_resume_batch_f32) against the call it extends,
ka_ctc_path_margins_batch_f32, and of that call against ITSELF IN THE PARENT COMMIT's library, loaded beside this tree's
(--parent <path to the parent's libkokoro_align_amd.so>; without it the parent lines are left out).  One cfg2 lattice and 1024
cfg2 lattices (T = 50 000, S = 5000, beam 1000, V = 64); device-resident hash-generated inputs over the diagonal's table; the
path is the banded call's own best path.  All calls alternate in one process after a warm-up round (every round in a shuffled order of
its own), 9 repetitions, the minimum counts; a call's time is a host clock around a call that synchronises.  The parent runs
twice per round (parent_a, parent_b): the difference of its own two minima is the noise margin the other figures are read against.

    python tools/bench_margins_resume.py [--parent PATH] [--cases single,b1024] [--reps 9] [--out profiles/margins_resume_bench.jsonl]

Calls:  path_margins (this tree's), parent_a / parent_b, resume_null (no rows in or out: the sibling's work), resume_rows (d_in,
e_in, d_out, e_out all given), forward_only (d_out and score alone), state_rows (rows at ~100 frames, no through / alt),
chunked8 (single only: ctc_path_margins_chunked in 8 chunks through the Python front end, against the uncut call through it).
One JSON line per case and call: ms (min), all repetitions, and the ratio to this tree's path_margins."""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import kokoro_align_amd as ka  # noqa: E402
from kokoro_align_amd import _lib  # noqa: E402
from kokoro_align_amd._lattices import _i64_array, _ptr_array  # noqa: E402

from bench_margins import BEAM, MAX_MOVE, V, inputs  # noqa: E402


def parent_library(path):
    """The parent commit's library beside this tree's: the three entry points it is timed through, with this tree's prototypes."""
    lib, own = ctypes.CDLL(path), _lib.load_library()
    for name in ("ka_engine_create", "ka_engine_destroy", "ka_ctc_path_margins_batch_f32", "ka_version"):
        getattr(lib, name).restype = getattr(own, name).restype
        getattr(lib, name).argtypes = getattr(own, name).argtypes
    h = ctypes.c_void_p()
    _lib.check(lib.ka_engine_create(torch.cuda.current_device(), ctypes.byref(h)), "parent engine")
    return lib, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--cases", default="single,b1024")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--T", type=int, default=50000)
    ap.add_argument("--S", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "margins_resume_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_margins_resume.py needs a GPU"
    eng = _lib.default_engine(torch.cuda.current_device())
    lib = eng.lib
    plib, peng = parent_library(args.parent) if args.parent else (None, None)
    T, S, L = args.T, args.S, 2 * args.S + 1
    W = min(BEAM, L)
    lines = []
    for case in args.cases.split(","):
        n = {"single": 1, "b1024": 1024}[case]
        lps, labs = inputs(n, T, S)
        ptrs = lambda xs: _ptr_array([x.data_ptr() for x in xs])
        dev = lambda shape, dt: [torch.empty(shape, dtype=dt, device="cuda") for _ in range(n)]
        p_lp, p_lab = ptrs(lps), ptrs(labs)
        p_T, p_S, p_ld = _i64_array([T] * n), _i64_array([S] * n), _i64_array([V] * n)
        table = torch.from_numpy(ka.diagonal_band(T, L, BEAM).astype(np.int32)).cuda()
        p_tab = ptrs([table] * n)
        paths, blabs, bsc = dev(T, torch.int32), dev(T, torch.int32), dev(T, torch.float32)
        p_path, p_blab, p_bsc = ptrs(paths), ptrs(blabs), ptrs(bsc)
        total = np.zeros(n, np.float32)
        through, alt, runner = dev(T, torch.float64), dev(T, torch.float64), dev(T, torch.int32)
        p_thr, p_alt, p_run = ptrs(through), ptrs(alt), ptrs(runner)
        d_in = [torch.full((L,), -np.inf, dtype=torch.float64, device="cuda") for _ in range(n)]
        for x in d_in:
            x[0] = 0.0                                        # the virtual start as a row
        e_in = [torch.zeros(L, dtype=torch.float64, device="cuda") for _ in range(n)]
        d_out, e_out = dev(L, torch.float64), dev(L, torch.float64)
        p_din, p_ein, p_dout, p_eout = ptrs(d_in), ptrs(e_in), ptrs(d_out), ptrs(e_out)
        K = 100
        frames = np.ascontiguousarray(np.linspace(0, T - 1, K).astype(np.int64))
        p_fr, _kf = _ptr_array([frames.ctypes.data] * n)
        p_K, _kk = _i64_array([K] * n)
        rows, rows_lo = dev((K, W), torch.float64), dev(K, torch.int64)
        p_rows, p_rlo = ptrs(rows), ptrs(rows_lo)
        p_ldr, _kl = _i64_array([W] * n)
        st = np.zeros(n, np.int32)
        z = np.zeros(n, np.float64)
        head = (n, p_lp[0], p_T[0], V, p_ld[0], p_lab[0], p_S[0], BEAM, MAX_MOVE)
        tail = (z.ctypes.data, st.ctypes.data, _lib.KA_MEM_DEVICE, None)
        _lib.check(lib.ka_ctc_best_path_banded_batch_f32(eng.handle, *head, p_tab[0], p_path[0], p_blab[0], p_bsc[0], total.ctypes.data,
                                                         st.ctypes.data, _lib.KA_MEM_DEVICE, None), "best path")

        def sibling(l, h):
            return lambda: l.ka_ctc_path_margins_batch_f32(h, *head, p_tab[0], p_path[0], 1, p_thr[0], p_alt[0], p_run[0], *tail)

        def resume(din=None, ein=None, path=p_path[0], thr=p_thr[0], al=p_alt[0], run=p_run[0], fr=None, k=None, rw=None, rlo=None, dout=None,
                   eout=None):
            return lambda: lib.ka_ctc_margins_resume_batch_f32(eng.handle, *head, p_tab[0], din, ein, None, path, 1, thr, al, run, fr, k, rw,
                                                               p_ldr, rlo, dout, eout, *tail)

        calls = [("path_margins", sibling(lib, eng.handle))]
        if plib:
            calls += [("parent_a", sibling(plib, peng)), ("parent_b", sibling(plib, peng))]
        calls += [
            ("resume_null", resume()),
            ("resume_rows", resume(p_din[0], p_ein[0], dout=p_dout[0], eout=p_eout[0])),
            ("forward_only", resume(p_din[0], p_ein[0], None, None, None, None, dout=p_dout[0])),
            ("state_rows", resume(None, p_ein[0], None, None, None, None, p_fr, p_K, p_rows[0], p_rlo[0])),
        ]
        if case == "single":
            lp_h, lab_h = lps[0].cpu().numpy(), labs[0].cpu().numpy()
            path_h, tab_h = paths[0].cpu().numpy(), table.cpu().numpy()
            calls += [
                ("uncut_front_end", lambda: ka.ctc_path_margins(lp_h, lab_h, path_h, BEAM, MAX_MOVE, "text", band_lo=tab_h) and 0),
                ("chunked8", lambda: ka.ctc_path_margins_chunked(lp_h, lab_h, path_h, tab_h, -(-T // 8), "text", BEAM, MAX_MOVE) and 0),
            ]
        times = {name: [] for name, _ in calls}
        for rep in range(-1, args.reps):                   # round -1 warms every shape up; every round runs the calls in an order
            order = list(calls)                            # of its own, so that no call always follows the same neighbour
            random.Random(rep).shuffle(order)
            for name, fn in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = fn()
                dt = (time.perf_counter() - t0) * 1e3
                _lib.check(rc, name)
                if rep >= 0:
                    times[name].append(dt)
        best = {name: min(v) for name, v in times.items()}
        for name, _ in calls:
            rec = dict(case=case, n=n, T=T, S=S, V=V, beam=BEAM, call=name, ms=round(best[name], 3), all_ms=[round(x, 3) for x in times[name]],
                       vs_path_margins=round(best[name] / best["path_margins"], 4))
            if name == "chunked8":
                rec["vs_uncut_front_end"] = round(best[name] / best["uncut_front_end"], 4)
            if name == "parent_b" and plib:
                rec["parent_spread_ms"] = round(abs(best["parent_a"] - best["parent_b"]), 3)
                rec["this_minus_parent_ms"] = round(best["path_margins"] - min(best["parent_a"], best["parent_b"]), 3)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del lps, labs, through, alt, runner, paths, blabs, bsc, d_in, e_in, d_out, e_out, rows, rows_lo
        torch.cuda.empty_cache()
    if plib:
        plib.ka_engine_destroy(peng)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "wt") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
