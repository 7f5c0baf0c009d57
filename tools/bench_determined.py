"""Wall time of the determined calls (ka_ctc_best_path_determined_batch_f32, ka_ctc_best_path_tracking_determined_batch_f32;
ka_determined.hpp) against their parent entry points of the same build on the same inputs, and of
StreamingAligner against ctc_best_path_tracking_chunked.  cfg2 shapes (T = 50 000, S = 5000, beam 1000, V = 64), 1 and 1024
lattices, periods 16 and 64, device-resident inputs of three kinds:
    hash     the hash generator's log-probs and labels
    peaked   one lattice (every pointer of a batch names it): the hash log-probs with the label of a diagonal path raised to -0.01
    worst    the walk never stops: flat log-probs, S = 499 so that the band (1000) is at least as wide as the label axis (999), and a
             free start row, so the lines never merge and the walk runs all T frames
The parent and the new call alternate in one process, `reps` repetitions, the minimum counts; the parent's max / min over the
repetitions is the run-to-run spread the ratio is read against.  Every output the two share is compared bit for bit while it
is there, and the merge lag T - determined is recorded.

    python tools/bench_determined.py [--cases single,b1024] [--periods 16,64] [--inputs hash,peaked,worst] [--reps 5] [--chunks 8]
                                     [--out profiles/determined_bench.jsonl]
"""
import argparse
import json
import os
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
from kokoro_align_amd.align import _i64_array, _ptr_array, _stream_ptr  # noqa: E402


def make_inputs(kind, n):
    """(log-probs list, labels list, start row or None)"""
    if kind == "hash":
        lps, labs = cfg2(n)
        return lps, labs, None
    if kind == "peaked":
        (lp,), (lab,) = cfg2(1)
        T, S = int(lp.shape[0]), int(lab.shape[0])
        L = 2 * S + 1
        pos = (torch.arange(T, device="cuda", dtype=torch.int64) * L) // T
        ext = torch.zeros(L, dtype=torch.int64, device="cuda")
        ext[1::2] = lab.to(torch.int64)
        lp[torch.arange(T, device="cuda"), ext[pos]] = -0.01
        return [lp] * n, [lab] * n, None
    (lp,), (lab,) = cfg2(1, S=499)
    lp.zero_()
    return [lp] * n, [lab] * n, torch.from_numpy(ka.free_start_scores(2 * 499 + 1)).cuda()


def run_case(name, kind, n, period, reps, inputs):
    lps, labs, start = inputs
    T, S, V = int(lps[0].shape[0]), int(labs[0].shape[0]), int(lps[0].shape[1])
    L = 2 * S + 1
    dev = torch.cuda.current_device()
    eng = _lib.default_engine(dev)
    band = torch.from_numpy(np.ascontiguousarray(ka.diagonal_band(T, L, BEAM), np.int32)).cuda()
    calls = ("resume", "determined", "tracking_resume", "tracking_determined")
    outs = {w: [[torch.empty(T, dtype=dt, device="cuda") for _ in range(n)] for dt in (torch.int32, torch.int32, torch.float32, torch.int32)]
            for w in calls}
    last = {w: [torch.empty(L, dtype=torch.float32, device="cuda") for _ in range(n)] for w in calls}
    k = {w: [_ptr_array([x.data_ptr() for x in xs]) for xs in o] for w, o in outs.items()}
    p_last = {w: _ptr_array([x.data_ptr() for x in xs]) for w, xs in last.items()}
    p_lp, p_lab, p_band = (_ptr_array([x.data_ptr() for x in xs]) for xs in (lps, labs, [band] * n))
    p_start = _ptr_array([start.data_ptr()] * n) if start is not None else (None, None)
    pT, pS, pld = _i64_array([T] * n), _i64_array([S] * n), _i64_array([x.stride(0) for x in lps])
    status = np.zeros(n, np.int32)
    total = {w: np.zeros(n, np.float32) for w in calls}
    entry = {w: np.zeros(n, np.int32) for w in calls}
    next_lo = {w: np.zeros(n, np.int32) for w in calls}
    det = {w: np.full(n, -9, np.int32) for w in calls}
    stream = _stream_ptr(dev)
    head = (eng.handle, n, p_lp[0], pT[0], V, pld[0], p_lab[0], pS[0], BEAM, MAX_MOVE)

    def banded(w, fn, more):
        o = k[w]
        _lib.check(fn(*head, p_band[0], p_start[0], None, o[0][0], o[1][0], o[2][0], p_last[w][0], entry[w].ctypes.data, *more,
                      total[w].ctypes.data, status.ctypes.data, _lib.KA_MEM_DEVICE, stream), w)

    def tracked(w, fn, more):
        o = k[w]
        _lib.check(fn(*head, period, None, p_start[0], None, o[0][0], o[1][0], o[2][0], o[3][0], p_last[w][0], entry[w].ctypes.data,
                      next_lo[w].ctypes.data, *more, total[w].ctypes.data, status.ctypes.data, _lib.KA_MEM_DEVICE, stream), w)

    lib = eng.lib
    run = {"resume": lambda: banded("resume", lib.ka_ctc_best_path_resume_batch_f32, ()),
           "determined": lambda: banded("determined", lib.ka_ctc_best_path_determined_batch_f32, (det["determined"].ctypes.data,)),
           "tracking_resume": lambda: tracked("tracking_resume", lib.ka_ctc_best_path_tracking_resume_batch_f32, ()),
           "tracking_determined": lambda: tracked("tracking_determined", lib.ka_ctc_best_path_tracking_determined_batch_f32,
                                                  (det["tracking_determined"].ctypes.data,))}
    eng.reserve(max(lib.ka_determined_workspace_bytes(n, pT[0], pS[0], V, BEAM, MAX_MOVE, _lib.KA_MEM_DEVICE, tr) for tr in (0, 1)))
    lines = []
    for parent, new in (("resume", "determined"), ("tracking_resume", "tracking_determined")):
        if parent == "resume" and period != 16:
            continue   # (no period in the table's call: measured once)
        run[parent]()
        run[new]()
        cols = 3 if parent == "resume" else 4
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for xs, ys in zip(outs[new][:cols], outs[parent][:cols]) for a, b in zip(xs, ys))
        same = same and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(last[new], last[parent]))
        same = same and np.array_equal(total[new].view(np.int32), total[parent].view(np.int32)) and np.array_equal(entry[new], entry[parent])
        same = same and np.array_equal(next_lo[new], next_lo[parent])
        ms = {parent: [], new: []}
        for _ in range(reps):
            for w in (parent, new):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run[w]()                             # (both synchronise their stream)
                ms[w].append((time.perf_counter() - t0) * 1e3)
        spread = max(ms[parent]) / min(ms[parent])
        d = det[new]
        for w in (parent, new):
            line = {"case": name, "input": kind, "call": w, "n": n, "T": T, "S": S, "V": V, "beam": BEAM, "ms_min": round(min(ms[w]), 4),
                    "ms_all": [round(x, 4) for x in ms[w]]}
            if parent != "resume":
                line["period"] = period
            if w == parent:
                line["spread_max_over_min"] = round(spread, 4)
            else:
                line["ratio_to_parent"] = round(min(ms[new]) / min(ms[parent]), 4)
                line["same_bits_as_parent"] = bool(same)
                line["determined_min_max"] = [int(d.min()), int(d.max())]
                line["merge_lag_min_max"] = [int(T - d.max()), int(T - d.min())] if d.min() >= 0 else None
            lines.append(line)
    return lines


def run_streaming(kind, chunks, period, reps, inputs):
    lp, lab, start = inputs[0][0], inputs[1][0], inputs[2]
    if start is not None:
        return []   # (the aligner starts at position 0: no free start row)
    T, S = int(lp.shape[0]), int(lab.shape[0])
    frames = -(-(-(-T // chunks)) // period) * period   # T / chunks, up to a multiple of the period

    def streamed():
        al = ka.StreamingAligner(lab, BEAM, MAX_MOVE, period)
        parts, first = [], None
        for a in range(0, T, frames):
            parts.append(al.push(lp[a:a + frames]))
            if first is None and parts[-1][0].shape[0]:
                first = (min(a + frames, T), int(parts[-1][0].shape[0]))
        parts.append(al.finish())
        return tuple(torch.cat([p[i] for p in parts]) for i in range(4)), first

    calls = (("chunked", lambda: (ka.ctc_best_path_tracking_chunked(lp, lab, frames, BEAM, MAX_MOVE, period), None)), ("streaming", streamed))
    res = {w: c() for w, c in calls}
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(res["streaming"][0], res["chunked"][0]))
    ms = {w: [] for w, _ in calls}
    for _ in range(reps):
        for w, call in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms[w].append((time.perf_counter() - t0) * 1e3)
    first = res["streaming"][1]
    return [{"case": "single", "input": kind, "call": w, "n": 1, "T": T, "S": S, "beam": BEAM, "period": period, "chunk_frames": frames,
             "ms_min": round(min(ms[w]), 4), "ms_all": [round(x, 4) for x in ms[w]],
             **({"ratio_to_chunked": round(min(ms[w]) / min(ms["chunked"]), 4), "same_bits_as_chunked": bool(same),
                 "frames_pushed_at_first_commit": first[0] if first else None, "frames_in_first_commit": first[1] if first else None}
                if w == "streaming" else {})} for w, _ in calls]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="single,b1024")
    ap.add_argument("--periods", default="16,64")
    ap.add_argument("--inputs", default="hash,peaked,worst")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = {"single": 1, "b1024": 1024}
    out = open(args.out, "a") if args.out else None

    def emit(lines):
        for line in lines:
            text = json.dumps(line)
            print(text, flush=True)
            if out:
                out.write(text + "\n")
                out.flush()

    for name in args.cases.split(","):
        for kind in args.inputs.split(","):
            inputs = make_inputs(kind, sizes[name])
            for period in (int(p) for p in args.periods.split(",")):
                emit(run_case(name, kind, sizes[name], period, args.reps, inputs))
                if name == "single" and args.chunks > 1:
                    emit(run_streaming(kind, args.chunks, period, args.reps, inputs))
            del inputs
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
