"""Wall time of ka_ctc_best_path_tracking_resume_batch_f32 (the resumable tracking best path, ka_banded.hpp's BandTrackingResume,
DESIGN.md section 4.35) against ka_ctc_best_path_tracking_batch_f32 of the same build, whose kernels the feature leaves as they
were.  One cfg2 lattice and 1024 cfg2 lattices at periods 16 and 64, device-resident hash-generated inputs, two variants of the
new call:
    tr_null   NULL start row, first_lo 0, end -1, no last row, no next_lo     (every output is the tracking call's)
    tr_rows   a start row (0.0 at position 0, dead elsewhere), the last row and next_lo asked for, end = the tracking call's end cell
The three calls alternate in one process, `reps` repetitions, the minimum counts; the tracking call's max / min over the
repetitions is the run-to-run spread the ratios are read against (accepted: ratio <= spread + 3 %).  The results are compared bit
for bit while they are there.  With --chunks N the single lattice is also run through ctc_best_path_tracking_chunked in N chunks
against ctc_best_path_tracking.

    python tools/bench_tracking_resume.py [--cases single,b1024] [--periods 16,64] [--reps 5] [--chunks 8]
                                          [--out profiles/tracking_resume_bench.jsonl]
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

CALLS = ("tracking", "tr_null", "tr_rows")


def run_case(name, n, period, reps, inputs):
    lps, labs = inputs
    T, S, V = int(lps[0].shape[0]), int(labs[0].shape[0]), int(lps[0].shape[1])
    L = 2 * S + 1
    dev = torch.cuda.current_device()
    eng = _lib.default_engine(dev)
    start = torch.from_numpy(ka.free_start_scores(L, 0, 1)).cuda()   # one start row, n pointers to it
    outs = {w: [[torch.empty(T, dtype=dt, device="cuda") for _ in range(n)] for dt in (torch.int32, torch.int32, torch.float32, torch.int32)]
            for w in CALLS}
    last = [torch.empty(L, dtype=torch.float32, device="cuda") for _ in range(n)]
    k = {w: [_ptr_array([x.data_ptr() for x in xs]) for xs in o] for w, o in outs.items()}
    p_lp, p_lab = (_ptr_array([x.data_ptr() for x in xs]) for xs in (lps, labs))
    p_start, p_last = _ptr_array([start.data_ptr()] * n), _ptr_array([x.data_ptr() for x in last])
    pT, pS, pld = _i64_array([T] * n), _i64_array([S] * n), _i64_array([x.stride(0) for x in lps])
    status = np.zeros(n, np.int32)
    total = {w: np.zeros(n, np.float32) for w in outs}
    entry, next_lo = np.zeros(n, np.int32), np.zeros(n, np.int32)
    first, ends = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    stream = _stream_ptr(dev)
    head = (eng.handle, n, p_lp[0], pT[0], V, pld[0], p_lab[0], pS[0], BEAM, MAX_MOVE, period)

    def call_tracking():
        o = k["tracking"]
        _lib.check(eng.lib.ka_ctc_best_path_tracking_batch_f32(*head, 0, o[0][0], o[1][0], o[2][0], o[3][0], total["tracking"].ctypes.data,
                                                               status.ctypes.data, _lib.KA_MEM_DEVICE, stream), "ka_ctc_best_path_tracking_batch_f32")

    def call_null():
        o = k["tr_null"]
        _lib.check(eng.lib.ka_ctc_best_path_tracking_resume_batch_f32(*head, None, None, None, o[0][0], o[1][0], o[2][0], o[3][0], None, None, None,
                                                                      total["tr_null"].ctypes.data, status.ctypes.data, _lib.KA_MEM_DEVICE, stream),
                   "ka_ctc_best_path_tracking_resume_batch_f32")

    def call_rows():
        o = k["tr_rows"]
        _lib.check(eng.lib.ka_ctc_best_path_tracking_resume_batch_f32(*head, first.ctypes.data, p_start[0], ends.ctypes.data, o[0][0], o[1][0],
                                                                      o[2][0], o[3][0], p_last[0], entry.ctypes.data, next_lo.ctypes.data,
                                                                      total["tr_rows"].ctypes.data, status.ctypes.data, _lib.KA_MEM_DEVICE, stream),
                   "ka_ctc_best_path_tracking_resume_batch_f32")

    eng.reserve(eng.lib.ka_tracking_resume_workspace_bytes(n, pT[0], pS[0], V, BEAM, MAX_MOVE, _lib.KA_MEM_DEVICE))
    call_tracking()                              # warm-up of the three, and the comparison
    ends[:] = [int(x[-1]) for x in outs["tracking"][0]]   # the end cell the tracking call chose, now given
    call_null()
    call_rows()
    same = {w: all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for xs, ys in zip(outs[w], outs["tracking"]) for a, b in zip(xs, ys)) and
            np.array_equal(total[w].view(np.int32), total["tracking"].view(np.int32)) for w in ("tr_null", "tr_rows")}
    calls = (("tracking", call_tracking), ("tr_null", call_null), ("tr_rows", call_rows))
    ms = {w: [] for w, _ in calls}
    for _ in range(reps):
        for what, call in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()                               # (all synchronise their stream)
            ms[what].append((time.perf_counter() - t0) * 1e3)
    lines = []
    spread = max(ms["tracking"]) / min(ms["tracking"])
    for what, _ in calls:
        line = {"case": name, "call": what, "n": n, "T": T, "S": S, "V": V, "beam": BEAM, "period": period, "ms_min": round(min(ms[what]), 4),
                "ms_all": [round(x, 4) for x in ms[what]], "frames_per_s": round(n * T / (min(ms[what]) * 1e-3))}
        if what == "tracking":
            line["spread_max_over_min"] = round(spread, 4)
        else:
            ratio = min(ms[what]) / min(ms["tracking"])
            line["ratio_to_tracking"] = round(ratio, 4)
            line["accepted"] = bool(ratio <= spread + 0.03)
            line["same_bits_as_tracking"] = bool(same[what])
        if what == "tr_rows":
            line["entries_all_zero"] = bool(np.all(entry == 0))
            line["next_lo"] = int(next_lo[0])
            line["last_row_live_cells"] = int(torch.count_nonzero(~torch.isnan(last[0])))
        lines.append(line)
    return lines


def run_chunked(chunks, period, reps, inputs):
    lp, lab = inputs[0][0], inputs[1][0]
    T, S = int(lp.shape[0]), int(lab.shape[0])
    frames = -(-(-(-T // chunks)) // period) * period   # T / chunks, up to a multiple of the period
    calls = (("tracking_front_end", lambda: ka.ctc_best_path_tracking(lp, lab, BEAM, MAX_MOVE, period)),
             ("chunked", lambda: ka.ctc_best_path_tracking_chunked(lp, lab, frames, BEAM, MAX_MOVE, period)))
    res = {w: c() for w, c in calls}
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(res["chunked"], res["tracking_front_end"]))
    ms = {w: [] for w, _ in calls}
    for _ in range(reps):
        for what, call in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms[what].append((time.perf_counter() - t0) * 1e3)
    n_chunks = -(-T // frames)
    return [{"case": "single", "call": w, "n": 1, "T": T, "S": S, "beam": BEAM, "period": period, "chunks": n_chunks if w == "chunked" else 1,
             "chunk_frames": frames if w == "chunked" else T, "ms_min": round(min(ms[w]), 4), "ms_all": [round(x, 4) for x in ms[w]],
             **({"ratio_to_uncut": round(min(ms[w]) / min(ms["tracking_front_end"]), 4), "forward_passes_expected": round(2 - 1 / n_chunks, 4),
                 "same_bits_as_uncut": bool(same)} if w == "chunked" else {})} for w, _ in calls]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="single,b1024")
    ap.add_argument("--periods", default="16,64")
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
        inputs = cfg2(sizes[name])
        for period in (int(p) for p in args.periods.split(",")):
            emit(run_case(name, sizes[name], period, args.reps, inputs))
            if name == "single" and args.chunks > 1:
                emit(run_chunked(args.chunks, period, args.reps, inputs))
        del inputs
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
