"""Wall time of ka_ctc_best_path_tracking_batch_f32 (best path over a self-steering band, ka_banded.hpp's BandTracking, DESIGN.md
section 4.32) against ka_ctc_best_path_banded_batch_f32 FED THE TABLE THE TRACKING CALL RETURNED: the same cells and the same
bits, by the table's own kernels.  One cfg2 lattice and 1024 cfg2 lattices at period 16 and period 64; device-resident
hash-generated inputs; the two calls alternate in one process, 3 repetitions, the minimum counts.  The results of the two calls
are compared bit for bit while they are there.

    python tools/bench_tracking.py [--cases single,b1024] [--periods 16,64] [--reps 3] [--out profiles/tracking_bench.jsonl]

One JSON line per case, period and call: ms per call (min and all repetitions), and on the tracking line its ratio to the banded
call, how far the table went and how often it moved."""
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

from bench_banded import BEAM, MAX_MOVE, cfg2  # noqa: E402
from kokoro_align_amd import _lib  # noqa: E402
from kokoro_align_amd.align import _i64_array, _ptr_array, _stream_ptr  # noqa: E402


def run_case(name, n, period, reps, inputs):
    lps, labs = inputs
    T, S, V = int(lps[0].shape[0]), int(labs[0].shape[0]), int(lps[0].shape[1])
    dev = torch.cuda.current_device()
    eng = _lib.default_engine(dev)
    # outputs of the tracking call (the fourth is the table) and of the banded call
    t_outs = [[torch.empty(T, dtype=dt, device="cuda") for _ in range(n)] for dt in (torch.int32, torch.int32, torch.float32, torch.int32)]
    b_outs = [[torch.empty(T, dtype=dt, device="cuda") for _ in range(n)] for dt in (torch.int32, torch.int32, torch.float32)]
    k = [_ptr_array([x.data_ptr() for x in xs]) for xs in (lps, labs, *t_outs, *b_outs)]
    pT, pS, pld = _i64_array([T] * n), _i64_array([S] * n), _i64_array([x.stride(0) for x in lps])
    status, total_t, total_b = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    stream = _stream_ptr(dev)

    def call_tracking():
        rc = eng.lib.ka_ctc_best_path_tracking_batch_f32(eng.handle, n, k[0][0], pT[0], V, pld[0], k[1][0], pS[0], BEAM, MAX_MOVE, period, 0,
                                                         k[2][0], k[3][0], k[4][0], k[5][0], total_t.ctypes.data, status.ctypes.data,
                                                         _lib.KA_MEM_DEVICE, stream)
        _lib.check(rc, "ka_ctc_best_path_tracking_batch_f32")

    def call_banded():
        rc = eng.lib.ka_ctc_best_path_banded_batch_f32(eng.handle, n, k[0][0], pT[0], V, pld[0], k[1][0], pS[0], BEAM, MAX_MOVE, k[5][0], k[6][0],
                                                       k[7][0], k[8][0], total_b.ctypes.data, status.ctypes.data, _lib.KA_MEM_DEVICE, stream)
        _lib.check(rc, "ka_ctc_best_path_banded_batch_f32")

    eng.reserve(max(eng.lib.ka_banded_workspace_bytes(n, pT[0], pS[0], V, BEAM, MAX_MOVE, _lib.KA_MEM_DEVICE),
                    eng.lib.ka_tracking_workspace_bytes(n, pT[0], pS[0], V, BEAM, MAX_MOVE, _lib.KA_MEM_DEVICE)))
    call_tracking()
    call_banded()                                # warm-up of both, and the comparison
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for xs, ys in zip(t_outs[:3], b_outs) for a, b in zip(xs, ys)) and \
        np.array_equal(total_t.view(np.int32), total_b.view(np.int32))
    table = t_outs[3][0].cpu().numpy()
    ms = {"tracking": [], "banded_on_returned_table": []}
    for _ in range(reps):
        for what, call in (("tracking", call_tracking), ("banded_on_returned_table", call_banded)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()                               # (both synchronise their stream)
            ms[what].append((time.perf_counter() - t0) * 1e3)
    lines = []
    for what in ("banded_on_returned_table", "tracking"):
        line = {"case": name, "call": what, "n": n, "T": T, "S": S, "V": V, "beam": BEAM, "period": period, "ms_min": round(min(ms[what]), 4),
                "ms_all": [round(x, 4) for x in ms[what]], "frames_per_s": round(n * T / (min(ms[what]) * 1e-3))}
        if what == "tracking":
            line["ratio_to_banded"] = round(min(ms["tracking"]) / min(ms["banded_on_returned_table"]), 4)
            line["same_bits_as_banded"] = bool(same)
            line["table_last"] = int(table[-1])
            line["table_moves"] = int(np.count_nonzero(np.diff(table)))
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="single,b1024")
    ap.add_argument("--periods", default="16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = {"single": 1, "b1024": 1024}
    out = open(args.out, "a") if args.out else None
    for name in args.cases.split(","):
        inputs = cfg2(sizes[name])
        for period in (int(p) for p in args.periods.split(",")):
            for line in run_case(name, sizes[name], period, args.reps, inputs):
                text = json.dumps(line)
                print(text, flush=True)
                if out:
                    out.write(text + "\n")
                    out.flush()
        del inputs
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
