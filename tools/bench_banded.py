"""Wall time of ka_ctc_best_path_banded_batch_f32 (best path over a caller-given band, ka_banded.hpp)
with the reference's own band as the table, against ka_ctc_best_path_batch_f32 in KA_MODE_WAVE_EXACT with
KA_BACKTRACE_SERIAL: the form that stores the same 256 bytes of codes per frame and whose kernels the banded call leaves
unchanged.  One cfg2 lattice and 1024 cfg2 lattices; device-resident hash-generated inputs; the two calls alternate in one
process, 3 repetitions, the minimum counts.  The results of the two calls are compared bit for bit while they are there.

    python tools/bench_banded.py [--cases single,b1024] [--reps 3] [--out profiles/banded_bench.jsonl]

One JSON line per case and call: ms per call (min and all repetitions), and on the banded line its ratio to the exact form."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import kokoro_align_amd as ka  # noqa: E402
from kokoro_align_amd import _lib  # noqa: E402
from kokoro_align_amd.align import DeviceBatch, _i64_array, _ptr_array, _stream_ptr  # noqa: E402

BEAM, MAX_MOVE = 1000, 4


def cfg2(n, seed0=9000, T=50000, V=64, S=5000):
    lib = _lib.load_library()
    lp = torch.empty((n, T, V), dtype=torch.float32, device="cuda")
    lab = torch.empty((n, S), dtype=torch.int32, device="cuda")
    _lib.check(lib.ka_hash_logprobs_batch_f32(lp.data_ptr(), n, T, V, V, T * V, seed0, None), "hash")
    _lib.check(lib.ka_hash_labels_batch_i32(lab.data_ptr(), n, S, V, S, seed0, None), "hash")
    torch.cuda.synchronize()
    return list(lp.unbind(0)), list(lab.unbind(0))


def run_case(name, n, reps):
    lps, labs = cfg2(n)
    T, S, V = int(lps[0].shape[0]), int(labs[0].shape[0]), int(lps[0].shape[1])
    dev = torch.cuda.current_device()
    eng = _lib.default_engine(dev)
    band = torch.from_numpy(np.ascontiguousarray(ka.diagonal_band(T, 2 * S + 1, BEAM), np.int32)).cuda()   # one table, n pointers to it
    outs = [[torch.empty(T, dtype=dt, device="cuda") for _ in range(n)] for dt in (torch.int32, torch.int32, torch.float32)]
    k = [_ptr_array([x.data_ptr() for x in xs]) for xs in (lps, labs, [band] * n, *outs)]
    pT, pS, pld = _i64_array([T] * n), _i64_array([S] * n), _i64_array([x.stride(0) for x in lps])
    status, total = np.zeros(n, np.int32), np.zeros(n, np.float32)
    stream = _stream_ptr(dev)
    exact = DeviceBatch(lps, labs, BEAM, MAX_MOVE)

    def call_banded():
        rc = eng.lib.ka_ctc_best_path_banded_batch_f32(eng.handle, n, k[0][0], pT[0], V, pld[0], k[1][0], pS[0], BEAM, MAX_MOVE, k[2][0], k[3][0],
                                                       k[4][0], k[5][0], total.ctypes.data, status.ctypes.data, _lib.KA_MEM_DEVICE, stream)
        _lib.check(rc, "ka_ctc_best_path_banded_batch_f32")

    def call_exact():
        exact.run()

    eng.set_mode("wave_exact")
    eng.set_backtrace("serial")
    try:
        eng.reserve(max(eng.lib.ka_banded_workspace_bytes(n, pT[0], pS[0], V, BEAM, MAX_MOVE, _lib.KA_MEM_DEVICE), exact.workspace_bytes()))
        call_banded()
        call_exact()                             # warm-up of both, and the comparison
        same = all(torch.equal(a, b) for a, b in zip(outs[0], exact.path)) and all(torch.equal(a, b) for a, b in zip(outs[1], exact.best_labels)) and \
            all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs[2], exact.best_scores)) and \
            np.array_equal(total.view(np.int32), exact.total.view(np.int32))
        ms = {"banded": [], "wave_exact_serial": []}
        for _ in range(reps):
            for what, call in (("banded", call_banded), ("wave_exact_serial", call_exact)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()                           # (both synchronise their stream)
                ms[what].append((time.perf_counter() - t0) * 1e3)
    finally:
        eng.set_mode("auto")
        eng.set_backtrace("auto")
    lines = []
    for what in ("wave_exact_serial", "banded"):
        line = {"case": name, "call": what, "n": n, "T": T, "S": S, "V": V, "beam": BEAM, "ms_min": round(min(ms[what]), 4),
                "ms_all": [round(x, 4) for x in ms[what]], "frames_per_s": round(n * T / (min(ms[what]) * 1e-3))}
        if what == "banded":
            line["ratio_to_wave_exact_serial"] = round(min(ms["banded"]) / min(ms["wave_exact_serial"]), 4)
            line["same_bits_as_wave_exact"] = bool(same)
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="single,b1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = {"single": 1, "b1024": 1024}
    out = open(args.out, "a") if args.out else None
    for name in args.cases.split(","):
        for line in run_case(name, sizes[name], args.reps):
            text = json.dumps(line)
            print(text, flush=True)
            if out:
                out.write(text + "\n")
                out.flush()
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
