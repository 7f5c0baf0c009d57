"""Wall time of ka_ctc_posteriors_resume_batch_f32 (forward-backward under the caller's boundary conditions, ka_fb_resume.hpp,
DESIGN.md section 4.37) against ka_ctc_label_posteriors_banded_batch_f32 of the same build on the same diagonal table, whose
kernels the feature leaves as they were.  One cfg2 lattice and 1024 cfg2 lattices, device-resident hash-generated inputs:
    sibling         ka_ctc_label_posteriors_banded_batch_f32, terminal 2S
    resume_null     NULL rows, the terminal, occupancy alone                  (every output is the sibling's)
    resume_rows     a start row (0.0 at position 0), an end row (0.0 at the terminal), occupancy and both rows out
    resume_forward  the same rows in, alpha_out and Z alone: one forward pass
The calls alternate in one process, `reps` repetitions, the minimum counts; the sibling's max / min over the repetitions is the
run-to-run spread the ratios are read against.  The occupancies are compared bit for bit while they are there.
With --chunks N the single lattice is also run through ctc_label_posteriors_chunked in N chunks against
ctc_label_posteriors(band_lo=) on host buffers: by pass count one forward pass more than the uncut call.

    python tools/bench_fb_resume.py [--cases single,b1024] [--reps 3] [--chunks 8] [--out profiles/fb_resume_bench.jsonl]
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


def run_case(name, n, reps, inputs):
    lps, labs = inputs
    T, S, V = int(lps[0].shape[0]), int(labs[0].shape[0]), int(lps[0].shape[1])
    L = 2 * S + 1
    dev = torch.cuda.current_device()
    eng = _lib.default_engine(dev)
    band = torch.from_numpy(np.ascontiguousarray(ka.diagonal_band(T, L, BEAM), np.int32)).cuda()   # one table, n pointers to it
    start, end = np.full(L, -np.inf), np.full(L, -np.inf)
    start[0] = end[L - 1] = 0.0
    start, end = torch.from_numpy(start).cuda(), torch.from_numpy(end).cuda()                      # ... one start row and one end row
    occ = {w: [torch.empty((T, V), dtype=torch.float32, device="cuda") for _ in range(n)] for w in ("sibling", "resume")}   # (resume_*: one set)
    a_out = [torch.empty(L, dtype=torch.float64, device="cuda") for _ in range(n)]
    b_out = [torch.empty(L, dtype=torch.float64, device="cuda") for _ in range(n)]
    ptrs = lambda xs: _ptr_array([x.data_ptr() for x in xs])
    p_lp, p_lab, p_band, p_start, p_end = ptrs(lps), ptrs(labs), ptrs([band] * n), ptrs([start] * n), ptrs([end] * n)
    p_occ = {w: ptrs(o) for w, o in occ.items()}
    p_aout, p_bout = ptrs(a_out), ptrs(b_out)
    pT, pS, pld, pldo, pterm = _i64_array([T] * n), _i64_array([S] * n), _i64_array([x.stride(0) for x in lps]), _i64_array([V] * n), _i64_array([L - 1] * n)
    status = np.zeros(n, np.int32)
    ll = {w: np.zeros(n, np.float64) for w in ("sibling", "resume_null", "resume_rows", "resume_forward")}
    stream = _stream_ptr(dev)
    head = (eng.handle, n, p_lp[0], pT[0], V, pld[0], p_lab[0], pS[0], BEAM, MAX_MOVE, p_band[0])

    def call_sibling():
        _lib.check(eng.lib.ka_ctc_label_posteriors_banded_batch_f32(*head, pterm[0], p_occ["sibling"][0], pldo[0], ll["sibling"].ctypes.data,
                                                                    status.ctypes.data, _lib.KA_MEM_DEVICE, stream), "ka_ctc_label_posteriors_banded_batch_f32")

    def resume(what, a_in, b_in, o, ao, bo):
        _lib.check(eng.lib.ka_ctc_posteriors_resume_batch_f32(*head, a_in, b_in, pterm[0], None, o, pldo[0], None, ao, bo, ll[what].ctypes.data,
                                                              status.ctypes.data, _lib.KA_MEM_DEVICE, stream), "ka_ctc_posteriors_resume_batch_f32")
    call_null = lambda: resume("resume_null", None, None, p_occ["resume"][0], None, None)
    call_rows = lambda: resume("resume_rows", p_start[0], p_end[0], p_occ["resume"][0], p_aout[0], p_bout[0])
    call_fwd = lambda: resume("resume_forward", p_start[0], p_end[0], None, p_aout[0], None)

    eng.reserve(eng.lib.ka_posteriors_resume_workspace_bytes(n, pT[0], pS[0], V, BEAM, MAX_MOVE, _lib.KA_MEM_DEVICE))
    same_occ = lambda: all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(occ["resume"], occ["sibling"]))
    call_sibling()                               # warm-up of the four, and the comparison
    call_null()
    same = {"resume_null": same_occ() and np.array_equal(ll["resume_null"].view(np.int64), ll["sibling"].view(np.int64))}
    call_rows()
    same["resume_rows"] = same_occ()             # (the same boundary conditions, given as rows: the same gamma; Z is formed in float64)
    z_rows = float(np.max(np.abs(ll["resume_rows"] - ll["sibling"])))
    call_fwd()
    calls = (("sibling", call_sibling), ("resume_null", call_null), ("resume_rows", call_rows), ("resume_forward", call_fwd))
    ms = {w: [] for w, _ in calls}
    for _ in range(reps):
        for what, call in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()                               # (all synchronise their stream)
            ms[what].append((time.perf_counter() - t0) * 1e3)
    lines = []
    for what, _ in calls:
        line = {"case": name, "call": what, "n": n, "T": T, "S": S, "V": V, "beam": BEAM, "ms_min": round(min(ms[what]), 4),
                "ms_all": [round(x, 4) for x in ms[what]], "frames_per_s": round(n * T / (min(ms[what]) * 1e-3))}
        if what == "sibling":
            line["spread_max_over_min"] = round(max(ms[what]) / min(ms[what]), 4)
        else:
            line["ratio_to_sibling"] = round(min(ms[what]) / min(ms["sibling"]), 4)
        if what in same:
            line["same_occupancy_bits_as_sibling"] = bool(same[what])
        if what == "resume_rows":
            line["z_max_abs_diff_to_sibling"] = z_rows
            line["ratio_to_resume_forward"] = round(min(ms[what]) / min(ms["resume_forward"]), 4)
        lines.append(line)
    return lines


def run_chunked(chunks, reps, inputs):
    lp, lab = inputs[0][0].cpu().numpy(), inputs[1][0].cpu().numpy()
    T, S = lp.shape[0], lab.shape[0]
    band = ka.diagonal_band(T, 2 * S + 1, BEAM)
    frames = -(-T // chunks)
    calls = (("uncut_front_end", lambda: ka.ctc_label_posteriors(lp, lab, 2 * S, BEAM, MAX_MOVE, band_lo=band)),
             ("chunked", lambda: ka.ctc_label_posteriors_chunked(lp, lab, band, frames, 2 * S, None, BEAM, MAX_MOVE)))
    res = {w: c() for w, c in calls}
    diff = float(np.max(np.abs(res["chunked"][0].astype(np.float64) - res["uncut_front_end"][0])))
    ms = {w: [] for w, _ in calls}
    for _ in range(reps):
        for what, call in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms[what].append((time.perf_counter() - t0) * 1e3)
    return [{"case": "single", "call": w, "n": 1, "T": T, "S": S, "beam": BEAM, "memory": "host", "chunks": chunks if w == "chunked" else 1,
             "chunk_frames": frames if w == "chunked" else T, "ms_min": round(min(ms[w]), 4), "ms_all": [round(x, 4) for x in ms[w]],
             **({"ratio_to_uncut": round(min(ms[w]) / min(ms["uncut_front_end"]), 4), "occupancy_max_abs_diff_to_uncut": diff,
                 "z_diff_to_uncut": float(res["chunked"][2] - res["uncut_front_end"][1])} if w == "chunked" else {})} for w, _ in calls]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="single,b1024")
    ap.add_argument("--reps", type=int, default=3)
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
        emit(run_case(name, sizes[name], args.reps, inputs))
        if name == "single" and args.chunks > 1:
            emit(run_chunked(args.chunks, args.reps, inputs))
        del inputs
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
