"""Wall time of the eight forward-backward calls over a caller-given band (ka_ctc_{path_posteriors, label_posteriors,
state_posteriors, state_durations, state_visits, boundary_quantiles, sample_paths, mea_path}_banded_batch_f32, DESIGN.md
sections 4.30 and 4.31) with the reference's own band as the table, against their unbanded siblings, whose kernels differ from
theirs only in the band policy.  One cfg2 lattice and 768 cfg2 lattices (three per CU), in the fast form (V = 64) and the generic
form (V = 65); device-resident hash-generated inputs; the terminal is the last position, the path the diagonal itself, the state
call asks for 200 frames, the quantile call for 100 cuts at text boundaries (even positions) and three levels, the sampler for
64 paths.  The two calls alternate in one process, 3 repetitions, the minimum counts.  The outputs of the two calls are compared
bit for bit while they are there.

    python tools/bench_banded_posteriors.py [--cases single,b768] [--forms fast,generic] [--calls path_posteriors,...] [--reps 3]
                                            [--out profiles/banded_posteriors_bench.jsonl]

One JSON line per case, form, call and symbol: ms per call (min and all repetitions), and on the banded line its ratio to the
sibling."""
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
from kokoro_align_amd.align import _i64_array, _ptr_array, _stream_ptr  # noqa: E402

BEAM, MAX_MOVE, QUERIES = 1000, 4, 200
CUTS, LEVELS, SAMPLES, SEED = 100, (0.05, 0.5, 0.95), 64, 20240
CALLS = ("path_posteriors", "label_posteriors", "state_posteriors", "state_durations",
         "state_visits", "boundary_quantiles", "sample_paths", "mea_path")


def cfg2(n, V, seed0=9000, T=50000, S=5000):
    lib = _lib.load_library()
    lp = torch.empty((n, T, V), dtype=torch.float32, device="cuda")
    lab = torch.empty((n, S), dtype=torch.int32, device="cuda")
    _lib.check(lib.ka_hash_logprobs_batch_f32(lp.data_ptr(), n, T, V, V, T * V, seed0, None), "hash")
    _lib.check(lib.ka_hash_labels_batch_i32(lab.data_ptr(), n, S, V, S, seed0, None), "hash")
    torch.cuda.synchronize()
    return list(lp.unbind(0)), list(lab.unbind(0))


def own_arguments(call, n, T, S, V):
    """(the call's own arguments behind max_move / the table, its output tensors, what must stay alive)."""
    L = 2 * S + 1
    ptrs = lambda xs: _ptr_array([x.data_ptr() for x in xs])
    terms = _i64_array([L - 1] * n)
    dev = lambda shape, dt: [torch.empty(shape, dtype=dt, device="cuda") for _ in range(n)]
    if call == "path_posteriors":
        path = np.minimum(np.int64(L) * np.arange(T, dtype=np.int64) // T, L - 1).astype(np.int32)
        path[-1] = L - 1
        d_path = torch.from_numpy(path).cuda()
        outs = dev(T, torch.float32)
        k = (ptrs([d_path] * n), ptrs(outs))
        return (k[0][0], k[1][0]), outs, (k, d_path)
    if call == "label_posteriors":
        outs = dev((T, V), torch.float32)
        k = (ptrs(outs), _i64_array([V] * n))
        return (terms[0], k[0][0], k[1][0]), outs, (k, terms)
    if call == "state_posteriors":
        frames = np.unique(np.linspace(0, T - 1, QUERIES).astype(np.int64))
        W = min(BEAM, L)
        outs, los = dev((len(frames), W), torch.float32), dev(len(frames), torch.int64)
        k = (_ptr_array([frames.ctypes.data] * n), _i64_array([len(frames)] * n), ptrs(outs), _i64_array([W] * n), ptrs(los))
        return (terms[0], k[0][0], k[1][0], k[2][0], k[3][0], k[4][0]), outs + los, (k, terms, frames)
    if call == "boundary_quantiles":
        cuts = np.unique(2 * np.linspace(0, S, CUTS).astype(np.int64))
        levels = np.asarray(LEVELS, np.float64)
        outs = dev((len(cuts), len(levels)), torch.int32)
        k = (_ptr_array([cuts.ctypes.data] * n), _i64_array([len(cuts)] * n), ptrs(outs), _i64_array([len(levels)] * n))
        return (terms[0], k[0][0], k[1][0], levels.ctypes.data, len(levels), k[2][0], k[3][0]), outs, (k, terms, cuts, levels)
    if call == "sample_paths":
        ks, seeds = np.full(n, SAMPLES, np.int32), np.full(n, SEED, np.uint64)
        outs = dev((SAMPLES, T), torch.int32)
        k = (ptrs(outs), _i64_array([T] * n))
        return (terms[0], ks.ctypes.data, seeds.ctypes.data, k[0][0], k[1][0]), outs, (k, terms, ks, seeds)
    if call == "mea_path":
        ea = np.zeros(n, np.float64)
        outs = dev(T, torch.int32)
        k = (ptrs(outs),)
        return (terms[0], k[0][0], ea.ctypes.data), outs, (k, terms, ea)
    outs, sums = dev(L, torch.float64), dev(L, torch.float64)      # state_durations, state_visits
    k = (ptrs(outs), ptrs(sums))
    return (terms[0], k[0][0], k[1][0]), outs + sums, (k, terms)


def run_case(name, n, form, calls, reps, out_path=None):
    V = 64 if form == "fast" else 65
    lps, labs = cfg2(n, V)
    T, S = int(lps[0].shape[0]), int(labs[0].shape[0])
    dev = torch.cuda.current_device()
    eng = _lib.default_engine(dev)
    band = torch.from_numpy(np.ascontiguousarray(ka.diagonal_band(T, 2 * S + 1, BEAM), np.int32)).cuda()   # one table, n pointers to it
    kb = _ptr_array([band.data_ptr()] * n)
    k_lp, k_lab = _ptr_array([x.data_ptr() for x in lps]), _ptr_array([x.data_ptr() for x in labs])
    pT, pS, pld = _i64_array([T] * n), _i64_array([S] * n), _i64_array([x.stride(0) for x in lps])
    status, ll = np.zeros(n, np.int32), np.zeros(n, np.float64)
    stream = _stream_ptr(dev)
    lines = []
    for call in calls:
        own, outs, _keep = own_arguments(call, n, T, S, V)
        head = (eng.handle, n, k_lp[0], pT[0], V, pld[0], k_lab[0], pS[0], BEAM, MAX_MOVE)
        tail = (ll.ctypes.data, status.ctypes.data, _lib.KA_MEM_DEVICE, stream)

        def sibling():
            _lib.check(getattr(eng.lib, f"ka_ctc_{call}_batch_f32")(*head, *own, *tail), call)

        def banded():
            _lib.check(getattr(eng.lib, f"ka_ctc_{call}_banded_batch_f32")(*head, kb[0], *own, *tail), call + "_banded")

        sibling()                                    # warm-up of both, and the comparison
        want = [x.clone() for x in outs]
        want_ll = ll.copy()
        for x in outs:
            x.fill_(-7)
        banded()
        same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs, want)) and \
            np.array_equal(ll.view(np.uint64), want_ll.view(np.uint64))
        del want
        ms = {"banded": [], "sibling": []}
        for _ in range(reps):
            for what, fn in (("banded", banded), ("sibling", sibling)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()                                 # (both synchronise their stream)
                ms[what].append((time.perf_counter() - t0) * 1e3)
        for what in ("sibling", "banded"):
            line = {"case": name, "form": form, "call": call, "symbol": what, "n": n, "T": T, "S": S, "V": V, "beam": BEAM,
                    "ms_min": round(min(ms[what]), 3), "ms_all": [round(x, 3) for x in ms[what]],
                    "frames_per_s": round(n * T / (min(ms[what]) * 1e-3))}
            if what == "banded":
                line["ratio_to_sibling"] = round(min(ms["banded"]) / min(ms["sibling"]), 4)
                line["same_bits_as_sibling"] = bool(same)
            lines.append(line)
            print(json.dumps(line), flush=True)
            if out_path:                             # (line by line: a run that is cut short keeps what it measured)
                with open(out_path, "a") as out:
                    out.write(json.dumps(line) + "\n")
        del outs, own, _keep
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="single,b768")
    ap.add_argument("--forms", default="fast,generic")
    ap.add_argument("--calls", default=",".join(CALLS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = {"single": 1, "b768": 768}
    for form in args.forms.split(","):
        for name in args.cases.split(","):
            run_case(name, sizes[name], form, args.calls.split(","), args.reps, args.out)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
