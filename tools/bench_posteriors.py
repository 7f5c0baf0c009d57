"""Wall time of ka_ctc_path_posteriors_batch_f32 (best-path posteriors + lattice log-likelihood, ka_posterior.hpp) on the
shapes of DESIGN.md section 4.17: one cfg2 lattice, cfg2 batches of 1024 and 8192, the corpus stand-in (workloads.corpus());
and of ka_ctc_label_posteriors_batch_f32 (label occupancy, ka_occupancy.hpp, section 4.18) on the same cfg2 shapes, the
terminal taken from the best path (cases occ_single, occ_b1024, occ_b8192); and of ka_ctc_state_posteriors_batch_f32 (state
posteriors at chosen frames, ka_state_posterior.hpp, section 4.19) with 200 query frames spread over every lattice (cases
state_single, state_b1024); and of ka_ctc_state_durations_batch_f32 (expected state durations, ka_duration.hpp, section 4.22)
on the occupancy's shapes and terminals (cases dur_single, dur_b1024); and of ka_ctc_sample_paths_batch_f32 (64 alignments
sampled from the band posterior per lattice, ka_sample.hpp, section 4.24) on the same shapes and terminals (cases smp_single,
smp_b1024); and of ka_ctc_mea_path_batch_f32 (the maximum-expected-accuracy alignment, ka_mea.hpp, section 4.26) on the same
shapes and terminals (cases mea_single, mea_b1024); and of ka_ctc_state_visits_batch_f32 (state visit probabilities,
ka_visit.hpp, section 4.27) on the same shapes and terminals (cases vis_single, vis_b1024); and of
ka_ctc_boundary_quantiles_batch_f32 (exact boundary-time quantiles, ka_quantile.hpp, section 4.28) at the levels 0.05, 0.5 and
0.95, with the cuts of boundary_cuts for a segment end every 500 frames of the best path (cases quant_single, quant_b768) and
with cuts at every even position (cases quantd_single, quantd_b768); b768 is a cfg2 batch of 768, three lattices per CU.

    python tools/bench_posteriors.py [--cases single,b1024,b8192,corpus] [--reps 3] [--out profiles/posteriors.jsonl]
    python tools/bench_posteriors.py --cases state_single,state_b1024 --out profiles/state_posteriors_bench.jsonl
    python tools/bench_posteriors.py --cases occ_single,dur_single,occ_b1024,dur_b1024,occ_single,dur_single,occ_b1024,dur_b1024 \
        --out profiles/duration_bench.jsonl
    python tools/bench_posteriors.py --cases occ_single,smp_single,occ_b1024,smp_b1024,occ_single,smp_single,occ_b1024,smp_b1024 \
        --out profiles/sample_bench.jsonl
    python tools/bench_posteriors.py --out profiles/mea_bench.jsonl --cases \
        occ_single,dur_single,mea_single,occ_b1024,dur_b1024,mea_b1024,occ_single,dur_single,mea_single,occ_b1024,dur_b1024,mea_b1024,occ_single,dur_single,mea_single,occ_b1024,dur_b1024,mea_b1024
    python tools/bench_posteriors.py --out profiles/visit_bench.jsonl --cases \
        occ_single,dur_single,vis_single,occ_b1024,dur_b1024,vis_b1024,occ_single,dur_single,vis_single,occ_b1024,dur_b1024,vis_b1024,occ_single,dur_single,vis_single,occ_b1024,dur_b1024,vis_b1024
    python tools/bench_posteriors.py --reps 5 --out profiles/quantile_bench.jsonl --cases \
        dur_single,quant_single,quantd_single,dur_b768,quant_b768,quantd_b768,dur_single,quant_single,quantd_single,dur_b768,quant_b768,quantd_b768,dur_single,quant_single,quantd_single,dur_b768,quant_b768,quantd_b768

Device-resident inputs (hash-generated); best paths from the library's own best-path call.  The 8192 batch points its
lattices at the 1024 batch's log-probs, labels and paths eight times over (distinct outputs): 105 GB of log-probs would
not be a better measurement.  One JSON line per case: ms per call (min, median over reps), frames/s."""
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
from kokoro_align_amd import _lib, workloads  # noqa: E402
from kokoro_align_amd.align import DeviceBatch, _i64_array, _ptr_array, _stream_ptr  # noqa: E402


def cfg2(n, seed0=9000, T=50000, V=64, S=5000):
    lib = _lib.load_library()
    lp = torch.empty((n, T, V), dtype=torch.float32, device="cuda")
    lab = torch.empty((n, S), dtype=torch.int32, device="cuda")
    _lib.check(lib.ka_hash_logprobs_batch_f32(lp.data_ptr(), n, T, V, V, T * V, seed0, None), "hash")
    _lib.check(lib.ka_hash_labels_batch_i32(lab.data_ptr(), n, S, V, S, seed0, None), "hash")
    torch.cuda.synchronize()
    return list(lp.unbind(0)), list(lab.unbind(0))


def best_paths(lps, labs):
    b = DeviceBatch(lps, labs, 1000, 4)
    b.run()
    return b.path


def time_batch(call_name, ws_name, lps, labs, own_args, reps, ws_own=()):
    """ms per call of ka_ctc_<call_name>_batch_f32 on device buffers: the arguments the six calls share around
    ``own_args`` (the caller keeps what they point to alive), the workspace reserved first, one warm-up call."""
    name = f"ka_ctc_{call_name}_batch_f32"
    n, V = len(lps), int(lps[0].shape[1])
    eng = _lib.default_engine(torch.cuda.current_device())
    ll = np.zeros(n, np.float64)
    st = np.zeros(n, np.int32)
    k = [_ptr_array([x.data_ptr() for x in xs]) for xs in (lps, labs)]
    T = _i64_array([x.shape[0] for x in lps])
    S = _i64_array([x.shape[0] for x in labs])
    ld = _i64_array([x.stride(0) for x in lps])
    stream = _stream_ptr(torch.cuda.current_device())

    def call():
        rc = getattr(eng.lib, name)(eng.handle, n, k[0][0], T[0], V, ld[0], k[1][0], S[0], 1000, 4, *own_args,
                                    ll.ctypes.data, st.ctypes.data, _lib.KA_MEM_DEVICE, stream)
        _lib.check(rc, name)

    eng.reserve(getattr(eng.lib, ws_name)(n, T[0], S[0], *ws_own, V, 1000, 4, _lib.KA_MEM_DEVICE))
    call()                                   # warm-up
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()                               # (the call synchronises its stream)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, st, ll


def time_posteriors(lps, labs, paths, reps):
    posts = [torch.empty(int(x.shape[0]), dtype=torch.float32, device="cuda") for x in lps]
    k = [_ptr_array([x.data_ptr() for x in xs]) for xs in (paths, posts)]
    return time_batch("path_posteriors", "ka_posterior_workspace_bytes", lps, labs, (k[0][0], k[1][0]), reps)


def time_occupancy(lps, labs, paths, reps):
    V = int(lps[0].shape[1])
    occs = [torch.empty((int(x.shape[0]), V), dtype=torch.float32, device="cuda") for x in lps]
    p_occ = _ptr_array([x.data_ptr() for x in occs])
    ldo = _i64_array([x.stride(0) for x in occs])
    term = _i64_array(torch.stack([p[-1] for p in paths]).cpu().tolist())
    return time_batch("label_posteriors", "ka_label_posterior_workspace_bytes", lps, labs, (term[0], p_occ[0], ldo[0]), reps)


def time_states(lps, labs, paths, reps, K=200):
    W = [min(1000, 2 * int(x.shape[0]) + 1) for x in labs]
    frames = [np.unique(np.linspace(0, int(x.shape[0]) - 1, K).astype(np.int64)) for x in lps]
    gammas = [torch.empty((len(f), w), dtype=torch.float32, device="cuda") for f, w in zip(frames, W)]
    los = [torch.empty(len(f), dtype=torch.int64, device="cuda") for f in frames]
    k = [_ptr_array([x.data_ptr() for x in xs]) for xs in (gammas, los)]
    fr = _ptr_array([f.ctypes.data for f in frames])
    Ks = _i64_array([len(f) for f in frames])
    ldo = _i64_array(W)
    term = _i64_array(torch.stack([p[-1] for p in paths]).cpu().tolist())
    return time_batch("state_posteriors", "ka_state_posterior_workspace_bytes", lps, labs, (term[0], fr[0], Ks[0], k[0][0], ldo[0], k[1][0]),
                      reps, ws_own=(Ks[0],))


def time_durations(lps, labs, paths, reps):
    durs = [torch.empty(2 * int(x.shape[0]) + 1, dtype=torch.float64, device="cuda") for x in labs]
    sums = [torch.empty(2 * int(x.shape[0]) + 1, dtype=torch.float64, device="cuda") for x in labs]
    k = [_ptr_array([x.data_ptr() for x in xs]) for xs in (durs, sums)]
    term = _i64_array(torch.stack([p[-1] for p in paths]).cpu().tolist())
    return time_batch("state_durations", "ka_state_duration_workspace_bytes", lps, labs, (term[0], k[0][0], k[1][0]), reps)


def time_visits(lps, labs, paths, reps):
    visits = [torch.empty(2 * int(x.shape[0]) + 1, dtype=torch.float64, device="cuda") for x in labs]
    exits = [torch.empty(2 * int(x.shape[0]) + 1, dtype=torch.float64, device="cuda") for x in labs]
    k = [_ptr_array([x.data_ptr() for x in xs]) for xs in (visits, exits)]
    term = _i64_array(torch.stack([p[-1] for p in paths]).cpu().tolist())
    return time_batch("state_visits", "ka_state_visit_workspace_bytes", lps, labs, (term[0], k[0][0], k[1][0]), reps)


def time_quantiles(lps, labs, paths, reps, dense, levels=(0.05, 0.5, 0.95)):
    if dense:
        cuts = [np.arange(0, 2 * int(x.shape[0]) + 2, 2, dtype=np.int64) for x in labs]
    else:
        cuts = [ka.boundary_cuts(p.cpu().numpy(), np.arange(500, int(p.shape[0]), 500), int(x.shape[0])) for p, x in zip(paths, labs)]
    lv = np.asarray(levels, np.float64)
    outs = [torch.empty((len(c), len(lv)), dtype=torch.int32, device="cuda") for c in cuts]
    p_out = _ptr_array([x.data_ptr() for x in outs])
    p_cut = _ptr_array([c.ctypes.data for c in cuts])
    Ks = _i64_array([len(c) for c in cuts])
    ldq = _i64_array([len(lv)] * len(cuts))
    term = _i64_array(torch.stack([p[-1] for p in paths]).cpu().tolist())
    return time_batch("boundary_quantiles", "ka_boundary_quantile_workspace_bytes", lps, labs,
                      (term[0], p_cut[0], Ks[0], lv.ctypes.data, len(lv), p_out[0], ldq[0]), reps, ws_own=(Ks[0], len(lv)))


def time_samples(lps, labs, paths, reps, K=64):
    outs = [torch.empty((K, int(x.shape[0])), dtype=torch.int32, device="cuda") for x in lps]
    p_out = _ptr_array([x.data_ptr() for x in outs])
    ldp = _i64_array([x.stride(0) for x in outs])
    term = _i64_array(torch.stack([p[-1] for p in paths]).cpu().tolist())
    Ks = np.full(len(lps), K, np.int32)
    seeds = np.arange(len(lps), dtype=np.uint64) + np.uint64(1)
    return time_batch("sample_paths", "ka_sample_paths_workspace_bytes", lps, labs, (term[0], Ks.ctypes.data, seeds.ctypes.data, p_out[0], ldp[0]),
                      reps, ws_own=(Ks.ctypes.data,))


def time_mea(lps, labs, paths, reps):
    outs = [torch.empty(int(x.shape[0]), dtype=torch.int32, device="cuda") for x in lps]
    p_out = _ptr_array([x.data_ptr() for x in outs])
    ea = np.zeros(len(lps), np.float64)
    term = _i64_array(torch.stack([p[-1] for p in paths]).cpu().tolist())
    return time_batch("mea_path", "ka_mea_path_workspace_bytes", lps, labs, (term[0], p_out[0], ea.ctypes.data), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="single,b1024,b8192,corpus")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = []
    cases = a.cases.split(",")
    b1024 = b768 = None
    for case in cases:
        kind = case.split("_")[0] if case.startswith(("occ_", "state_", "dur_", "smp_", "mea_", "vis_", "quant_", "quantd_")) else "path"
        case_in = case[len(kind) + 1:] if kind != "path" else case
        if case_in == "single":
            lps, labs = cfg2(1)
        elif case_in in ("b1024", "b8192"):
            if b1024 is None:
                lps, labs = cfg2(1024)
                b1024 = (lps, labs, best_paths(lps, labs))
            lps, labs, paths = b1024
            if case_in == "b8192":
                lps, labs, paths = lps * 8, labs * 8, paths * 8
        elif case_in == "b768":
            if b768 is None:
                lps, labs = cfg2(768)
                b768 = (lps, labs, best_paths(lps, labs))
            lps, labs, paths = b768
        elif case_in == "corpus":
            lps, labs = [], []
            for k, (name, shapes) in enumerate(workloads.corpus()):
                x, y = workloads.device_book(shapes, seed0=workloads.corpus_seed0(k))
                lps += x
                labs += y
        else:
            raise SystemExit(f"unknown case {case}")
        if case_in in ("single", "corpus"):
            paths = best_paths(lps, labs)
        ms, st, ll = {"path": time_posteriors, "occ": time_occupancy, "state": time_states, "dur": time_durations, "smp": time_samples,
                       "mea": time_mea, "vis": time_visits, "quant": lambda *x: time_quantiles(*x, dense=False),
                       "quantd": lambda *x: time_quantiles(*x, dense=True)}[kind](lps, labs, paths, a.reps)
        frames = sum(int(x.shape[0]) for x in lps)
        line = dict(case=case, lattices=len(lps), frames=frames, ms_min=round(min(ms), 3), ms_median=round(float(np.median(ms)), 3),
                    frames_per_s=frames / (min(ms) / 1e3), status_ok=int((st == 0).sum()), reps=a.reps)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
