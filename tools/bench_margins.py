"""Wall time of the path-margin call (ka_ctc_path_margins_batch_f32) against the two calls it sits
between: ka_ctc_label_posteriors_batch_f32, the cheapest existing call that recomputes whole columns (the same three passes
with five software transcendentals per cell), and ka_ctc_best_path_banded_batch_f32 on the diagonal table, the one-wavefront
best path.  One cfg2 lattice and 1024 cfg2 lattices (T = 50 000, S = 5000, beam 1000, V = 64); device-resident hash-generated
inputs; the path is the banded call's own best path, the terminal its last position.  The three calls alternate in one process
after a warm-up round, 3 repetitions, the minimum counts; a call's time is a host clock around a call that synchronises.

    python tools/bench_margins.py [--cases single,b1024] [--reps 3] [--out profiles/margin_bench.jsonl] [--T 50000 --S 5000]

One JSON line per case and call: ms per call (min and all repetitions); on the margin line its ratios to the other two, the
share of frames without an alternative, the share at which
the float32 best path is the float64 recurrence's best, and the median margin."""
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
from kokoro_align_amd._lattices import _i64_array, _ptr_array  # noqa: E402

BEAM, MAX_MOVE, V = 1000, 4, 64


def inputs(n, T, S, seed0=9000):
    lib = _lib.load_library()
    lp = torch.empty((n, T, V), dtype=torch.float32, device="cuda")
    lab = torch.empty((n, S), dtype=torch.int32, device="cuda")
    _lib.check(lib.ka_hash_logprobs_batch_f32(lp.data_ptr(), n, T, V, V, T * V, seed0, None), "hash")
    _lib.check(lib.ka_hash_labels_batch_i32(lab.data_ptr(), n, S, V, S, seed0, None), "hash")
    torch.cuda.synchronize()
    return list(lp.unbind(0)), list(lab.unbind(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="single,b1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--T", type=int, default=50000)
    ap.add_argument("--S", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "margin_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_margins.py needs a GPU"
    eng = _lib.default_engine(torch.cuda.current_device())
    lib = eng.lib
    T, S, L = args.T, args.S, 2 * args.S + 1
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
        occ = dev((T, V), torch.float32)
        p_occ = ptrs(occ)
        through, alt, runner = dev(T, torch.float64), dev(T, torch.float64), dev(T, torch.int32)
        p_thr, p_alt, p_run = ptrs(through), ptrs(alt), ptrs(runner)
        st = np.zeros(n, np.int32)
        z = np.zeros(n, np.float64)
        terms = None
        head = (eng.handle, n, p_lp[0], p_T[0], V, p_ld[0], p_lab[0], p_S[0], BEAM, MAX_MOVE)
        tail = (st.ctypes.data, _lib.KA_MEM_DEVICE, None)

        def best_path():
            return lib.ka_ctc_best_path_banded_batch_f32(*head, p_tab[0], p_path[0], p_blab[0], p_bsc[0], total.ctypes.data, *tail)

        def label_posteriors():
            return lib.ka_ctc_label_posteriors_batch_f32(*head, terms[0], p_occ[0], p_ld[0], z.ctypes.data, *tail)

        def margins():
            return lib.ka_ctc_path_margins_batch_f32(*head, None, p_path[0], 1, p_thr[0], p_alt[0], p_run[0], z.ctypes.data, *tail)

        _lib.check(best_path(), "best path")               # the path the other two are asked about
        terms = _i64_array([int(p[-1].item()) for p in paths])
        calls = (("best_path_banded", best_path), ("label_posteriors", label_posteriors), ("path_margins", margins))
        times = {name: [] for name, _ in calls}
        for rep in range(-1, args.reps):                   # round -1 warms every shape up
            for name, fn in calls:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = fn()
                dt = (time.perf_counter() - t0) * 1e3
                _lib.check(rc, name)
                if rep >= 0:
                    times[name].append(dt)
        th, al = through[0].cpu().numpy(), alt[0].cpu().numpy()
        with np.errstate(invalid="ignore"):
            margin = th - al
        # (the banded call's path is best in float32; the share of frames at which it is also the float64 recurrence's best)
        on_best = float(np.mean(th == z[0]))
        best = {name: min(v) for name, v in times.items()}
        for name, _ in calls:
            rec = dict(case=case, n=n, T=T, S=S, V=V, beam=BEAM, call=name, ms=round(best[name], 3), all_ms=[round(x, 3) for x in times[name]])
            if name == "path_margins":
                rec.update(vs_label_posteriors=round(best[name] / best["label_posteriors"], 4),
                           vs_best_path_banded=round(best[name] / best["best_path_banded"], 3),
                           frames_per_s=round(n * T / (best[name] * 1e-3), 1), no_alternative=float(np.mean(np.isinf(margin))), path_on_float64_best=on_best,
                           median_margin=float(np.median(margin[np.isfinite(margin)])))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del lps, labs, occ, through, alt, runner, paths, blabs, bsc
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "wt") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
