// ka_engine.hip — the engine and the best-path calls of the C ABI declared in include/kokoro_align_amd.h.
//
// Host code only: the kernels live in the device translation units and are reached through ka_launch.hpp; the planning of a
// launch (forms, tile plans, cost models, workspace layout) is ka_plan.hpp; the engine object is ka_engine.hpp.  Here: create
// and destroy, the settings, a best-path launch - plan_launch (checks and planning: no HIP call, the engine untouched), then
// enqueue_planned (descriptors, copies, kernel order, the second stream of mixed launches) - ka_batch_finish with its redo, and
// the ka_debug_* entry points.  The forward-backward calls are ka_engine_fb.hip, the entry points that need no engine
// ka_entry_misc.hip.  No torch, no oracle, no CPU fallback: if HIP fails the call fails.
#include "ka_engine.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

static_assert(ka::plan::kModeAuto == KA_MODE_AUTO && ka::plan::kModeWave == KA_MODE_WAVE && ka::plan::kModeWaveExact == KA_MODE_WAVE_EXACT &&
                  ka::plan::kModeTiled == KA_MODE_TILED && ka::plan::kBacktraceAuto == KA_BACKTRACE_AUTO &&
                  ka::plan::kBacktraceSerial == KA_BACKTRACE_SERIAL && ka::plan::kBacktraceParallel == KA_BACKTRACE_PARALLEL,
              "ka_plan.hpp's mode codes are the public header's");

thread_local std::string ka::host::g_err;

namespace {

using namespace ka::host;
using ka::plan::align_up;
using ka::plan::LaunchPlan;
using ka::plan::Shape;

// the caller's arrays of one batch call
struct BatchArgs {
    const float *const *log_probs;
    const int64_t *T;
    const int64_t *ld;
    const int32_t *const *labels;
    const int64_t *S;
    int32_t *const *best_path;
    int32_t *const *best_labels;
    float *const *best_scores;
};

// device addresses of the launch's shared structures
struct DevicePtrs {
    ka::Lattice *lats;
    int32_t *meta;
};

// ---- step 3b: descriptors (pinned memory), in descriptor order ----
// (`redo`: where the wide tiled lattices are noted for ka_batch_finish, or nullptr)
void fill_descriptors(char *ws, const LaunchPlan &p, const BatchArgs &a, ka::Lattice *h_lats, std::vector<ka_engine::Redo> *redo)
{
    using ka::plan::chunks_of_T;
    int64_t chunk_cursor = 0;
    for (int32_t k = 0; k < p.n; ++k) {
        const int32_t i = p.order[k];
        const Shape &sh = p.sh[i];
        const ka::plan::Carve &cv = p.cv[i];
        ka::Lattice &d = h_lats[k];
        std::memset(&d, 0, sizeof(d));
        // chunks of the launch's chunk-parallel lattices are numbered consecutively; a lattice that is walked back serially
        // carries the running total and owns none (lattice_of_chunk picks the LAST descriptor whose chunk0 <= chunk)
        d.chunk0 = chunk_cursor;
        d.par = sh.par_bt ? 1 : 0;
        if (sh.par_bt) chunk_cursor += chunks_of_T(sh.T);
        if (p.host_buffers) {
            d.lp = reinterpret_cast<const float *>(ws + cv.lp);
            d.labels = reinterpret_cast<const int32_t *>(ws + cv.lab);
            d.path = reinterpret_cast<int32_t *>(ws + cv.path);
            d.lab_out = reinterpret_cast<int32_t *>(ws + cv.labo);
            d.sc_out = reinterpret_cast<float *>(ws + cv.sco);
            d.ld = p.V;
        } else {
            d.lp = a.log_probs[i];
            d.labels = a.labels[i];
            d.path = a.best_path[i];
            d.lab_out = a.best_labels[i];
            d.sc_out = a.best_scores[i];
            d.ld = a.ld[i];
        }
        d.labx = reinterpret_cast<int32_t *>(ws + cv.labx);
        d.bp = ws + cv.bp;
        d.col = reinterpret_cast<float *>(ws + cv.col);
        d.T = (int32_t)sh.T;
        d.S = (int32_t)sh.S;
        d.L = (int32_t)sh.L;
        d.V = p.V;
        d.beam = p.beam;
        d.max_move = p.max_move;
        d.labx_len = sh.labx_len;
        d.W = (int32_t)sh.W;
        d.idx = i;
        d.n_final = sh.tiled ? sh.n_final : 0;
        d.ck_mask = sh.tiled ? sh.ck_mask : 1023u;
        d.ck_pitch = sh.tiled ? (int32_t)sh.ck_pitch : 4096;
        d.map0 = reinterpret_cast<uint8_t *>(ws + cv.map0);
        d.map1 = reinterpret_cast<uint16_t *>(ws + cv.map1);
        d.entry = reinterpret_cast<int32_t *>(ws + cv.entry);
        if (redo && sh.tiled && !sh.fast) redo->push_back({a.log_probs[i], a.labels[i], a.best_path[i], a.best_labels[i], a.best_scores[i], a.T[i], a.S[i], a.ld[i], i});
    }
}

// ---- what ka_debug_chunk_entries and ka_debug_tile_stats may read back after this launch ----
ka_engine::DebugView debug_view_of(const LaunchPlan &p)
{
    using ka::plan::chunks_of_T;
    using ka::plan::supers_of_T;
    const Shape &sh = p.sh[p.order[0]];
    const ka::plan::Carve &cv = p.cv[p.order[0]];
    ka_engine::DebugView v;
    v.entry = cv.entry;
    v.entry_n = sh.par_bt ? (size_t)(chunks_of_T(sh.T) + supers_of_T(sh.T)) : 0;
    v.map0 = cv.map0;
    v.map0_bytes = sh.par_bt ? (size_t)chunks_of_T(sh.T) * ((sh.tiled ? sh.ck_pitch : 4096) / 4) : 0;
    // checkpoint rows: the tiled forms, and the one-wavefront form unless it stores back-pointers (enqueue_forward)
    const bool checkpointed = sh.tiled || (sh.fast && p.checkpointed_waves && sh.T < (int64_t(1) << 26));
    v.ck = cv.bp;
    v.ck_pitch = sh.tiled ? sh.ck_pitch : 4096;
    v.ck_bytes = checkpointed ? (size_t)(chunks_of_T(sh.T) - 1) * v.ck_pitch : 0;
    v.ck_idx = p.order[0];
    v.tasks = p.off_tasks;
    v.stats = p.off_stats;
    v.n_tasks = p.n_tasks;
    return v;
}

// A mixed launch runs its two kernel forms side by side: the second one on the engine's own stream, forked from the
// caller's stream and joined to it again (events; nothing here blocks the host).
hipError_t fork_aux(ka_engine *e, hipStream_t stream, int k)
{
    if (!e->res.aux) {
        hipError_t er = hipStreamCreateWithFlags(&e->res.aux, hipStreamNonBlocking);
        if (er != hipSuccess) return er;
    }
    hipError_t er = hipEventRecord(e->res.sync[k], stream);
    return er != hipSuccess ? er : hipStreamWaitEvent(e->res.aux, e->res.sync[k], 0);
}
hipError_t join_aux(ka_engine *e, hipStream_t stream, int k)
{
    hipError_t er = hipEventRecord(e->res.sync[k], e->res.aux);
    return er != hipSuccess ? er : hipStreamWaitEvent(stream, e->res.sync[k], 0);
}

// The halo slots of the launch start as the NaN sentinel: always for the 128-position tiles' self-vouching packets
// (ka_tiled128.hpp), and under ka_engine_set_verify(1) for the 256-position form (a tile that consumes a slot nobody wrote
// reports KA_ERR_INTERNAL).
bool wants_halo_sentinel(const ka_engine *e, const LaunchPlan &p) { return p.halo_bytes && ((e->set.verify & 1) || p.narrow); }
int fill_halo_sentinel(ka_engine *e, const LaunchPlan &p, hipStream_t stream)
{
    if (!wants_halo_sentinel(e, p)) return KA_OK;
    const size_t lo = p.off_halo + p.ninf_bytes, hi = lo + p.halo_bytes;
    if (lo >= e->clean.lo && hi <= e->clean.hi) return KA_OK;      // (the refill behind the last launch's tiles: enqueue_planned has waited for it)
    KA_HIP(hipMemsetD32Async((hipDeviceptr_t)(e->res.ws + lo), (int)ka::kTpSentinel, p.halo_bytes / 4, stream));
    return KA_OK;
}
// ... and behind the launch's forward pass the slots are made the sentinel again, beside the backtrace (which does not touch
// them), for the next launch with the same or a smaller halo region.
int refill_halo_sentinel(ka_engine *e, const LaunchPlan &p, hipStream_t stream)
{
    e->clean.invalidate();
    if (!wants_halo_sentinel(e, p)) return KA_OK;
    if (!e->res.refill_done) KA_HIP(hipEventCreateWithFlags(&e->res.refill_done, hipEventDisableTiming));
    if (!e->res.refill_go) KA_HIP(hipEventCreateWithFlags(&e->res.refill_go, hipEventDisableTiming));
    if (!e->res.fill) KA_HIP(hipStreamCreateWithFlags(&e->res.fill, hipStreamNonBlocking));
    KA_HIP(hipEventRecord(e->res.refill_go, stream));
    KA_HIP(hipStreamWaitEvent(e->res.fill, e->res.refill_go, 0));
    const size_t lo = p.off_halo + p.ninf_bytes;
    KA_HIP(hipMemsetD32Async((hipDeviceptr_t)(e->res.ws + lo), (int)ka::kTpSentinel, p.halo_bytes / 4, e->res.fill));
    KA_HIP(hipEventRecord(e->res.refill_done, e->res.fill));
    e->clean.lo = lo;
    e->clean.hi = lo + p.halo_bytes;
    return KA_OK;
}

// ---- the tile pipeline of the launch's tiled lattices (descriptors [0, n_tiled)) ----
int enqueue_tiles(ka_engine *e, const LaunchPlan &p, const BatchArgs &a, const DevicePtrs &dv, hipStream_t stream)
{
    // 40 KB of LDS per tile workgroup = four workgroups per CU; when the launch has no more tiles than two per CU, 80 KB
    // keeps them at two per CU, i.e. (two wavefronts each) one wavefront per SIMD: two tiles whose wavefronts share a SIMD
    // run at 95-106 ns per frame instead of 55-62, and a chain runs at the pace of its slowest tile (cfg5's whole lattice,
    // 391 tiles alive for all 500 000 frames: profiles/r03_tile_stats_cfg5_full.txt)
    const unsigned lds = e->set.tile_lds ? (unsigned)e->set.tile_lds : ((int64_t)p.n_tasks <= (int64_t)e->set.knobs.n_simd / 2 ? 2u * ka::kTpLdsRequest : ka::kTpLdsRequest);
    ka::TileLaunch tl;
    tl.lats = dv.lats;
    tl.tasks = reinterpret_cast<const ka::TileTask *>(e->res.ws + p.off_tasks);
    tl.n_tasks = (int)p.n_tasks;
    tl.meta = dv.meta;
    tl.halo = e->res.ws + p.off_halo;
    tl.prog = reinterpret_cast<uint32_t *>(e->res.ws + p.off_prog);
    tl.aux = reinterpret_cast<ka::TileAux *>(e->res.ws + p.off_aux);
    tl.ticket = reinterpret_cast<uint32_t *>(e->res.ws + p.off_ticket);
    tl.verify = e->set.verify;
    tl.stats = reinterpret_cast<ka::TpStats *>(e->res.ws + p.off_stats);
    tl.cu_rank = reinterpret_cast<uint32_t *>(e->res.ws + p.off_cu_rank);
    tl.max_move = p.max_move;
    // staging mode: when every tiled lattice's rows are contiguous (row stride = V, V = 64 or 39, 16-byte aligned) a block
    // is copied as it lies in memory (1 KB per LDS-DMA instruction); otherwise row by row
    tl.pitch = ((p.V == 64 || p.V == 39) && p.max_move == 4) ? 4 * p.V : 0;
    for (int32_t k = 0; k < p.n_tiled && tl.pitch; ++k) {
        const int32_t i = p.order[k];
        const bool contiguous = p.host_buffers || (a.ld[i] == p.V && ((uintptr_t)a.log_probs[i] & 15) == 0);
        if (!contiguous) tl.pitch = 0;
    }
    if (p.narrow) {
        // Three of these workgroups fit a CU, and three that are alive together slow each other down: a tile puts ~28 cycles of
        // traffic per frame on the CU's LDS pipe (pairs written and read, emission gathers, packets, staging) and runs a frame in
        // 86, so the pipe saturates (the Kokoro stand-in's frames took 101 cycles at three per CU, 95 at two, 86 alone:
        // tools/tile_stats_book.py).  While the launch's tiles that are alive at once fit two per CU - with some slack: a tile
        // that waits a little for a slot costs less than sharing the pipe - ask for the LDS that keeps them at two.
        const int64_t n_cu = e->set.knobs.n_simd / 4;
        tl.lds = (unsigned)e->set.tile_lds;      // (0: what the kernel needs, 46-52 KB; the launch function takes the larger)
        if (!tl.lds && p.alive_tiles <= 11 * n_cu / 4) tl.lds = 64 * 1024;
        ka::launch_forward_tiled128(tl, stream);
    } else {
        // ... and when the tiles alive at once outnumber four per CU, no more than the kernel uses: with V = 39 and contiguous rows
        // that is 27 KB, FIVE workgroups per CU - a slot-bound launch (the corpus) wants slots more than it wants fast tiles
        tl.lds = (!e->set.tile_lds && p.alive_tiles > (int64_t)e->set.knobs.n_simd) ? 0u : lds;
        ka::launch_forward_tiled256(tl, stream);
    }
    return KA_OK;
}

// ---- forward pass: [0, n_tiled) tiled, [n_tiled, n_ring) one wavefront each, the rest generic.  Returns (through
// `wave_form`) which form the one-wavefront lattices ended up in. ----
int enqueue_forward(ka_engine *e, const LaunchPlan &p, const BatchArgs &a, const DevicePtrs &dv, hipStream_t stream, ka::WaveForm *wave_form)
{
    const int32_t n_tiled = p.n_tiled, n_fast = p.n_fast, n_ring = p.n_ring();
    const bool two_forward = n_tiled > 0 && n_fast > 0;
    if (two_forward) KA_HIP(fork_aux(e, stream, 0));      // (before the tile kernel is enqueued: the second stream must not wait for it)
    ka::WaveForm form = n_tiled > 0 ? ka::kWaveCheckpointed : ka::kWaveExact;
    if (n_tiled > 0) {
        const int rc = enqueue_tiles(e, p, a, dv, stream);
        if (rc != KA_OK) return rc;
    }
    if (n_fast > 0) {
        form = p.checkpointed_waves ? ka::kWaveCheckpointed : ka::kWaveExact;
        // backtrace_rc_kernel keeps 34*T in 32 bits (descriptors are sorted longest first)
        if (form == ka::kWaveCheckpointed && p.sh[p.order[n_tiled]].T >= (int64_t(1) << 26)) form = ka::kWaveExact;
        ka::launch_forward_wave(p.max_move, dv.lats + n_tiled, n_fast, dv.meta, two_forward ? e->res.aux : stream, form);
    }
    // tiled lattices that the scores-only form declined (non-finite log-probs) and that fit the one-wavefront ring are
    // redone by the exact kernels (kFlagExact; wider ones get kFlagDeclined and are handed to the generic kernels by
    // ka_batch_finish)
    if (n_tiled > 0) ka::launch_forward_flagged(p.max_move, dv.lats, n_tiled, dv.meta, stream);
    if (two_forward) KA_HIP(join_aux(e, stream, 1));
    if (p.n > n_ring) ka::launch_forward_generic(dv.lats + n_ring, p.n - n_ring, dv.meta, stream);
    *wave_form = form;
    return KA_OK;
}

// ---- backtrace: checkpointed results (tiled + checkpointed one-wavefront form) by recomputation, stored back-pointers by
// the walk.  Returns (through `rc_hi`) the end of the descriptor range [0, rc_hi) whose outputs backtrace_rc writes itself. ----
int enqueue_backtrace(ka_engine *e, const LaunchPlan &p, const DevicePtrs &dv, hipStream_t stream, ka::WaveForm wave_form, int32_t *rc_hi_out)
{
    using ka::plan::chunks_of_T;
    using ka::plan::supers_of_T;
    const int32_t n_ring = p.n_ring();
    const int32_t rc_hi = p.n_tiled + (wave_form == ka::kWaveCheckpointed ? p.n_fast : 0);
    if (rc_hi > 0) {
        // the chunk-parallel lattices of the range (Lattice::par; their chunks are numbered consecutively) and the others
        int64_t total_chunks = 0, max_seg = 1, max_sup = 1, max_w = 1;
        int32_t n_par = 0;
        for (int32_t k = 0; k < rc_hi; ++k) {
            const Shape &q = p.sh[p.order[k]];
            if (!q.par_bt) continue;
            ++n_par;
            total_chunks += chunks_of_T(q.T);
            max_sup = std::max<int64_t>(max_sup, supers_of_T(q.T));
            max_w = std::max<int64_t>(max_w, q.W);
        }
        // segments of the band a map wavefront delivers: 408 positions (8 cells per lane) when every band fits one such
        // wavefront, else 1048 (18 cells: the reference's band of 1000 in one wavefront instead of three)
        max_seg = (max_w + 7 + ka::cm_out_for(max_w) - 1) / ka::cm_out_for(max_w);
        const bool two_backtraces = n_par > 0 && n_par < rc_hi;
        if (n_par < rc_hi) {      // one wavefront per lattice, chunk after chunk (skips the chunk-parallel ones)
            if (two_backtraces) KA_HIP(fork_aux(e, stream, 2));
            ka::launch_backtrace_rc_serial(p.max_move, dv.lats, rc_hi, dv.meta, two_backtraces ? e->res.aux : stream);
        }
        if (n_par > 0) {
            ka::launch_chunk_entries(p.max_move, dv.lats, rc_hi, dv.meta, stream, (unsigned)total_chunks, (unsigned)max_seg, (unsigned)max_sup, (unsigned)max_w);
            ka::launch_backtrace_rc_chunks(p.max_move, dv.lats, rc_hi, dv.meta, stream, (unsigned)total_chunks);
        }
        if (two_backtraces) KA_HIP(join_aux(e, stream, 3));
        ka::launch_backtrace_w16(dv.lats, rc_hi, dv.meta, stream, 1);      // only what the exact kernels redid
    }
    if (n_ring > rc_hi) ka::launch_backtrace_w16(dv.lats + rc_hi, n_ring - rc_hi, dv.meta, stream, 0);
    if (p.n > n_ring) ka::launch_backtrace_generic(dv.lats + n_ring, p.n - n_ring, dv.meta, stream);
    *rc_hi_out = rc_hi;
    return KA_OK;
}

// ---- labels and scores of the lattices whose backtrace wrote the path only ----
void enqueue_output_gathers(const LaunchPlan &p, const DevicePtrs &dv, hipStream_t stream, int32_t rc_hi)
{
    int64_t t_max = 1;
    for (int32_t i = 0; i < p.n; ++i) t_max = std::max<int64_t>(t_max, p.sh[i].T);
    const unsigned gx = (unsigned)((t_max + 1023) / 1024);
    for (int32_t y0 = 0; y0 < rc_hi; y0 += 65535)     // only what the exact kernels redid
        ka::launch_gather_outputs(dv.lats + y0, 1, (unsigned)std::min<int32_t>(65535, rc_hi - y0), dv.meta, stream, 1);
    for (int32_t y0 = rc_hi; y0 < p.n; y0 += 65535)   // grid.y limit
        ka::launch_gather_outputs(dv.lats + y0, gx, (unsigned)std::min<int32_t>(65535, p.n - y0), dv.meta, stream, 0);
}

// The caller's side of a launch that needs no engine: argument checks, then steps 1 and 2 (ka_plan.hpp).  No HIP call, and
// nothing but `p` is written; n = 0 leaves the empty plan.
int plan_launch(const ka::plan::Knobs &kn, int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move, int32_t mem,
                LaunchPlan &p)
{
    p = LaunchPlan();
    if (n < 0 || (n > 0 && (!T || !S))) return fail(KA_ERR_BAD_ARGS, "batch: NULL array argument");
    if (mem != KA_MEM_HOST && mem != KA_MEM_DEVICE) return fail(KA_ERR_BAD_ARGS, "mem must be KA_MEM_HOST or KA_MEM_DEVICE");
    if (n == 0) return KA_OK;
    const int32_t bad = ka::plan::plan_forms(p, n, T, S, V, beam_size, max_move, mem == KA_MEM_HOST, kn);
    if (bad >= 0) return fail(KA_ERR_BAD_ARGS, "lattice " + std::to_string(bad) + ": unsupported T/S/V/ld/beam_size/max_move");
    ka::plan::carve_workspace(p);
    return KA_OK;
}

// Step 3: enqueues a planned launch (p.n > 0) on `stream`: descriptors and tile tasks in pinned memory, copies in, kernels,
// copies out.  `timed`: the five profiling events are recorded around the kernels.  `redo`: see fill_descriptors.  The pinned
// status records, valid once the stream has been synchronised, come back through `meta_out`.  The engine's buffers, halo-clean
// range and debug view follow the launch; the batch in flight is the caller's business.
int enqueue_planned(ka_engine *e, const LaunchPlan &p, const BatchArgs &a, hipStream_t stream, bool timed, std::vector<ka_engine::Redo> *redo,
                    const ka::LatticeMeta **meta_out)
{
    const int32_t n = p.n, V = p.V;
    int rc = ensure_ws(e, p.total_bytes);
    if (rc != KA_OK) return rc;
    rc = ensure_pin(e, p.pinned_bytes());
    if (rc != KA_OK) return rc;
    // The refill behind the LAST launch's tiles runs on a stream of its own and nothing has waited for it yet: this launch
    // lays its regions out from the start of the same workspace, and its first copies and fills must not race a fill that is
    // still writing sentinels there (descriptors overwritten by a late refill were a memory fault with four engines running
    // launches of different shapes: tools/stress_streams_tiled.py).
    if (e->res.refill_done) KA_HIP(hipStreamWaitEvent(stream, e->res.refill_done, 0));
    // (... and a launch without the sentinel protocol - other kernel forms, the generic redo of ka_batch_finish - writes over
    //  what that refill left clean)
    if (!wants_halo_sentinel(e, p)) e->clean.invalidate();
    e->dbg = debug_view_of(p);

    ka::Lattice *h_lats = reinterpret_cast<ka::Lattice *>(e->res.pin);
    ka::LatticeMeta *h_meta = reinterpret_cast<ka::LatticeMeta *>(e->res.pin + align_up((size_t)n * sizeof(ka::Lattice)));
    ka::TileTask *h_tasks = reinterpret_cast<ka::TileTask *>(e->res.pin + align_up((size_t)n * sizeof(ka::Lattice)) + align_up((size_t)n * sizeof(ka::LatticeMeta)));
    fill_descriptors(e->res.ws, p, a, h_lats, redo);
    if (p.host_buffers)
        for (int32_t i = 0; i < n; ++i) {
            KA_HIP(hipMemcpy2DAsync(e->res.ws + p.cv[i].lp, (size_t)V * 4, a.log_probs[i], (size_t)a.ld[i] * 4, (size_t)V * 4, (size_t)p.sh[i].T,
                                    hipMemcpyHostToDevice, stream));
            if (p.sh[i].S > 0) KA_HIP(hipMemcpyAsync(e->res.ws + p.cv[i].lab, a.labels[i], (size_t)p.sh[i].S * 4, hipMemcpyHostToDevice, stream));
        }
    DevicePtrs dv;
    dv.lats = reinterpret_cast<ka::Lattice *>(e->res.ws + p.off_desc);
    dv.meta = reinterpret_cast<int32_t *>(e->res.ws + p.off_meta);
    KA_HIP(hipMemcpyAsync(dv.lats, h_lats, (size_t)n * sizeof(ka::Lattice), hipMemcpyHostToDevice, stream));
    KA_HIP(hipMemsetAsync(dv.meta, 0, (size_t)n * sizeof(ka::LatticeMeta), stream));
    // the device starts on what needs no tile tasks - the fills of the tile pipeline's regions, the label preparation - while
    // the host lists the tasks (a book has ~10 000)
    if (p.n_tiled) {
        KA_HIP(hipMemsetAsync(e->res.ws + p.off_zero, 0, p.zero_bytes, stream));
        KA_HIP(hipMemsetD32Async((hipDeviceptr_t)(e->res.ws + p.off_prog), (int)ka::kTpProgDone, 1, stream));
        KA_HIP(hipMemsetD32Async((hipDeviceptr_t)(e->res.ws + p.off_halo), (int)0xff800000u, p.ninf_bytes / 4, stream));   // -inf packets
        const int rcf = fill_halo_sentinel(e, p, stream);
        if (rcf != KA_OK) return rcf;
    }
    if (p.n_tiled) {
        // (the copy goes in FRONT of the label preparation, not between it and the tile kernel: with a copy right before them the
        //  whole 500 000 x 100 001 lattice's 391 permanent tiles were placed differently and ran 69 ms instead of 52)
        ka::plan::fill_tile_tasks(p, h_tasks);
        KA_HIP(hipMemcpyAsync(e->res.ws + p.off_tasks, h_tasks, p.n_tasks * sizeof(ka::TileTask), hipMemcpyHostToDevice, stream));
    }
    if (timed) KA_HIP(hipEventRecord(e->res.ev[0], stream));
    ka::launch_prep_labels(dv.lats, n, dv.meta, stream);
    if (timed) KA_HIP(hipEventRecord(e->res.ev[1], stream));
    ka::WaveForm wave_form = ka::kWaveExact;
    rc = enqueue_forward(e, p, a, dv, stream, &wave_form);
    if (rc != KA_OK) return rc;
    if (timed) KA_HIP(hipEventRecord(e->res.ev[2], stream));
    if (p.n_tiled) {
        rc = refill_halo_sentinel(e, p, stream);
        if (rc != KA_OK) return rc;
    }
    int32_t rc_hi = 0;
    rc = enqueue_backtrace(e, p, dv, stream, wave_form, &rc_hi);
    if (rc != KA_OK) return rc;
    if (timed) KA_HIP(hipEventRecord(e->res.ev[3], stream));
    enqueue_output_gathers(p, dv, stream, rc_hi);
    if (timed) KA_HIP(hipEventRecord(e->res.ev[4], stream));
    KA_HIP(hipGetLastError());

    KA_HIP(hipMemcpyAsync(h_meta, dv.meta, (size_t)n * sizeof(ka::LatticeMeta), hipMemcpyDeviceToHost, stream));
    if (p.host_buffers)
        for (int32_t i = 0; i < n; ++i) {
            const size_t b = (size_t)p.sh[i].T * 4;
            KA_HIP(hipMemcpyAsync(a.best_path[i], e->res.ws + p.cv[i].path, b, hipMemcpyDeviceToHost, stream));
            KA_HIP(hipMemcpyAsync(a.best_labels[i], e->res.ws + p.cv[i].labo, b, hipMemcpyDeviceToHost, stream));
            KA_HIP(hipMemcpyAsync(a.best_scores[i], e->res.ws + p.cv[i].sco, b, hipMemcpyDeviceToHost, stream));
        }
    *meta_out = h_meta;
    return KA_OK;
}

// The public enqueue: refuses a second batch, plans, enqueues, and only then notes the batch in flight for ka_batch_finish.
// (A call refused for its arrays or `mem` leaves even the last batch's times standing, so those checks come first here,
// with the arrays only a launch needs.)
int enqueue_batch(ka_engine *e, int32_t n, const BatchArgs &a, int32_t V, int32_t beam_size, int32_t max_move, int32_t mem, hipStream_t stream)
{
    if (!e) return fail(KA_ERR_BAD_ARGS, "engine is NULL");
    ka_engine::Batch &b = e->batch;
    if (b.pending) return fail(KA_ERR_BAD_ARGS, "a batch is already enqueued: call ka_batch_finish first");
    if (n < 0 || (n > 0 && (!a.T || !a.S || !a.log_probs || !a.ld || !a.labels || !a.best_path || !a.best_labels || !a.best_scores)))
        return fail(KA_ERR_BAD_ARGS, "batch: NULL array argument");
    if (mem != KA_MEM_HOST && mem != KA_MEM_DEVICE) return fail(KA_ERR_BAD_ARGS, "mem must be KA_MEM_HOST or KA_MEM_DEVICE");
    DeviceGuard guard;
    KA_HIP(guard.enter(e->device));
    b.have_times = false;
    b.redo.clear();
    LaunchPlan p;
    int rc = plan_launch(e->set.knobs, n, a.T, a.S, V, beam_size, max_move, mem, p);
    if (rc != KA_OK) return rc;
    for (int32_t i = 0; i < n; ++i) {
        if (a.ld[i] < V) return fail(KA_ERR_BAD_ARGS, "lattice " + std::to_string(i) + ": unsupported T/S/V/ld/beam_size/max_move");
        if (!a.log_probs[i] || !a.best_path[i] || !a.best_labels[i] || !a.best_scores[i] || (a.S[i] > 0 && !a.labels[i]))
            return fail(KA_ERR_BAD_ARGS, "lattice " + std::to_string(i) + ": NULL buffer");
    }
    if (n > 0 && (rc = enqueue_planned(e, p, a, stream, e->set.profiling, &b.redo, &b.meta)) != KA_OK) return rc;
    b.n = n;
    b.stream = stream;
    b.V = V;
    b.beam = beam_size;
    b.max_move = max_move;
    b.mem = mem;
    b.pending = true;
    return KA_OK;
}

// ka_batch_finish, second part: lattices in the tiled form whose band is wider than the exact kernels' ring and whose
// log-probs are not all finite (flag set by the forward kernel) have no result yet - the scores-only forms are valid only
// while "live" and "score > -inf" coincide.  The reference answers such input (align.py:67-85 tracks the live set
// explicitly), so they are handed to the generic kernels now, into the caller's buffers.  `meta` is the finished batch's
// host copy; a redo that cannot run marks ITS lattices with the error and leaves the others' results standing.
void redo_declined(ka_engine *e, const std::vector<ka_engine::Redo> &again, std::vector<ka::LatticeMeta> &meta)
{
    const int32_t m = (int32_t)again.size();
    std::vector<const float *> lp(m);
    std::vector<const int32_t *> lab(m);
    std::vector<int32_t *> path(m), lab_out(m);
    std::vector<float *> sc(m);
    std::vector<int64_t> T(m), S(m), ld(m);
    for (int32_t j = 0; j < m; ++j) {
        lp[j] = again[j].lp; lab[j] = again[j].labels; path[j] = again[j].path; lab_out[j] = again[j].lab_out; sc[j] = again[j].sc_out;
        T[j] = again[j].T; S[j] = again[j].S; ld[j] = again[j].ld;
    }
    const BatchArgs a{lp.data(), T.data(), ld.data(), lab.data(), S.data(), path.data(), lab_out.data(), sc.data()};
    // a launch of its own on the batch's stream, without timing events and without a redo list: nothing it calls writes
    // what belongs to the batch itself
    const ka_engine::Batch &b = e->batch;
    ka::plan::Knobs kn = e->set.knobs;
    kn.force_generic = true;
    LaunchPlan p;
    const ka::LatticeMeta *redone = nullptr;
    int rc = plan_launch(kn, m, T.data(), S.data(), b.V, b.beam, b.max_move, b.mem, p);
    if (rc == KA_OK) rc = enqueue_planned(e, p, a, b.stream, /*timed=*/false, /*redo=*/nullptr, &redone);
    if (rc == KA_OK && hipStreamSynchronize(b.stream) != hipSuccess) rc = fail(KA_ERR_HIP, "hipStreamSynchronize after the redo of wide lattices with non-finite log-probs failed");
    for (int32_t j = 0; j < m; ++j) {
        ka::LatticeMeta &dst = meta[again[j].idx];
        if (rc == KA_OK) dst = redone[j];
        else dst.status = rc;       // (KA_ERR_NOMEM for the byte-per-cell workspace of a very wide lattice, most likely)
    }
}

}  // namespace

extern "C" {

int32_t ka_version(void) { return KA_VERSION; }

const char *ka_last_error(void) { return g_err.c_str(); }

int ka_engine_create(int32_t device, ka_engine **out)
{
    if (!out) return fail(KA_ERR_BAD_ARGS, "ka_engine_create: out is NULL");
    int ndev = 0;
    KA_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return fail(KA_ERR_BAD_ARGS, "ka_engine_create: device " + std::to_string(device) + " of " + std::to_string(ndev));
    DeviceGuard guard;
    KA_HIP(guard.enter(device));
    ka_engine *e = new ka_engine();
    e->device = device;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) e->set.knobs.n_simd = 4 * prop.multiProcessorCount;
    }
    for (int i = 0; i < 5; ++i) {
        hipError_t er = hipEventCreate(&e->res.ev[i]);
        if (er != hipSuccess) {
            delete e;
            return fail(KA_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(er));
        }
    }
    for (int i = 0; i < 4; ++i) {
        hipError_t er = hipEventCreateWithFlags(&e->res.sync[i], hipEventDisableTiming);
        if (er != hipSuccess) {
            ka_engine_destroy(e);
            return fail(KA_ERR_HIP, std::string("hipEventCreateWithFlags: ") + hipGetErrorString(er));
        }
    }
    *out = e;
    return KA_OK;
}

void ka_engine_destroy(ka_engine *e)
{
    if (!e) return;
    DeviceGuard guard;
    (void)guard.enter(e->device);
    (void)hipDeviceSynchronize();
    if (e->res.ws) (void)hipFree(e->res.ws);
    if (e->res.pin) (void)hipHostFree(e->res.pin);
    for (int i = 0; i < 5; ++i)
        if (e->res.ev[i]) (void)hipEventDestroy(e->res.ev[i]);
    for (int i = 0; i < 4; ++i)
        if (e->res.sync[i]) (void)hipEventDestroy(e->res.sync[i]);
    if (e->res.aux) (void)hipStreamDestroy(e->res.aux);
    if (e->res.refill_done) (void)hipEventDestroy(e->res.refill_done);
    if (e->res.refill_go) (void)hipEventDestroy(e->res.refill_go);
    if (e->res.fill) (void)hipStreamDestroy(e->res.fill);
    delete e;
}

int ka_stream_create(int32_t device, void **stream)
{
    if (!stream) return fail(KA_ERR_BAD_ARGS, "ka_stream_create: stream is NULL");
    DeviceGuard guard;
    KA_HIP(guard.enter(device));
    hipStream_t s = nullptr;
    KA_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void *)s;
    return KA_OK;
}

int ka_stream_destroy(int32_t device, void *stream)
{
    if (!stream) return KA_OK;
    DeviceGuard guard;
    KA_HIP(guard.enter(device));
    KA_HIP(hipStreamSynchronize((hipStream_t)stream));
    KA_HIP(hipStreamDestroy((hipStream_t)stream));
    return KA_OK;
}

int ka_engine_reserve(ka_engine *e, size_t workspace_bytes)
{
    if (!e) return fail(KA_ERR_BAD_ARGS, "engine is NULL");
    DeviceGuard guard;
    KA_HIP(guard.enter(e->device));
    return ensure_ws(e, workspace_bytes);
}

size_t ka_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move)
{
    if (n < 0 || !T || !S) return 0;
    return ka::plan::workspace_upper_bound(n, T, S, V, beam_size, max_move);
}

// Must be called from the engine's own host thread (like every other call on an engine); it reads the engine's settings and
// changes nothing.
size_t ka_engine_workspace_bytes(ka_engine *e, int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                 int32_t mem)
{
    if (!e) return 0;
    LaunchPlan p;
    return plan_launch(e->set.knobs, n, T, S, V, beam_size, max_move, mem, p) == KA_OK ? p.total_bytes : 0;
}

int ka_engine_set_mode(ka_engine *e, int32_t mode)
{
    if (!e) return fail(KA_ERR_BAD_ARGS, "engine is NULL");
    if (mode != KA_MODE_AUTO && mode != KA_MODE_WAVE && mode != KA_MODE_WAVE_EXACT && mode != KA_MODE_TILED)
        return fail(KA_ERR_BAD_ARGS, "ka_engine_set_mode: unknown mode");
    e->set.knobs.mode = mode;
    return KA_OK;
}

int ka_engine_set_backtrace(ka_engine *e, int32_t how)
{
    if (!e) return fail(KA_ERR_BAD_ARGS, "engine is NULL");
    if (how != KA_BACKTRACE_AUTO && how != KA_BACKTRACE_SERIAL && how != KA_BACKTRACE_PARALLEL)
        return fail(KA_ERR_BAD_ARGS, "ka_engine_set_backtrace: unknown value");
    e->set.knobs.backtrace = how;
    return KA_OK;
}

int ka_engine_set_verify(ka_engine *e, int32_t flags)
{
    if (!e) return fail(KA_ERR_BAD_ARGS, "engine is NULL");
    if (flags < 0 || flags > 7) return fail(KA_ERR_BAD_ARGS, "ka_engine_set_verify: flags are a combination of 1, 2 and 4");
    e->set.verify = flags;
    return KA_OK;
}

int ka_debug_set_tile_lds(ka_engine *e, int32_t bytes)
{
    if (!e) return fail(KA_ERR_BAD_ARGS, "engine is NULL");
    if (bytes < 0 || bytes > 160 * 1024) return fail(KA_ERR_BAD_ARGS, "ka_debug_set_tile_lds: 0 .. 160 KB");
    e->set.tile_lds = bytes;
    return KA_OK;
}

int ka_debug_set_split(ka_engine *e, int32_t n_tiled, int32_t n_parallel)
{
    if (!e) return fail(KA_ERR_BAD_ARGS, "engine is NULL");
    e->set.knobs.split_tiled = n_tiled < 0 ? -1 : n_tiled;
    e->set.knobs.split_par = n_parallel < 0 ? -1 : n_parallel;
    return KA_OK;
}

int ka_debug_set_tile_width(ka_engine *e, int32_t positions)
{
    if (!e) return fail(KA_ERR_BAD_ARGS, "engine is NULL");
    if (positions != 0 && positions != ka::kTnTile && positions != ka::kTpTile) return fail(KA_ERR_BAD_ARGS, "ka_debug_set_tile_width: 0, 128 or 256");
    e->set.knobs.tile_width = positions;
    return KA_OK;
}

int ka_engine_set_profiling(ka_engine *e, int32_t on)
{
    if (!e) return fail(KA_ERR_BAD_ARGS, "engine is NULL");
    e->set.profiling = on != 0;
    e->batch.have_times = false;
    return KA_OK;
}

int ka_engine_last_kernel_ms(ka_engine *e, float ms[4])
{
    if (!e || !ms) return fail(KA_ERR_BAD_ARGS, "engine or ms is NULL");
    if (!e->batch.have_times) return fail(KA_ERR_BAD_ARGS, "no profiled batch has been finished");
    for (int i = 0; i < 4; ++i) KA_HIP(hipEventElapsedTime(&ms[i], e->res.ev[i], e->res.ev[i + 1]));
    return KA_OK;
}

int ka_ctc_best_path_batch_enqueue_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T,
                                       int32_t V, const int64_t *ld, const int32_t *const *labels, const int64_t *S,
                                       int32_t beam_size, int32_t max_move, int32_t *const *best_path,
                                       int32_t *const *best_labels, float *const *best_scores, void *stream)
{
    const BatchArgs a{log_probs, T, ld, labels, S, best_path, best_labels, best_scores};
    return enqueue_batch(e, n, a, V, beam_size, max_move, KA_MEM_DEVICE, (hipStream_t)stream);
}

int ka_batch_finish(ka_engine *e, float *total_score, int32_t *status)
{
    if (!e) return fail(KA_ERR_BAD_ARGS, "engine is NULL");
    ka_engine::Batch &b = e->batch;
    if (!b.pending) return fail(KA_ERR_BAD_ARGS, "no batch enqueued");
    b.pending = false;
    DeviceGuard guard;
    KA_HIP(guard.enter(e->device));
    KA_HIP(hipStreamSynchronize(b.stream));
    if (e->set.profiling && b.n > 0) b.have_times = true;
    // (a copy: the redo lays its own descriptors and status records over the pinned ones)
    std::vector<ka::LatticeMeta> meta(b.meta, b.meta + (size_t)b.n);
    if (e->dbg.ck_idx < b.n && (meta[e->dbg.ck_idx].flags & (ka::kFlagExact | ka::kFlagDeclined))) e->dbg.ck_bytes = 0;
    e->dbg.flags.resize((size_t)b.n);
    for (int32_t i = 0; i < b.n; ++i) e->dbg.flags[(size_t)i] = meta[i].flags;
    // wide tiled lattices the scores-only form declined: KA_MODE_AUTO redoes them through the generic kernels, an explicit
    // KA_MODE_TILED reports KA_ERR_NONFINITE
    std::vector<ka_engine::Redo> again;
    for (const ka_engine::Redo &r : b.redo) {
        ka::LatticeMeta &m = meta[r.idx];
        if (m.status != KA_OK || !(m.flags & ka::kFlagDeclined)) continue;
        if (e->set.knobs.mode == KA_MODE_TILED) m.status = KA_ERR_NONFINITE;
        else again.push_back(r);
    }
    std::string redo_error;
    if (!again.empty()) {
        redo_declined(e, again, meta);
        redo_error = g_err;
    }
    int first_bad = KA_OK;
    for (int32_t i = 0; i < b.n; ++i) {
        const ka::LatticeMeta &m = meta[i];
        if (status) status[i] = m.status;
        if (total_score) total_score[i] = m.score;
        if (m.status != KA_OK && first_bad == KA_OK) {
            first_bad = m.status;
            g_err = "lattice " + std::to_string(i) +
                    status_message(m.status, {": no live state in the last frame (empty beam)", ": internal error in the tile hand-off",
                                              ": log-probs with infinities in a band wider than 1009 positions (KA_MODE_TILED cannot answer it: use KA_MODE_AUTO)",
                                              nullptr, nullptr,
                                              redo_error.empty() ? ": failed" : ": the redo through the generic kernels failed: " + redo_error});
        }
    }
    return first_bad;
}

int ka_ctc_best_path_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                               const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                               int32_t max_move, int32_t *const *best_path, int32_t *const *best_labels,
                               float *const *best_scores, float *total_score, int32_t *status, int32_t mem,
                               void *stream)
{
    const BatchArgs a{log_probs, T, ld, labels, S, best_path, best_labels, best_scores};
    int rc = enqueue_batch(e, n, a, V, beam_size, max_move, mem, (hipStream_t)stream);
    if (rc != KA_OK) return rc;
    return ka_batch_finish(e, total_score, status);
}

int ka_ctc_best_path_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld,
                         const int32_t *labels, int64_t S, int32_t beam_size, int32_t max_move, int32_t *best_path,
                         int32_t *best_labels, float *best_scores, float *total_score, int32_t mem, void *stream)
{
    int32_t status = 0;
    float total = 0.0f;
    int rc = ka_ctc_best_path_batch_f32(e, 1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, &best_path,
                                        &best_labels, &best_scores, &total, &status, mem, stream);
    if (total_score) *total_score = total;
    return rc;
}

int ka_debug_chunk_entries(ka_engine *e, int32_t *out, int32_t max_entries, uint8_t *map0_out, int64_t map0_max)
{
    if (!e || !out || max_entries < 0) return fail(KA_ERR_BAD_ARGS, "ka_debug_chunk_entries: bad arguments");
    DeviceGuard guard;
    KA_HIP(guard.enter(e->device));
    const size_t n = std::min<size_t>(e->dbg.entry_n, (size_t)max_entries);
    if (n) KA_HIP(hipMemcpy(out, e->res.ws + e->dbg.entry, n * 4, hipMemcpyDeviceToHost));
    if (map0_out && map0_max > 0 && e->dbg.map0_bytes)
        KA_HIP(hipMemcpy(map0_out, e->res.ws + e->dbg.map0, std::min<size_t>(e->dbg.map0_bytes, (size_t)map0_max), hipMemcpyDeviceToHost));
    return (int)n;
}

int ka_debug_meta_flags(ka_engine *e, int32_t *out, int32_t max_lattices)
{
    if (!e || max_lattices < 0 || (max_lattices > 0 && !out)) return fail(KA_ERR_BAD_ARGS, "ka_debug_meta_flags: bad arguments");
    if (e->batch.pending) return fail(KA_ERR_BAD_ARGS, "ka_debug_meta_flags: a batch is enqueued and not finished");
    const size_t n = std::min<size_t>(e->dbg.flags.size(), (size_t)max_lattices);
    for (size_t i = 0; i < n; ++i) out[i] = e->dbg.flags[i];
    return (int)e->dbg.flags.size();
}

int ka_debug_checkpoints(ka_engine *e, float *out, int64_t max_floats, int64_t *pitch)
{
    if (!e || max_floats < 0 || (max_floats > 0 && !out)) return fail(KA_ERR_BAD_ARGS, "ka_debug_checkpoints: bad arguments");
    if (e->batch.pending) return fail(KA_ERR_BAD_ARGS, "ka_debug_checkpoints: a batch is enqueued and not finished");
    DeviceGuard guard;
    KA_HIP(guard.enter(e->device));
    if (pitch) *pitch = e->dbg.ck_bytes ? (int64_t)e->dbg.ck_pitch : 0;
    const size_t n = std::min<size_t>(e->dbg.ck_bytes / 4, (size_t)max_floats);
    if (n) KA_HIP(hipMemcpy(out, e->res.ws + e->dbg.ck, n * 4, hipMemcpyDeviceToHost));
    return e->dbg.ck_bytes ? (int)(e->dbg.ck_bytes / e->dbg.ck_pitch) : 0;
}

int ka_debug_plan_tiles_width(int64_t T, int64_t S, int32_t V, int32_t beam_size, int32_t max_move, int32_t positions, int32_t *t_in, int32_t *t_end,
                              int32_t max_tiles, int64_t *checkpoint_pitch)
{
    Shape sh;
    if (max_tiles < 0 || (max_tiles > 0 && (!t_in || !t_end)) || (positions != ka::kTnTile && positions != ka::kTpTile) ||
        !ka::plan::shape_of(T, S, V, beam_size, max_move, sh))
        return fail(KA_ERR_BAD_ARGS, "ka_debug_plan_tiles_width: bad arguments");
    ka::plan::plan_tiles(sh, V, beam_size, max_move, positions);
    {   // the O(1) count the planner decides by must agree with the listing (the CPU tests of the tile plan come through here)
        const ka::plan::TileCount tc = ka::plan::count_tiles(sh, V, beam_size, max_move, positions);
        if (tc.tileable != sh.tileable || (sh.tileable && tc.n_tiles != (int64_t)sh.t_in.size()))
            return fail(KA_ERR_INTERNAL, "ka_debug_plan_tiles_width: count_tiles disagrees with plan_tiles");
    }
    if (!sh.tileable) return 0;
    for (size_t b = 0; b < sh.t_in.size() && b < (size_t)max_tiles; ++b) {
        t_in[b] = sh.t_in[b];
        t_end[b] = sh.t_end[b];
    }
    if (checkpoint_pitch) *checkpoint_pitch = (int64_t)sh.ck_pitch;
    return (int)sh.t_in.size();
}

int ka_debug_plan_tiles(int64_t T, int64_t S, int32_t V, int32_t beam_size, int32_t max_move, int32_t *t_in, int32_t *t_end,
                        int32_t max_tiles, int64_t *checkpoint_pitch)
{
    return ka_debug_plan_tiles_width(T, S, V, beam_size, max_move, ka::kTpTile, t_in, t_end, max_tiles, checkpoint_pitch);
}

int ka_debug_tile_width_choice(const int64_t *T, const int64_t *S, int32_t n, int32_t V, int32_t beam_size, int32_t max_move, int32_t n_simd)
{
    if (n < 0 || (n > 0 && (!T || !S)) || n_simd < 4) return fail(KA_ERR_BAD_ARGS, "ka_debug_tile_width_choice: bad arguments");
    std::vector<ka::plan::TileCount> counts(n);
    std::vector<int64_t> widths(n);
    for (int32_t i = 0; i < n; ++i) {
        Shape sh;
        if (!ka::plan::shape_of(T[i], S[i], V, beam_size, max_move, sh)) return fail(KA_ERR_BAD_ARGS, "ka_debug_tile_width_choice: bad shape");
        if (!ka::plan::count_tiles(sh, V, beam_size, max_move, ka::kTpTile).tileable) return 0;
        counts[i] = ka::plan::count_tiles(sh, V, beam_size, max_move, ka::kTnTile);
        widths[i] = sh.W;
    }
    return ka::plan::narrow_tiles_pay(counts, widths, n_simd, 0) ? ka::kTnTile : ka::kTpTile;
}

int ka_debug_auto_split(const int64_t *T, int32_t n, int32_t tiles_alive, int32_t n_simd, int32_t *n_tiled, int32_t *n_parallel)
{
    if (n < 0 || (n > 0 && !T) || tiles_alive < 1 || n_simd < 1 || !n_tiled || !n_parallel)
        return fail(KA_ERR_BAD_ARGS, "ka_debug_auto_split: bad arguments");
    std::vector<int64_t> Ts(T, T + n);
    std::sort(Ts.begin(), Ts.end(), [](int64_t a, int64_t b) { return a > b; });
    std::vector<int32_t> alive((size_t)n, tiles_alive);
    *n_tiled = ka::plan::auto_split_forward(Ts, alive, n_simd);
    *n_parallel = ka::plan::auto_split_backtrace(Ts, n_simd);
    return KA_OK;
}

int ka_debug_tile_stats(ka_engine *e, uint64_t *out, int32_t max_tasks)
{
    if (!e || !out || max_tasks < 0) return fail(KA_ERR_BAD_ARGS, "ka_debug_tile_stats: bad arguments");
    DeviceGuard guard;
    KA_HIP(guard.enter(e->device));
    const size_t n = std::min<size_t>(e->dbg.n_tasks, (size_t)max_tasks);
    std::vector<ka::TileTask> tk(n);
    std::vector<ka::TpStats> st(n);
    if (n) {
        KA_HIP(hipMemcpy(tk.data(), e->res.ws + e->dbg.tasks, n * sizeof(ka::TileTask), hipMemcpyDeviceToHost));
        KA_HIP(hipMemcpy(st.data(), e->res.ws + e->dbg.stats, n * sizeof(ka::TpStats), hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < n; ++i) {
        uint64_t *o = out + 8 * i;
        o[0] = (uint64_t)tk[i].lat; o[1] = (uint64_t)tk[i].tile; o[2] = (uint64_t)tk[i].t_in; o[3] = (uint64_t)tk[i].t_end;
        o[4] = st[i].wait_ticks; o[5] = st[i].total_ticks; o[6] = st[i].spins; o[7] = st[i].start_tick;
        o[2] |= (st[i].phase[2] >> 32) << 32;      // (two-wavefront tiles: HW_ID of the compute wavefront in the high half of t_in)
        if ((e->set.verify & 4) && (i == 0 || i == 10 || i == 20)) std::fprintf(stderr, "[ka_debug_tile_stats] ticket %zu cycles per phase: wait %llu, check+sum %llu, progress %llu, requests %llu, publish %llu\n", i,
                                 (unsigned long long)(uint32_t)st[i].phase[0], (unsigned long long)(st[i].phase[0] >> 32), (unsigned long long)(uint32_t)st[i].phase[1],
                                 (unsigned long long)(st[i].phase[1] >> 32), (unsigned long long)(uint32_t)st[i].phase[2]);
        if ((e->set.verify & 4) && (i == 0 || i == 10 || i == 20) && st[i].extra[0]) std::fprintf(stderr, "[ka_debug_tile_stats] ticket %zu compute wavefront: %llu cycles in frame blocks, %llu at barriers; look-up wavefront busy %llu\n", i,
                                 (unsigned long long)(st[i].extra[0] >> 32), (unsigned long long)(uint32_t)st[i].extra[0], (unsigned long long)st[i].extra[1]);
    }
    return (int)n;
}

}  // extern "C"
