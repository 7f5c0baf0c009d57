// ka_engine.hpp — what the host translation units (ka_engine.hip, ka_engine_fb.hip, ka_engine_band.hip, ka_entry_misc.hip)
// share: the engine object, the error string and its helpers, the device guard, the two growing buffers and the
// status-to-message table; and, for the two drivers that lay their own layout over the engine's buffers (fb_impl in
// ka_engine_fb.hip, banded_impl in ka_engine_band.hip), the head of their call record and the steps they take alike.
#pragma once
#include "../../include/kokoro_align_amd.h"
#include "ka_launch.hpp"
#include "ka_plan.hpp"

#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

namespace ka {
namespace host {

extern thread_local std::string g_err;      // what ka_last_error returns (defined in ka_engine.hip)

inline int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define KA_HIP(expr)                                                                                    \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return ka::host::fail(KA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
    } while (0)

// The engine works on ITS device and leaves the caller's current device (which PyTorch shares, per thread) as it
// found it, on every exit path.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t enter(int dev)
    {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess || prev == dev) return e;
        e = hipSetDevice(dev);
        switched = e == hipSuccess;
        return e;
    }
    ~DeviceGuard()
    {
        if (switched) (void)hipSetDevice(prev);
    }
};

}  // namespace host
}  // namespace ka

// The engine's state, grouped by lifetime.
struct ka_engine {
    int device = 0;

    // what the ka_engine_set_* / ka_debug_set_* entry points write; a launch only reads it
    struct Settings {
        ka::plan::Knobs knobs;      // mode, backtrace, tile width, split (ka_debug_set_split), SIMDs of the device: what the planner reads
        int32_t verify = 0;         // ka_engine_set_verify: self-checks of the tiled form's hand-off
        int32_t tile_lds = 0;       // ka_debug_set_tile_lds: LDS bytes a tile workgroup requests (0: the library's choice)
        bool profiling = false;
    } set;

    // what lives as long as the engine (the buffers grow: ensure_ws, ensure_pin; aux, fill and the refill events are created by
    // the first launch that needs them)
    struct Resources {
        char *ws = nullptr;
        size_t ws_bytes = 0;
        char *pin = nullptr;
        size_t pin_bytes = 0;
        hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // ka_engine_set_profiling: around prep, forward, backtrace, gathers
        hipStream_t aux = nullptr;             // second stream: the other kernel form of a mixed launch runs beside the first
        hipEvent_t sync[4] = {nullptr, nullptr, nullptr, nullptr};
        hipStream_t fill = nullptr;            // the stream of the halo refill (not `aux`: a mixed launch's second backtrace runs there)
        hipEvent_t refill_done = nullptr, refill_go = nullptr;
    } res;

    // what ka_batch_finish needs to hand the wide tiled lattices that the scores-only form declined (non-finite log-probs) to
    // the generic kernels: the caller's buffers (valid until finish returns, by the contract of the split form)
    struct Redo { const float *lp; const int32_t *labels; int32_t *path, *lab_out; float *sc_out; int64_t T, S, ld; int32_t idx; };

    // the one enqueued batch: written by the public enqueue, read by ka_batch_finish
    struct Batch {
        bool pending = false;                   // this record is live: enqueued and not finished
        int32_t n = 0;
        hipStream_t stream = nullptr;
        const ka::LatticeMeta *meta = nullptr;  // the status records, pinned
        int32_t V = 0, beam = 0, max_move = 0, mem = KA_MEM_DEVICE;
        std::vector<Redo> redo;
        bool have_times = false;                // finished with profiling on: Resources::ev hold its times
    } batch;

    // Workspace bytes [lo, hi) hold the halo sentinel already: refilled BEHIND the last tile kernel, on the side stream,
    // while that launch's backtrace ran (refill_done marks the end of it).  A launch whose halo slots lie inside the range skips
    // its own fill - 0.15-0.2 ms for a book, in front of the first tile - and only waits for the event.
    struct HaloClean {
        size_t lo = 0, hi = 0;
        void invalidate() { lo = hi = 0; }
    } clean;

    // workspace offsets of the last launch, for ka_debug_chunk_entries (descriptor 0: chunk entries and chunk maps),
    // ka_debug_checkpoints (descriptor 0: the checkpoint rows of the forward pass; ck_bytes = 0 where it stored none: the exact
    // and generic forms, and a lattice the checkpointed forms declined - ka_batch_finish sees that in its flags) and
    // ka_debug_tile_stats (the tile tasks and their timing records)
    struct DebugView {
        size_t entry = 0, entry_n = 0, map0 = 0, map0_bytes = 0;
        size_t ck = 0, ck_bytes = 0, ck_pitch = 0;
        int32_t ck_idx = 0;      // the caller's index of descriptor 0
        size_t tasks = 0, stats = 0, n_tasks = 0;
        std::vector<int32_t> flags;   // ka_debug_meta_flags: the kFlag* word of every lattice of the last finished batch
    } dbg;
};

namespace ka {
namespace host {

inline int ensure_ws(ka_engine *e, size_t bytes)
{
    ka_engine::Resources &r = e->res;
    if (bytes <= r.ws_bytes) return KA_OK;
    KA_HIP(hipDeviceSynchronize());
    if (r.ws) KA_HIP(hipFree(r.ws));
    r.ws = nullptr;
    r.ws_bytes = 0;
    e->clean.invalidate();
    const size_t want = plan::align_up(bytes + bytes / 16, 1 << 20);
    hipError_t er = hipMalloc((void **)&r.ws, want);
    if (er != hipSuccess) {
        (void)hipGetLastError();
        return fail(KA_ERR_NOMEM, "hipMalloc of " + std::to_string(want) + " workspace bytes failed: " + hipGetErrorString(er));
    }
    r.ws_bytes = want;
    return KA_OK;
}

inline int ensure_pin(ka_engine *e, size_t bytes)
{
    ka_engine::Resources &r = e->res;
    if (bytes <= r.pin_bytes) return KA_OK;
    KA_HIP(hipDeviceSynchronize());
    if (r.pin) KA_HIP(hipHostFree(r.pin));
    r.pin = nullptr;
    r.pin_bytes = 0;
    const size_t want = plan::align_up(bytes * 2, 4096);
    KA_HIP(hipHostMalloc((void **)&r.pin, want, hipHostMallocDefault));
    r.pin_bytes = want;
    return KA_OK;
}

// What follows "lattice <i>" in the message of a lattice's status.  A call brings the texts that are its own (nullptr: it has
// none for that status) and what it says about a status the table does not know.
struct StatusTexts {
    const char *empty_beam, *internal, *nonfinite, *bad_args, *zero_mass;
    std::string other = ": failed";
};
inline std::string status_message(int32_t status, const StatusTexts &t)
{
    const char *own = status == KA_ERR_EMPTY_BEAM  ? t.empty_beam
                      : status == KA_ERR_INTERNAL  ? t.internal
                      : status == KA_ERR_NONFINITE ? t.nonfinite
                      : status == KA_ERR_BAD_ARGS  ? t.bad_args
                      : status == KA_ERR_ZERO_MASS ? t.zero_mass
                                                   : nullptr;
    if (own) return own;
    return status == KA_ERR_BAD_LABEL ? ": label outside [0, V)" : status == KA_ERR_NAN ? ": a log-prob is NaN" : t.other;
}

// ---- what fb_impl and banded_impl do alike.  What differs stays in each driver: its own checks and their order, its planner,
// its result records, its rows, launches and copy-out ----

// the head of a call's record: the lattices, as every batch entry point takes them
struct LatticeArgs {
    int32_t n;
    const float *const *log_probs;
    const int64_t *T;
    int32_t V;
    const int64_t *ld;
    const int32_t *const *labels;
    const int64_t *S;
    int32_t beam_size, max_move;
    int32_t mem;
    hipStream_t stream;
    bool host() const { return mem == KA_MEM_HOST; }
};

// The refusals that precede planning.  `name`: what the call is called in the message; `arrays`: the caller's answer to
// "are the arrays of my own there" (asked for n > 0 only).
inline int refuse_call(const ka_engine *e, const LatticeArgs &a, const char *name, bool arrays)
{
    if (!e) return fail(KA_ERR_BAD_ARGS, "engine is NULL");
    if (e->batch.pending) return fail(KA_ERR_BAD_ARGS, "a batch is already enqueued: call ka_batch_finish first");
    if (a.n < 0 || (a.n > 0 && (!a.log_probs || !a.T || !a.ld || !a.labels || !a.S || !arrays)))
        return fail(KA_ERR_BAD_ARGS, std::string(name) + ": NULL array argument");
    if (a.mem != KA_MEM_HOST && a.mem != KA_MEM_DEVICE) return fail(KA_ERR_BAD_ARGS, "mem must be KA_MEM_HOST or KA_MEM_DEVICE");
    return KA_OK;
}

// what every *_workspace_bytes export answers 0 to before it plans: a negative count, a NULL table among those it needs
// (for n > 0), a bad mem
inline bool countable(int32_t n, int32_t mem, std::initializer_list<const void *> tables)
{
    for (const void *t : tables)
        if (n > 0 && !t) return false;
    return n >= 0 && (mem == KA_MEM_HOST || mem == KA_MEM_DEVICE);
}

// The start of a call, with the engine's device current (the DeviceGuard is the driver's own): both buffers large enough, and
// the workspace is shared with the best-path calls: wait for the refill behind their last tile launch, and what it left clean
// is clean no more.
inline int begin_call(ka_engine *e, size_t ws_bytes, size_t pin_bytes, hipStream_t stream)
{
    int rc = ensure_ws(e, ws_bytes);
    if (rc != KA_OK) return rc;
    rc = ensure_pin(e, pin_bytes);
    if (rc != KA_OK) return rc;
    if (e->res.refill_done) KA_HIP(hipStreamWaitEvent(stream, e->res.refill_done, 0));
    e->clean.invalidate();
    e->dbg = ka_engine::DebugView();
    return KA_OK;
}

// descriptor order: fast-form lattices first, then the generic ones, each in batch order (the order occupancy slots assume).
// next(fast), asked for lattice 0, 1, ... in turn, is that lattice's descriptor slot.
struct SlotOrder {
    int32_t n_fast = 0, k_fast = 0, k_gen = 0;
    template <class Carve>
    SlotOrder(const Carve *cv, int32_t n)
    {
        for (int32_t i = 0; i < n; ++i) n_fast += cv[i].fast ? 1 : 0;
    }
    int32_t next(bool fast) { return fast ? k_fast++ : n_fast + k_gen++; }
};

// the head of lattice i's descriptor (a BandLattice, or one of the FbLattice family: the same field names), zeroed first; the
// log-probs and labels are the staged copies (plan::FbCarve) for host buffers
template <class Desc>
inline void fill_head(Desc &d, const plan::FbCarve &c, const LatticeArgs &a, int32_t i, char *ws)
{
    std::memset(&d, 0, sizeof(d));
    if (a.host()) {
        d.lp = reinterpret_cast<const float *>(ws + c.lp);
        d.labels = reinterpret_cast<const int32_t *>(ws + c.lab);
        d.ld = a.V;
    } else {
        d.lp = a.log_probs[i];
        d.labels = a.labels[i];
        d.ld = a.ld[i];
    }
    d.T = (int32_t)a.T[i];
    d.S = (int32_t)a.S[i];
    d.L = (int32_t)(2 * a.S[i] + 1);
    d.V = a.V;
    d.beam = a.beam_size;
    d.max_move = a.max_move;
    d.idx = i;
}
// ... and, for host buffers, that staging: lattice i's log-probs, packed to V columns, and its labels
inline int stage_lattice(const plan::FbCarve &c, const LatticeArgs &a, int32_t i, char *ws)
{
    KA_HIP(hipMemcpy2DAsync(ws + c.lp, (size_t)a.V * 4, a.log_probs[i], (size_t)a.ld[i] * 4, (size_t)a.V * 4, (size_t)a.T[i], hipMemcpyHostToDevice,
                            a.stream));
    if (a.S[i] > 0) KA_HIP(hipMemcpyAsync(ws + c.lab, a.labels[i], (size_t)a.S[i] * 4, hipMemcpyHostToDevice, a.stream));
    return KA_OK;
}

}  // namespace host
}  // namespace ka
