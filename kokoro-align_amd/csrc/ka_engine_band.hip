// ka_engine_band.hip — the best path over a band of the C ABI: over a caller-given band (ka_banded.hpp), over a self-steering
// one (ka_tracking.hip), both resumed from the caller's boundary conditions (ka_resume.hip, ka_tracking_resume.hip) and both
// with the determined prefix behind them (ka_determined.hpp).  One driver, banded_impl, over one call record, BandArgs, and one
// workspace layout, plan::BandLayout; the call's mode (plan::BandMode) says which of the six it is.  Host code only.  Like the
// forward-backward calls (ka_engine_fb.hip) they use the engine's workspace and pinned buffer with their own kernels and layout,
// whatever the engine's mode, and run to the end inside the call: no batch stays in flight.
#include "ka_engine.hpp"

namespace {

using namespace ka::host;

// The record of a call.  tracking: the self-steering band, whose table the call WRITES, a fourth output.  resumed: the caller's
// boundary conditions, a last row and an entry cell per lattice; under tracking its end is the record's `end` too, and it adds
// lo_0 and the low end of frame T, a second cell beside the entry.  walk: the determined calls, the walk from every live cell
// behind the call.
struct BandArgs {
    LatticeArgs lat;
    ka::plan::BandMode mode;
    int32_t period = 0, end_rule = 0;             // tracking (tracking_args has checked them); end_rule: not resumed
    // the table, [n] tables of [T] int32 where `mem` says: exactly one of the two, by mode.tracking
    const int32_t *const *band_lo = nullptr;      // the caller's band, read
    int32_t *const *band_lo_out = nullptr;        // tracking: the band the call steered
    int32_t *const *best_path = nullptr;
    int32_t *const *best_labels = nullptr;
    float *const *best_scores = nullptr;
    float *total_score = nullptr;                 // [n] host, or NULL
    int32_t *status = nullptr;                    // [n] host, or NULL
    // resumed
    const float *const *init_scores = nullptr;    // [n] or NULL; an entry may be NULL
    const int32_t *end = nullptr;                 // [n] host, or NULL: all -1
    float *const *final_scores = nullptr;         // [n] or NULL; an entry may be NULL
    int32_t *entry = nullptr;                     // [n] host, or NULL
    const int32_t *first_lo = nullptr;            // tracking: [n] host, or NULL: all 0
    int32_t *next_lo = nullptr;                   // tracking: [n] host, or NULL
    int32_t *determined = nullptr;                // walk: its result, [n] host, required

    bool arrays() const { return (mode.tracking ? band_lo_out != nullptr : band_lo != nullptr) && best_path && best_labels && best_scores; }
    const int32_t *table(int32_t i) const { return mode.tracking ? band_lo_out[i] : band_lo[i]; }
    const float *init(int32_t i) const { return init_scores ? init_scores[i] : nullptr; }
    float *fin(int32_t i) const { return final_scores ? final_scores[i] : nullptr; }
};

int banded_impl(ka_engine *e, const BandArgs &a)
{
    using Desc = ka::BandLattice;
    const LatticeArgs &l = a.lat;
    const int32_t n = l.n;
    const hipStream_t stream = l.stream;
    const bool host = l.host(), tracking = a.mode.tracking, resumed = a.mode.resumed, walk = a.mode.walk;
    int rc = refuse_call(e, l, "banded best path", a.arrays());
    if (rc != KA_OK) return rc;
    if (walk && !a.determined) return fail(KA_ERR_BAD_ARGS, "determined best path: determined is NULL");
    if (n == 0) return KA_OK;
    ka::plan::BandLayout lay;
    if (ka::plan::band_workspace(n, l.T, l.S, l.V, l.beam_size, l.max_move, host, a.mode, &lay) == 0)
        return fail(KA_ERR_BAD_ARGS, "banded best path: unsupported T/S/V/beam_size/max_move");
    const std::vector<ka::plan::BandCarve> &cv = lay.cv;
    if (resumed && a.end)
        for (int32_t i = 0; i < n; ++i)
            if (a.end[i] < -2 || a.end[i] > 2 * l.S[i])
                return fail(KA_ERR_BAD_ARGS, "lattice " + std::to_string(i) + ": end must be -1 (highest live), -2 (best live) or a position in [0, 2S+1)");
    if (resumed && a.first_lo)
        for (int32_t i = 0; i < n; ++i)
            if (a.first_lo[i] < 0 || a.first_lo[i] > 2 * l.S[i])
                return fail(KA_ERR_BAD_ARGS, "lattice " + std::to_string(i) + ": first_lo must be a position in [0, 2S+1)");
    for (int32_t i = 0; i < n; ++i) {
        if (l.ld[i] < l.V) return fail(KA_ERR_BAD_ARGS, "lattice " + std::to_string(i) + ": ld < V");
        if (!l.log_probs[i] || !a.table(i) || !a.best_path[i] || !a.best_labels[i] || !a.best_scores[i] || (l.S[i] > 0 && !l.labels[i]))
            return fail(KA_ERR_BAD_ARGS, "lattice " + std::to_string(i) + ": NULL buffer");
    }
    DeviceGuard guard;
    KA_HIP(guard.enter(e->device));
    // the pinned buffer: the layout's descriptors, results, rows and cells one behind the other, then the determined cells
    const size_t pin_meta = lay.desc_bytes, pin_rows = pin_meta + lay.meta_bytes, pin_entry = pin_rows + lay.rows_bytes,
                 pin_det = pin_entry + lay.entry_bytes;
    if ((rc = begin_call(e, lay.total, pin_det + (walk ? (size_t)n * sizeof(int32_t) : 0), stream)) != KA_OK) return rc;
    char *ws = e->res.ws;
    Desc *h = reinterpret_cast<Desc *>(e->res.pin);
    ka::LatticeMeta *h_meta = reinterpret_cast<ka::LatticeMeta *>(e->res.pin + pin_meta);
    ka::ResumeRows *h_rows = reinterpret_cast<ka::ResumeRows *>(e->res.pin + pin_rows);
    int32_t *h_entry = reinterpret_cast<int32_t *>(e->res.pin + pin_entry);
    int32_t *h_det = reinterpret_cast<int32_t *>(e->res.pin + pin_det);
    const int32_t cells = lay.cells;
    SlotOrder order(cv.data(), n);
    const int32_t n_fast = order.n_fast;
    for (int32_t i = 0; i < n; ++i) {
        const ka::plan::BandCarve &c = cv[i];
        const int32_t slot = order.next(c.fast);
        Desc &d = h[slot];
        fill_head(d, c, l, i, ws);
        if (resumed) {   // (a staged row is in the workspace; a caller's device row is used where it lies)
            ka::ResumeRows &r = h_rows[slot];
            r.init = !a.init(i) ? nullptr : host ? reinterpret_cast<const float *>(ws + c.init) : a.init(i);
            r.fin = !a.fin(i) ? nullptr : host ? reinterpret_cast<float *>(ws + c.fin) : a.fin(i);
            // (the walk starts from the last row: where the caller wants none, the staged row or one of the engine's own)
            if (walk && !a.fin(i)) r.fin = reinterpret_cast<float *>(ws + (host ? c.fin : c.own_fin));
            r.entry = reinterpret_cast<int32_t *>(ws + lay.off_entry) + (size_t)i * cells;
            r.end = a.end ? a.end[i] : -1;
            r.first_lo = a.first_lo ? a.first_lo[i] : 0;
        }
        if (host) {
            d.band_lo = reinterpret_cast<const int32_t *>(ws + c.band);
            d.path = reinterpret_cast<int32_t *>(ws + c.path);
            d.lab_out = reinterpret_cast<int32_t *>(ws + c.lab_out);
            d.sc_out = reinterpret_cast<float *>(ws + c.sc_out);
        } else {
            d.band_lo = a.table(i);
            d.path = a.best_path[i];
            d.lab_out = a.best_labels[i];
            d.sc_out = a.best_scores[i];
        }
        d.labx = reinterpret_cast<int32_t *>(ws + c.labx);
        d.tab = c.fast && !tracking ? reinterpret_cast<int32_t *>(ws + c.tab) : nullptr;
        d.bp = ws + c.bp;
        d.col = c.fast ? nullptr : reinterpret_cast<float *>(ws + c.col);
        d.labx_len = c.labx_len;
        d.W = c.W;
        d.tab_len = c.tab_len;
    }
    if (host)
        for (int32_t i = 0; i < n; ++i) {
            if ((rc = stage_lattice(cv[i], l, i, ws)) != KA_OK) return rc;
            if (!tracking) KA_HIP(hipMemcpyAsync(ws + cv[i].band, a.band_lo[i], (size_t)l.T[i] * 4, hipMemcpyHostToDevice, stream));
            if (resumed && a.init(i)) KA_HIP(hipMemcpyAsync(ws + cv[i].init, a.init(i), (size_t)(2 * l.S[i] + 1) * 4, hipMemcpyHostToDevice, stream));
        }
    Desc *d_lats = reinterpret_cast<Desc *>(ws);
    int32_t *d_meta = reinterpret_cast<int32_t *>(ws + lay.off_meta);
    int32_t *d_det = reinterpret_cast<int32_t *>(ws + lay.off_det);
    KA_HIP(hipMemcpyAsync(d_lats, h, (size_t)n * sizeof(Desc), hipMemcpyHostToDevice, stream));
    KA_HIP(hipMemsetAsync(d_meta, 0, (size_t)n * sizeof(ka::LatticeMeta), stream));
    if (resumed) {
        ka::ResumeRows *d_rows = reinterpret_cast<ka::ResumeRows *>(ws + lay.off_rows);
        KA_HIP(hipMemcpyAsync(d_rows, h_rows, (size_t)n * sizeof(ka::ResumeRows), hipMemcpyHostToDevice, stream));
        if (tracking) ka::launch_best_path_tracking_resume(d_lats, d_rows, n_fast, n - n_fast, l.max_move, a.period, d_meta, stream);
        else ka::launch_best_path_resume(d_lats, d_rows, n_fast, n - n_fast, l.max_move, d_meta, stream);
        if (walk) ka::launch_determined(d_lats, d_rows, n_fast, n - n_fast, d_meta, d_det, stream);
    } else if (tracking) ka::launch_best_path_tracking(d_lats, n_fast, n - n_fast, l.max_move, a.period, a.end_rule, d_meta, stream);
    else ka::launch_best_path_banded(d_lats, n_fast, n - n_fast, l.max_move, d_meta, stream);
    KA_HIP(hipGetLastError());
    KA_HIP(hipMemcpyAsync(h_meta, d_meta, (size_t)n * sizeof(ka::LatticeMeta), hipMemcpyDeviceToHost, stream));
    if (resumed) KA_HIP(hipMemcpyAsync(h_entry, ws + lay.off_entry, (size_t)n * cells * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (walk) KA_HIP(hipMemcpyAsync(h_det, d_det, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    KA_HIP(hipStreamSynchronize(stream));
    if (host) {   // only what succeeded is copied out: a failed lattice's outputs stay as the caller left them
        for (int32_t i = 0; i < n; ++i) {
            // (but the last row of every lattice: all dead where the forward pass did not run, or found a NaN or a bad label)
            if (resumed && a.fin(i)) KA_HIP(hipMemcpyAsync(a.fin(i), ws + cv[i].fin, (size_t)(2 * l.S[i] + 1) * 4, hipMemcpyDeviceToHost, stream));
            const size_t bytes = (size_t)l.T[i] * 4;
            // (and the table of a resumed tracking call whose forward pass ran to its end: a dead end cell leaves it valid)
            if (resumed && tracking && h_meta[i].status == KA_ERR_EMPTY_BEAM)
                KA_HIP(hipMemcpyAsync(a.band_lo_out[i], ws + cv[i].band, bytes, hipMemcpyDeviceToHost, stream));
            if (h_meta[i].status != KA_OK) continue;
            KA_HIP(hipMemcpyAsync(a.best_path[i], ws + cv[i].path, bytes, hipMemcpyDeviceToHost, stream));
            KA_HIP(hipMemcpyAsync(a.best_labels[i], ws + cv[i].lab_out, bytes, hipMemcpyDeviceToHost, stream));
            KA_HIP(hipMemcpyAsync(a.best_scores[i], ws + cv[i].sc_out, bytes, hipMemcpyDeviceToHost, stream));
            if (tracking) KA_HIP(hipMemcpyAsync(a.band_lo_out[i], ws + cv[i].band, bytes, hipMemcpyDeviceToHost, stream));
        }
        KA_HIP(hipStreamSynchronize(stream));
    }
    int first_bad = KA_OK;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t st = h_meta[i].status;
        if (a.status) a.status[i] = st;
        if (a.total_score) a.total_score[i] = h_meta[i].score;
        if (resumed && a.entry) a.entry[i] = st == KA_OK ? h_entry[(size_t)i * cells] : -1;
        if (resumed && tracking && a.next_lo) a.next_lo[i] = st == KA_OK || st == KA_ERR_EMPTY_BEAM ? h_entry[(size_t)i * cells + 1] : -1;
        if (walk) a.determined[i] = h_det[i];
        if (st != KA_OK && first_bad == KA_OK) {
            first_bad = st;
            g_err = "lattice " + std::to_string(i) +
                    status_message(st, {resumed ? ": no live state in the last frame, or the end cell is not live" : ": no live state in the last frame",
                                        nullptr, nullptr,
                                        resumed && tracking ? ": init_scores must hold no +inf"
                                        : resumed           ? ": band_lo must hold non-decreasing values in [0, 2S+1) and init_scores no +inf"
                                                            : ": band_lo must hold non-decreasing values in [0, 2S+1)",
                                        nullptr});
        }
    }
    return first_bad;
}

// the two arguments ka_ctc_best_path_tracking adds: checked before anything else, the engine included
int tracking_args(int32_t period, int32_t end_rule)
{
    if (period < 4 || period > 65536 || period % 4 != 0) return fail(KA_ERR_BAD_ARGS, "tracking best path: period must be a multiple of 4 in [4, 65536]");
    if (end_rule != 0 && end_rule != 1) return fail(KA_ERR_BAD_ARGS, "tracking best path: end_rule must be 0 (highest live) or 1 (best live)");
    return KA_OK;
}

size_t band_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move, int32_t mem, ka::plan::BandMode mode)
{
    if (!countable(n, mem, {T, S})) return 0;
    return ka::plan::band_workspace(n, T, S, V, beam_size, max_move, mem == KA_MEM_HOST, mode, nullptr);
}

}  // namespace

// Every entry point names the fields of its record; a single-lattice call is a batch of one, its scalars and buffers the arrays.
extern "C" {

int ka_ctc_best_path_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                      const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                      const int32_t *const *band_lo, int32_t *const *best_path, int32_t *const *best_labels,
                                      float *const *best_scores, float *total_score, int32_t *status, int32_t mem, void *stream)
{
    return banded_impl(e, {.lat = {n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, .band_lo = band_lo,
                           .best_path = best_path, .best_labels = best_labels, .best_scores = best_scores, .total_score = total_score,
                           .status = status});
}

int ka_ctc_best_path_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                int32_t beam_size, int32_t max_move, const int32_t *band_lo, int32_t *best_path, int32_t *best_labels,
                                float *best_scores, float *total_score, int32_t mem, void *stream)
{
    return banded_impl(e, {.lat = {1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream}, .band_lo = &band_lo,
                           .best_path = &best_path, .best_labels = &best_labels, .best_scores = &best_scores, .total_score = total_score});
}

size_t ka_banded_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move, int32_t mem)
{
    return band_bytes(n, T, S, V, beam_size, max_move, mem, {});
}

int ka_ctc_best_path_tracking_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                        const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move, int32_t period,
                                        int32_t end_rule, int32_t *const *best_path, int32_t *const *best_labels, float *const *best_scores,
                                        int32_t *const *band_lo_out, float *total_score, int32_t *status, int32_t mem, void *stream)
{
    const int rc = tracking_args(period, end_rule);
    if (rc != KA_OK) return rc;
    return banded_impl(e, {.lat = {n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, .mode = {.tracking = true},
                           .period = period, .end_rule = end_rule, .band_lo_out = band_lo_out, .best_path = best_path, .best_labels = best_labels,
                           .best_scores = best_scores, .total_score = total_score, .status = status});
}

int ka_ctc_best_path_tracking_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                  int32_t beam_size, int32_t max_move, int32_t period, int32_t end_rule, int32_t *best_path,
                                  int32_t *best_labels, float *best_scores, int32_t *band_lo_out, float *total_score, int32_t mem, void *stream)
{
    const int rc = tracking_args(period, end_rule);
    if (rc != KA_OK) return rc;
    return banded_impl(e, {.lat = {1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream},
                           .mode = {.tracking = true}, .period = period, .end_rule = end_rule, .band_lo_out = &band_lo_out,
                           .best_path = &best_path, .best_labels = &best_labels, .best_scores = &best_scores, .total_score = total_score});
}

size_t ka_tracking_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move, int32_t mem)
{
    return band_bytes(n, T, S, V, beam_size, max_move, mem, {.tracking = true});
}

int ka_ctc_best_path_resume_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                      const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                      const int32_t *const *band_lo, const float *const *init_scores, const int32_t *end,
                                      int32_t *const *best_path, int32_t *const *best_labels, float *const *best_scores,
                                      float *const *final_scores, int32_t *entry, float *total_score, int32_t *status, int32_t mem, void *stream)
{
    return banded_impl(e, {.lat = {n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream}, .mode = {.resumed = true},
                           .band_lo = band_lo, .best_path = best_path, .best_labels = best_labels, .best_scores = best_scores,
                           .total_score = total_score, .status = status, .init_scores = init_scores, .end = end, .final_scores = final_scores,
                           .entry = entry});
}

int ka_ctc_best_path_resume_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                int32_t beam_size, int32_t max_move, const int32_t *band_lo, const float *init_scores, int32_t end,
                                int32_t *best_path, int32_t *best_labels, float *best_scores, float *final_scores, int32_t *entry,
                                float *total_score, int32_t mem, void *stream)
{
    return banded_impl(e, {.lat = {1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream},
                           .mode = {.resumed = true}, .band_lo = &band_lo, .best_path = &best_path, .best_labels = &best_labels,
                           .best_scores = &best_scores, .total_score = total_score, .init_scores = &init_scores, .end = &end,
                           .final_scores = &final_scores, .entry = entry});
}

size_t ka_resume_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move, int32_t mem)
{
    return band_bytes(n, T, S, V, beam_size, max_move, mem, {.resumed = true});
}

int ka_ctc_best_path_tracking_resume_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                               const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                               int32_t max_move, int32_t period, const int32_t *first_lo, const float *const *init_scores,
                                               const int32_t *end, int32_t *const *best_path, int32_t *const *best_labels,
                                               float *const *best_scores, int32_t *const *band_lo_out, float *const *final_scores,
                                               int32_t *entry, int32_t *next_lo, float *total_score, int32_t *status, int32_t mem, void *stream)
{
    const int rc = tracking_args(period, 0);
    if (rc != KA_OK) return rc;
    return banded_impl(e, {.lat = {n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream},
                           .mode = {.tracking = true, .resumed = true}, .period = period, .band_lo_out = band_lo_out, .best_path = best_path,
                           .best_labels = best_labels, .best_scores = best_scores, .total_score = total_score, .status = status,
                           .init_scores = init_scores, .end = end, .final_scores = final_scores, .entry = entry, .first_lo = first_lo,
                           .next_lo = next_lo});
}

int ka_ctc_best_path_tracking_resume_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                         int32_t beam_size, int32_t max_move, int32_t period, int32_t first_lo, const float *init_scores,
                                         int32_t end, int32_t *best_path, int32_t *best_labels, float *best_scores, int32_t *band_lo_out,
                                         float *final_scores, int32_t *entry, int32_t *next_lo, float *total_score, int32_t mem, void *stream)
{
    const int rc = tracking_args(period, 0);
    if (rc != KA_OK) return rc;
    return banded_impl(e, {.lat = {1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream},
                           .mode = {.tracking = true, .resumed = true}, .period = period, .band_lo_out = &band_lo_out, .best_path = &best_path,
                           .best_labels = &best_labels, .best_scores = &best_scores, .total_score = total_score, .init_scores = &init_scores,
                           .end = &end, .final_scores = &final_scores, .entry = entry, .first_lo = &first_lo, .next_lo = next_lo});
}

size_t ka_tracking_resume_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                          int32_t mem)
{
    return band_bytes(n, T, S, V, beam_size, max_move, mem, {.tracking = true, .resumed = true});
}

int ka_ctc_best_path_determined_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                          const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                          const int32_t *const *band_lo, const float *const *init_scores, const int32_t *end,
                                          int32_t *const *best_path, int32_t *const *best_labels, float *const *best_scores,
                                          float *const *final_scores, int32_t *entry, int32_t *determined, float *total_score, int32_t *status,
                                          int32_t mem, void *stream)
{
    return banded_impl(e, {.lat = {n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream},
                           .mode = {.resumed = true, .walk = true}, .band_lo = band_lo, .best_path = best_path, .best_labels = best_labels,
                           .best_scores = best_scores, .total_score = total_score, .status = status, .init_scores = init_scores, .end = end,
                           .final_scores = final_scores, .entry = entry, .determined = determined});
}

int ka_ctc_best_path_determined_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                    int32_t beam_size, int32_t max_move, const int32_t *band_lo, const float *init_scores, int32_t end,
                                    int32_t *best_path, int32_t *best_labels, float *best_scores, float *final_scores, int32_t *entry,
                                    int32_t *determined, float *total_score, int32_t mem, void *stream)
{
    return banded_impl(e, {.lat = {1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream},
                           .mode = {.resumed = true, .walk = true}, .band_lo = &band_lo, .best_path = &best_path, .best_labels = &best_labels,
                           .best_scores = &best_scores, .total_score = total_score, .init_scores = &init_scores, .end = &end,
                           .final_scores = &final_scores, .entry = entry, .determined = determined});
}

int ka_ctc_best_path_tracking_determined_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                                   const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                                   int32_t max_move, int32_t period, const int32_t *first_lo, const float *const *init_scores,
                                                   const int32_t *end, int32_t *const *best_path, int32_t *const *best_labels,
                                                   float *const *best_scores, int32_t *const *band_lo_out, float *const *final_scores,
                                                   int32_t *entry, int32_t *next_lo, int32_t *determined, float *total_score, int32_t *status,
                                                   int32_t mem, void *stream)
{
    const int rc = tracking_args(period, 0);
    if (rc != KA_OK) return rc;
    return banded_impl(e, {.lat = {n, log_probs, T, V, ld, labels, S, beam_size, max_move, mem, (hipStream_t)stream},
                           .mode = {.tracking = true, .resumed = true, .walk = true}, .period = period, .band_lo_out = band_lo_out,
                           .best_path = best_path, .best_labels = best_labels, .best_scores = best_scores, .total_score = total_score,
                           .status = status, .init_scores = init_scores, .end = end, .final_scores = final_scores, .entry = entry,
                           .first_lo = first_lo, .next_lo = next_lo, .determined = determined});
}

int ka_ctc_best_path_tracking_determined_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels,
                                             int64_t S, int32_t beam_size, int32_t max_move, int32_t period, int32_t first_lo,
                                             const float *init_scores, int32_t end, int32_t *best_path, int32_t *best_labels,
                                             float *best_scores, int32_t *band_lo_out, float *final_scores, int32_t *entry, int32_t *next_lo,
                                             int32_t *determined, float *total_score, int32_t mem, void *stream)
{
    const int rc = tracking_args(period, 0);
    if (rc != KA_OK) return rc;
    return banded_impl(e, {.lat = {1, &log_probs, &T, V, &ld, &labels, &S, beam_size, max_move, mem, (hipStream_t)stream},
                           .mode = {.tracking = true, .resumed = true, .walk = true}, .period = period, .band_lo_out = &band_lo_out,
                           .best_path = &best_path, .best_labels = &best_labels, .best_scores = &best_scores, .total_score = total_score,
                           .init_scores = &init_scores, .end = &end, .final_scores = &final_scores, .entry = entry, .first_lo = &first_lo,
                           .next_lo = next_lo, .determined = determined});
}

size_t ka_determined_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move, int32_t mem,
                                     int32_t tracking)
{
    return band_bytes(n, T, S, V, beam_size, max_move, mem, {.tracking = tracking != 0, .resumed = true, .walk = true});
}

}  // extern "C"
