// ka_launch.hpp — the host-callable launch functions of every device translation unit.
//
// The library is built from thirty-four translation units so that the device code compiles in parallel (a single unit took three
// minutes): ka_engine.hip, ka_engine_fb.hip, ka_engine_band.hip and ka_entry_misc.hip are host code only and reach the kernels
// through these functions; each kernel family lives in the .hip file named below and nowhere else.  A forward-backward call's launch is a
// template over the band, defined in the call's header; its units hold nothing but that template's explicit instantiation, one
// band each.  All functions only enqueue; errors surface through hipGetLastError().
#pragma once
#include "ka_types.hpp"

namespace ka {

// which forward kernels of the one-wavefront-per-lattice family run over a range of descriptors
enum WaveForm { kWaveExact = 0, kWaveCheckpointed = 1 };

// ---- ka_wave_fwd.hip ----
void launch_prep_labels(const Lattice *lats, int n, int32_t *meta, hipStream_t s);
// checkpointed: forward_ck over all, then the exact kernels over what it flagged; exact: forward_w16 over all
void launch_forward_wave(int max_move, const Lattice *lats, int n, int32_t *meta, hipStream_t s, WaveForm form);
// the exact kernels over lattices another forward kernel has flagged kFlagExact
void launch_forward_flagged(int max_move, const Lattice *lats, int n, int32_t *meta, hipStream_t s);
void launch_forward_generic(const Lattice *lats, int n, int32_t *meta, hipStream_t s);

// ---- ka_wave_bt.hip ----
// serial: one wavefront per lattice (skips Lattice::par ones)
void launch_backtrace_rc_serial(int max_move, const Lattice *lats, int n, int32_t *meta, hipStream_t s);
// one wavefront per chunk of the launch's chunk-parallel lattices (Lattice::entry holds where the path enters each)
void launch_backtrace_rc_chunks(int max_move, const Lattice *lats, int n, int32_t *meta, hipStream_t s, unsigned total_chunks);
void launch_backtrace_w16(const Lattice *lats, int n, const int32_t *meta, hipStream_t s, int only_flagged);
void launch_gather_outputs(const Lattice *lats, unsigned grid_x, unsigned grid_y, const int32_t *meta, hipStream_t s, int only_flagged);
void launch_backtrace_generic(const Lattice *lats, int n, const int32_t *meta, hipStream_t s);

// ---- ka_pbt.hip: chunk maps -> super-chunk maps -> entry position of every chunk (ka_parallel_bt.hpp) ----
void launch_chunk_entries(int max_move, const Lattice *lats, int n, int32_t *meta, hipStream_t s, unsigned total_chunks, unsigned max_seg,
                          unsigned max_sup, unsigned max_w);

// ---- ka_tiled256.hip / ka_tiled128.hip: the tile pipelines ----
struct TileLaunch {
    const Lattice *lats;
    const TileTask *tasks;
    int n_tasks;
    int32_t *meta;
    char *halo;
    uint32_t *prog;
    TileAux *aux;
    uint32_t *ticket;
    int verify;
    TpStats *stats;
    uint32_t *cu_rank;  // [kCuSlots] workgroups per CU, zeroed per launch (128-position tiles: ka_tiled128.hpp)
    unsigned lds;       // LDS bytes a workgroup requests (at least what the kernel uses)
    int max_move;
    int pitch;          // 0: rows staged one by one; 256 (V = 64) or 156 (V = 39): contiguous rows, copied as they lie
};
void launch_forward_tiled256(const TileLaunch &a, hipStream_t s);               // two wavefronts per 256-position tile (ka_tiled256.hpp)
void launch_forward_tiled128(const TileLaunch &a, hipStream_t s);               // three wavefronts per 128-position tile (ka_tiled128.hpp); `prog` unused
// The kernel instance <max_move, PITCH, CONTIG> of a tile launch, for either width: Form<M, PITCH, CONTIG>::launch(a, s).
// Contiguous rows (pitch 256 or 156) have one instance each, with max_move 4; rows staged one by one, one per max_move.
template <template <int, int, bool> class Form>
void launch_tile_instance(const TileLaunch &a, hipStream_t s)
{
    if (a.pitch == 256) return Form<4, 256, true>::launch(a, s);
    if (a.pitch == 156) return Form<4, 156, true>::launch(a, s);
    switch (a.max_move) {
    case 1: Form<1, 256, false>::launch(a, s); break;
    case 2: Form<2, 256, false>::launch(a, s); break;
    case 3: Form<3, 256, false>::launch(a, s); break;
    default: Form<4, 256, false>::launch(a, s); break;
    }
}

// ---- ka_misc.hip: log-softmax, hash generators, the log-prob producer's LSTM, the audio front end ----
void launch_log_softmax(const float *in, float *out, int64_t T, int V, int64_t ld_in, int64_t ld_out, hipStream_t s);
void launch_hash_logprobs(float *lp, unsigned blocks, unsigned n, int64_t T, int V, int64_t ld, uint64_t seed0, int64_t lattice_stride, hipStream_t s);
void launch_hash_labels(int32_t *labels, unsigned blocks, unsigned n, int64_t S, int V, uint64_t seed0, int64_t lattice_stride, hipStream_t s);
void launch_lstm_step(const float *gin, int64_t ldg, const float *rec, int64_t rec_dir_stride, float *c, float *h, int64_t state_dir_stride,
                      float *out, int64_t ldo, const int32_t *rows, int64_t rows_dir_stride, int n, int H, hipStream_t s);
// x_in: layer 0 with its input projection inside (gin is x [frames, ldg >= 40]; w_ih, bias given)
void launch_lstm_layer(bool x_in, const float *gin, int64_t ldg, const float *w_hh, float *out, int64_t ldo, const int32_t *seq_off,
                       const int32_t *seq_len, int nseq, const float *w_ih, const float *bias, hipStream_t s);
void launch_window_energy(const float *x, int64_t n_windows, float *out, hipStream_t s);
void launch_stft_frames(const float *y, const int64_t *seg_start, const int64_t *seg_len, const int64_t *frame_off, unsigned grid_x, unsigned nseg,
                        int n_fft, int hop, const float *window, float *frames, int64_t ld, hipStream_t s);
void launch_power(const float *reim, int64_t ld_in, float *power, int64_t ld_out, int64_t n, int nf, hipStream_t s);
void launch_power_to_db(float *x, int64_t ld, int cols, const int64_t *frame_off, unsigned grid_x, unsigned nseg, float top_db, float *segmax, hipStream_t s);

// ---- the forward-backward calls: one launch per call, a template over the band (BandWalk: the reference's diagonal, on the
// call's descriptors; BandTable: a caller's table, on Banded<> descriptors, Banded<>::band_lo in place of the diagonal, with
// the same split, grid and slots).  A call's header defines the template; the unit named holds the instantiation of a band, and
// a band with no unit does not link ----
// ka_posterior.hip, ka_posterior_banded.hip: posteriors of the caller's best path (ka_posterior.hpp).  Descriptors [0, n_fast):
// one wavefront per lattice (band <= kFastMaxBand, V <= 64, max_move <= 4), then [n_fast, n_fast + n_generic): one 256-thread
// workgroup per lattice, columns in global memory
template <class Band>
void launch_posteriors(const BandDesc<PostLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s);
// The calls below go through launch_fb_ck (ka_fb_ck.hpp): descriptors [0, n_fast): one wavefront per lattice on min(n_fast,
// kOccFastSlots) workgroups, lattice i on workgroup i mod grid (its workspace slot); then [n_fast, n_fast + n_generic):
// 256-thread workgroups, min(n_generic, kOccGenericSlots)
// ka_occupancy.hip, ka_occupancy_banded.hip: label occupancy (ka_occupancy.hpp)
template <class Band>
void launch_label_posteriors(const BandDesc<OccLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s);
// ka_state_posterior.hip, ka_state_posterior_banded.hip: state posteriors at chosen frames (ka_state_posterior.hpp)
template <class Band>
void launch_state_posteriors(const BandDesc<StateLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s);
// ka_duration.hip, ka_duration_banded.hip: expected state durations (ka_duration.hpp)
template <class Band>
void launch_state_durations(const BandDesc<DurLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s);
// ka_visit.hip, ka_visit_banded.hip: state visit probabilities (ka_visit.hpp)
template <class Band>
void launch_state_visits(const BandDesc<VisitLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s);
// ka_quantile.hip, ka_quantile_banded.hip: exact boundary-time quantiles (ka_quantile.hpp)
template <class Band>
void launch_boundary_quantiles(const BandDesc<QuantLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s);
// ka_mea.hip, ka_mea_banded.hip: the maximum-expected-accuracy alignment (ka_mea.hpp)
template <class Band>
void launch_mea_path(const BandDesc<MeaLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s);

// ka_fb_resume.hip: label occupancy and path posteriors under the caller's boundary conditions (ka_fb_resume.hpp); BandTable only
template <class Band>
void launch_posteriors_resume(const BandDesc<ResumeFbLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s);

// ka_sample.hip, ka_sample_banded.hip: alignments sampled from the band posterior (ka_sample.hpp): ka_fb_ck.hpp's forward pass
// and block recompute with kernels of its own, launch_fb_ck's form split, grid and slots
template <class Band>
void launch_sample_paths(const BandDesc<SampleLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s);

// ---- ka_margin.hip: best-path margins from max-marginals (ka_margin.hpp): launch_fb_slots' form split, grid and slots; a
// descriptor with a table (MarginLattice::band_lo) runs over it, one without over the reference's diagonal ----
void launch_path_margins(const MarginLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s);
// ---- ka_margin_resume.hip: the same pass under the caller's boundary conditions, with rows of m at chosen frames
// (ka_margin_resume.hpp) ----
void launch_margins_resume(const MarginResumeLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s);

// ---- ka_banded.hip: best path over a caller-given band (ka_banded.hpp).  Descriptors [0, n_fast): one wavefront per lattice
// (band <= kFastMaxBand, V <= 64, max_move <= 4), then [n_fast, n_fast + n_generic): one 256-thread workgroup per lattice.
// `meta` (zeroed by the caller): a LatticeMeta per lattice of the batch ----
void launch_best_path_banded(const BandLattice *lats, int n_fast, int n_generic, int max_move, int32_t *meta, hipStream_t s);
// ... its walk back alone, over a table some forward pass has used
void launch_backtrace_banded(const BandLattice *lats, int n_fast, int n_generic, const int32_t *meta, hipStream_t s);
// ---- ka_tracking.hip: best path over a self-steering band (ka_banded.hpp's BandTracking): the same descriptors, band_lo
// the table the forward kernels WRITE; period a multiple of 4, end_rule 0 (highest live position) or 1 (best live position) ----
void launch_best_path_tracking(const BandLattice *lats, int n_fast, int n_generic, int max_move, int period, int end_rule, int32_t *meta,
                               hipStream_t s);
// ---- ka_resume.hip: the resumable best path (ka_banded.hpp's BandResume): the same descriptors and, in their order, a
// ResumeRows per lattice: start row, last row, end cell or rule, and where the walk back puts the cell it ends on ----
void launch_best_path_resume(const BandLattice *lats, const ResumeRows *rows, int n_fast, int n_generic, int max_move, int32_t *meta,
                             hipStream_t s);
// ... its walk back alone, over a table some forward pass has used
void launch_backtrace_resume(const BandLattice *lats, const ResumeRows *rows, int n_fast, int n_generic, const int32_t *meta, hipStream_t s);
// ---- ka_tracking_resume.hip: the resumable tracking best path (ka_banded.hpp's BandTrackingResume): the two above together.
// A lattice's ResumeRows brings first_lo, and entry points at two cells: the entry and the low end frame T would get ----
void launch_best_path_tracking_resume(const BandLattice *lats, const ResumeRows *rows, int n_fast, int n_generic, int max_move, int period,
                                      int32_t *meta, hipStream_t s);
// ---- ka_determined.hip: the determined prefix of a resumed call (ka_determined.hpp), behind either launch above: the walk
// from every live cell of the last row (ResumeRows::fin, which must be there) back to where the lines merge.  `det`: one int32
// per lattice of the batch, in the caller's order ----
void launch_determined(const BandLattice *lats, const ResumeRows *rows, int n_fast, int n_generic, const int32_t *meta, int32_t *det,
                       hipStream_t s);

}  // namespace ka
