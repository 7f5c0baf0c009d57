/*
 * kokoro_align_amd.h — C ABI of the MI355X (gfx950) CTC forced-alignment hot path.
 *
 * Drop-in boundary for the alignment step of kaiidams/Kokoro-Align.  The reference has no
 * FFI layer: its boundary is three Python functions in kokoro_align/align.py.  Each entry
 * point below names the reference interface it replaces (file:line); the Python mirror
 * that keeps the reference's signatures lives in kokoro-align_amd/align.py and binds these
 * symbols with ctypes.
 *
 * Plain pointers and sizes only; no torch types.  Device pointers may come from any
 * allocator (hipMalloc, a torch tensor's data_ptr(), ...).  The library never retains a
 * caller pointer after a call returns.
 *
 * Thread-safety: one ka_engine per host thread / stream; distinct engines are independent.
 */
#ifndef KOKORO_ALIGN_AMD_H
#define KOKORO_ALIGN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KA_VERSION 104 /* 0.1.4: the serial backtrace's second output form and its debug switch removed */

/* status codes (per call and per lattice) */
#define KA_OK 0
#define KA_ERR_EMPTY_BEAM (-1) /* no live state in the last frame: reference raises ValueError, align.py:101 */
#define KA_ERR_BAD_ARGS (-2)
#define KA_ERR_HIP (-3)       /* HIP runtime error, text in ka_last_error() */
#define KA_ERR_NOMEM (-4)
#define KA_ERR_BAD_LABEL (-5) /* label outside [0,V): reference raises IndexError at align.py:77 */
#define KA_ERR_NONFINITE (-7) /* explicit KA_MODE_TILED only: an infinity among the log-probs of a lattice whose band is wider
                                 than 1009 positions.  KA_MODE_AUTO answers such lattices (the exact kernels for bands up to
                                 1009, the generic kernels above): -inf is legal input, as in the reference */
#define KA_ERR_INTERNAL (-8)  /* tiled form: a tile's hand-off timed out (an internal error, never an input condition) */
#define KA_ERR_NAN (-6)       /* a log-prob is NaN: the reference's np.argmax treats NaN as the maximum (align.py:83); that
                                 is not reproduced - the lattice is rejected (fast path, V <= 64, band <= 1009 or tiled form) */

#define KA_ERR_ZERO_MASS (-9) /* posteriors: no path of finite score reaches the best path's terminal (the lattice
                                 log-likelihood is -inf; the reference can end its path on a state reached only through -inf).
                                 The test is made on the float the log-likelihood is reported from (below): a lattice whose
                                 terminal lies beyond float32's range below the offset of its last 32-frame block, more than
                                 2.3e38 nats within those frames, reports it too */

/* where the caller's buffers live */
#define KA_MEM_HOST 0
#define KA_MEM_DEVICE 1

typedef struct ka_engine ka_engine;

int32_t ka_version(void);
/* message of the last error on the calling thread ("" if none) */
const char *ka_last_error(void);

/* An engine owns the device workspace (back-pointer storage, padded labels, descriptors),
 * pinned staging and timing events for ONE device.  device = HIP ordinal. */
int ka_engine_create(int32_t device, ka_engine **out);
void ka_engine_destroy(ka_engine *e);
/* A HIP stream (hipStream_t, non-blocking) for launches that should run beside others: one engine + one such stream per
 * host thread lets the forward pass of one launch overlap the backtrace of another (kokoro_align_amd.streams).  Streams
 * created one after the other land on different hardware queues while the runtime has any to spare (4 per device). */
int ka_stream_create(int32_t device, void **stream);
int ka_stream_destroy(int32_t device, void *stream);
/* pre-size the workspace so that later calls do not allocate (optional) */
int ka_engine_reserve(ka_engine *e, size_t workspace_bytes);
/* device-workspace bytes one batch call needs at most, whatever the engine's mode (every lattice priced in its most
 * expensive form: tiled with chunk-parallel backtrace); ka_engine_workspace_bytes gives the exact figure for an engine */
size_t ka_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V,
                          int32_t beam_size, int32_t max_move);

/* ... exactly what THIS engine (its mode, backtrace and device) will carve for such a call: the same planning code as the
 * call itself, nothing is launched.  ka_workspace_bytes above is an upper bound over all modes. */
size_t ka_engine_workspace_bytes(ka_engine *e, int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size,
                                 int32_t max_move, int32_t mem);

/*
 * ctc_best_path(log_probs, labels, beam_size=1000, max_move=4) -> (best_path, best_labels, best_scores)
 * replaces kokoro_align/align.py:43-109 (DP align.py:62-93, backtrace :21-40,:99-102, gathers :105-107).
 *
 *   log_probs  [T, V] float32, row stride ld (elements)
 *   labels     [S] int32, values in [0, V)   (un-expanded transcript; blanks are inserted here)
 *   best_path  [T] int32  positions in the blank-expanded label sequence (0 .. 2S)
 *   best_labels[T] int32, best_scores [T] float32 (per-frame emission of the chosen label)
 *   total_score  optional (may be NULL): cumulative float32 score of the terminal state
 *   mem        KA_MEM_HOST: all pointers are host memory (the call copies in and out)
 *              KA_MEM_DEVICE: all pointers except total_score are device memory
 *   stream     hipStream_t to launch on (NULL = default stream).  The call returns after the
 *              outputs are valid (it synchronises the stream).
 * Returns KA_OK, KA_ERR_EMPTY_BEAM (-> ValueError), KA_ERR_BAD_LABEL, KA_ERR_BAD_ARGS, KA_ERR_HIP.
 */
int ka_ctc_best_path_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld,
                         const int32_t *labels, int64_t S, int32_t beam_size, int32_t max_move,
                         int32_t *best_path, int32_t *best_labels, float *best_scores,
                         float *total_score, int32_t mem, void *stream);

/*
 * The same over n independent lattices (one per audio file; the reference loops files
 * sequentially, run_example.py:248-254).  Arrays of n pointers / sizes are HOST arrays;
 * the pointed-to buffers live where `mem` says.  status[n] and total_score[n] are host
 * arrays (either may be NULL).  Returns KA_OK if every lattice succeeded, otherwise the
 * status of the first lattice that failed; the other lattices' outputs are still valid.
 */
int ka_ctc_best_path_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs,
                               const int64_t *T, int32_t V, const int64_t *ld,
                               const int32_t *const *labels, const int64_t *S,
                               int32_t beam_size, int32_t max_move, int32_t *const *best_path,
                               int32_t *const *best_labels, float *const *best_scores,
                               float *total_score, int32_t *status, int32_t mem, void *stream);

/* Split form for device-resident batches: enqueue launches everything on `stream` without a
 * host sync; finish synchronises and fetches per-lattice status / total scores. */
int ka_ctc_best_path_batch_enqueue_f32(ka_engine *e, int32_t n, const float *const *log_probs,
                                       const int64_t *T, int32_t V, const int64_t *ld,
                                       const int32_t *const *labels, const int64_t *S,
                                       int32_t beam_size, int32_t max_move,
                                       int32_t *const *best_path, int32_t *const *best_labels,
                                       float *const *best_scores, void *stream);
int ka_batch_finish(ka_engine *e, float *total_score, int32_t *status);

/*
 * Posterior of a best path and the lattice log-likelihood: the forward-backward pass over the same band, moves and veto
 * as ctc_best_path, with sums where the best path takes maxima.
 *   alpha_t(s) = logsumexp_j alpha_{t-1}(s-j) + lp[t, lab'[s]],  Z = alpha_{T-1}(s*), s* = best_path[T-1]
 *   beta_{T-1} = {s*: 0},  beta_t(s) = logsumexp_j beta_{t+1}(s+j) + lp[t+1, lab'[s+j]]
 *   posteriors[t] = exp(alpha_t(p_t) + beta_t(p_t) - Z), p_t = best_path[t]  (0 where p_t is outside band t)
 * Arguments as ka_ctc_best_path[_batch]_f32, plus best_path [T] int32 (input: any path, usually that call's output) and
 *   posteriors      [T] float32 output (where `mem` says)
 *   log_likelihood  Z in nats, HOST double array [n] (may be NULL): float32 cannot hold it to a useful precision
 *   status          per lattice, HOST [n] (may be NULL)
 * Per lattice: KA_ERR_BAD_LABEL, KA_ERR_NAN, KA_ERR_NONFINITE (+inf among the log-probs; -inf is legal), KA_ERR_BAD_ARGS
 * (a best_path value outside [0, 2S+1)) - posteriors NaN, log-likelihood NaN; KA_ERR_ZERO_MASS - posteriors NaN,
 * log-likelihood -inf.  The call returns KA_OK or the status of the first lattice that failed.  It uses its own kernels
 * (ka_engine_set_mode / set_backtrace do not apply) and synchronises `stream` before it returns.
 *
 * Magnitude (this call and every forward-backward call below).  Log-probs are float32 and the
 * recurrences float64, all of it, their maxima included: any finite log-prob is legal, and a frame c nats below its neighbours
 * (padding, a row of masked logits after log_softmax) changes no posterior.  What float64 itself costs is an ulp of c per
 * step: posteriors, occupancies, durations and visits keep their usual accuracy to a relative 2^-10 up to c = 2^37 for one such
 * frame, 2^33 for eight, 2^30 for seventy; beyond that every call still returns KA_OK, finite values, probabilities in [0, 1]
 * and legal paths (a visit probability, a sum, may exceed 1 by its error: 3e-2 at 2^44).  Two float32 steps of the design see
 * the magnitude sooner.  THIS call stores alpha at the path relative to the offset of its 32-frame block as a float, so a frame
 * c below its neighbours costs the posteriors of the later frames of its block half a float32 ulp of 1.44 c in the exponent:
 * 2^-7 from c = 2^17.  And every call reports log_likelihood from such a float at the terminal: a deep frame in the last block
 * costs it 2^-25 of that block's share; deep frames in earlier blocks cost it nothing beyond float64's own rounding.
 */
int ka_ctc_path_posteriors_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld,
                               const int32_t *labels, int64_t S, int32_t beam_size, int32_t max_move,
                               const int32_t *best_path, float *posteriors, double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_path_posteriors_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                     const int64_t *ld, const int32_t *const *labels, const int64_t *S,
                                     int32_t beam_size, int32_t max_move, const int32_t *const *best_path,
                                     float *const *posteriors, double *log_likelihood, int32_t *status, int32_t mem,
                                     void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments): reserving the larger of this and
 * ka_engine_workspace_bytes keeps both calls free of allocations */
size_t ka_posterior_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size,
                                    int32_t max_move, int32_t mem);

/*
 * Label occupancy posteriors and the lattice log-likelihood of a terminal: the forward-backward pass
 * of ka_ctc_path_posteriors over the same band, moves and veto, for a caller-given terminal s* (host array, one per lattice).
 *   Z = alpha_{T-1}(s*)  (the value ka_ctc_path_posteriors returns for a path that ends at s*)
 *   gamma_t(s) = exp(alpha_t(s) + beta_t(s) - Z),  beta_{T-1} = {s*: 0}
 *   occupancy[t, v] = sum over s in band t with lab'[s] = v of gamma_t(s)   (= dZ / d log_probs[t, v]; rows sum to 1)
 * Arguments as ka_ctc_path_posteriors[_batch]_f32, with terminal in place of best_path and
 *   occupancy       [T_i rows of V] float32 output (where `mem` says), row pitch ld_out[i] >= V elements (other columns untouched)
 * Rows are accumulated in 32.32 fixed point: bit-stable, within 2.5e-7 of their float sum, occupancy[T-1, lab'[s*]] = 1 exactly.
 * Per lattice: KA_ERR_BAD_LABEL, KA_ERR_NAN, KA_ERR_NONFINITE, KA_ERR_BAD_ARGS (terminal outside [0, 2S+1)) - rows NaN,
 * log-likelihood NaN; KA_ERR_ZERO_MASS - rows NaN, log-likelihood -inf.  The call returns KA_OK or the status of the first
 * lattice that failed, uses its own kernels (mode and backtrace settings do not apply) and synchronises `stream`.
 */
int ka_ctc_label_posteriors_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                int32_t beam_size, int32_t max_move, int64_t terminal, float *occupancy, int64_t ld_out,
                                double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_label_posteriors_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                      const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                      int32_t max_move, const int64_t *terminal, float *const *occupancy, const int64_t *ld_out,
                                      double *log_likelihood, int32_t *status, int32_t mem, void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments); bounded by the lattices resident at once, not by n */
size_t ka_label_posterior_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size,
                                          int32_t max_move, int32_t mem);

/*
 * State posteriors at chosen frames and the lattice log-likelihood of a terminal: the forward-backward
 * pass of ka_ctc_label_posteriors (same band, moves, veto, terminal s* and Z), read out per band POSITION at K query frames
 *   gamma[k, j] = gamma_{f_k}(lo_k + j) = exp(alpha_{f_k}(lo_k + j) + beta_{f_k}(lo_k + j) - Z)   for j in [0, hi_k - lo_k)
 *   gamma[k, j] = 0                                                                           for j in [hi_k - lo_k, W)
 *   band_lo[k]  = lo_k, the low end of band f_k;  W = min(beam_size, 2S+1) (at least 1), the widest band
 * Arguments as ka_ctc_label_posteriors[_batch]_f32, with in place of occupancy
 *   frames          [K] int64 query frames, strictly increasing in [0, T): HOST arrays in both memory modes (K = 0 is legal:
 *                   only Z is computed)
 *   gamma           [K rows of W] float32 output (where `mem` says), row pitch ld_out >= W elements (other columns untouched)
 *   band_lo         [K] int64 output (where `mem` says)
 * gamma is formed with the exponent and hardware exp2 of the occupancy: rows sum to 1 within 1e-5, gamma summed by label
 * value is the occupancy row within 1e-5, and at f_k = T-1 the row is exactly 1.0 at s* and 0 elsewhere.  Only the 32-frame
 * blocks that hold a query frame are recomputed: a few frames cost about a path-posterior call.  Per lattice: statuses as
 * ka_ctc_label_posteriors, with NaN rows (columns [0, W)) and band_lo -1 for a failed lattice.  Frames out of order or out
 * of range, or ld_out < W, fail the call with KA_ERR_BAD_ARGS before anything is launched.
 */
int ka_ctc_state_posteriors_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                int32_t beam_size, int32_t max_move, int64_t terminal, const int64_t *frames, int64_t K, float *gamma,
                                int64_t ld_out, int64_t *band_lo, double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_state_posteriors_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                      const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                      int32_t max_move, const int64_t *terminal, const int64_t *const *frames, const int64_t *K,
                                      float *const *gamma, const int64_t *ld_out, int64_t *const *band_lo, double *log_likelihood,
                                      int32_t *status, int32_t mem, void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments); bounded by the lattices resident at once, plus
 * the frame lists (and, for KA_MEM_HOST, the staged inputs and outputs) of every lattice */
size_t ka_state_posterior_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, const int64_t *K, int32_t V,
                                          int32_t beam_size, int32_t max_move, int32_t mem);

/*
 * Expected state durations and the lattice log-likelihood of a terminal: the forward-backward pass of
 * ka_ctc_label_posteriors (same band, moves, veto, terminal s* and Z), summed over time per POSITION of the blank-expanded labels
 *   duration[s] = D(s) = sum over t of gamma_t(s)      expected number of frames spent in s (odd s: phoneme (s-1)/2, even: a blank)
 *   time_sum[s] = B(s) = sum over t of t gamma_t(s)    its first time moment (B / D: the expected centre frame of s)
 * The prefix sums of D are the expected boundary frames: with tau_c the first frame whose state is >= c, E[tau_c] = sum over
 * s < c of D(s).  Arguments as ka_ctc_label_posteriors[_batch]_f32, with in place of occupancy
 *   duration        [2S+1] float64 output (where `mem` says)
 *   time_sum        [2S+1] float64 output (where `mem` says); may be NULL (batch: the array, or any of its entries)
 * gamma is the float the state posteriors write; a position receives one float64 add per frame whose band holds it, in
 * descending frame order, so the sums are those of a sequential float64 loop over the rows of ka_ctc_state_posteriors at
 * every frame, bit for bit, and sum_s D(s) = T within 1e-5 T.  Positions no band holds read 0.  Per lattice: statuses as
 * ka_ctc_label_posteriors, with NaN over [0, 2S+1) for a failed lattice.  Costs a label-posterior call for up to 768 lattices
 * resident at once (three workgroups of 50 KB LDS per CU), two rounds of it from there to 1536.
 */
int ka_ctc_state_durations_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                               int32_t beam_size, int32_t max_move, int64_t terminal, double *duration, double *time_sum,
                               double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_state_durations_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                     const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                     int32_t max_move, const int64_t *terminal, double *const *duration, double *const *time_sum,
                                     double *log_likelihood, int32_t *status, int32_t mem, void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments); bounded by the lattices resident at once (and, for
 * KA_MEM_HOST, the staged inputs and outputs of every lattice) */
size_t ka_state_duration_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size,
                                         int32_t max_move, int32_t mem);

/*
 * State visit probabilities and the lattice log-likelihood of a terminal: on the lattice of
 * ka_ctc_label_posteriors (same band [lo_t, hi_t), moves j in [0, max_move), label-0 veto, terminal s*, statuses and Z), per
 * POSITION of the blank-expanded labels, with exit_t(s) = P(state_t = s and (t = T-1 or state_{t+1} != s)) = gamma_t(s) r_t(s):
 *   visit[s]     = V(s) = sum over t of exit_t(s)     the probability that the path passes through s (paths only move up, so a
 *                                                     position is left once or never: V(s) is in [0, 1])
 *   exit_time[s] = X(s) = sum over t of t exit_t(s)   X / V: the expected LAST frame of s, given that it is visited
 * gamma_t(s) is the float the state posteriors write, widened to double.  r_t(s) is the share of the backward recurrence's
 * log-sum-exp at (t, s) that does not come from the stay j = 0; with x_j the recurrence's terms (-inf for s+j outside band t+1
 * or a vetoed move): r = 1 at t = T-1; r = 1 exactly when x_0 is -inf; r = 0 exactly when no x_j with j >= 1 is finite;
 * otherwise r = 1 - 2^(x_0 - lse_j x_j) in float64, clamped to [0, 1].  A cell with gamma = 0 adds exactly 0.0.  A position
 * receives one float64 add per frame whose band holds it, in descending frame order, as the durations do; so visit[s*] = 1.0,
 * visit[s] = 0.0 for s > s* and for a position no band holds, 0 <= visit[s] <= duration[s] and exit_time[s] <= time_sum[s]
 * against ka_ctc_state_durations on the same input without any tolerance, and visit[s] has the bits of duration[s] for a
 * position that a single frame's band holds.  The expected first frame follows from the two calls: E[first; visited] =
 * X - D + V.  Arguments as ka_ctc_state_durations[_batch]_f32, with in place of duration and time_sum
 *   visit           [2S+1] float64 output (where `mem` says)
 *   exit_time       [2S+1] float64 output (where `mem` says); may be NULL (batch: the array, or any of its entries)
 * Per lattice: statuses as ka_ctc_label_posteriors, with NaN over [0, 2S+1) for a failed lattice; nothing is written beyond
 * [0, 2S+1).  Resources as the state durations' (50 KB of LDS, three workgroups per CU); measured at 1.05 (1024 lattices) to
 * 1.08 (one lattice) times a state-duration call.
 */
int ka_ctc_state_visits_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                            int32_t beam_size, int32_t max_move, int64_t terminal, double *visit, double *exit_time,
                            double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_state_visits_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                  const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                  int32_t max_move, const int64_t *terminal, double *const *visit, double *const *exit_time,
                                  double *log_likelihood, int32_t *status, int32_t mem, void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments); bounded by the lattices resident at once (and, for
 * KA_MEM_HOST, the staged inputs and outputs of every lattice) */
size_t ka_state_visit_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                      int32_t mem);

/*
 * Exact boundary-time quantiles and the lattice log-likelihood of a terminal: on the lattice of
 * ka_ctc_label_posteriors (same band [lo_t, hi_t), moves j in [0, max_move), label-0 veto, terminal s*, statuses and Z), with
 * L = 2S+1 and tau_c the first frame whose state is >= c (as expected_crossing_frames reads it): paths only move up, so
 * P(tau_c <= t) = P(state_t >= c) = sum over s >= c of gamma_t(s), and a quantile of tau_c is the first frame at which that sum
 * passes a level.  The sum is taken in the occupancy's 32.32 fixed point, an integer, so the result does not depend on the
 * order of the adds and is defined bit for bit by the rows of ka_ctc_state_posteriors:
 *   F_t(c) = 2^32 where c <= lo_t (the whole band lies at or above the cut: every path is there), 0 where c >= hi_t, else the
 *            sum over p in [c, hi_t) of fix(gamma_t(p)), fix(g) = (uint64_t)(g 2^32), gamma the float the state posteriors write
 *   thr_m  = (uint64_t)ceil(levels[m] 2^32), computed on the host in double
 *   quantile[k, m] = the smallest t in [0, T) with F_t(cuts[k]) >= thr_m, and T if there is none
 * a minimum over ALL frames (F need not be monotone in t in float).  c = 0 gives 0; c > s* or c = L gives T; quantile[k, m] <=
 * quantile[k, m+1] and quantile[k, m] <= quantile[k+1, m] hold without tolerance.  Arguments as ka_ctc_state_durations[_batch]_f32,
 * with in place of duration and time_sum
 *   cuts            [K] int64 HOST array in both memory modes (as the state posteriors' frames): strictly increasing in [0, L];
 *                   K = 0 is legal, and then only Z is computed
 *   levels, M       [M] double HOST array, 1 <= M <= 8, strictly increasing in [2^-10, 1 - 2^-10] (the upper limit keeps every
 *                   threshold clear of a row's own sum, which is 1 within 1e-5); one array for every lattice of a batch
 *   quantile, ld_q  [K, ld_q] int32 output (where `mem` says), ld_q >= M the row pitch; columns [0, M) are written, others untouched
 * Per lattice: statuses as ka_ctc_label_posteriors, with -1 over [K, M] for a failed lattice.  KA_ERR_BAD_ARGS before anything is
 * launched for cuts out of order or range, M outside [1, 8], a level outside its interval, levels out of order, ld_q < M.
 * Resources: the state durations' slots; 42 496 B of LDS in the one-wavefront form (three workgroups per CU), no scratch.
 * Measured at 1.04 (one lattice) to 1.05 (768 lattices) times a state-duration call with the ~100 cuts of a file's text
 * boundaries, and at 1.09 to 1.11 times with a cut at every even position (5001 cuts): a dense cut list costs about twice the
 * excess of a sparse one.
 */
int ka_ctc_boundary_quantiles_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                  int32_t beam_size, int32_t max_move, int64_t terminal, const int64_t *cuts, int64_t K,
                                  const double *levels, int32_t M, int32_t *quantile, int64_t ld_q, double *log_likelihood, int32_t mem,
                                  void *stream);
int ka_ctc_boundary_quantiles_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                        const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                        int32_t max_move, const int64_t *terminal, const int64_t *const *cuts, const int64_t *K,
                                        const double *levels, int32_t M, int32_t *const *quantile, const int64_t *ld_q,
                                        double *log_likelihood, int32_t *status, int32_t mem, void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments): the state durations' slots, the cuts and start frames of
 * every lattice, the thresholds, one row of 64-bit words per generic slot (and, for KA_MEM_HOST, the staged inputs and outputs) */
size_t ka_boundary_quantile_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, const int64_t *K, int32_t M, int32_t V,
                                            int32_t beam_size, int32_t max_move, int32_t mem);

/*
 * Alignments sampled from the band posterior, and the lattice log-likelihood of a terminal: forward
 * filter, backward sample on the lattice of ka_ctc_label_posteriors (same band [lo_t, hi_t), moves j in [0, max_move), label-0
 * veto, terminal s*, statuses and Z).  With u_t(s) the forward value and lab' the blank-expanded labels, sample k is the path
 *   s_{T-1} = s*;  for t = T-1 ... 1, p = s_t:
 *     x_j = u_{t-1}(p - j) if p - j is in [lo_{t-1}, hi_{t-1}) and not (j even, j >= 2, lab'[p] == 0), else -inf
 *     w_j = 2^(x_j - max_j x_j);  tot = w_0 + ... + w_{M-1} (ascending j, float64);  r = U(k, t-1) tot
 *     s_{t-1} = p - j*, j* the smallest j with w_0 + ... + w_j > r (if rounding leaves none: the largest j with w_j > 0)
 *   U(k, t) = (mix(seed, k T + t) >> 11) 2^-53, mix the 64-bit generator of ka_hash_logprobs_f32
 * so a path is drawn with its share of Z, and sample k has the same bits whatever n_samples is and whether its lattice is sent
 * alone or in a batch.  Arguments as ka_ctc_label_posteriors[_batch]_f32, with in place of occupancy
 *   n_samples       in [1, 64]
 *   seed            the lattice's own 64-bit seed (more than 64 samples: further calls with other seeds)
 *   paths           [n_samples rows of T] int32 output (where `mem` says): row k is sample k's position at every frame, row
 *                   pitch ld_paths >= T elements (columns [T, ld_paths) untouched)
 * Per lattice: statuses and log-likelihood as ka_ctc_label_posteriors (the same bits), with -1 over [0, T) of every row of a
 * failed lattice.  n_samples outside [1, 64] or ld_paths < T fail the call with KA_ERR_BAD_ARGS before anything is launched.
 */
int ka_ctc_sample_paths_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                            int32_t beam_size, int32_t max_move, int64_t terminal, int32_t n_samples, uint64_t seed, int32_t *paths,
                            int64_t ld_paths, double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_sample_paths_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                  const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                  int32_t max_move, const int64_t *terminal, const int32_t *n_samples, const uint64_t *seed,
                                  int32_t *const *paths, const int64_t *ld_paths, double *log_likelihood, int32_t *status, int32_t mem,
                                  void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments); bounded by the lattices resident at once (and, for
 * KA_MEM_HOST, the staged inputs and outputs of every lattice) */
size_t ka_sample_paths_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, const int32_t *n_samples, int32_t V,
                                       int32_t beam_size, int32_t max_move, int32_t mem);

/*
 * The maximum-expected-accuracy alignment (posterior-decoded path) and the lattice log-likelihood of a terminal (DESIGN.md
 * section 4.26): on the lattice of ka_ctc_label_posteriors (same band [lo_t, hi_t), moves j in [0, max_move), label-0 veto,
 * terminal s*, statuses and Z), the band path that ends at s* with the most frames at the right state in expectation,
 *   path = argmax over paths of sum over t of gamma_t(path[t]),   gamma the float ka_ctc_state_posteriors writes.
 * With lab' the blank-expanded labels, in float64 (one add per cell, so the sums have no order dependence):
 *   W_{T-1}(p) = gamma_{T-1}(p) if p = s*, else -inf
 *   W_t(p)     = gamma_t(p) + max over j in [0, max_move) with p + j in [lo_{t+1}, hi_{t+1}) and not (j even, j >= 2,
 *                lab'[p + j] == 0) of W_{t+1}(p + j)   (-inf where no such j has a finite W);  c_t(p) = the SMALLEST such j
 *   path[0]    = the smallest j < max_move in [lo_0, hi_0), not (j even, j >= 2, lab'[j] == 0), that maximises W_0(j)
 *   path[t+1]  = path[t] + c_t(path[t]);   expected_accuracy = W_0(path[0])
 * so the path and expected_accuracy equal that recursion run on the rows of ka_ctc_state_posteriors at every frame, bit for
 * bit, without the [T, W] matrix.  expected_accuracy / T is the expected fraction of correctly placed frames.
 * Arguments as ka_ctc_label_posteriors[_batch]_f32, with in place of occupancy
 *   path               [T] int32 output (where `mem` says): the path's position in the blank-expanded labels at every frame
 *   expected_accuracy  float64 output, HOST memory in both modes (batch: [n]); may be NULL
 * Per lattice: statuses and log-likelihood as ka_ctc_label_posteriors (the same bits), with -1 over [0, T) of the path and NaN
 * as the expected accuracy of a failed lattice.  Measured at 1.03 (1024 lattices) to 1.08 (one lattice) times a state-duration
 * call; like it, up to 768 lattices are resident at once and 769 to 1536 run in two rounds.
 */
int ka_ctc_mea_path_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                        int32_t beam_size, int32_t max_move, int64_t terminal, int32_t *path, double *expected_accuracy,
                        double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_mea_path_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                              const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                              const int64_t *terminal, int32_t *const *path, double *expected_accuracy, double *log_likelihood,
                              int32_t *status, int32_t mem, void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments): the slots of ka_label_posterior_workspace_bytes plus,
 * per slot, the back-pointers of the longest lattice it serves (256 bytes per frame in the one-wavefront form) */
size_t ka_mea_path_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                   int32_t mem);

/*
 * Best path over a caller-given band: ka_ctc_best_path with the band's low end read from a table
 * instead of the diagonal of align.py:64-65.  With lab' the blank-expanded labels, L = 2S+1, A_{-1} = {0}, sc_{-1}[0] = 0:
 *   frame t:  lo_t = band_lo[t],  hi_t = min(lo_t + beam_size, L)
 *     p in [lo_t, hi_t):  c_j = sc_{t-1}[p-j] (+) lp[t, lab'[p]] for j in [0, max_move) with p-j live after frame t-1, else -inf
 *                         (float32 add, then compare);  j even, j >= 2, lab'[p] == 0  ->  c_j = -inf
 *                         j* = the first j attaining the maximum;  p is live iff p-j* is;  sc_t[p] = c_j*
 *   end = the highest live position of frame T-1 (none: KA_ERR_EMPTY_BEAM); the path is walked back over the j*.
 * A valid table holds 0 <= band_lo[t] < L and band_lo[t] <= band_lo[t+1]; the step is not limited (one that leaves frame t+1
 * without a live predecessor is legal and ends in KA_ERR_EMPTY_BEAM).  With band_lo[t] = max(0, L t / T - beam_size / 2) the
 * call returns the bits of ka_ctc_best_path_f32: path, labels, scores, total score and status.
 * Arguments and return convention as ka_ctc_best_path[_batch]_f32, plus
 *   band_lo   [T] int32, where `mem` says (batch: a HOST array of n such pointers)
 * Per lattice: KA_ERR_BAD_ARGS for an invalid table (checked on the device before any value of it is used; the lattice's
 * outputs are left untouched), KA_ERR_BAD_LABEL, KA_ERR_NAN, KA_ERR_EMPTY_BEAM; -inf log-probs are legal.  A batch answers
 * its other lattices and returns the status of the first that failed.  The call uses its own kernels (ka_engine_set_mode /
 * ka_engine_set_backtrace do not apply): one wavefront per lattice for min(beam_size, L) <= 1009, V <= 64, max_move <= 4, else
 * one 256-thread workgroup per lattice (any band, any V, max_move <= 255; not tuned).  It synchronises `stream` before it
 * returns.  Cost against ka_ctc_best_path_batch_f32 in KA_MODE_WAVE_EXACT with KA_BACKTRACE_SERIAL on the diagonal table
 * (tools/bench_banded.py, profiles/banded_bench.jsonl; MI355X): 1.08 times that call for one cfg2 lattice (33.35 against 30.94 ms),
 * 1.26 times for 1024 (42.69 against 33.96 ms).
 */
int ka_ctc_best_path_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                int32_t beam_size, int32_t max_move, const int32_t *band_lo, int32_t *best_path, int32_t *best_labels,
                                float *best_scores, float *total_score, int32_t mem, void *stream);
int ka_ctc_best_path_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                      const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                      const int32_t *const *band_lo, int32_t *const *best_path, int32_t *const *best_labels,
                                      float *const *best_scores, float *total_score, int32_t *status, int32_t mem, void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments): per lattice the prepared labels and, in the
 * one-wavefront form, a copy of the table and 256 bytes of codes per frame (generic: a byte per band cell and four columns);
 * for KA_MEM_HOST also the staged inputs and outputs */
size_t ka_banded_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                 int32_t mem);

/*
 * Best path over a self-steering band: ka_ctc_best_path_banded with the table computed on the fly and
 * returned.  Every `period` frames the band is re-centred on the best-scoring live cell, so it waits while the reader pauses
 * and moves as fast as they read.  With L = 2S+1, B = beam_size, P = period, and "the scores after frame k" the live cells and
 * float32 scores of the banded recurrence after frame k (after frame -1: the virtual state {0: 0.0}):
 *   lo_0 = 0
 *   t > 0, t % P != 0:  lo_t = lo_{t-1}
 *   t > 0, t % P == 0:  c = the position of the FIRST maximum of the scores after frame t-2 over the live cells, in ascending
 *                       position (ties to the lowest position, values compared as floats, an all -inf list gives its lowest
 *                       live position);  lo_t = min(max(lo_{t-1}, c - B / 2), L - 1);  no live cell: lo_t = lo_{t-1}
 *   hi_t = min(lo_t + B, L);  everything else is the frame of ka_ctc_best_path_banded (moves, float32 add then compare, first
 *   maximum, the veto on the label value, liveness, outputs, total score).
 * The lag of two frames is the kernel's: where it needs the band of frame t it holds the scores after frame t-2.
 *   period    a multiple of 4 in [4, 65536], else KA_ERR_BAD_ARGS before anything is launched
 *   end_rule  0: the path ends at the highest live position of frame T-1 (the reference's rule); 1: at the first maximum of the
 *             scores after frame T-1 over the live cells (audio that ends before the text does: under a tracking band the
 *             highest live cell is just the band's top); anything else KA_ERR_BAD_ARGS
 *   band_lo_out  [T] int32 output, where `mem` says (batch: a HOST array of n such pointers): the table the call walked.
 *             Required: NULL is KA_ERR_BAD_ARGS.
 * Other arguments, memory modes, return convention and stream synchronisation as ka_ctc_best_path_banded[_batch]_f32.
 * What follows, exactly:
 *   1. the table is valid for ka_ctc_best_path_banded and its posterior siblings: non-decreasing, in [0, L), constant
 *      between multiples of P;
 *   2. with end_rule 0, ka_ctc_best_path_banded over the returned table returns the same path, labels, scores, total score
 *      and status, bit for bit;
 *   3. with B >= 2L the table is all zeros and every output is ka_ctc_best_path_f32's at the same beam_size, for any period;
 *   4. the arg-max cell of frame t-2 can stay (a move of 0 is never vetoed) and is never below the new lo, so a lattice with
 *      valid labels, no NaN and B >= 1 never ends in KA_ERR_EMPTY_BEAM (the status is kept for the ABI's symmetry);
 *   5. a lattice gives the same bits alone or inside a batch.
 * Per lattice: KA_ERR_BAD_LABEL, KA_ERR_NAN, KA_ERR_EMPTY_BEAM.  A failed lattice's three path outputs are left as the banded
 * call leaves them; its band_lo_out may hold anything within its own T elements.  A NaN never becomes an index: the retarget is
 * clamped to [lo_{t-1}, L - 1] whatever the floats are, and the lattice is rejected at the end.
 * Rule of thumb: the path is kept while period x (positions the reader advances per frame) < beam_size / 2.  The steering is
 * greedy: a long passage of audio that the text does not hold can pull the band away, and nothing pulls it back.
 * band_edge_contact (Python) on the returned table shows when that happened.
 * Forms as ka_ctc_best_path_banded: one wavefront per lattice for min(beam_size, L) <= 1009, V <= 64, max_move <= 4 (a retarget
 * is one cross-lane arg-max per period on top of the banded frame loop), else one 256-thread workgroup per lattice (not tuned).
 * Cost against ka_ctc_best_path_banded_batch_f32 fed the returned table (tools/bench_tracking.py, profiles/tracking_bench.jsonl;
 * MI355X, cfg2): one lattice 1.009 times that call at period 16 (31.59 against 31.32 ms) and 0.955 times at period 64; 1024
 * lattices 0.996 times at period 16 (33.92 against 34.07 ms) and 0.947 times at period 64.
 */
int ka_ctc_best_path_tracking_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                  int32_t beam_size, int32_t max_move, int32_t period, int32_t end_rule, int32_t *best_path,
                                  int32_t *best_labels, float *best_scores, int32_t *band_lo_out, float *total_score, int32_t mem,
                                  void *stream);
int ka_ctc_best_path_tracking_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                        const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move, int32_t period,
                                        int32_t end_rule, int32_t *const *best_path, int32_t *const *best_labels, float *const *best_scores,
                                        int32_t *const *band_lo_out, float *total_score, int32_t *status, int32_t mem, void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments): ka_banded_workspace_bytes without the copy of the
 * table; for KA_MEM_HOST the staged table is the fourth staged output */
size_t ka_tracking_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                   int32_t mem);

/*
 * Resumable best path: ka_ctc_best_path_banded started from a caller-given score row, ended at a
 * caller-given cell or rule, and returning the score row after its last frame and the cell of the start row its path left
 * from.  The recurrence, the table and its check, forms, limits, memory modes, statuses, return convention and stream
 * synchronisation are ka_ctc_best_path_banded[_batch]_f32's; only the boundary conditions are the caller's.  L = 2S+1.
 *   init_scores   [L] float32, where `mem` says, or NULL (batch: a HOST array of n such pointers, itself or any entry NULL).
 *                 NULL: the virtual state {0: 0.0}.  Else the state before frame 0 is A_{-1} = {p : init_scores[p] is not a
 *                 NaN} with sc_{-1}[p] = init_scores[p]; -inf is a LIVE cell of score -inf (liveness is separate from the
 *                 score, and a resumed chunk keeps it).  No band applies to this row: frame 0 reads sc_{-1}[p-j] for p in
 *                 [lo_0, hi_0), so only the cells [lo_0 - (max_move-1), hi_0) can matter; no live cell among them ends in
 *                 KA_ERR_EMPTY_BEAM.  A +inf anywhere in the row is KA_ERR_BAD_ARGS for that lattice alone, found on the
 *                 device by the preparation kernel.  In KA_MEM_DEVICE the row must not overlap final_scores.
 *   end           int32 (batch: a HOST array of n, NULL = all -1).  -1: the path ends at the highest live position of frame
 *                 T-1 (the reference's rule); -2: at the first maximum of the scores after frame T-1 over the live cells in
 *                 ascending position (ka_ctc_best_path_tracking's end_rule 1); p >= 0: at p, and if p is not live after frame
 *                 T-1 the lattice ends in KA_ERR_EMPTY_BEAM.  A value < -2 or >= L is KA_ERR_BAD_ARGS before anything is
 *                 launched or written.
 *   final_scores  [L] float32 output, where `mem` says; NULL as init_scores.  A position live after frame T-1 gets
 *                 sc_{T-1}[p], every other position of [0, L) the quiet NaN of bits 0x7fc00000.  Written whenever the forward
 *                 pass ran, so also for a dead end cell and for an empty beam (all NaN); a lattice that ends in
 *                 KA_ERR_BAD_LABEL, KA_ERR_NAN or KA_ERR_BAD_ARGS (as a lattice's status) gets all NaN, so that a chunk
 *                 resumed from it ends in KA_ERR_EMPTY_BEAM, never in numbers.
 *   entry         int32 output, HOST memory in both modes (batch: [n]); may be NULL.  The cell of A_{-1} the path left from,
 *                 path[0] - j*_0(path[0]); 0 for a NULL init_scores; -1 for a lattice without a path.
 *   total_score   sc_{T-1}[end cell], as in the banded call.
 * What follows, exactly:
 *   1. with init_scores NULL (or NaN everywhere but 0.0 at position 0), end -1 and final_scores NULL every output is
 *      ka_ctc_best_path_banded's, bit for bit;
 *   2. cut and resume: for any table and k in [1, T), chunk A = frames [0, k) with band_lo[:k], chunk B = frames [k, T) with
 *      band_lo[k:], init_scores = A's final_scores and end -1, then A again with end = B's entry: the two paths, label and score
 *      arrays concatenated are the uncut banded call's and B's total_score has its bits; if the uncut call ends in
 *      KA_ERR_EMPTY_BEAM, so does A or B;
 *   3. a lattice gives the same bits alone or inside a batch, whatever its neighbours' rows and ends are.
 * Cost: the start and last rows are O(L) once per call against the frame loop's O(T x band), and the frame loop is the banded
 * call's instruction for instruction (the start row goes through the re-labelling block a band step takes, in frame 0 only).
 * Measured against ka_ctc_best_path_banded_batch_f32 of the same build on the same table (tools/bench_resume.py,
 * profiles/resume_bench.jsonl; MI355X, cfg2): 1.0035 times that call for one lattice with NULL rows and 1.0033 with a start row,
 * a last row and a given end (33.50 and 33.49 against 33.38 ms); 1.0050 and 1.0055 for 1024 lattices (36.36 and 36.38 against
 * 36.18 ms).  Cutting one lattice into 8 chunks that resume from each other (ctc_best_path_chunked) costs 1.888 times the
 * uncut call, (2 - 1/8) forward passes, and needs the move codes of one chunk.
 */
int ka_ctc_best_path_resume_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                int32_t beam_size, int32_t max_move, const int32_t *band_lo, const float *init_scores, int32_t end,
                                int32_t *best_path, int32_t *best_labels, float *best_scores, float *final_scores, int32_t *entry,
                                float *total_score, int32_t mem, void *stream);
int ka_ctc_best_path_resume_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                      const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                      const int32_t *const *band_lo, const float *const *init_scores, const int32_t *end,
                                      int32_t *const *best_path, int32_t *const *best_labels, float *const *best_scores,
                                      float *const *final_scores, int32_t *entry, float *total_score, int32_t *status, int32_t mem,
                                      void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments): ka_banded_workspace_bytes plus 36 bytes per lattice
 * (its rows' descriptor and entry cell, rounded up for the batch) and, for KA_MEM_HOST, the two staged rows of every lattice */
size_t ka_resume_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                 int32_t mem);

/*
 * Resumable tracking best path: ka_ctc_best_path_tracking under ka_ctc_best_path_resume's boundary
 * conditions, plus one value in and one value out, so that a self-steering band crosses a cut: a long recording is aligned
 * chunk by chunk, in the memory of one chunk, without a table known in advance.  L = 2S+1, B = beam_size, P = period.
 *   init_scores, end, final_scores, entry, total_score
 *                 exactly as in ka_ctc_best_path_resume: a NaN is a dead cell, -inf a live cell, a +inf that lattice's
 *                 KA_ERR_BAD_ARGS, found by the preparation kernel; no band applies to the start row; end is -1, -2 or a
 *                 position (it replaces ka_ctc_best_path_tracking's end_rule: -2 is end_rule 1); the last row holds 0x7fc00000
 *                 in dead cells and is all dead for a lattice that failed; entry is -1 without a path, 0 for a NULL row.
 *   first_lo      int32 (batch: a HOST array of n, NULL = all 0): lo_0, the band of the chunk's frame 0.  A value outside
 *                 [0, L) is KA_ERR_BAD_ARGS before anything is launched or written.
 *   retargets     fall on the chunk's OWN frames t > 0 with t % P == 0, by ka_ctc_best_path_tracking's rule, unchanged: c = the
 *                 first maximum of the float32 scores after local frame t-2 over the live cells in ascending position,
 *                 lo_t = min(max(lo_{t-1}, c - B / 2), L - 1); no live cell keeps lo_{t-1}.  Frame 0 never retargets: its band
 *                 is first_lo.  (A chunk of the caller's therefore continues an uncut call only if it starts at a multiple of P.)
 *   band_lo_out   [T] the table walked, as in the tracking call.  Required.
 *   next_lo       int32 output, HOST memory in both modes (batch: [n]); may be NULL.  The low end local frame T would get:
 *                 if T % P == 0 the retarget rule applied to lo_{T-1} and the scores after frame T-2, else lo_{T-1}.  It is the
 *                 first_lo of a call on the frames that follow.  -1 for a lattice that ends in KA_ERR_BAD_LABEL, KA_ERR_NAN or
 *                 KA_ERR_BAD_ARGS.  A lattice that ends in KA_ERR_EMPTY_BEAM (its forward pass ran to the last frame: a dead
 *                 end cell, or no live cell at all) still gets its table and next_lo, like final_scores.
 *   period        a multiple of 4 in [4, 65536], else KA_ERR_BAD_ARGS before anything is launched.
 * Statuses, forms, limits, memory modes, return convention and stream synchronisation are those of the two parent calls.
 * ka_ctc_best_path_tracking's property 4 (never KA_ERR_EMPTY_BEAM) does NOT carry over: a start row without a live cell in
 * reach of [first_lo, first_lo + B) (a NULL row with first_lo >= max_move, for one) and a given end that is dead both end there.
 * What follows, exactly, bit for bit:
 *   1. with init_scores NULL, first_lo 0, final_scores NULL and end -1 or -2, every output (path, labels, scores, table, total
 *      score, status) is ka_ctc_best_path_tracking's for end_rule 0 or 1;
 *   2. cut and resume: for any k in [P, T) with k % P == 0, chunk A = frames [0, k), chunk B = frames [k, T) with init_scores =
 *      A's final_scores, first_lo = A's next_lo and the uncut call's end, then A again with end = B's entry: the tables, paths,
 *      label and score arrays concatenated are the uncut tracking call's; B's total_score, final_scores and next_lo are those of
 *      the uncut call run through this entry point; where the uncut call fails, A or B fails too.  (A's next_lo is the uncut
 *      lo_k because the retarget at global frame k reads the scores after frame k-2, which A holds when it computes next_lo,
 *      and B's own retargets fall on global multiples of P because k is one.)
 *   3. ka_ctc_best_path_resume over a chunk's returned table, with the same start row and end, returns that chunk's path,
 *      labels, scores, total score, entry and last row (ctc_best_path_tracking_chunked's second sweep relies on it);
 *   4. a lattice gives the same bits alone or inside a batch, whatever its neighbours' rows, ends and first_lo are.
 * Cost: the frame loop is the tracking call's; next_lo is computed in the once-per-period retarget branch, for the last frame
 * only; the start and last rows are O(L) once per call.  Measured against ka_ctc_best_path_tracking_batch_f32 of the same build
 * (tools/bench_tracking_resume.py, profiles/tracking_resume_bench.jsonl; MI355X, cfg2): one lattice 0.975 times that call with NULL
 * rows and 0.976 with a start row, a last row, a given end and next_lo at period 16 (30.44 and 30.49 against 31.24 ms), 0.972 and
 * 0.974 at period 64; 1024 lattices 0.976 and 0.974 at period 16 (33.06 and 33.01 against 33.88 ms), 0.975 and 0.974 at period 64.
 * One lattice in 8 chunks that resume from each other (ctc_best_path_tracking_chunked) costs 1.866 times the uncut tracking call at
 * period 16 and 1.912 times at period 64, against (2 - 1/8) forward passes, and needs the move codes of one chunk.
 */
int ka_ctc_best_path_tracking_resume_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                         int32_t beam_size, int32_t max_move, int32_t period, int32_t first_lo, const float *init_scores,
                                         int32_t end, int32_t *best_path, int32_t *best_labels, float *best_scores, int32_t *band_lo_out,
                                         float *final_scores, int32_t *entry, int32_t *next_lo, float *total_score, int32_t mem, void *stream);
int ka_ctc_best_path_tracking_resume_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                               const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                               int32_t max_move, int32_t period, const int32_t *first_lo, const float *const *init_scores,
                                               const int32_t *end, int32_t *const *best_path, int32_t *const *best_labels,
                                               float *const *best_scores, int32_t *const *band_lo_out, float *const *final_scores,
                                               int32_t *entry, int32_t *next_lo, float *total_score, int32_t *status, int32_t mem, void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments): ka_tracking_workspace_bytes plus 40 bytes per lattice
 * (its rows' descriptor, entry cell and next_lo cell, rounded up for the batch) and, for KA_MEM_HOST, the two staged rows of
 * every lattice */
size_t ka_tracking_resume_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                          int32_t mem);

/*
 * Determined prefix of a resumed best path: ka_ctc_best_path_resume and
 * ka_ctc_best_path_tracking_resume with one more output, how many frames of the returned path are final whatever audio
 * follows.  It is the reference's flush_determined_path (kokoro_align/align.py:21-40) as a call: a walk back from ALL live
 * cells of the last frame until their back-pointers meet in one cell.  The arguments are the parent call's, in its order, with
 *   determined    int32 output behind entry (tracking: behind next_lo), HOST memory in both modes (batch: [n]).  Required: NULL
 *                 is KA_ERR_BAD_ARGS before anything is launched or written.
 * Definition, no tolerance anywhere.  A_{-1} the start row's live cells, A_t the live cells after frame t, j*_t(p) the move
 * chosen for cell p in frame t (the first maximum, as in every best-path call):
 *   anc_{T-1} = A_{T-1}                          (every live cell after the last frame, NOT only the end cell)
 *   anc_{t-1} = { p - j*_t(p) : p in anc_t }     for t = T-1 ... 0     (anc_{-1} is a set of cells of the start row)
 *   determined = 1 + max{ t in [-1, T-1] : |anc_t| == 1 },   -1 if there is no such t
 * |anc_t| does not increase going back, so determined is the first frame, walking back, at which one cell is left.
 *   d >= 1        frames [0, d) of the returned path are the same whichever live cell the path ends at, and stay the same if the
 *                 alignment continues from final_scores; with a live end cell path[d-1] is the merge cell.  d = T: one live cell
 *                 after the last frame.
 *   d = 0         no frame of this chunk is final, but all live cells leave the start row from one cell: the returned entry,
 *                 which closes the chunk before this one.  A NULL init_scores has the start row {0}: d >= 0 whenever a cell is live.
 *   d = -1        the live cells trace back to more than one start cell, or no cell is live after frame T-1 (a lattice that
 *                 ends in KA_ERR_BAD_LABEL, KA_ERR_NAN or KA_ERR_BAD_ARGS included).
 * determined depends on the live set, not on end: a given end cell that is dead still ends in KA_ERR_EMPTY_BEAM with entry -1,
 * and determined is reported as defined.  An ancestor of a live cell is live, and a live cell of score -inf counts like any other.
 * Every other output, status, return value and stream synchronisation is the parent call's, bit for bit; a lattice gives the
 * same bits alone or inside a batch.  The forward kernels and walks back are the parent's; one kernel more runs behind them
 * (ka_determined.hpp): one wavefront per lattice over the 2-bit move codes with the set as a bit mask over the ring, or a
 * 256-thread workgroup over the byte codes in the generic form.  It stops at the merge frame: its cost is the merge lag
 * T - determined, not T.
 * Measured against the parent entry point of the same build on the same inputs (tools/bench_determined.py,
 * profiles/determined_bench.jsonl; MI355X, cfg2: T = 50000, S = 5000, beam 1000, V = 64): the walk costs about 96 ns per frame
 * walked.  One lattice whose lines merge 2579 frames before the end (a peaked input): 1.0075 times ka_ctc_best_path_resume
 * (33.64 against 33.39 ms) and 1.0070 / 1.0082 times ka_ctc_best_path_tracking_resume at periods 16 / 64; 1024 such lattices
 * 1.0097, 1.0119 and 1.0099.  The hash input (noise: merge lags of 39 000 to 43 000 frames): 1.11, 1.13 and 1.14 for one lattice,
 * 1.15, 1.16 and 1.17 for 1024.  The worst case, where the walk runs all T frames (flat log-probs, a band as wide as the label
 * axis, a free start row: determined = -1): 1.16, 1.16 and 1.17 for one lattice, 1.19, 1.19 and 1.20 for 1024.  StreamingAligner
 * (Python) in 8 chunks costs 1.04 (peaked) to 1.09 (hash) times ctc_best_path_tracking_chunked and commits its first frames
 * after the first chunk.
 */
int ka_ctc_best_path_determined_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                    int32_t beam_size, int32_t max_move, const int32_t *band_lo, const float *init_scores, int32_t end,
                                    int32_t *best_path, int32_t *best_labels, float *best_scores, float *final_scores, int32_t *entry,
                                    int32_t *determined, float *total_score, int32_t mem, void *stream);
int ka_ctc_best_path_determined_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                          const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                          const int32_t *const *band_lo, const float *const *init_scores, const int32_t *end,
                                          int32_t *const *best_path, int32_t *const *best_labels, float *const *best_scores,
                                          float *const *final_scores, int32_t *entry, int32_t *determined, float *total_score, int32_t *status,
                                          int32_t mem, void *stream);
int ka_ctc_best_path_tracking_determined_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels,
                                             int64_t S, int32_t beam_size, int32_t max_move, int32_t period, int32_t first_lo,
                                             const float *init_scores, int32_t end, int32_t *best_path, int32_t *best_labels,
                                             float *best_scores, int32_t *band_lo_out, float *final_scores, int32_t *entry, int32_t *next_lo,
                                             int32_t *determined, float *total_score, int32_t mem, void *stream);
int ka_ctc_best_path_tracking_determined_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                                   const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                                   int32_t max_move, int32_t period, const int32_t *first_lo, const float *const *init_scores,
                                                   const int32_t *end, int32_t *const *best_path, int32_t *const *best_labels,
                                                   float *const *best_scores, int32_t *const *band_lo_out, float *const *final_scores,
                                                   int32_t *entry, int32_t *next_lo, int32_t *determined, float *total_score, int32_t *status,
                                                   int32_t mem, void *stream);
/* device-workspace bytes such a call carves (0 for unsupported arguments): the parent's figure (tracking 0:
 * ka_resume_workspace_bytes, else ka_tracking_resume_workspace_bytes) plus the determined cell of every lattice (4 bytes,
 * rounded up for the batch) and, for KA_MEM_DEVICE, a last row of the engine's own per lattice (the walk starts from the last
 * row, whether or not the caller asks for it; with KA_MEM_HOST the staged row serves).  After ka_engine_reserve of it the call
 * allocates nothing. */
size_t ka_determined_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                     int32_t mem, int32_t tracking);

/*
 * Best-path margins from max-marginals: how much score the best alignment would lose if, at frame t, it had to be somewhere
 * else.  The best path's own recurrence in max-plus arithmetic, run forwards (D) and backwards (E): adds and compares only, no
 * transcendental, float64 throughout, so every output is defined bit for bit by IEEE add and max.
 *
 * The lattice is that of ka_ctc_best_path_banded: lab' the blank-expanded labels, L = 2S+1; lo_t = band_lo[t], or the
 * reference's diagonal max(0, L t / T - beam_size / 2) when the table argument is NULL; hi_t = min(lo_t + beam_size, L); moves
 * j in [0, max_move); the veto: j even, j >= 2, target label == 0 is not a move; before frame 0 the virtual state is {0: 0.0};
 * the terminal is s* = path[T-1], as ka_ctc_path_posteriors takes it.  All values are float64, each log-prob is widened
 * exactly, each + is one IEEE double add, absent and vetoed candidates are -inf.
 *
 *   D_t(p) = max over j of ( D_{t-1}(p-j) + lp[t, lab'[p]] )         p in [lo_t, hi_t), p-j in band t-1, veto on lab'[p]
 *   E_{T-1} = {s*: 0.0};
 *   E_t(p) = max over j of ( E_{t+1}(p+j) + lp[t+1, lab'[p+j]] )     p+j in band t+1, veto on lab'[p+j]
 *   m_t(p) = D_t(p) + E_t(p)
 *   score      = D_{T-1}(s*)                                          (host double, per lattice)
 *   through[t] = m_t(path[t]) if path[t] in [lo_t, hi_t) else -inf
 *   alt[t]     = max of m_t(p) over p in [lo_t, hi_t) with (p >> unit) != (path[t] >> unit);  -inf if there is none
 *   runner_up[t] = the LOWEST p attaining alt[t];  -1 where alt[t] is -inf
 *
 * unit is 0 (another state) or 1 (another text index p / 2, which is what align() reads off the path at a segment's ends).
 * The path is input only: any values in [0, L) are legal, it need not be connected and need not be a best path; then
 * through[t] - alt[t] is signed and says how much better the best path through the caller's state is than the best path that
 * avoids it.  (Rounding is monotone: max_j(D_{t-1}(p-j)) + lp has the bits of the maximum of the sums.)
 *
 * log_probs, labels, band_lo, path, through, alt and runner_up lie where `mem` says; band_lo [T] int32 may be NULL (the batch
 * call: the array may be NULL, every lattice on the diagonal, or hold NULL entries), runner_up may be NULL (likewise), score
 * (a host double per lattice) and status (host) may be NULL.  Statuses are the family's, per lattice: KA_ERR_BAD_LABEL;
 * KA_ERR_NAN / KA_ERR_NONFINITE for a NaN / +inf among the log-probs (-inf is legal); KA_ERR_BAD_ARGS for a path value outside
 * [0, L) or an invalid table (checked on the device before use), for that lattice alone; KA_ERR_ZERO_MASS where score is -inf.
 * A failed lattice gets NaN over [0, T) of through and alt, -1 over runner_up and a NaN score (-inf for KA_ERR_ZERO_MASS).
 * unit outside {0, 1} is KA_ERR_BAD_ARGS before anything is launched or written.  The batch call returns the first failed
 * lattice's status.  The call synchronises `stream`; the engine's mode and backtrace settings do not apply.
 * Forms: one wavefront per lattice (band <= 1009, V <= 64, max_move <= 4), else a 256-thread workgroup (max_move <= 255).
 * Cost (MI355X, cfg2: T = 50 000, S = 5000, beam 1000, V = 64): one lattice 564 ms, 0.32 x the
 * label-posterior call and 17.0 x ka_ctc_best_path_banded_batch_f32; 1024 lattices in one call 623 ms, 0.29 x and 17.1 x.
 * ka_path_margin_workspace_bytes: the engine workspace a call of these shapes needs (0 for unsupported shapes); after
 * ka_engine_reserve of that figure the call allocates nothing.
 */
int ka_ctc_path_margins_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                            int32_t beam_size, int32_t max_move, const int32_t *band_lo, const int32_t *path, int32_t unit, double *through,
                            double *alt, int32_t *runner_up, double *score, int32_t mem, void *stream);
int ka_ctc_path_margins_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                  const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                  const int32_t *const *band_lo, const int32_t *const *path, int32_t unit, double *const *through,
                                  double *const *alt, int32_t *const *runner_up, double *score, int32_t *status, int32_t mem, void *stream);
size_t ka_path_margin_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size, int32_t max_move,
                                      int32_t mem);

/*
 * Best-path margins under the caller's boundary conditions, and rows of max-marginals at chosen frames:
 * ka_ctc_path_margins over ONE CHUNK of a recording.  Lattice, band, moves and veto are ka_ctc_path_margins' (lab' the
 * blank-expanded labels, L = 2S+1, M = max_move, band [lo_t, hi_t) from band_lo or, for a NULL table, the diagonal); what
 * stands before frame 0 and at frame T-1 is the caller's, and the two rows a neighbouring chunk needs are handed back.  Every
 * value is a float64, every + one IEEE add, every max exact: all outputs are defined bit for bit.
 *   d_in      [L] float64 or NULL: D of the row before frame 0, -inf = no path.  NULL: the virtual state {0: 0.0}.  No band
 *             applies to it: D_0(p) = max_j d_in[p-j] + lp[0, lab'[p]] for p in band 0, p-j >= 0, veto on lab'[p]; only
 *             [lo_0 - (M-1), hi_0) can matter
 *   e_in      [L] float64 or NULL: E_{T-1}(p) = e_in[p] over band T-1 (zeros: the path may end anywhere); `terminal` is then
 *             ignored.  NULL: E_{T-1} = {terminal: 0.0}, terminal = -1 meaning path[T-1] (path is then required)
 *   score     max over band T-1 of D_{T-1}(p) + E_{T-1}(p); with a NULL e_in that is D_{T-1}(terminal), the sibling's value.
 *             -inf: KA_ERR_ZERO_MASS
 *   d_out     [L] float64 or NULL: D_{T-1}(p) over band T-1, -inf elsewhere: the next chunk's d_in
 *   e_out     [L] float64 or NULL: the E of the row before frame 0, e_out[p] = max_j (E_0(p+j) + lp[0, lab'[p+j]]), p+j in band 0,
 *             veto on lab'[p+j], for p in [max(lo_0 - (M-1), 0), hi_0), -inf elsewhere: the previous chunk's e_in
 *   through, alt, runner_up   the sibling's definitions with m_t(p) = D_t(p) + E_t(p); each may be NULL (NULL arrays, or NULL
 *             entries); path is required if any is asked for
 *   frames    [K] HOST int64 in both memory modes, strictly increasing in [0, T); K = 0 is legal (K NULL in the batch form: all 0)
 *   rows      [K, ld_rows] float64: rows[k][j] = m_{f_k}(lo_k + j) for j < hi_k - lo_k, -inf for j in [hi_k - lo_k, W),
 *             W = min(beam_size, L); absolute values: subtract score for "how far behind the best path".  ld_rows >= W
 *   rows_lo   [K] int64: lo_k
 * The batch form takes HOST arrays of n pointers; any of band_lo, d_in, e_in, path, through, alt, runner_up, frames, rows,
 * rows_lo, d_out, e_out may be NULL or hold NULL entries, and terminal, K, ld_rows may be NULL where nothing needs them.
 * What runs: the forward pass always; checkpoints and the recompute of D for every 32-frame block if through, alt or
 * runner_up is asked for, else only for blocks that hold a query frame; the backward pass only if one of through, alt,
 * runner_up, rows or e_out is asked for.  d_out and score alone are one forward pass.
 * Properties (each holds bit for bit, and is tested so):
 *   1. With d_in, e_in, frames, d_out and e_out absent and terminal = -1 every output, status and return code is
 *      ka_ctc_path_margins[_batch]_f32's, over a table and over the diagonal.
 *   2. Cut a lattice at any k in [1, T): A = frames [0, k) with band_lo[:k], B = frames [k, T) with band_lo[k:], d_in = A's
 *      d_out and the uncut terminal; then A with e_in = B's e_out.  The concatenated through, alt and runner_up are the uncut
 *      call's, B's score has the uncut score's bits, and state rows at any frame equal the uncut call's rows.
 *   3. rows[k] reproduces frame f_k's through (at path[f_k] - lo_k), alt (its maximum outside the path's group) and runner_up
 *      (the lowest position attaining it).
 *   4. A lattice gives the same bits alone or in a batch, whatever its neighbours bring.
 *   5. d_out is the same whether or not anything else is asked for.
 * Failures: a NaN or +inf anywhere in d_in or e_in, a terminal or path value outside [0, L), or a table that is no band is
 * KA_ERR_BAD_ARGS for that lattice alone (status), as are the sibling's statuses for labels and log-probs.  A failed lattice has
 * NaN over every requested float output, rows and d_out / e_out included, -1 over runner_up and rows_lo, and a NaN score (-inf
 * for KA_ERR_ZERO_MASS): a chunk resumed from a failed chunk fails too.  Refused on the host before any launch, with every
 * output untouched (KA_ERR_BAD_ARGS): a unit other than 0 or 1, frames out of order or range, K outside [0, T], ld_rows < W,
 * an output asked for without what it needs (path; rows with rows_lo), no end at all, and an output row (d_out, e_out) that
 * overlaps an input row (d_in, e_in).
 * Cost (MI355X, cfg2: T = 50 000, S = 5000, beam 1000, V = 64, minimum of nine; ms for one lattice / for
 * 1024 in one call): ka_ctc_path_margins_batch_f32 562.9 / 616.1, its machine code and its time unchanged from the commit before
 * this call (562.9 / 616.2 there, run alternately); this call with NULL rows 581.9 / 635.3 (1.034 x / 1.031 x), with both rows
 * in and out 582.0 / 635.0; d_out and score alone 147.5 / 150.7 (0.26 x / 0.24 x: one forward pass); state rows at 100 frames
 * without through / alt 317.3 / 335.2 (0.56 x / 0.54 x); the Python ctc_path_margins_chunked in 8 chunks 1.26 x the uncut call.
 * ka_margins_resume_workspace_bytes: the engine workspace a call of these shapes and K needs (K may be NULL; 0 for unsupported
 * shapes): the sibling's slots, these descriptors, the frame lists and, for KA_MEM_HOST, the staged rows.
 */
int ka_ctc_margins_resume_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                              int32_t beam_size, int32_t max_move, const int32_t *band_lo, const double *d_in, const double *e_in,
                              int64_t terminal, const int32_t *path, int32_t unit, double *through, double *alt, int32_t *runner_up,
                              const int64_t *frames, int64_t K, double *rows, int64_t ld_rows, int64_t *rows_lo, double *d_out, double *e_out,
                              double *score, int32_t mem, void *stream);
int ka_ctc_margins_resume_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                    const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                    const int32_t *const *band_lo, const double *const *d_in, const double *const *e_in, const int64_t *terminal,
                                    const int32_t *const *path, int32_t unit, double *const *through, double *const *alt,
                                    int32_t *const *runner_up, const int64_t *const *frames, const int64_t *K, double *const *rows,
                                    const int64_t *ld_rows, int64_t *const *rows_lo, double *const *d_out, double *const *e_out, double *score,
                                    int32_t *status, int32_t mem, void *stream);
size_t ka_margins_resume_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, const int64_t *K, int32_t V, int32_t beam_size,
                                         int32_t max_move, int32_t mem);

/*
 * Forward-backward posteriors over a caller-given band: ka_ctc_path_posteriors, ka_ctc_label_posteriors,
 * ka_ctc_state_posteriors and ka_ctc_state_durations on the band of ka_ctc_best_path_banded instead of the reference's
 * diagonal, so that a path found under a table can be judged under the same table.  Each call is its sibling with one
 * argument added behind max_move, the table:
 *   single call   const int32_t *band_lo          [T] int32, where `mem` says
 *   batch call    const int32_t *const *band_lo   a HOST array of n such pointers
 * (the state-posterior calls name it band_table: their band_lo is the output they always had, which now holds the table's
 * value at every query frame).  lo_t = band_lo[t], hi_t = min(lo_t + beam_size, 2S+1); a valid table holds
 * 0 <= band_lo[t] < 2S+1 and band_lo[t] <= band_lo[t+1], with steps of any size.  Everything else - the recurrences, the veto,
 * the statuses, the outputs of a failed lattice, the stream synchronisation, the Z bits the calls share - is as the sibling
 * documents.  The table is checked on the device before any of its values is used: an invalid one gives its lattice
 * KA_ERR_BAD_ARGS and the sibling's failure outputs (NaN outputs, band_lo -1, log-likelihood NaN) while the other lattices of
 * the batch are answered; a step that leaves a frame without a live predecessor ends in KA_ERR_ZERO_MASS.  A position that no
 * frame's band holds has duration and time_sum 0.  A NULL array or entry fails the call with KA_ERR_BAD_ARGS before anything is
 * launched.  With the reference's diagonal as the table every call returns its sibling's bits.
 */
int ka_ctc_path_posteriors_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels,
                                      int64_t S, int32_t beam_size, int32_t max_move, const int32_t *band_lo, const int32_t *best_path,
                                      float *posteriors, double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_path_posteriors_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                            const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                            int32_t max_move, const int32_t *const *band_lo, const int32_t *const *best_path,
                                            float *const *posteriors, double *log_likelihood, int32_t *status, int32_t mem,
                                            void *stream);
int ka_ctc_label_posteriors_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels,
                                       int64_t S, int32_t beam_size, int32_t max_move, const int32_t *band_lo, int64_t terminal,
                                       float *occupancy, int64_t ld_out, double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_label_posteriors_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                             const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                             int32_t max_move, const int32_t *const *band_lo, const int64_t *terminal,
                                             float *const *occupancy, const int64_t *ld_out, double *log_likelihood, int32_t *status,
                                             int32_t mem, void *stream);
int ka_ctc_state_posteriors_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels,
                                       int64_t S, int32_t beam_size, int32_t max_move, const int32_t *band_table, int64_t terminal,
                                       const int64_t *frames, int64_t K, float *gamma, int64_t ld_out, int64_t *band_lo,
                                       double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_state_posteriors_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                             const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                             int32_t max_move, const int32_t *const *band_table, const int64_t *terminal,
                                             const int64_t *const *frames, const int64_t *K, float *const *gamma,
                                             const int64_t *ld_out, int64_t *const *band_lo, double *log_likelihood, int32_t *status,
                                             int32_t mem, void *stream);
int ka_ctc_state_durations_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels,
                                      int64_t S, int32_t beam_size, int32_t max_move, const int32_t *band_lo, int64_t terminal,
                                      double *duration, double *time_sum, double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_state_durations_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                            const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                            int32_t max_move, const int32_t *const *band_lo, const int64_t *terminal,
                                            double *const *duration, double *const *time_sum, double *log_likelihood, int32_t *status,
                                            int32_t mem, void *stream);
/* device-workspace bytes a banded call carves BEYOND its sibling's ka_*_workspace_bytes figure (the descriptors that carry the
 * table and, for KA_MEM_HOST, the staged tables): reserving the sum keeps the call free of allocations.  0 for unsupported
 * arguments.  For the four calls above and, of the block below, the visits, the samples and the MEA path; the banded boundary
 * quantiles have a figure of their own (ka_boundary_quantile_band_table_workspace_bytes). */
size_t ka_band_table_workspace_bytes(int32_t n, const int64_t *T, int32_t mem);

/*
 * Forward-backward posteriors under the caller's boundary conditions: the posterior side of
 * ka_ctc_best_path_resume.  The checkpointed forward-backward of ka_ctc_label_posteriors_banded over a table band_lo (required;
 * there is no diagonal form) with the row before frame 0 and the row at frame T-1 given by the caller, and the two rows a
 * neighbouring chunk needs handed back.  Recurrence, veto, forms, memory modes, statuses, return convention and stream
 * synchronisation are that call's.  L = 2S+1.  Every row is [L] float64 in nats, absolute; -inf is no mass.
 *   alpha_in   NULL: the virtual state {0: 0.0}.  Else ln alpha of the row before frame 0.  No band applies to it: frame 0
 *              reads alpha_in[p-j] for p in [lo_0, hi_0), so only [lo_0 - (max_move-1), hi_0) matters; the veto applies to frame
 *              0's moves as to any frame's.
 *   beta_in    NULL: beta_{T-1} = {terminal: 0}.  Else beta_{T-1}(p) = beta_in[p] over band T-1 (cells outside it are checked
 *              for NaN and +inf and otherwise unused) and `terminal` is ignored.  A row of zeros lets the path end anywhere: Z is the mass of the audio so far.
 *   path       [T] int32 or NULL; required by path_post.
 *   occupancy  [T, ld_out] or NULL: the sibling's output.
 *   path_post  [T] float32 or NULL: gamma at (t, path[t]) as the state posteriors form it; 0 where path[t] is outside band t.
 *   alpha_out  [L] or NULL: ln alpha_{T-1}(p) over band T-1, -inf elsewhere.
 *   beta_out   [L] or NULL: the beta of the row before frame 0: logsumexp_j(beta_0(p+j) + lp[0, lab'[p+j]]) over the moves into
 *              band 0 (a skip into a cell whose label value is 0 is vetoed), for p in [max(lo_0 - (max_move-1), 0), hi_0); -inf
 *              elsewhere.
 *   log_likelihood   Z = logsumexp over band T-1 of alpha_{T-1}(p) + beta_{T-1}(p); with a NULL beta_in the sibling's Z.
 * In the batch call alpha_in, beta_in, path, occupancy, path_post, alpha_out and beta_out are HOST arrays of n pointers; an array
 * or any entry may be NULL (ld_out is required with occupancy; terminal may be NULL if every lattice brings a beta_in).
 * alpha_out and beta_out may not overlap alpha_in or beta_in (the kernel reads the input rows again after it has written
 * alpha_out): such a call fails with KA_ERR_BAD_ARGS before anything is launched.  To move a row on, write it beside the old one.
 * A NaN or +inf anywhere in either row (all 2S+1 cells, read or not) is KA_ERR_BAD_ARGS for that lattice alone.  Any status but KA_OK fills every requested output of
 * the lattice with NaN, rows included, so a chunk resumed from a failed chunk fails too; KA_ERR_ZERO_MASS is Z = -inf.
 * The forward pass always runs; checkpoints and the block recompute only for occupancy or path_post; the backward pass only
 * for occupancy, path_post or beta_out: alpha_out and Z alone cost one forward pass.
 * What follows:
 *   1. alpha_in NULL, beta_in NULL, no rows out: occupancy, log_likelihood, status and return code are
 *      ka_ctc_label_posteriors_banded[_batch]_f32's bit for bit.
 *   2. alpha_out has the same bits whether or not the backward pass ran, beta_out whether or not gamma was asked for.
 *   3. A lattice gives the same bits alone or inside a batch, whatever its neighbours' rows.
 *   4. Cut at any k in [1, T): chunk A = frames [0, k), chunk B = frames [k, T), B's alpha_in = A's alpha_out, A's beta_in = B's
 *      beta_out.  The occupancies and path posteriors, concatenated, are the uncut lattice's; A's Z, B's Z and the uncut Z
 *      agree; logsumexp(alpha_in + beta_out) over a chunk's start row is its Z.
 * Cost as measured (cfg2: T = 50000, V = 64, S = 5000, beam 1000, one MI355X, against ka_ctc_label_posteriors_banded_batch_f32
 * of the same build, minimum of nine; tools/bench_fb_resume.py): NULL rows 1.018 x (one lattice) and 1.017 x (1024 lattices) the
 * sibling, whose run-to-run spread is 1.003; both rows in and out 1.028 x and 1.017 x; alpha_out and Z alone 0.300 x and 0.273 x.
 * A recording in 8 chunks (a forward-only sweep, then the chunks newest first) 1.29 x the uncut call.
 * ka_posteriors_resume_workspace_bytes: the device-workspace bytes of a call (the sibling's figure plus the descriptors, the
 * staged tables and, for KA_MEM_HOST, the staged path, path posteriors and four rows); 0 for unsupported arguments.
 */
int ka_ctc_posteriors_resume_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                 int32_t beam_size, int32_t max_move, const int32_t *band_lo, const double *alpha_in,
                                 const double *beta_in, int64_t terminal, const int32_t *path, float *occupancy, int64_t ld_out,
                                 float *path_post, double *alpha_out, double *beta_out, double *log_likelihood, int32_t mem,
                                 void *stream);
int ka_ctc_posteriors_resume_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                       const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                       int32_t max_move, const int32_t *const *band_lo, const double *const *alpha_in,
                                       const double *const *beta_in, const int64_t *terminal, const int32_t *const *path,
                                       float *const *occupancy, const int64_t *ld_out, float *const *path_post,
                                       double *const *alpha_out, double *const *beta_out, double *log_likelihood, int32_t *status,
                                       int32_t mem, void *stream);
size_t ka_posteriors_resume_workspace_bytes(int32_t n, const int64_t *T, const int64_t *S, int32_t V, int32_t beam_size,
                                            int32_t max_move, int32_t mem);

/*
 * State visits, boundary quantiles, sampled paths and the MEA path over a caller-given band: the
 * other half of the forward-backward family on the table of the block above, by the same rule.  Each call is its sibling with
 * the table behind max_move (single call: const int32_t *band_lo, [T] int32 where `mem` says; batch call: a HOST array of n
 * such pointers); lo_t, hi_t, what a valid table is, the device-side check, the NULL rules and everything the sibling
 * documents - recurrences, veto, terminal, statuses, stream synchronisation, the Z bits the family shares - are as above.
 * A lattice that fails (an invalid table: KA_ERR_BAD_ARGS for that lattice alone) gets its sibling's failure outputs: NaN over
 * [0, 2S+1) of visit and exit_time; -1 over [K, M] of quantile; -1 over [0, T) of every sampled row; a -1 path and a NaN
 * expected accuracy.  What the table changes in the outputs:
 *   visits      a position that no frame's band holds, and every position below band_lo[0], has visit and exit_time 0
 *   quantiles   F_t(c) is 2^32 from the first t with band_lo[t] >= c on, so a cut at or below band_lo[0] (not only cut 0)
 *               reads 0 at every level, and a cut that the band's low end never reaches reads its own crossing, or T.  The
 *               start frames are found on the device from the accepted table; nothing of the table is read on the host
 *   samples     every draw into frame t-1 is over the band of frame t-1, band_lo[t-1]; sample k keeps its bits whatever the
 *               batch and n_samples, as in the sibling
 *   MEA path    path[0] is the smallest allowed j < max_move inside [band_lo[0], hi_0), so it may lie above 0; a table with
 *               band_lo[0] >= max_move is KA_ERR_ZERO_MASS
 * With the reference's diagonal as the table every call returns its sibling's bits: outputs, log-likelihood, status, return code.
 * Workspace beyond the sibling's ka_*_workspace_bytes figure: ka_band_table_workspace_bytes for the visits, the samples and
 * the MEA path; ka_boundary_quantile_band_table_workspace_bytes for the quantiles, whose descriptor is larger.
 */
int ka_ctc_state_visits_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                   int32_t beam_size, int32_t max_move, const int32_t *band_lo, int64_t terminal, double *visit,
                                   double *exit_time, double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_state_visits_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                         const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                         int32_t max_move, const int32_t *const *band_lo, const int64_t *terminal, double *const *visit,
                                         double *const *exit_time, double *log_likelihood, int32_t *status, int32_t mem, void *stream);
int ka_ctc_boundary_quantiles_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels,
                                         int64_t S, int32_t beam_size, int32_t max_move, const int32_t *band_lo, int64_t terminal,
                                         const int64_t *cuts, int64_t K, const double *levels, int32_t M, int32_t *quantile, int64_t ld_q,
                                         double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_boundary_quantiles_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                               const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                               int32_t max_move, const int32_t *const *band_lo, const int64_t *terminal,
                                               const int64_t *const *cuts, const int64_t *K, const double *levels, int32_t M,
                                               int32_t *const *quantile, const int64_t *ld_q, double *log_likelihood, int32_t *status,
                                               int32_t mem, void *stream);
int ka_ctc_sample_paths_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                                   int32_t beam_size, int32_t max_move, const int32_t *band_lo, int64_t terminal, int32_t n_samples,
                                   uint64_t seed, int32_t *paths, int64_t ld_paths, double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_sample_paths_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V,
                                         const int64_t *ld, const int32_t *const *labels, const int64_t *S, int32_t beam_size,
                                         int32_t max_move, const int32_t *const *band_lo, const int64_t *terminal,
                                         const int32_t *n_samples, const uint64_t *seed, int32_t *const *paths, const int64_t *ld_paths,
                                         double *log_likelihood, int32_t *status, int32_t mem, void *stream);
int ka_ctc_mea_path_banded_f32(ka_engine *e, const float *log_probs, int64_t T, int32_t V, int64_t ld, const int32_t *labels, int64_t S,
                               int32_t beam_size, int32_t max_move, const int32_t *band_lo, int64_t terminal, int32_t *path,
                               double *expected_accuracy, double *log_likelihood, int32_t mem, void *stream);
int ka_ctc_mea_path_banded_batch_f32(ka_engine *e, int32_t n, const float *const *log_probs, const int64_t *T, int32_t V, const int64_t *ld,
                                     const int32_t *const *labels, const int64_t *S, int32_t beam_size, int32_t max_move,
                                     const int32_t *const *band_lo, const int64_t *terminal, int32_t *const *path,
                                     double *expected_accuracy, double *log_likelihood, int32_t *status, int32_t mem, void *stream);
/* ka_band_table_workspace_bytes for ka_ctc_boundary_quantiles_banded_*: the bytes that call carves beyond
 * ka_boundary_quantile_workspace_bytes (its descriptors carry the cuts' arrays as well as the table).  0 for unsupported arguments. */
size_t ka_boundary_quantile_band_table_workspace_bytes(int32_t n, const int64_t *T, int32_t mem);

/* Kernel form of the fast path.
 *   KA_MODE_WAVE        one wavefront per lattice, checkpointed (throughput; fills the chip from ~4096
 *                       lattices): the forward kernel keeps scores only and stores the score ring every 32
 *                       frames; the backtrace kernel recomputes the back-pointers of the ~100 cells around the
 *                       path from those checkpoints and writes all three outputs.  Lattices whose log-probs are
 *                       not all finite are redone by the exact kernels in the same call; a call with a lattice of
 *                       2^26 frames or more runs entirely in the exact form.
 *   KA_MODE_WAVE_EXACT  one wavefront per lattice, every back-pointer stored (2 bits per band cell).
 *   KA_MODE_TILED       a workgroup of two or three wavefronts per 256- or 128-position TILE of the label axis, the tiles of a lattice run as a pipeline
 *                       (scores only, checkpoints as WAVE): a lone lattice or a book's few dozen chapters, and ANY band
 *                       width (beam_size >= 2L is the reference's unbanded DP).  Non-finite log-probs: bands up to 1009 are
 *                       redone by the exact kernels, wider ones return KA_ERR_NONFINITE in this explicit mode.
 *   KA_MODE_AUTO        (default) per launch: lattices whose band is wider than 1009 positions always run TILED (and are
 *                       handed to the generic kernels by ka_batch_finish if their log-probs turn out to hold infinities);
 *                       the others run TILED while the launch is too small to fill the chip with one wavefront per lattice
 *                       (the rule is in ka_engine.hip, next to its measurements), else WAVE.
 * Results are identical in every form. */
#define KA_MODE_AUTO 0
#define KA_MODE_WAVE 1
/* (2 was KA_MODE_WORKGROUP, four wavefronts per lattice: superseded by the tiled form in round 2, removed in round 4) */
#define KA_MODE_WAVE_EXACT 3
#define KA_MODE_TILED 4
int ka_engine_set_mode(ka_engine *e, int32_t mode);

/* How the checkpointed forms (KA_MODE_WAVE, KA_MODE_TILED) walk the best path back.
 *   KA_BACKTRACE_SERIAL    one wavefront per lattice, chunk after chunk of 32 frames (the position a chunk is entered
 *                          at comes out of the chunk above it): least work, right for thousands of lattices.
 *   KA_BACKTRACE_PARALLEL  every chunk of every lattice at once: per chunk a map "position at its last frame -> rise
 *                          over the chunk" is recomputed for the whole band, 32 maps are composed into a super-chunk map,
 *                          the end position is run down the super-chunk maps and then, in parallel, down the chunk maps,
 *                          which gives every chunk its entry position.  ~8x the work, ~60x shorter for a lone lattice.
 *   KA_BACKTRACE_AUTO      (default) PARALLEL up to a few hundred lattices per call, else SERIAL.
 * Results are identical. */
#define KA_BACKTRACE_AUTO 0
#define KA_BACKTRACE_SERIAL 1
#define KA_BACKTRACE_PARALLEL 2
int ka_engine_set_backtrace(ka_engine *e, int32_t how);

/* Per-kernel timing of the LAST enqueued batch, measured with HIP events recorded on the
 * launch stream: ms[0] label prep, ms[1] forward DP, ms[2] backtrace walk, ms[3] output
 * gathers (best_labels / best_scores).  Enable before the call; costs one event per kernel. */
/* Calibration of KA_MODE_AUTO / KA_BACKTRACE_AUTO (tools/sweep_auto.py): with the lattices of a launch sorted longest
 * first, run the longest n_tiled in the tiled form and walk the longest n_parallel back chunk-parallel instead of asking
 * the cost model (ka_engine.hip); -1 = the cost model.  Results are identical whatever the split. */
int ka_debug_set_split(ka_engine *e, int32_t n_tiled, int32_t n_parallel);
/* Host-side probe of that cost model (no GPU needed): for a launch of n lattices of T[i] frames whose band keeps
 * `tiles_alive` tiles running at once (5 for the reference's beam of 1000) on a device of n_simd SIMDs, how many of the
 * longest it runs tiled and how many it walks back chunk-parallel. */
int ka_debug_auto_split(const int64_t *T, int32_t n, int32_t tiles_alive, int32_t n_simd, int32_t *n_tiled, int32_t *n_parallel);
/* LDS bytes a tile workgroup of the tiled form requests (0 = the library's choice; 40 KB lets four workgroups share a CU, 80 KB
 * two; a request below what the kernel uses - 27-52 KB by tile width, V and row layout - is raised to that): an occupancy
 * experiment knob, results are identical. */
int ka_debug_set_tile_lds(ka_engine *e, int32_t bytes);
/* Positions per tile of the tiled form: 256 (four cells per lane, two wavefronts per tile: ka_tiled256.hpp), 128 (two cells per lane,
 * three wavefronts per tile, self-vouching halo packets: ka_tiled128.hpp - a shorter frame, twice the tiles), or 0 = the
 * library's choice (128 while the tiles alive at once are no more than 3.2 per workgroup slot of the device).  Results are identical. */
int ka_debug_set_tile_width(ka_engine *e, int32_t positions);
/* Host-side probe of the library's choice (no GPU needed): the tile width - 128 or 256 - a launch of these n lattices, ALL run in
 * the tiled form, gets on a device of n_simd SIMDs; 0 if one of them is not run in the tiled form at all, a negative status for
 * bad arguments. */
int ka_debug_tile_width_choice(const int64_t *T, const int64_t *S, int32_t n, int32_t V, int32_t beam_size, int32_t max_move, int32_t n_simd);
/* Self-checks of the tiled form's hand-off, a combination of:
 *   1  the halo region is filled with a NaN sentinel before the launch and every packet a tile consumes is checked
 *      against it: a packet read before it was written gives the lattice KA_ERR_INTERNAL (tests)
 *   2  every publish waits for all of the tile's outstanding memory operations (rules out the counted waits)
 *   4  per-tile phase stamps for ka_debug_tile_stats
 * 0 (default) = none.  Applies to the engine's later launches. */
int ka_engine_set_verify(ka_engine *e, int32_t flags);
/* Diagnostics of the tiled form (after ka_engine_set_verify(e, 4)): per tile of the last batch, 8 values
 * {descriptor, tile, t_in, t_end, ticks spent waiting for the tile below, ticks alive, waits, start tick}, 100 MHz
 * ticks, in ticket order.  Returns the number of tiles written (at most max_tasks). */
int ka_debug_tile_stats(ka_engine *e, uint64_t *out, int32_t max_tasks);
/* Diagnostics of the chunk-parallel backtrace: for the first lattice of the last batch, the best-path position at the
 * last frame of every chunk followed by that of every super-chunk (returns how many values), and optionally its
 * chunk maps (one row of ring-size bytes per chunk). */
int ka_debug_chunk_entries(ka_engine *e, int32_t *out, int32_t max_entries, uint8_t *map0_out, int64_t map0_max);
/* Diagnostics of the forward pass: for the first lattice of the last finished batch, the score rows its checkpointed
 * forward kernel stored, row k after frame 32 (k + 1) - 1, (T - 1) / 32 rows of *pitch bytes; position p lies at float
 * p & (*pitch / 4 - 1) of its row when the label axis is longer than a row (always in the one-wavefront form: 1024
 * slots), else at float p.  Only the band of that frame is defined.  Copies at most max_floats values and returns the
 * number of rows: 0 (and *pitch = 0) where no checkpoints were stored - the exact and generic forms, and a lattice that
 * the checkpointed forms declined (non-finite log-probs). */
int ka_debug_checkpoints(ka_engine *e, float *out, int64_t max_floats, int64_t *pitch);
/* Diagnostics of the kernels' routing: the flag word the kernels left for every lattice of the last finished best-path batch,
 * in the caller's order (at most max_lattices are copied; returns the number of lattices of that batch).  Bit 0: a transcript
 * label is 0; bit 1: the checkpointed form declined the lattice to the exact kernels (non-finite log-probs); bit 2: declined
 * and too wide for them; bit 3: the checkpointed one-wavefront forward pass found the sign bit set in every log-prob (a +0.0
 * clears it), so its serial backtrace took the keyed frames. */
int ka_debug_meta_flags(ka_engine *e, int32_t *out, int32_t max_lattices);
/* Host-side probe of the tiled form's plan (no GPU needed): for a lattice of T frames, S phonemes, V classes the
 * 256-position tiles the band of align.py:64-65 ever touches and the frames [t_in, t_end) each of them is alive in.
 * Returns the number of tiles (t_in / t_end are filled up to max_tiles), 0 if the shape is not run in the tiled form,
 * a negative status for bad arguments.  checkpoint_pitch (may be NULL): bytes per checkpoint row. */
int ka_debug_plan_tiles(int64_t T, int64_t S, int32_t V, int32_t beam_size, int32_t max_move, int32_t *t_in, int32_t *t_end,
                        int32_t max_tiles, int64_t *checkpoint_pitch);
/* The same for tiles of `positions` = 128 or 256 positions (ka_debug_set_tile_width). */
int ka_debug_plan_tiles_width(int64_t T, int64_t S, int32_t V, int32_t beam_size, int32_t max_move, int32_t positions, int32_t *t_in,
                              int32_t *t_end, int32_t max_tiles, int64_t *checkpoint_pitch);
int ka_engine_set_profiling(ka_engine *e, int32_t on);
int ka_engine_last_kernel_ms(ka_engine *e, float ms[4]);

/*
 * Mean-subtracted log-softmax of kokoro_align/align.py:116-117 on device:
 *   x = logits - mean(logits, -1);  log_probs = x - log(sum(exp(x), -1))
 * (float32, not max-subtracted, like the reference).  In-place allowed.
 */
int ka_log_softmax_f32(const float *logits, float *log_probs, int64_t T, int32_t V,
                       int64_t ld_in, int64_t ld_out, void *stream);

/*
 * One time step of one layer of the log-prob producer's bidirectional LSTM (AudioToChar, kokoro_align/train.py:54-65;
 * called from predict, train.py:201-231), both directions at once, for the n sequences that are still running
 * (sequences sorted by length, longest first: the running ones are a prefix).  Fused element-wise part:
 *   gates = gin[rows[dir][s], dir*4H : (dir+1)*4H] + rec[dir][s]          (PyTorch order i, f, g, o)
 *   c[dir][s] = sigmoid(f)*c[dir][s] + sigmoid(i)*tanh(g);   h[dir][s] = sigmoid(o)*tanh(c[dir][s])
 *   out[rows[dir][s], dir*H : (dir+1)*H] = h[dir][s]
 * gin [frames, ldg >= 8H] = x @ W_ih^T + b_ih + b_hh of both directions (one library GEMM per layer),
 * rec [2][n][4H] = h @ W_hh^T (one batched library GEMM per step; *_dir_stride = elements between directions),
 * rows [2][..] int32 = frame row of sequence s at this step (forward: offset+t, backward: offset+len-1-t).
 * All pointers are device pointers.
 */
int ka_lstm_step_f32(const float *gin, int64_t ldg, const float *rec, int64_t rec_dir_stride, float *c, float *h,
                     int64_t state_dir_stride, float *out, int64_t ldo, const int32_t *rows, int64_t rows_dir_stride,
                     int32_t n, int32_t H, void *stream);

/*
 * One whole layer of the same LSTM (hidden size 128), both directions, every time step, in ONE persistent launch:
 * a workgroup owns 16 sequences of one direction, the recurrent product runs on the float32 MFMA with its slice
 * of W_hh register-resident, h in LDS.  Sequences must be sorted by length, longest first; they may lie anywhere
 * in gin / out (frames need not be reordered); gin must hold at least one row.  sigmoid/tanh use the hardware
 * exp2 and reciprocal (about 1 ulp each).
 *   gin [frames, ldg >= 8H] as above; w_hh [2][4H][H] = weight_hh of the forward and the backward direction
 *   (PyTorch layout, gate order i, f, g, o); out [frames, ldo >= 2H] = layer output (forward | backward);
 *   seq_off / seq_len [nseq] int32 = first frame row and length of every sequence.  Device pointers.
 */
int ka_lstm_layer_f32(const float *gin, int64_t ldg, const float *w_hh, float *out, int64_t ldo, const int32_t *seq_off,
                      const int32_t *seq_len, int32_t nseq, int32_t H, void *stream);
/* The FIRST layer with its input projection inside the step (n_in = 40 MFCC coefficients, train.py:54-65 `n_mfcc`): x [frames,
 * ldx >= 40] instead of gin; w_ih [2][4H][40] = weight_ih of the two directions, bias [2][4H] = bias_ih + bias_hh.  The
 * [frames, 8H] projection is never materialised (11 GB for an 8.8-hour book).  Otherwise as ka_lstm_layer_f32. */
int ka_lstm_layer0_f32(const float *x, int64_t ldx, int32_t n_in, const float *w_ih, const float *bias, const float *w_hh, float *out, int64_t ldo,
                       const int32_t *seq_off, const int32_t *seq_len, int32_t nseq, int32_t H, void *stream);

/*
 * Audio front end (kokoro_align/preprocess.py:51-131).  Device pointers throughout.
 *
 * ka_window_energy_f32: out[w] = mean(x[256w : 256w+256]**2), the level get_split_points thresholds
 *   (preprocess.py:53-54), float32 summed in NumPy's order for a contiguous row of 256 so that the split points
 *   are the reference's bit for bit (the remaining steps of get_split_points run on the host on these values).
 * ka_stft_frames_f32: windowed frames of torchaudio's Spectrogram as called by split_audio (preprocess.py:110-127:
 *   center=True, reflect padding, frame f of a segment starts at f*hop - n_fft/2) for all segments of a recording:
 *   frames[frame_off[s] + f][k] = window[k] * y[seg_start[s] + reflect(f*hop - n_fft/2 + k)], f < 1 + seg_len[s]/hop.
 *   Every segment must be longer than n_fft/2 samples (as the reference's transform requires).
 * ka_power_f32: power[r][c] = re^2 + im^2 of a transform stored [n][2*nf] = (real | imaginary) - the output of one
 *   library GEMM of the frames with the [n_fft][2*nf] cosine / sine basis.
 * ka_power_to_db_f32: AmplitudeToDB("power", top_db) per segment, in place: x = 10*log10(max(x, 1e-10)), then
 *   x = max(x, max over the segment - top_db).  frame_off has nseg+1 entries; segmax [nseg] must hold -inf on entry
 *   and returns the segment maxima.
 */
int ka_window_energy_f32(const float *x, int64_t n_windows, int32_t window, float *out, void *stream);
int ka_stft_frames_f32(const float *y, const int64_t *seg_start, const int64_t *seg_len, const int64_t *frame_off, int32_t nseg,
                       int64_t max_frames, int32_t n_fft, int32_t hop, const float *window, float *frames, int64_t ld, void *stream);
int ka_power_f32(const float *reim, int64_t ld_in, float *power, int64_t ld_out, int64_t n, int32_t nf, void *stream);
int ka_power_to_db_f32(float *x, int64_t ld, int32_t cols, const int64_t *frame_off, int32_t nseg, int64_t max_frames, float top_db,
                       float *segmax, void *stream);

/* Bit-reproducible synthetic inputs generated in HBM (same definition as the CPU oracle's
 * hash generator):  lp[t,c] = -8*u24(mix(seed, t*V+c)),
 * labels[k] = 1 + mix(seed^salt, k) % (V-1). */
int ka_hash_logprobs_f32(float *dev_log_probs, int64_t T, int32_t V, int64_t ld, uint64_t seed,
                         void *stream);
int ka_hash_labels_i32(int32_t *dev_labels, int64_t S, int32_t V, uint64_t seed, void *stream);
/* n lattices in one launch: lattice i at base + i*lattice_stride (elements) with seed0 + i */
int ka_hash_logprobs_batch_f32(float *dev_log_probs, int32_t n, int64_t T, int32_t V, int64_t ld,
                               int64_t lattice_stride, uint64_t seed0, void *stream);
int ka_hash_labels_batch_i32(int32_t *dev_labels, int32_t n, int64_t S, int32_t V,
                             int64_t lattice_stride, uint64_t seed0, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KOKORO_ALIGN_AMD_H */
