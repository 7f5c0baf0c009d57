// ka_entry_misc.hip — the C entry points that need no engine: log-softmax, the log-prob producer's LSTM, the audio front end
// and the hash generators.  Host code only: argument checks, then the launch functions of ka_misc.hip (ka_launch.hpp).
#include "ka_engine.hpp"

#include <algorithm>

using ka::host::fail;

extern "C" {

int ka_log_softmax_f32(const float *logits, float *log_probs, int64_t T, int32_t V, int64_t ld_in, int64_t ld_out,
                       void *stream)
{
    if (!logits || !log_probs || T < 0 || V < 1 || ld_in < V || ld_out < V) return fail(KA_ERR_BAD_ARGS, "ka_log_softmax_f32: bad arguments");
    if (T == 0) return KA_OK;
    if ((T + 3) / 4 > 0x7fffffff) return fail(KA_ERR_BAD_ARGS, "ka_log_softmax_f32: T too large");
    ka::launch_log_softmax(logits, log_probs, T, V, ld_in, ld_out, (hipStream_t)stream);
    KA_HIP(hipGetLastError());
    return KA_OK;
}

int ka_lstm_step_f32(const float *gin, int64_t ldg, const float *rec, int64_t rec_dir_stride, float *c, float *h,
                     int64_t state_dir_stride, float *out, int64_t ldo, const int32_t *rows, int64_t rows_dir_stride,
                     int32_t n, int32_t H, void *stream)
{
    if (!gin || !rec || !c || !h || !out || !rows || n < 0 || H < 1 || ldg < 8 * (int64_t)H || ldo < 2 * (int64_t)H)
        return fail(KA_ERR_BAD_ARGS, "ka_lstm_step_f32: bad arguments");
    if (n == 0) return KA_OK;
    ka::launch_lstm_step(gin, ldg, rec, rec_dir_stride, c, h, state_dir_stride, out, ldo, rows, rows_dir_stride, n, H, (hipStream_t)stream);
    KA_HIP(hipGetLastError());
    return KA_OK;
}

int ka_lstm_layer_f32(const float *gin, int64_t ldg, const float *w_hh, float *out, int64_t ldo, const int32_t *seq_off,
                      const int32_t *seq_len, int32_t nseq, int32_t H, void *stream)
{
    if (!gin || !w_hh || !out || !seq_off || !seq_len || nseq < 0 || ldg < 8 * (int64_t)H || ldo < 2 * (int64_t)H)
        return fail(KA_ERR_BAD_ARGS, "ka_lstm_layer_f32: bad arguments");
    if (H != ka::kLstmH) return fail(KA_ERR_BAD_ARGS, "ka_lstm_layer_f32: the persistent kernel is built for hidden size 128");
    if (nseq == 0) return KA_OK;
    ka::launch_lstm_layer(false, gin, ldg, w_hh, out, ldo, seq_off, seq_len, nseq, nullptr, nullptr, (hipStream_t)stream);
    KA_HIP(hipGetLastError());
    return KA_OK;
}

int ka_lstm_layer0_f32(const float *x, int64_t ldx, int32_t n_in, const float *w_ih, const float *bias, const float *w_hh, float *out, int64_t ldo,
                       const int32_t *seq_off, const int32_t *seq_len, int32_t nseq, int32_t H, void *stream)
{
    if (!x || !w_ih || !bias || !w_hh || !out || !seq_off || !seq_len || nseq < 0 || ldx < n_in || ldo < 2 * (int64_t)H)
        return fail(KA_ERR_BAD_ARGS, "ka_lstm_layer0_f32: bad arguments");
    if (H != ka::kLstmH || n_in != ka::kLstmIn)
        return fail(KA_ERR_BAD_ARGS, "ka_lstm_layer0_f32: built for hidden size 128 and 40 input features");
    if (nseq == 0) return KA_OK;
    ka::launch_lstm_layer(true, x, ldx, w_hh, out, ldo, seq_off, seq_len, nseq, w_ih, bias, (hipStream_t)stream);
    KA_HIP(hipGetLastError());
    return KA_OK;
}

int ka_window_energy_f32(const float *x, int64_t n_windows, int32_t window, float *out, void *stream)
{
    if (!x || !out || n_windows < 0) return fail(KA_ERR_BAD_ARGS, "ka_window_energy_f32: bad arguments");
    if (window != 256) return fail(KA_ERR_BAD_ARGS, "ka_window_energy_f32: the summation order is NumPy's for windows of 256 samples only");
    if (n_windows == 0) return KA_OK;
    if ((n_windows + 15) / 16 > 0x7fffffff) return fail(KA_ERR_BAD_ARGS, "ka_window_energy_f32: too many windows");
    ka::launch_window_energy(x, n_windows, out, (hipStream_t)stream);
    KA_HIP(hipGetLastError());
    return KA_OK;
}

int ka_stft_frames_f32(const float *y, const int64_t *seg_start, const int64_t *seg_len, const int64_t *frame_off, int32_t nseg,
                       int64_t max_frames, int32_t n_fft, int32_t hop, const float *window, float *frames, int64_t ld, void *stream)
{
    if (!y || !seg_start || !seg_len || !frame_off || !window || !frames || nseg < 0 || n_fft < 2 || hop < 1 || ld < n_fft || max_frames < 0)
        return fail(KA_ERR_BAD_ARGS, "ka_stft_frames_f32: bad arguments");
    if (nseg == 0 || max_frames == 0) return KA_OK;
    if (nseg > 65535) return fail(KA_ERR_BAD_ARGS, "ka_stft_frames_f32: more than 65535 segments in one call");
    ka::launch_stft_frames(y, seg_start, seg_len, frame_off, (unsigned)std::min<int64_t>(max_frames, 4096), (unsigned)nseg, n_fft, hop, window, frames, ld,
                           (hipStream_t)stream);
    KA_HIP(hipGetLastError());
    return KA_OK;
}

int ka_power_f32(const float *reim, int64_t ld_in, float *power, int64_t ld_out, int64_t n, int32_t nf, void *stream)
{
    if (!reim || !power || n < 0 || nf < 1 || ld_in < 2 * (int64_t)nf || ld_out < nf) return fail(KA_ERR_BAD_ARGS, "ka_power_f32: bad arguments");
    if (n == 0) return KA_OK;
    ka::launch_power(reim, ld_in, power, ld_out, n, nf, (hipStream_t)stream);
    KA_HIP(hipGetLastError());
    return KA_OK;
}

int ka_power_to_db_f32(float *x, int64_t ld, int32_t cols, const int64_t *frame_off, int32_t nseg, int64_t max_frames, float top_db,
                       float *segmax, void *stream)
{
    if (!x || !frame_off || !segmax || nseg < 0 || cols < 1 || ld < cols || max_frames < 0) return fail(KA_ERR_BAD_ARGS, "ka_power_to_db_f32: bad arguments");
    if (nseg == 0 || max_frames == 0) return KA_OK;
    if (nseg > 65535) return fail(KA_ERR_BAD_ARGS, "ka_power_to_db_f32: more than 65535 segments in one call");
    ka::launch_power_to_db(x, ld, cols, frame_off, (unsigned)std::min<int64_t>((max_frames * cols + 255) / 256, 256), (unsigned)nseg, top_db, segmax,
                           (hipStream_t)stream);
    KA_HIP(hipGetLastError());
    return KA_OK;
}

int ka_hash_logprobs_batch_f32(float *dev_log_probs, int32_t n, int64_t T, int32_t V, int64_t ld, int64_t lattice_stride,
                               uint64_t seed0, void *stream)
{
    if (!dev_log_probs || n < 0 || T < 0 || V < 1 || ld < V || (n > 1 && lattice_stride < T * ld))
        return fail(KA_ERR_BAD_ARGS, "ka_hash_logprobs_batch_f32: bad arguments");
    if (T == 0 || n == 0) return KA_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>((T * V + 255) / 256, 512);
    for (int32_t y0 = 0; y0 < n; y0 += 65535)
        ka::launch_hash_logprobs(dev_log_probs + (size_t)y0 * (size_t)lattice_stride, blocks, (unsigned)std::min<int32_t>(65535, n - y0), T, V, ld,
                                 seed0 + (uint64_t)y0, lattice_stride, (hipStream_t)stream);
    KA_HIP(hipGetLastError());
    return KA_OK;
}

int ka_hash_labels_batch_i32(int32_t *dev_labels, int32_t n, int64_t S, int32_t V, int64_t lattice_stride, uint64_t seed0,
                             void *stream)
{
    if (!dev_labels || n < 0 || S < 0 || V < 2 || (n > 1 && lattice_stride < S))
        return fail(KA_ERR_BAD_ARGS, "ka_hash_labels_batch_i32: bad arguments");
    if (S == 0 || n == 0) return KA_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>((S + 255) / 256, 64);
    for (int32_t y0 = 0; y0 < n; y0 += 65535)
        ka::launch_hash_labels(dev_labels + (size_t)y0 * (size_t)lattice_stride, blocks, (unsigned)std::min<int32_t>(65535, n - y0), S, V, seed0 + (uint64_t)y0,
                               lattice_stride, (hipStream_t)stream);
    KA_HIP(hipGetLastError());
    return KA_OK;
}

int ka_hash_logprobs_f32(float *dev_log_probs, int64_t T, int32_t V, int64_t ld, uint64_t seed, void *stream)
{
    return ka_hash_logprobs_batch_f32(dev_log_probs, 1, T, V, ld, T * ld, seed, stream);
}

int ka_hash_labels_i32(int32_t *dev_labels, int64_t S, int32_t V, uint64_t seed, void *stream)
{
    return ka_hash_labels_batch_i32(dev_labels, 1, S, V, S, seed, stream);
}

}  // extern "C"
