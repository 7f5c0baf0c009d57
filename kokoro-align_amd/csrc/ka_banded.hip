// ka_banded.hip — translation unit of the kernels of the best path over a caller-given band (ka_banded.hpp): table and label
// preparation, the one-wavefront forward pass and walk back, the generic pair.  The walks back also serve ka_tracking.hip.
#include "ka_launch.hpp"
#include "ka_banded.hpp"

namespace ka {

// ---------------------------------------------------------------------------------------
// preparation: labels (validate, scale by 4, zero-pad), the band table (validate, shift, pad)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_banded_kernel(const BandLattice *__restrict__ lats, int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    int32_t *m = meta_of(meta, d.idx);
    prep_labels(d, m);
    // the table: in range and non-decreasing
    int bad_tab = 0;
    for (int i = threadIdx.x; i < d.T; i += blockDim.x) {
        const int v = d.band_lo[i];
        if (v < 0 || v >= d.L) bad_tab = 1;
        if (i > 0 && d.band_lo[i - 1] > v) bad_tab = 1;
    }
    if (__syncthreads_or(bad_tab)) {
        if (threadIdx.x == 0) {
            atomicMin(&m[0], kStatusBadArgs);
            atomicOr(&m[2], kBandFlagBadTable);
            m[1] = -1;
        }
        return;
    }
    if (d.tab)
        for (int i = threadIdx.x; i < d.tab_len; i += blockDim.x) d.tab[i] = d.band_lo[i + 1 < d.T ? i + 1 : d.T - 1];
}
// ---------------------------------------------------------------------------------------
// the walk back, one wavefront per lattice: path, labels and scores of 16 frames at a time
//
// A path drops at most 3 positions per frame.  The chunk entered at position p (its last frame) stays within [p - 45, p];
// the chunk below it within [p - 93, p]: its window of 8 blocks from block (p - 96) >> 4 is loaded while the current
// chunk is walked.  Window register r[v]: lane = (f & 7) * 8 + j holds the code dword of frame 8 v + (f & 7), block j.
// ---------------------------------------------------------------------------------------
constexpr int kBandBtChunk = 16;
__device__ __forceinline__ int band_bt_window(int p_entry)
{
    const int lo = p_entry - 6 * kBandBtChunk;
    return (lo > 0 ? lo : 0) >> 4;
}
__device__ __forceinline__ void band_bt_load(uint32_t (&r)[2], gcu32_t bp, int t0, int n, int w0, int lane)
{
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int f = 8 * v + (lane >> 3);
        const int t = t0 + f;
        const size_t at = (size_t)(t >> 2) * 256 + (size_t)((w0 + (lane & 7)) & 63) * 4 + (size_t)(t & 3);
        r[v] = f < n ? bp[at] : 0u;
    }
}
__global__ __launch_bounds__(64) void backtrace_banded_wave_kernel(const BandLattice *__restrict__ lats, const int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    const int lane = threadIdx.x;
    int p = __builtin_amdgcn_readfirstlane(meta[4 * (size_t)d.idx + 1]);
    if (p < 0) return;   // no path: the status says why
    const int T = __builtin_amdgcn_readfirstlane(d.T);
    gcu32_t bp = (gcu32_t)d.bp;
    gci32_t labx = (gci32_t)d.labx;
    gcf32_t lp = (gcf32_t)d.lp;
    const size_t ld = (size_t)d.ld;
    int t0 = ((T - 1) / kBandBtChunk) * kBandBtChunk;
    int n = T - t0;
    int w = band_bt_window(p + 3 * kBandBtChunk);   // the tail chunk is entered at the end position itself
    uint32_t cur[2], nxt[2] = {0u, 0u};
    band_bt_load(cur, bp, t0, n, w, lane);
    for (;;) {
        const int t1 = t0 - kBandBtChunk;
        const int wn = band_bt_window(p);
        if (t1 >= 0) band_bt_load(nxt, bp, t1, kBandBtChunk, wn, lane);
        const uint32_t c0 = blank_to_uniform(cur[0]), c1 = blank_to_uniform(cur[1]);
        int q = p - 16 * w;   // position relative to the window: 0 .. 127
        int pathv = 0;
#pragma unroll
        for (int f = kBandBtChunk - 1; f >= 0; --f) {
            if (f < n) {
                const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)(f >= 8 ? c1 : c0), (f & 7) * 8 + (q >> 4));
                pathv = lane == f ? q : pathv;
                q -= bp_decode(word >> ((q * 2) & 31));
            }
        }
        if (lane < n) {
            const int pos = pathv + 16 * w;
            const int t = t0 + lane;
            const int lab = (pos & 1) ? (labx[pos >> 1] >> 2) : 0;
            ((gi32_t)d.path)[t] = pos;
            ((gi32_t)d.lab_out)[t] = lab;
            ((gf32_t)d.sc_out)[t] = lp[(size_t)t * ld + (size_t)lab];
        }
        if (t1 < 0) break;
        p = q + 16 * w;
        cur[0] = nxt[0];
        cur[1] = nxt[1];
        w = wn;
        t0 = t1;
        n = kBandBtChunk;
    }
}

// ---------------------------------------------------------------------------------------
// generic form: the forward kernel over the table, the walk back
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void forward_banded_generic_kernel(const BandLattice *__restrict__ lats, int32_t *meta)
{
    forward_banded_generic<false>(lats[blockIdx.x], meta, 0, 0);
}

__global__ __launch_bounds__(64) void backtrace_banded_generic_kernel(const BandLattice *__restrict__ lats, const int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    int64_t p = meta[4 * (size_t)d.idx + 1];
    if (p < 0 || threadIdx.x != 0) return;
    const int64_t T = d.T, W = d.W;
    const uint8_t *bp = reinterpret_cast<const uint8_t *>(d.bp);
    for (int64_t t = T - 1; t >= 0; --t) {
        const int lab = (p & 1) ? (d.labx[p >> 1] >> 2) : 0;
        d.path[t] = (int32_t)p;
        d.lab_out[t] = lab;
        d.sc_out[t] = d.lp[(size_t)t * (size_t)d.ld + (size_t)lab];
        p -= bp[(size_t)t * (size_t)W + (size_t)(p - d.band_lo[t])];
    }
}

template <int M>
static void launch_forward_banded_wave(const BandLattice *lats, int n, int32_t *meta, hipStream_t s)
{
    forward_banded_wave_kernel<M, false><<<dim3(n), dim3(64), 0, s>>>(lats, meta);
    forward_banded_wave_kernel<M, true><<<dim3(n), dim3(64), 0, s>>>(lats, meta);
}

void launch_backtrace_banded(const BandLattice *lats, int n_fast, int n_generic, const int32_t *meta, hipStream_t s)
{
    if (n_fast > 0) backtrace_banded_wave_kernel<<<dim3(n_fast), dim3(64), 0, s>>>(lats, meta);
    if (n_generic > 0) backtrace_banded_generic_kernel<<<dim3(n_generic), dim3(64), 0, s>>>(lats + n_fast, meta);
}

void launch_best_path_banded(const BandLattice *lats, int n_fast, int n_generic, int max_move, int32_t *meta, hipStream_t s)
{
    prep_banded_kernel<<<dim3(n_fast + n_generic), dim3(256), 0, s>>>(lats, meta);
    if (n_fast > 0) {
        switch (max_move) {
        case 1: launch_forward_banded_wave<1>(lats, n_fast, meta, s); break;
        case 2: launch_forward_banded_wave<2>(lats, n_fast, meta, s); break;
        case 3: launch_forward_banded_wave<3>(lats, n_fast, meta, s); break;
        default: launch_forward_banded_wave<4>(lats, n_fast, meta, s); break;
        }
    }
    if (n_generic > 0) forward_banded_generic_kernel<<<dim3(n_generic), dim3(256), 0, s>>>(lats + n_fast, meta);
    launch_backtrace_banded(lats, n_fast, n_generic, meta, s);
}

}  // namespace ka
