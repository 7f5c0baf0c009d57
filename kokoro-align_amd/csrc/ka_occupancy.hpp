// ka_occupancy.hpp — label occupancy posteriors: for every frame the probability of each label value, over the band's paths
// that end at a caller-given terminal s*, and Z = alpha_{T-1}(s*).  Included by ka_occupancy.hip and ka_occupancy_banded.hip.
//
// Same lattice, band, moves, veto and numerics as ka_posterior.hpp:
//   occ[t, v] = sum over s in [lo_t, hi_t) with lab'[s] = v of gamma_t(s),  gamma_t(s) = 2^(alpha_t(s) + beta_t(s) - Z)
// which is also dZ / d log_probs[t, v].  The checkpointed forward-backward of ka_fb_ck.hpp computes gamma at every band cell;
// the kernel here is its driver with OccOut, which recomputes every block and bins every cell.
// Binning: gamma is formed in double, rounded to float and raised by the hardware exp2 (an output in [0, 1] needs no more),
// then added as an unsigned 32.32 fixed-point integer, so the row's bits do not depend on the order of the adds: blank cells
// (even positions) through a register sum and a wave reduction, the other cells through 64-bit LDS atomics (the generic
// form's above kOccLdsBins through global atomics on a workspace row).  At most 1009 cells of at most 2^32 each: no overflow;
// truncation costs < 2^-32 per cell.
#pragma once
#include "ka_fb_ck.hpp"

namespace ka {

constexpr float kOccFix = 4294967296.0f;   // 2^32
constexpr double kOccUnfix = 1.0 / 4294967296.0;

// one cell's gamma in 32.32 fixed point from its log2 argument (double in, one hardware exp2)
__device__ __forceinline__ unsigned long long occ_fix(double arg)
{
    float g = __builtin_amdgcn_exp2f((float)arg);
    g = g < 1.0f ? g : 1.0f;
    return (unsigned long long)(g * kOccFix);
}
__device__ __forceinline__ float occ_unfix(unsigned long long b) { return (float)((double)b * kOccUnfix); }
__device__ __forceinline__ unsigned long long occ_wave_sum(unsigned long long x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// fb_ck's policy: every block recomputed, gamma binned per label value, a row of occ per frame.  The forms differ in how a
// frame's bins are summed and emptied: one wavefront sums its blank cells in registers and owns bin `lane`, a workgroup goes
// through atomics and a barrier.
template <class Form_, class Band>
struct OccOut {
    using Form = Form_;
    using Desc = OccLattice;
    struct Lds {
        unsigned long long bins[Form::kWave ? 64 : kOccLdsBins];
    };
    static constexpr int NT = Form::NT;
    const OccLattice &d;
    unsigned long long *bins;   // fast form: 64 in LDS; generic: V in LDS up to kOccLdsBins, above it the slot's global row
    unsigned long long blank;   // this thread's blank cells of the frame
    __device__ __forceinline__ OccOut(const OccLattice &d_, Form &, Lds &lds)
        : d(d_), bins(Form::kWave || d_.V <= kOccLdsBins ? lds.bins : d_.gbin), blank(0)
    {
        if (Form::kWave) bins[threadIdx.x] = 0;
        else for (int64_t v = threadIdx.x; v < d.V; v += NT) atomicExch(&bins[v], 0ull);
    }
    // a lattice without a result: NaN rows, and the status and log-likelihood of fb_fail_result
    __device__ __forceinline__ void fail(PostResult *res, int status)
    {
        const int64_t n = (int64_t)d.T * d.V;
        for (int64_t k = threadIdx.x; k < n; k += blockDim.x) {
            const int64_t t = k / d.V, v = k - t * d.V;
            reinterpret_cast<uint32_t *>(d.occ)[t * d.ld_out + v] = 0x7fc00000u;
        }
        fb_fail_result(d, res, status);
    }
    __device__ __forceinline__ bool recompute(int64_t) const { return true; }
    __device__ __forceinline__ auto cells(int64_t, int64_t)
    {
        return [this](int64_t p, int32_t lab, auto arg) {
            const unsigned long long f = occ_fix(arg());
            if ((p & 1) == 0) blank += f;
            else if (f) atomicAdd(&bins[lab], f);
        };
    }
    __device__ __forceinline__ void cells_done()
    {
        if (Form::kWave) blank = occ_wave_sum(blank);
        else if (blank) atomicAdd(&bins[0], blank);   // (the reduction's barrier closes the frame's atomics)
    }
    __device__ __forceinline__ void frame_end(int64_t t, int64_t, int64_t)
    {
        if (Form::kWave) {
            const int lane = threadIdx.x;
            post_wave_sync();
            if (lane < d.V) {
                const unsigned long long b = bins[lane] + (lane == 0 ? blank : 0ull);
                bins[lane] = 0;
                d.occ[(size_t)t * (size_t)d.ld_out + lane] = occ_unfix(b);
            }
        } else {
            float *orow = d.occ + (size_t)t * (size_t)d.ld_out;
            for (int64_t v = threadIdx.x; v < d.V; v += NT) orow[v] = occ_unfix(atomicExch(&bins[v], 0ull));
            __syncthreads();
        }
        blank = 0;
    }
};

template <class Band>
void launch_label_posteriors(const BandDesc<OccLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<OccOut, Band>(lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
