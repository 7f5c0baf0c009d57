// ka_posterior_common.hpp — the forward-backward helpers shared by ka_posterior.hpp (best-path posteriors) and
// ka_occupancy.hpp (label occupancy posteriors): base-2 log-sum-exp, the band, status flags, wave and block reductions.
#pragma once
#include "ka_types.hpp"

namespace ka {

constexpr double kLog2e64 = 1.44269504088896340736;
constexpr double kLn2 = 0.693147180559945309417;

__device__ __forceinline__ float post_ninf() { return -__builtin_inff(); }
// (integer tests on the bits, hidden from the optimiser: the library is built with -fno-honor-nans, under which a test of a
//  float's bits may be folded as a floating-point class test that assumes no NaN)
__device__ __forceinline__ int post_bad_bits(float x)
{
    uint32_t b = __builtin_bit_cast(uint32_t, x);
    asm volatile("" : "+v"(b));
    return ((b & 0x7fffffffu) > 0x7f800000u ? 1 : 0) | (b == 0x7f800000u ? 2 : 0);   // 1: NaN, 2: +inf
}
__device__ __forceinline__ double post_wave_max(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = fmaxf(x, __shfl_xor(x, off));
    return x;
}
// One wavefront: its LDS operations execute in program order, so a frame hand-off needs no s_barrier (whose fence would also
// wait for the global loads prefetched for the next frame), only a compiler fence that keeps the accesses in order.
__device__ __forceinline__ void post_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ double post_dninf() { return -__builtin_inf(); }
// log2(sum 2^x_j) from the running maximum; all -inf -> -inf (never 2^(-inf - -inf))
__device__ __forceinline__ double post_lse2(const double *x, int n, double mx)
{
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += exp2(x[j] - mx);
    return mx == post_dninf() ? post_dninf() : mx + log2(s);
}
// band of align.py:64-65 from q = floor(L t / T)
__device__ __forceinline__ void post_band(int64_t q, int64_t L, int64_t B, int64_t &lo, int64_t &hi)
{
    lo = q - B / 2;
    lo = lo < 0 ? 0 : lo;
    hi = (L - lo < B) ? L : lo + B;
}
// error flags -> status: a bad label is reported before anything runs; then NaN, +inf, a path value outside [0, L)
__device__ __forceinline__ int post_status_of(int flags)
{
    return (flags & 1) ? kStatusNaN : (flags & 2) ? kStatusNonFinite : (flags & 4) ? kStatusBadArgs : kStatusOk;
}
// the OR of every thread's error flags (__syncthreads_or is a predicate: it answers 0 or 1)
__device__ __forceinline__ int post_block_flags(int flags)
{
    return (__syncthreads_or(flags & 1) ? 1 : 0) | (__syncthreads_or(flags & 2) ? 2 : 0) | (__syncthreads_or(flags & 4) ? 4 : 0);
}
// a lattice without a result: NaN posteriors; log-likelihood NaN, or -inf for kStatusZeroMass (stored as bits: the library
// is built with -fno-honor-nans, under which a NaN constant is undefined)
constexpr uint64_t kNaN64 = 0x7ff8000000000000ull, kNinf64 = 0xfff0000000000000ull;
__device__ __forceinline__ void post_fail(const PostLattice &d, PostResult *res, int status)
{
    uint32_t *post = reinterpret_cast<uint32_t *>(d.post);
    for (int t = threadIdx.x; t < d.T; t += blockDim.x) post[t] = 0x7fc00000u;
    if (threadIdx.x == 0) {
        res[d.idx].status = status;
        *reinterpret_cast<uint64_t *>(&res[d.idx].log_likelihood) = status == kStatusZeroMass ? kNinf64 : kNaN64;
    }
}
__device__ __forceinline__ bool post_labels_bad(const PostLattice &d)
{
    int bad = 0;
    for (int i = threadIdx.x; i < d.S; i += blockDim.x) {
        const int l = d.labels[i];
        bad |= (l < 0 || l >= d.V) ? 1 : 0;
    }
    return __syncthreads_or(bad) != 0;
}
// posterior of one frame from its two halves (log2 units), clamped to a probability
__device__ __forceinline__ float post_value(double cb, float dt, double D, double w, double Z)
{
    const double l2 = (cb + (double)dt) + (D + w) - Z;
    const double p = exp2(l2);
    return (float)(p < 1.0 ? p : 1.0);
}

__device__ __forceinline__ double post_block_max(double x, double *red)   // red: 4 values of this frame's parity
{
    x = post_wave_max(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

}  // namespace ka
