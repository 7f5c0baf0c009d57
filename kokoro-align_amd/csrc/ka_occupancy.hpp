// ka_occupancy.hpp — label occupancy posteriors: for every frame the probability of each label value, over the band's paths
// that end at a caller-given terminal s*, and Z = alpha_{T-1}(s*).  Included by ka_occupancy.hip only.
//
// Same lattice, band, moves, veto and numerics as ka_posterior.hpp:
//   occ[t, v] = sum over s in [lo_t, hi_t) with lab'[s] = v of gamma_t(s),  gamma_t(s) = 2^(alpha_t(s) + beta_t(s) - Z)
// which is also dZ / d log_probs[t, v].  The posterior kernels keep alpha only at the path; this backward pass needs it at
// every band cell, so the forward pass checkpoints the whole column before the first frame of every 32-frame block (with
// the offset C and the frame maximum m it runs on), and the backward pass, last block first, recomputes the block's alpha
// from its checkpoint into a per-slot slab with the forward pass's own frame function (fb_fast_fwd / fb_gen_fwd of
// ka_posterior_common.hpp), then steps beta back through the block (fb_fast_bwd / fb_gen_bwd).  The recompute runs the same instructions on the same operands: its alpha is the forward pass's bit for bit, so
// gamma at (T-1, s*) is 2^0 exactly.
// Binning: gamma is formed in double, rounded to float and raised by the hardware exp2 (an output in [0, 1] needs no more),
// then added as an unsigned 32.32 fixed-point integer, so the row's bits do not depend on the order of the adds: blank cells
// (even positions) through a register sum and a wave reduction, the other cells through 64-bit LDS atomics (the generic
// form's above kOccLdsBins through global atomics on a workspace row).  At most 1009 cells of at most 2^32 each: no overflow;
// truncation costs < 2^-32 per cell.
// Storage: lattices walk slots (launch grid = slots, lattice i on slot i mod grid), so the workspace is bounded by the slots,
// not by the batch.
#pragma once
#include "ka_posterior_common.hpp"

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
// a lattice without a result: NaN rows, and the status and log-likelihood of fb_fail_result
__device__ __forceinline__ void occ_fail(const OccLattice &d, PostResult *res, int status)
{
    const int64_t n = (int64_t)d.T * d.V;
    for (int64_t k = threadIdx.x; k < n; k += blockDim.x) {
        const int64_t t = k / d.V, v = k - t * d.V;
        reinterpret_cast<uint32_t *>(d.occ)[t * d.ld_out + v] = 0x7fc00000u;
    }
    fb_fail_result(d, res, status);
}

// ---------------------------------------------------------------------------------------
// fast form: one wavefront per lattice, band <= kFastMaxBand, V <= 64, M = max_move <= 4; the cell layout of
// posterior_fast_kernel (position p at slot p & 1023 of an LDS column; lane l owns lo + l + 64 k).  The forward pass and
// the recompute both run fb_fast_fwd with the same label source, so the two produce the same bits.
// ---------------------------------------------------------------------------------------
template <int M>
__device__ __forceinline__ void occ_fast_one(const OccLattice &d, PostResult *res, double (*col)[1024], double *row, double *cav,
                                             unsigned long long *bins)
{
    const int lane = threadIdx.x;
    const int64_t T = d.T, L = d.L, B = d.beam, V = d.V;
    const size_t ld = (size_t)d.ld;
    const double NINF = post_dninf();
    if (fb_labels_bad(d)) {
        occ_fail(d, res, kStatusBadLabel);
        return;
    }
    bins[lane] = 0;
    auto lab_of = [&](int64_t p) { return fb_lab(d, p); };
    auto no_cell = [](int64_t, double) {};

    // ---- forward: Z, and a checkpoint before every block ----
    double *prev = col[0], *cur = col[1];
    if (lane == 0) prev[0] = 0.0;   // virtual state before frame 0
    int64_t plo = 0, phi = 1;
    BandWalk bw(L, B, T);
    double C = 0.0, Cb = 0.0, Ca = 0.0, mprev = 0.0;
    int flags = 0;
    float rv = lane < V ? d.lp[lane] : 0.0f;
    post_wave_sync();
    for (int64_t t = 0; t < T; ++t) {
        int64_t lo, hi;
        bw.band(lo, hi);
        if (lane < V) {
            flags |= post_bad_bits(rv);
            row[lane] = (double)rv * kLog2e64;
        }
        if (t + 1 < T && lane < V) rv = d.lp[(size_t)(t + 1) * ld + lane];
        if (t % kPostCk == 0) {
            const int64_t k = t / kPostCk;
            Cb = C;
            if (lane == 0) {
                d.ck[2 * k] = C;
                d.ck[2 * k + 1] = mprev;
            }
            for (int s = lane; s < 1024; s += 64) d.ckcol[k * 1024 + s] = prev[s];
        }
        post_wave_sync();
        double m = post_wave_max(fb_fast_fwd<M>(lo, hi, plo, phi, prev, cur, row, mprev, lab_of, no_cell));
        m = (m == NINF) ? 0.0 : m;
        Ca = C;
        C += m;
        mprev = m;
        { double *x = prev; prev = cur; cur = x; }
        plo = lo;
        phi = hi;
        bw.next();
        post_wave_sync();
    }
    const int64_t sstar = d.terminal;
    flags |= (sstar < 0 || sstar >= L) ? 4 : 0;
    flags = post_block_flags(flags);
    if (flags) {
        occ_fail(d, res, post_status_of(flags));
        return;
    }
    const double us = (sstar >= plo && sstar < phi) ? prev[sstar & 1023] : NINF;
    if ((float)((Ca - Cb) + us) == post_ninf()) {
        occ_fail(d, res, kStatusZeroMass);
        return;
    }
    const double Z = Ca + us;   // log2 alpha_{T-1}(s*), the expression gamma's alpha is formed with
    const double Zr = fb_reported_z(Cb, Ca, us);
    post_wave_sync();

    // ---- backward, a block at a time ----
    double *gn = col[0], *vn = col[1], *gc = col[2], *vc = col[3];   // G_{t+1} and its vetoable copy; scratch
    int64_t nlo = 0, nhi = 0;
    double D = 0.0, nprev = 0.0;   // D_T = 0: beta_{T-1} = {s*: 0}
    for (int64_t k = (T - 1) / kPostCk; k >= 0; --k) {
        const int64_t t0 = k * kPostCk, t1 = (t0 + kPostCk < T) ? t0 + kPostCk : T;
        // recompute alpha over [t0, t1) into the slab, gc / vc as the working columns
        double *pv = gc, *cu = vc;
        for (int s = lane; s < 1024; s += 64) pv[s] = d.ckcol[k * 1024 + s];
        double C2 = d.ck[2 * k], mp = d.ck[2 * k + 1];
        int64_t rlo = 0, rhi = 1;
        bw.seek(t0);
        if (t0 > 0) {
            bw.prev();
            bw.band(rlo, rhi);
            bw.next();
        }
        float rv2 = lane < V ? d.lp[(size_t)t0 * ld + lane] : 0.0f;
        post_wave_sync();
        for (int64_t t = t0; t < t1; ++t) {
            int64_t lo, hi;
            bw.band(lo, hi);
            if (lane < V) row[lane] = (double)rv2 * kLog2e64;
            if (t + 1 < t1 && lane < V) rv2 = d.lp[(size_t)(t + 1) * ld + lane];
            if (lane == 0) cav[t - t0] = C2;
            post_wave_sync();
            double *al = d.slab + (t - t0) * 1024;
            double m = post_wave_max(fb_fast_fwd<M>(lo, hi, rlo, rhi, pv, cu, row, mp, lab_of, [&](int64_t p, double val) { al[p & 1023] = val; }));
            m = (m == NINF) ? 0.0 : m;
            C2 += m;
            mp = m;
            { double *x = pv; pv = cu; cu = x; }
            rlo = lo;
            rhi = hi;
            bw.next();
            post_wave_sync();
        }
        // beta back through the block (bw walks back from t1); gamma binned per frame
        float rv3 = lane < V ? d.lp[(size_t)(t1 - 1) * ld + lane] : 0.0f;
        for (int64_t t = t1 - 1; t >= t0; --t) {
            bw.prev();
            int64_t lo, hi;
            bw.band(lo, hi);
            if (lane < V) row[lane] = (double)rv3 * kLog2e64;
            if (t > t0 && lane < V) rv3 = d.lp[(size_t)(t - 1) * ld + lane];
            const double ca = cav[t - t0];
            const double *al = d.slab + (t - t0) * 1024;
            post_wave_sync();
            unsigned long long blank = 0;
            const double mymax = fb_fast_bwd<M>(lo, hi, nlo, nhi, gn, vn, gc, vc, row, nprev, t == T - 1, sstar, lab_of,
                                                [&](int64_t p, int32_t lab, double w) {
                                                    const unsigned long long f = occ_fix(((ca + al[p & 1023]) + (D + w)) - Z);
                                                    if ((p & 1) == 0) blank += f;
                                                    else if (f) atomicAdd(&bins[lab], f);
                                                });
            blank = occ_wave_sum(blank);
            double n = post_wave_max(mymax);
            n = (n == NINF) ? 0.0 : n;
            D += n;
            nprev = n;
            { double *x = gn; gn = gc; gc = x; }
            { double *x = vn; vn = vc; vc = x; }
            nlo = lo;
            nhi = hi;
            post_wave_sync();
            if (lane < V) {
                const unsigned long long b = bins[lane] + (lane == 0 ? blank : 0ull);
                bins[lane] = 0;
                d.occ[(size_t)t * (size_t)d.ld_out + lane] = occ_unfix(b);
            }
            post_wave_sync();
        }
    }
    if (lane == 0) {
        res[d.idx].status = kStatusOk;
        res[d.idx].log_likelihood = Zr;
    }
}

template <int M>
__global__ __launch_bounds__(64) void occupancy_fast_kernel(const OccLattice *__restrict__ lats, int n, PostResult *res)
{
    __shared__ double col[4][1024];
    __shared__ double row[64];
    __shared__ double cav[kPostCk];
    __shared__ unsigned long long bins[64];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        occ_fast_one<M>(lats[i], res, col, row, cav, bins);
        post_wave_sync();
    }
}

// ---------------------------------------------------------------------------------------
// generic form: any band, any V, max_move <= 255.  One 256-thread workgroup per lattice, working columns at absolute
// positions in global memory, checkpoints and slab relative to the band's low end.  A correctness path, not tuned.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void occ_gen_one(const OccLattice &d, PostResult *res, double (*red)[4], double *cav, unsigned long long *lbins)
{
    const int tid = threadIdx.x;
    const int64_t T = d.T, L = d.L, B = d.beam, V = d.V;
    const int64_t cw = d.cw;
    const size_t ld = (size_t)d.ld;
    const double NINF = post_dninf();
    if (fb_labels_bad(d)) {
        occ_fail(d, res, kStatusBadLabel);
        return;
    }
    unsigned long long *bins = V <= kOccLdsBins ? lbins : d.gbin;
    for (int64_t v = tid; v < V; v += 256) atomicExch(&bins[v], 0ull);
    double *A[4] = {d.col, d.col + L, d.col + 2 * L, d.col + 3 * L};
    int ph = 0;   // parity of the reduction slots
    auto no_cell = [](int64_t, double) {};

    // ---- forward ----
    double *prev = A[0], *cur = A[1];
    if (tid == 0) prev[0] = 0.0;
    int64_t plo = 0, phi = 1;
    BandWalk bw(L, B, T);
    double C = 0.0, Cb = 0.0, Ca = 0.0, mprev = 0.0;
    int flags = 0;
    __syncthreads();
    for (int64_t t = 0; t < T; ++t) {
        int64_t lo, hi;
        bw.band(lo, hi);
        const float *lrow = d.lp + (size_t)t * ld;
        for (int64_t v = tid; v < V; v += 256) flags |= post_bad_bits(lrow[v]);
        if (t % kPostCk == 0) {
            const int64_t k = t / kPostCk;
            Cb = C;
            if (tid == 0) {
                d.ck[2 * k] = C;
                d.ck[2 * k + 1] = mprev;
            }
            for (int64_t p = plo + tid; p < phi; p += 256) d.ckcol[k * cw + (p - plo)] = prev[p];
        }
        double m = post_block_max(fb_gen_fwd(d, lrow, lo, hi, plo, phi, prev, cur, mprev, no_cell), red[ph]);
        ph ^= 1;
        m = (m == NINF) ? 0.0 : m;
        Ca = C;
        C += m;
        mprev = m;
        { double *x = prev; prev = cur; cur = x; }
        plo = lo;
        phi = hi;
        bw.next();
    }
    const int64_t sstar = d.terminal;
    flags |= (sstar < 0 || sstar >= L) ? 4 : 0;
    flags = post_block_flags(flags);
    if (flags) {
        occ_fail(d, res, post_status_of(flags));
        return;
    }
    const double us = (sstar >= plo && sstar < phi) ? prev[sstar] : NINF;
    if ((float)((Ca - Cb) + us) == post_ninf()) {
        occ_fail(d, res, kStatusZeroMass);
        return;
    }
    const double Z = Ca + us;
    const double Zr = fb_reported_z(Cb, Ca, us);
    __syncthreads();

    // ---- backward, a block at a time ----
    double *gn = A[0], *vn = A[1], *gc = A[2], *vc = A[3];
    int64_t nlo = 0, nhi = 0;
    double D = 0.0, nprev = 0.0;
    for (int64_t k = (T - 1) / kPostCk; k >= 0; --k) {
        const int64_t t0 = k * kPostCk, t1 = (t0 + kPostCk < T) ? t0 + kPostCk : T;
        double *pv = gc, *cu = vc;
        int64_t rlo = 0, rhi = 1;
        bw.seek(t0);
        if (t0 > 0) {
            bw.prev();
            bw.band(rlo, rhi);
            bw.next();
        }
        for (int64_t p = rlo + tid; p < rhi; p += 256) pv[p] = d.ckcol[k * cw + (p - rlo)];
        double C2 = d.ck[2 * k], mp = d.ck[2 * k + 1];
        __syncthreads();
        for (int64_t t = t0; t < t1; ++t) {
            int64_t lo, hi;
            bw.band(lo, hi);
            if (tid == 0) cav[t - t0] = C2;
            double *al = d.slab + (t - t0) * cw;
            double m = post_block_max(fb_gen_fwd(d, d.lp + (size_t)t * ld, lo, hi, rlo, rhi, pv, cu, mp,
                                                 [&](int64_t p, double val) { al[p - lo] = val; }),
                                      red[ph]);
            ph ^= 1;
            m = (m == NINF) ? 0.0 : m;
            C2 += m;
            mp = m;
            { double *x = pv; pv = cu; cu = x; }
            rlo = lo;
            rhi = hi;
            bw.next();
        }
        __syncthreads();
        for (int64_t t = t1 - 1; t >= t0; --t) {
            bw.prev();
            int64_t lo, hi;
            bw.band(lo, hi);
            const double ca = cav[t - t0];
            const double *al = d.slab + (t - t0) * cw;
            unsigned long long blank = 0;
            const double mymax = fb_gen_bwd(d, d.lp + (size_t)t * ld, lo, hi, nlo, nhi, gn, vn, gc, vc, nprev, t == T - 1, sstar,
                                            [&](int64_t p, int32_t lab, double w) {
                                                const unsigned long long f = occ_fix(((ca + al[p - lo]) + (D + w)) - Z);
                                                if ((p & 1) == 0) blank += f;
                                                else if (f) atomicAdd(&bins[lab], f);
                                            });
            if (blank) atomicAdd(&bins[0], blank);
            double n = post_block_max(mymax, red[ph]);   // (its barrier also closes the frame's atomics)
            ph ^= 1;
            n = (n == NINF) ? 0.0 : n;
            D += n;
            nprev = n;
            { double *x = gn; gn = gc; gc = x; }
            { double *x = vn; vn = vc; vc = x; }
            nlo = lo;
            nhi = hi;
            float *orow = d.occ + (size_t)t * (size_t)d.ld_out;
            for (int64_t v = tid; v < V; v += 256) orow[v] = occ_unfix(atomicExch(&bins[v], 0ull));
            __syncthreads();
        }
    }
    if (tid == 0) {
        res[d.idx].status = kStatusOk;
        res[d.idx].log_likelihood = Zr;
    }
}

__global__ __launch_bounds__(256) void occupancy_generic_kernel(const OccLattice *__restrict__ lats, int n, PostResult *res)
{
    __shared__ double red[2][4];
    __shared__ double cav[kPostCk];
    __shared__ unsigned long long lbins[kOccLdsBins];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        occ_gen_one(lats[i], res, red, cav, lbins);
        __syncthreads();
    }
}

}  // namespace ka
