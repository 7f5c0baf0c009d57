// ka_occupancy.hpp — label occupancy posteriors: for every frame the probability of each label value, over the band's paths
// that end at a caller-given terminal s*, and Z = alpha_{T-1}(s*).  Included by ka_occupancy.hip only.
//
// Same lattice, band, moves, veto and numerics as ka_posterior.hpp:
//   occ[t, v] = sum over s in [lo_t, hi_t) with lab'[s] = v of gamma_t(s),  gamma_t(s) = 2^(alpha_t(s) + beta_t(s) - Z)
// which is also dZ / d log_probs[t, v].  The posterior kernels keep alpha only at the path; this backward pass needs it at
// every band cell, so the forward pass checkpoints the whole column before the first frame of every 32-frame block (with
// the offset C and the frame maximum m it runs on), and the backward pass, last block first, recomputes the block's alpha
// from its checkpoint into a per-slot slab with the forward pass's own frame function, then steps beta back through the
// block.  The recompute runs the same instructions on the same operands: its alpha is the forward pass's bit for bit, so
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
__device__ __forceinline__ int32_t occ_lab(const OccLattice &d, int64_t p) { return (p & 1) ? d.labels[p >> 1] : 0; }
// a lattice without a result: NaN rows; log-likelihood NaN, or -inf for kStatusZeroMass
__device__ __forceinline__ void occ_fail(const OccLattice &d, PostResult *res, int status)
{
    const int64_t n = (int64_t)d.T * d.V;
    for (int64_t k = threadIdx.x; k < n; k += blockDim.x) {
        const int64_t t = k / d.V, v = k - t * d.V;
        reinterpret_cast<uint32_t *>(d.occ)[t * d.ld_out + v] = 0x7fc00000u;
    }
    if (threadIdx.x == 0) {
        res[d.idx].status = status;
        *reinterpret_cast<uint64_t *>(&res[d.idx].log_likelihood) = status == kStatusZeroMass ? kNinf64 : kNaN64;
    }
}
__device__ __forceinline__ bool occ_labels_bad(const OccLattice &d)
{
    int bad = 0;
    for (int i = threadIdx.x; i < d.S; i += blockDim.x) {
        const int l = d.labels[i];
        bad |= (l < 0 || l >= d.V) ? 1 : 0;
    }
    return __syncthreads_or(bad) != 0;
}
// Z as ka_posterior.hpp forms it (the block offset plus the float-stored relative alpha), in nats: the value the
// path-posterior call returns for a path that ends at s*
__device__ __forceinline__ double occ_reported_z(double cb, double ca, double us)
{
    return (cb + (double)(float)((ca - cb) + us)) * kLn2;
}

// ---------------------------------------------------------------------------------------
// fast form: one wavefront per lattice, band <= kFastMaxBand, V <= 64, M = max_move <= 4; the cell layout of
// posterior_fast_kernel (position p at slot p & 1023 of an LDS column; lane l owns lo + l + 64 k)
// ---------------------------------------------------------------------------------------
// One forward frame: u_t over [lo, hi) from u_{t-1} over [plo, phi).  Both the forward pass and the recompute call this, so
// the two produce the same bits.  Returns the lane's maximum.
template <int M>
__device__ __forceinline__ double occ_fast_fwd(const OccLattice &d, int64_t lo, int64_t hi, int64_t plo, int64_t phi, const double *prev,
                                              double *cur, const double *row, double mprev, double *alpha_out)
{
    const double NINF = post_dninf();
    double mymax = NINF;
    for (int64_t p = lo + threadIdx.x; p < hi; p += 64) {
        const int32_t lab = occ_lab(d, p);
        const double e = row[lab];
        double x[M];
        double mx = NINF;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int64_t u = p - j;
            const bool ok = u >= plo && u < phi && !(j >= 2 && (j & 1) == 0 && lab == 0);
            x[j] = ok ? prev[u & 1023] : NINF;
            mx = fmaxf(mx, x[j]);
        }
        const double val = post_lse2(x, M, mx) + (e - mprev);
        cur[p & 1023] = val;
        if (alpha_out) alpha_out[p & 1023] = val;
        mymax = fmaxf(mymax, val);
    }
    return mymax;
}

template <int M>
__device__ __forceinline__ void occ_fast_one(const OccLattice &d, PostResult *res, double (*col)[1024], double *row, double *cav,
                                             unsigned long long *bins)
{
    const int lane = threadIdx.x;
    const int64_t T = d.T, L = d.L, B = d.beam, V = d.V;
    const int64_t dq = L / T, dr = L % T;
    const size_t ld = (size_t)d.ld;
    const double NINF = post_dninf();
    if (occ_labels_bad(d)) {
        occ_fail(d, res, kStatusBadLabel);
        return;
    }
    bins[lane] = 0;

    // ---- forward: Z, and a checkpoint before every block ----
    double *prev = col[0], *cur = col[1];
    if (lane == 0) prev[0] = 0.0;   // virtual state before frame 0
    int64_t plo = 0, phi = 1, q = 0, r = 0;
    double C = 0.0, Cb = 0.0, Ca = 0.0, mprev = 0.0;
    int flags = 0;
    float rv = lane < V ? d.lp[lane] : 0.0f;
    post_wave_sync();
    for (int64_t t = 0; t < T; ++t) {
        int64_t lo, hi;
        post_band(q, L, B, lo, hi);
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
        double m = post_wave_max(occ_fast_fwd<M>(d, lo, hi, plo, phi, prev, cur, row, mprev, nullptr));
        m = (m == NINF) ? 0.0 : m;
        Ca = C;
        C += m;
        mprev = m;
        { double *x = prev; prev = cur; cur = x; }
        plo = lo;
        phi = hi;
        q += dq;
        r += dr;
        if (r >= T) { r -= T; ++q; }
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
    const double Zr = occ_reported_z(Cb, Ca, us);
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
        if (t0 > 0) post_band((L * (t0 - 1)) / T, L, B, rlo, rhi);
        int64_t q2 = (L * t0) / T, r2 = (L * t0) % T;
        float rv2 = lane < V ? d.lp[(size_t)t0 * ld + lane] : 0.0f;
        post_wave_sync();
        for (int64_t t = t0; t < t1; ++t) {
            int64_t lo, hi;
            post_band(q2, L, B, lo, hi);
            if (lane < V) row[lane] = (double)rv2 * kLog2e64;
            if (t + 1 < t1 && lane < V) rv2 = d.lp[(size_t)(t + 1) * ld + lane];
            if (lane == 0) cav[t - t0] = C2;
            post_wave_sync();
            double m = post_wave_max(occ_fast_fwd<M>(d, lo, hi, rlo, rhi, pv, cu, row, mp, d.slab + (t - t0) * 1024));
            m = (m == NINF) ? 0.0 : m;
            C2 += m;
            mp = m;
            { double *x = pv; pv = cu; cu = x; }
            rlo = lo;
            rhi = hi;
            q2 += dq;
            r2 += dr;
            if (r2 >= T) { r2 -= T; ++q2; }
            post_wave_sync();
        }
        // beta back through the block; gamma binned per frame
        float rv3 = lane < V ? d.lp[(size_t)(t1 - 1) * ld + lane] : 0.0f;
        for (int64_t t = t1 - 1; t >= t0; --t) {
            int64_t lo, hi;
            post_band((L * t) / T, L, B, lo, hi);
            if (lane < V) row[lane] = (double)rv3 * kLog2e64;
            if (t > t0 && lane < V) rv3 = d.lp[(size_t)(t - 1) * ld + lane];
            const double ca = cav[t - t0];
            const double *al = d.slab + (t - t0) * 1024;
            const bool last = t == T - 1;
            post_wave_sync();
            double mymax = NINF;
            unsigned long long blank = 0;
            for (int64_t p = lo + lane; p < hi; p += 64) {
                const int32_t lab = occ_lab(d, p);
                double w;
                if (last) {
                    w = (p == sstar) ? 0.0 : NINF;
                } else {
                    double x[M];
                    double mx = NINF;
#pragma unroll
                    for (int j = 0; j < M; ++j) {
                        const int64_t u = p + j;
                        const bool ok = u >= nlo && u < nhi;
                        const double g = (j >= 2 && (j & 1) == 0) ? vn[u & 1023] : gn[u & 1023];
                        x[j] = ok ? g : NINF;
                        mx = fmaxf(mx, x[j]);
                    }
                    w = post_lse2(x, M, mx) - nprev;
                }
                const double g = w + row[lab];
                gc[p & 1023] = g;
                vc[p & 1023] = lab == 0 ? NINF : g;
                mymax = fmaxf(mymax, g);
                const unsigned long long f = occ_fix(((ca + al[p & 1023]) + (D + w)) - Z);
                if ((p & 1) == 0) blank += f;
                else if (f) atomicAdd(&bins[lab], f);
            }
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
__device__ __forceinline__ double occ_gen_fwd(const OccLattice &d, const float *lrow, int64_t lo, int64_t hi, int64_t plo, int64_t phi,
                                             const double *prev, double *cur, double mprev, double *alpha_out)
{
    const int M = d.max_move;
    const double NINF = post_dninf();
    double mymax = NINF;
    for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
        const int32_t lab = occ_lab(d, p);
        const double e = (double)lrow[lab] * kLog2e64;
        double mx = NINF;
        for (int j = 0; j < M && j <= p; ++j) {
            const int64_t u = p - j;
            if (u >= plo && u < phi && !(j >= 2 && (j & 1) == 0 && lab == 0)) mx = fmaxf(mx, prev[u]);
        }
        double s = 0.0;
        for (int j = 0; j < M && j <= p; ++j) {
            const int64_t u = p - j;
            if (u >= plo && u < phi && !(j >= 2 && (j & 1) == 0 && lab == 0)) s += exp2(prev[u] - mx);
        }
        const double l = mx == NINF ? NINF : mx + log2(s);
        const double val = l + (e - mprev);
        cur[p] = val;
        if (alpha_out) alpha_out[p - lo] = val;
        mymax = fmaxf(mymax, val);
    }
    return mymax;
}

__device__ __forceinline__ void occ_gen_one(const OccLattice &d, PostResult *res, double (*red)[4], double *cav, unsigned long long *lbins)
{
    const int tid = threadIdx.x;
    const int64_t T = d.T, L = d.L, B = d.beam, V = d.V;
    const int M = d.max_move;
    const int64_t dq = L / T, dr = L % T, cw = d.cw;
    const size_t ld = (size_t)d.ld;
    const double NINF = post_dninf();
    if (occ_labels_bad(d)) {
        occ_fail(d, res, kStatusBadLabel);
        return;
    }
    unsigned long long *bins = V <= kOccLdsBins ? lbins : d.gbin;
    for (int64_t v = tid; v < V; v += 256) atomicExch(&bins[v], 0ull);
    double *A[4] = {d.col, d.col + L, d.col + 2 * L, d.col + 3 * L};
    int ph = 0;   // parity of the reduction slots

    // ---- forward ----
    double *prev = A[0], *cur = A[1];
    if (tid == 0) prev[0] = 0.0;
    int64_t plo = 0, phi = 1, q = 0, r = 0;
    double C = 0.0, Cb = 0.0, Ca = 0.0, mprev = 0.0;
    int flags = 0;
    __syncthreads();
    for (int64_t t = 0; t < T; ++t) {
        int64_t lo, hi;
        post_band(q, L, B, lo, hi);
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
        double m = post_block_max(occ_gen_fwd(d, lrow, lo, hi, plo, phi, prev, cur, mprev, nullptr), red[ph]);
        ph ^= 1;
        m = (m == NINF) ? 0.0 : m;
        Ca = C;
        C += m;
        mprev = m;
        { double *x = prev; prev = cur; cur = x; }
        plo = lo;
        phi = hi;
        q += dq;
        r += dr;
        if (r >= T) { r -= T; ++q; }
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
    const double Zr = occ_reported_z(Cb, Ca, us);
    __syncthreads();

    // ---- backward, a block at a time ----
    double *gn = A[0], *vn = A[1], *gc = A[2], *vc = A[3];
    int64_t nlo = 0, nhi = 0;
    double D = 0.0, nprev = 0.0;
    for (int64_t k = (T - 1) / kPostCk; k >= 0; --k) {
        const int64_t t0 = k * kPostCk, t1 = (t0 + kPostCk < T) ? t0 + kPostCk : T;
        double *pv = gc, *cu = vc;
        int64_t rlo = 0, rhi = 1;
        if (t0 > 0) post_band((L * (t0 - 1)) / T, L, B, rlo, rhi);
        for (int64_t p = rlo + tid; p < rhi; p += 256) pv[p] = d.ckcol[k * cw + (p - rlo)];
        double C2 = d.ck[2 * k], mp = d.ck[2 * k + 1];
        int64_t q2 = (L * t0) / T, r2 = (L * t0) % T;
        __syncthreads();
        for (int64_t t = t0; t < t1; ++t) {
            int64_t lo, hi;
            post_band(q2, L, B, lo, hi);
            if (tid == 0) cav[t - t0] = C2;
            double m = post_block_max(occ_gen_fwd(d, d.lp + (size_t)t * ld, lo, hi, rlo, rhi, pv, cu, mp, d.slab + (t - t0) * cw), red[ph]);
            ph ^= 1;
            m = (m == NINF) ? 0.0 : m;
            C2 += m;
            mp = m;
            { double *x = pv; pv = cu; cu = x; }
            rlo = lo;
            rhi = hi;
            q2 += dq;
            r2 += dr;
            if (r2 >= T) { r2 -= T; ++q2; }
        }
        __syncthreads();
        for (int64_t t = t1 - 1; t >= t0; --t) {
            int64_t lo, hi;
            post_band((L * t) / T, L, B, lo, hi);
            const float *lrow = d.lp + (size_t)t * ld;
            const double ca = cav[t - t0];
            const double *al = d.slab + (t - t0) * cw;
            const bool last = t == T - 1;
            double mymax = NINF;
            unsigned long long blank = 0;
            for (int64_t p = lo + tid; p < hi; p += 256) {
                const int32_t lab = occ_lab(d, p);
                const double e = (double)lrow[lab] * kLog2e64;
                double w;
                if (last) {
                    w = (p == sstar) ? 0.0 : NINF;
                } else {
                    double mx = NINF;
                    for (int j = 0; j < M; ++j) {
                        const int64_t u = p + j;
                        if (u >= nlo && u < nhi) mx = fmaxf(mx, (j >= 2 && (j & 1) == 0) ? vn[u] : gn[u]);
                    }
                    double s = 0.0;
                    for (int j = 0; j < M; ++j) {
                        const int64_t u = p + j;
                        if (u >= nlo && u < nhi) s += exp2(((j >= 2 && (j & 1) == 0) ? vn[u] : gn[u]) - mx);
                    }
                    w = (mx == NINF ? NINF : mx + log2(s)) - nprev;
                }
                const double g = w + e;
                gc[p] = g;
                vc[p] = lab == 0 ? NINF : g;
                mymax = fmaxf(mymax, g);
                const unsigned long long f = occ_fix(((ca + al[p - lo]) + (D + w)) - Z);
                if ((p & 1) == 0) blank += f;
                else if (f) atomicAdd(&bins[lab], f);
            }
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
