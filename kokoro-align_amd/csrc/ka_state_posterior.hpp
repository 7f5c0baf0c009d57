// ka_state_posterior.hpp — state posteriors at chosen frames: for every query frame f_k the posterior gamma_{f_k}(s) of every
// band position, over the band's paths that end at a caller-given terminal s*, and Z = alpha_{T-1}(s*).  Included by
// ka_state_posterior.hip only.
//
// Same lattice, band, moves, veto, statuses and form split as ka_occupancy.hpp (DESIGN.md sections 4.18 and 4.19), and the
// same checkpoint-and-recompute scheme with two changes:
//   - the backward pass recomputes alpha only for the 32-frame blocks that hold a query frame; beta is still stepped
//     through every frame (it carries from block to block), so a call costs the two passes of the path posterior plus one
//     recomputed block per query block;
//   - a query frame's cells are written, not binned: gamma_t(s) = min(1, exp2f((float)(((ca + alpha) + (D + w)) - Z))), the
//     expression and hardware exp2 that occ_fix of ka_occupancy.hpp bins, so gamma_{T-1}(s*) = 1.0 exactly and gamma summed
//     by label agrees with the occupancy to its 32.32 truncation.  Row k holds gamma_{f_k}(lo_k + j) for j in
//     [0, hi_k - lo_k) from the lanes that own the cells (coalesced), then 0.0 up to W = min(beam, L).
// Frames are ascending; the backward pass walks them from the last (kq = K-1) down.
#pragma once
#include "ka_posterior_common.hpp"

namespace ka {

// one cell's gamma from its log2 argument (occ_fix of ka_occupancy.hpp before the fixed-point step)
__device__ __forceinline__ float st_gamma(double arg)
{
    const float g = __builtin_amdgcn_exp2f((float)arg);
    return g < 1.0f ? g : 1.0f;
}
// a lattice without a result: NaN rows over [0, W), band_lo -1, and the status and log-likelihood of fb_fail_result
__device__ __forceinline__ void st_fail(const StateLattice &d, PostResult *res, int status)
{
    const int64_t n = (int64_t)d.K * d.W;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const int64_t k = i / d.W, j = i - k * d.W;
        reinterpret_cast<uint32_t *>(d.gamma)[k * d.ld_out + j] = 0x7fc00000u;
    }
    for (int64_t k = threadIdx.x; k < d.K; k += blockDim.x) d.band_lo[k] = -1;
    fb_fail_result(d, res, status);
}
// the query frame at index kq, or -1 below the first
__device__ __forceinline__ int64_t st_frame(const StateLattice &d, int64_t kq) { return kq >= 0 ? d.frames[kq] : -1; }

// ---------------------------------------------------------------------------------------
// fast form: one wavefront per lattice, band <= kFastMaxBand, V <= 64, M = max_move <= 4; occ_fast_one's cell layout and
// forward pass (position p at slot p & 1023 of an LDS column; lane l owns lo + l + 64 k).
// ---------------------------------------------------------------------------------------
template <int M>
__device__ __forceinline__ void state_fast_one(const StateLattice &d, PostResult *res, double (*col)[1024], double *row, double *cav)
{
    const int lane = threadIdx.x;
    const int64_t T = d.T, L = d.L, B = d.beam, V = d.V;
    const size_t ld = (size_t)d.ld;
    const double NINF = post_dninf();
    if (fb_labels_bad(d)) {
        st_fail(d, res, kStatusBadLabel);
        return;
    }
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
        st_fail(d, res, post_status_of(flags));
        return;
    }
    const double us = (sstar >= plo && sstar < phi) ? prev[sstar & 1023] : NINF;
    if ((float)((Ca - Cb) + us) == post_ninf()) {
        st_fail(d, res, kStatusZeroMass);
        return;
    }
    const double Z = Ca + us;   // log2 alpha_{T-1}(s*), the expression gamma's alpha is formed with
    const double Zr = fb_reported_z(Cb, Ca, us);
    post_wave_sync();

    // ---- backward, a block at a time; alpha recomputed only where a query frame lies ----
    double *gn = col[0], *vn = col[1], *gc = col[2], *vc = col[3];   // G_{t+1} and its vetoable copy; scratch
    int64_t nlo = 0, nhi = 0;
    double D = 0.0, nprev = 0.0;   // D_T = 0: beta_{T-1} = {s*: 0}
    int64_t kq = (int64_t)d.K - 1;
    int64_t fq = st_frame(d, kq);
    for (int64_t k = (T - 1) / kPostCk; k >= 0; --k) {
        const int64_t t0 = k * kPostCk, t1 = (t0 + kPostCk < T) ? t0 + kPostCk : T;
        if (fq >= t0) {   // (every frame above t1 is done: fq < t1)
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
        } else {
            bw.seek(t1);   // where the recompute would have left the walk
        }
        // beta back through the block (bw walks back from t1); a query frame's row written from its cells
        float rv3 = lane < V ? d.lp[(size_t)(t1 - 1) * ld + lane] : 0.0f;
        for (int64_t t = t1 - 1; t >= t0; --t) {
            bw.prev();
            int64_t lo, hi;
            bw.band(lo, hi);
            if (lane < V) row[lane] = (double)rv3 * kLog2e64;
            if (t > t0 && lane < V) rv3 = d.lp[(size_t)(t - 1) * ld + lane];
            const bool hit = fq == t;
            const double ca = hit ? cav[t - t0] : 0.0;
            const double *al = d.slab + (t - t0) * 1024;
            float *grow = d.gamma + (size_t)(hit ? kq : 0) * (size_t)d.ld_out;
            post_wave_sync();
            const double mymax = fb_fast_bwd<M>(lo, hi, nlo, nhi, gn, vn, gc, vc, row, nprev, t == T - 1, sstar, lab_of,
                                                [&](int64_t p, int32_t, double w) {
                                                    if (hit) grow[p - lo] = st_gamma(((ca + al[p & 1023]) + (D + w)) - Z);
                                                });
            double n = post_wave_max(mymax);
            n = (n == NINF) ? 0.0 : n;
            D += n;
            nprev = n;
            { double *x = gn; gn = gc; gc = x; }
            { double *x = vn; vn = vc; vc = x; }
            nlo = lo;
            nhi = hi;
            if (hit) {
                for (int64_t j = (hi - lo) + lane; j < d.W; j += 64) grow[j] = 0.0f;
                if (lane == 0) d.band_lo[kq] = lo;
                fq = st_frame(d, --kq);
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
__global__ __launch_bounds__(64) void state_posterior_fast_kernel(const StateLattice *__restrict__ lats, int n, PostResult *res)
{
    __shared__ double col[4][1024];
    __shared__ double row[64];
    __shared__ double cav[kPostCk];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        state_fast_one<M>(lats[i], res, col, row, cav);
        post_wave_sync();
    }
}

// ---------------------------------------------------------------------------------------
// generic form: any band, any V, max_move <= 255.  One 256-thread workgroup per lattice; occ_gen_one's layout (working
// columns at absolute positions in global memory, checkpoints and slab relative to the band's low end).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void state_gen_one(const StateLattice &d, PostResult *res, double (*red)[4], double *cav)
{
    const int tid = threadIdx.x;
    const int64_t T = d.T, L = d.L, B = d.beam, V = d.V;
    const int64_t cw = d.cw;
    const size_t ld = (size_t)d.ld;
    const double NINF = post_dninf();
    if (fb_labels_bad(d)) {
        st_fail(d, res, kStatusBadLabel);
        return;
    }
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
        st_fail(d, res, post_status_of(flags));
        return;
    }
    const double us = (sstar >= plo && sstar < phi) ? prev[sstar] : NINF;
    if ((float)((Ca - Cb) + us) == post_ninf()) {
        st_fail(d, res, kStatusZeroMass);
        return;
    }
    const double Z = Ca + us;
    const double Zr = fb_reported_z(Cb, Ca, us);
    __syncthreads();

    // ---- backward, a block at a time; alpha recomputed only where a query frame lies ----
    double *gn = A[0], *vn = A[1], *gc = A[2], *vc = A[3];
    int64_t nlo = 0, nhi = 0;
    double D = 0.0, nprev = 0.0;
    int64_t kq = (int64_t)d.K - 1;
    int64_t fq = st_frame(d, kq);
    for (int64_t k = (T - 1) / kPostCk; k >= 0; --k) {
        const int64_t t0 = k * kPostCk, t1 = (t0 + kPostCk < T) ? t0 + kPostCk : T;
        if (fq >= t0) {
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
        } else {
            bw.seek(t1);
        }
        for (int64_t t = t1 - 1; t >= t0; --t) {
            bw.prev();
            int64_t lo, hi;
            bw.band(lo, hi);
            const bool hit = fq == t;
            const double ca = hit ? cav[t - t0] : 0.0;
            const double *al = d.slab + (t - t0) * cw;
            float *grow = d.gamma + (size_t)(hit ? kq : 0) * (size_t)d.ld_out;
            const double mymax = fb_gen_bwd(d, d.lp + (size_t)t * ld, lo, hi, nlo, nhi, gn, vn, gc, vc, nprev, t == T - 1, sstar,
                                            [&](int64_t p, int32_t, double w) {
                                                if (hit) grow[p - lo] = st_gamma(((ca + al[p - lo]) + (D + w)) - Z);
                                            });
            double n = post_block_max(mymax, red[ph]);   // (its barrier also orders this frame's columns before the next)
            ph ^= 1;
            n = (n == NINF) ? 0.0 : n;
            D += n;
            nprev = n;
            { double *x = gn; gn = gc; gc = x; }
            { double *x = vn; vn = vc; vc = x; }
            nlo = lo;
            nhi = hi;
            if (hit) {
                for (int64_t j = (hi - lo) + tid; j < d.W; j += 256) grow[j] = 0.0f;
                if (tid == 0) d.band_lo[kq] = lo;
                fq = st_frame(d, --kq);
            }
        }
    }
    if (tid == 0) {
        res[d.idx].status = kStatusOk;
        res[d.idx].log_likelihood = Zr;
    }
}

__global__ __launch_bounds__(256) void state_posterior_generic_kernel(const StateLattice *__restrict__ lats, int n, PostResult *res)
{
    __shared__ double red[2][4];
    __shared__ double cav[kPostCk];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        state_gen_one(lats[i], res, red, cav);
        __syncthreads();
    }
}

}  // namespace ka
