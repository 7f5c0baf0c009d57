// ka_posterior.hpp — forward-backward over the band of align.py:64-65: the posterior of the caller's best path at every frame
// and the lattice log-likelihood.  Included by ka_posterior.hip only.
//
// What is computed, with lab'[2i] = 0, lab'[2i+1] = labels[i], L = 2S+1 and the band and moves of
// the best-path DP (the label-VALUE-0 veto of align.py:80-81 included):
//   alpha_t(s) = logsumexp_j alpha_{t-1}(s-j) + lp[t, lab'[s]]     s in band t, alpha_{-1} = {0: 0}
//   Z          = alpha_{T-1}(s*),  s* = path[T-1]
//   beta_t(s)  = logsumexp_j beta_{t+1}(s+j) + lp[t+1, lab'[s+j]]   s+j in band t+1, beta_{T-1} = {s*: 0}
//   post[t]    = exp(alpha_t(p_t) + beta_t(p_t) - Z)                 (0 where p_t is outside band t)
// Numerics: cells are float64 base-2 logs held RELATIVE to a per-frame offset, the frame's largest cell; the offsets are
// summed in double.  A linear-domain scaling would underflow the terminal of a poorly aligned chapter.  Float32 cells are not
// enough: alpha and Z come from one pass, beta from the other, and rounding that does not cancel between them grows with the
// frames behind t (1.3e-3 of a posterior at T = 8000 in a float32 build).
//   forward:  u_t(s) = lse2_j u_{t-1}(s-j) - m_{t-1} + e_t(s),  m_t = max_s u_t(s),  C_t = C_{t-1} + m_t,
//             alpha_t(s) = C_{t-1} + u_t(s)   (log2 units; m = 0 for a frame without mass)
//   backward: G_t(s) = w_t(s) + e_t(s),  n_t = max_s G_t(s),  D_t = D_{t+1} + n_t,
//             w_t(s) = lse2_j G_{t+1}(s+j) - n_{t+1},  beta_t(s) = D_{t+1} + w_t(s)
// No alpha lattice is stored: the forward pass writes alpha_t(p_t) - C_{32k-1} (k = t / 32) into the caller's posterior
// buffer as a float and C_{32k-1} into a double per 32 frames; the backward pass carries beta across the band and
// overwrites the buffer with the posterior, combining the two halves and Z in double before the one exp.
// The frame recurrences themselves are fb_fast_fwd / fb_fast_bwd and fb_gen_fwd / fb_gen_bwd of ka_posterior_common.hpp;
// the kernels here bring the label ring, the prefetches and what happens at the path.
#pragma once
#include "ka_posterior_common.hpp"

namespace ka {

// a lattice without a result: NaN posteriors, and the status and log-likelihood of fb_fail_result
__device__ __forceinline__ void post_fail(const PostLattice &d, PostResult *res, int status)
{
    uint32_t *post = reinterpret_cast<uint32_t *>(d.post);
    for (int t = threadIdx.x; t < d.T; t += blockDim.x) post[t] = 0x7fc00000u;
    fb_fail_result(d, res, status);
}

// ---------------------------------------------------------------------------------------
// fast form: one wavefront per lattice, band <= kFastMaxBand, V <= 64, M = max_move <= 4
// ---------------------------------------------------------------------------------------
// Cell k of lane l is position lo + l + 64 k (16 cells cover the widest band).  Everything a frame exchanges lives in LDS,
// addressed by slot = position & 1023 (the band is narrower than the ring, so slots never alias within a frame): the
// previous column (forward: u; backward: G and its vetoable copy), the frame's log-prob row (scaled to log2) and a ring of
// labels that is refilled, one frame ahead, as the band slides.  Global loads (the next row, the next path value, the
// labels entering the ring) are issued a frame before their use.
template <int M>
__global__ __launch_bounds__(64) void posterior_fast_kernel(const PostLattice *__restrict__ lats, PostResult *res)
{
    const PostLattice &d = lats[blockIdx.x];
    __shared__ double colA[1024], colB[1024], vetA[1024], vetB[1024];
    __shared__ double row[64];
    __shared__ int32_t ring[1024];
    const int lane = threadIdx.x;
    const int64_t T = d.T, L = d.L, B = d.beam, V = d.V;
    const double NINF = post_dninf();

    if (fb_labels_bad(d)) {
        post_fail(d, res, kStatusBadLabel);
        return;
    }
    auto lab_of = [&](int64_t p) { return fb_lab(d, p); };
    auto ring_lab = [&](int64_t p) { return ring[p & 1023]; };

    // ---- forward ----
    for (int64_t p = lane; p < (L < 1024 ? L : 1024); p += 64) ring[p] = lab_of(p);
    int64_t lfill = L < 1024 ? L : 1024;   // ring holds positions [lfill - 1024, lfill)
    if (lane == 0) colA[0] = 0.0f;         // virtual state before frame 0
    double *prev = colA, *cur = colB;
    int64_t plo = 0, phi = 1;
    BandWalk bw(L, B, T);
    double C = 0.0, Cb = 0.0;
    double mprev = 0.0;
    int flags = 0;
    float rv = lane < V ? d.lp[lane] : 0.0f;
    int32_t ptn = d.path[0];
    post_wave_sync();
    for (int64_t t = 0; t < T; ++t) {
        int64_t lo, hi;
        bw.band(lo, hi);
        // next frame's band: where the label ring has to reach
        bw.next();
        int64_t lon, hin;
        bw.band(lon, hin);
        const int64_t want = (lon + 1024 < L) ? lon + 1024 : L;
        const int64_t np = lfill + lane;
        const bool fill = np < want;
        const int32_t nlab = fill ? lab_of(np) : 0;
        if (lane < V) {
            flags |= post_bad_bits(rv);
            row[lane] = (double)rv * kLog2e64;
        }
        if (t + 1 < T && lane < V) rv = d.lp[(size_t)(t + 1) * (size_t)d.ld + lane];
        const int32_t pt = ptn;
        if (t + 1 < T) ptn = d.path[t + 1];
        flags |= (pt < 0 || pt >= L) ? 4 : 0;
        if (t % kPostCk == 0) {
            Cb = C;
            if (lane == 0) d.ck[t / kPostCk] = C;
        }
        post_wave_sync();
        const double mymax = fb_fast_fwd<M>(lo, hi, plo, phi, prev, cur, row, mprev, ring_lab, [&](int64_t p, double val) {
            if (p == pt) d.post[t] = (float)((C - Cb) + val);
        });
        if (lane == 0 && !(pt >= lo && pt < hi)) d.post[t] = post_ninf();
        double m = post_wave_max(mymax);
        m = (m == NINF) ? 0.0 : m;
        C += m;
        mprev = m;
        { double *x = prev; prev = cur; cur = x; }
        plo = lo;
        phi = hi;
        if (fill) ring[np & 1023] = nlab;
        lfill = (lfill + 64 < want) ? lfill + 64 : (want > lfill ? want : lfill);
        for (int64_t p = lfill + lane; lfill < want; p = lfill + lane) {   // the band jumped more than 64 positions (L > 64 T)
            if (p < want) ring[p & 1023] = lab_of(p);
            lfill = (lfill + 64 < want) ? lfill + 64 : want;
        }
        post_wave_sync();
    }
    flags = post_block_flags(flags);
    if (flags) {
        post_fail(d, res, post_status_of(flags));
        return;
    }
    // ---- Z ----
    const int64_t tl = T - 1;
    const double cbl = d.ck[tl / kPostCk];
    const float dl = d.post[tl];
    const int32_t sstar = d.path[tl];
    if (dl == post_ninf()) {
        post_fail(d, res, kStatusZeroMass);
        return;
    }
    const double Z = cbl + (double)dl;
    post_wave_sync();
    // ---- backward ----
    // frame T-1: G = e at s* (beta = 0 there), -inf elsewhere
    if (lane < V) row[lane] = (double)d.lp[(size_t)tl * (size_t)d.ld + lane] * kLog2e64;
    post_wave_sync();
    int64_t nlo = plo, nhi = phi;          // band of frame t+1
    double *gn = colA, *gc = colB, *vn = vetA, *vc = vetB;
    for (int64_t p = nlo + lane; p < nhi; p += 64) {
        const int32_t lab = ring[p & 1023];
        const double g = (p == sstar) ? row[lab] : NINF;
        gn[p & 1023] = g;
        vn[p & 1023] = lab == 0 ? NINF : g;
    }
    const double nT = row[ring[sstar & 1023]];
    double nprev = nT;
    double D = nT;
    if (lane == 0) d.post[tl] = 1.0f;
    // the ring holds [lbot, lbot + 1024) from here on; frame T-2 must find its band in it
    int64_t lbot = lfill - 1024 > 0 ? lfill - 1024 : 0;
    bw.prev();                              // bw was one frame past the end
    bw.prev();                              // frame T-2
    {
        int64_t lo, hi;
        bw.band(lo, hi);
        for (int64_t p = lo + lane; p < lbot && p < lo + 1024; p += 64) ring[p & 1023] = lab_of(p);
        if (lo < lbot) lbot = lo;
    }
    if (T >= 2) {
        rv = lane < V ? d.lp[(size_t)(T - 2) * (size_t)d.ld + lane] : 0.0f;
        ptn = d.path[T - 2];
    }
    float dtn = T >= 2 ? d.post[T - 2] : 0.0f;
    post_wave_sync();
    for (int64_t t = T - 2; t >= 0; --t) {
        int64_t lo, hi;
        bw.band(lo, hi);
        bw.prev();
        int64_t lon = 0, hin = 0;
        if (t >= 1) bw.band(lon, hin);
        const int64_t np = lbot - 1 - lane;
        const bool fill = t >= 1 && np >= lon;
        const int32_t nlab = fill ? lab_of(np) : 0;
        if (lane < V) row[lane] = (double)rv * kLog2e64;
        if (t >= 1 && lane < V) rv = d.lp[(size_t)(t - 1) * (size_t)d.ld + lane];
        const int32_t pt = ptn;
        const float dt = dtn;
        if (t >= 1) {
            ptn = d.path[t - 1];
            dtn = d.post[t - 1];
        }
        const double cb = d.ck[t / kPostCk];
        post_wave_sync();
        const double mymax = fb_fast_bwd<M>(lo, hi, nlo, nhi, gn, vn, gc, vc, row, nprev, false, 0, ring_lab,
                                            [&](int64_t p, int32_t, double w) {
                                                if (p == pt) d.post[t] = post_value(cb, dt, D, w, Z);
                                            });
        if (lane == 0 && !(pt >= lo && pt < hi)) d.post[t] = 0.0f;
        double n = post_wave_max(mymax);
        n = (n == NINF) ? 0.0 : n;
        D += n;
        nprev = n;
        { double *x = gn; gn = gc; gc = x; }
        { double *x = vn; vn = vc; vc = x; }
        nlo = lo;
        nhi = hi;
        if (fill) ring[np & 1023] = nlab;
        if (t >= 1) {
            lbot = (lbot - 64 > lon) ? lbot - 64 : (lon < lbot ? lon : lbot);
            for (int64_t p = lbot - 1 - lane; lbot > lon; p = lbot - 1 - lane) {   // the band jumped more than 64 positions
                if (p >= lon) ring[p & 1023] = lab_of(p);
                lbot = (lbot - 64 > lon) ? lbot - 64 : lon;
            }
        }
        post_wave_sync();
    }
    if (lane == 0) {
        res[d.idx].status = kStatusOk;
        res[d.idx].log_likelihood = Z * kLn2;
    }
}

// ---------------------------------------------------------------------------------------
// generic form: any band, any V, max_move <= 255.  One 256-thread workgroup per lattice, the columns in global memory
// (absolute positions, L2-resident), labels and emissions read where they lie.  A correctness path, not tuned.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void posterior_generic_kernel(const PostLattice *__restrict__ lats, PostResult *res)
{
    const PostLattice &d = lats[blockIdx.x];
    __shared__ double red[2][4];
    const int tid = threadIdx.x;
    const int64_t T = d.T, L = d.L, B = d.beam, V = d.V;
    const double NINF = post_dninf();
    if (fb_labels_bad(d)) {
        post_fail(d, res, kStatusBadLabel);
        return;
    }
    double *A0 = d.col, *A1 = d.col + L, *V0 = d.col + 2 * L, *V1 = d.col + 3 * L;

    // ---- forward ----
    if (tid == 0) A0[0] = 0.0;
    double *prev = A0, *cur = A1;
    int64_t plo = 0, phi = 1;
    BandWalk bw(L, B, T);
    double C = 0.0, Cb = 0.0;
    double mprev = 0.0;
    int flags = 0;
    __syncthreads();
    for (int64_t t = 0; t < T; ++t) {
        int64_t lo, hi;
        bw.band(lo, hi);
        const float *lrow = d.lp + (size_t)t * (size_t)d.ld;
        for (int64_t v = tid; v < V; v += 256) flags |= post_bad_bits(lrow[v]);
        const int32_t pt = d.path[t];
        flags |= (pt < 0 || pt >= L) ? 4 : 0;
        if (t % kPostCk == 0) {
            Cb = C;
            if (tid == 0) d.ck[t / kPostCk] = C;
        }
        const double mymax = fb_gen_fwd(d, lrow, lo, hi, plo, phi, prev, cur, mprev, [&](int64_t p, double val) {
            if (p == pt) d.post[t] = (float)((C - Cb) + val);
        });
        if (tid == 0 && !(pt >= lo && pt < hi)) d.post[t] = post_ninf();
        double m = post_block_max(mymax, red[t & 1]);
        m = (m == NINF) ? 0.0 : m;
        C += m;
        mprev = m;
        { double *x = prev; prev = cur; cur = x; }
        plo = lo;
        phi = hi;
        bw.next();
    }
    flags = post_block_flags(flags);
    if (flags) {
        post_fail(d, res, post_status_of(flags));
        return;
    }
    const int64_t tl = T - 1;
    const double cbl = d.ck[tl / kPostCk];
    const float dl = d.post[tl];
    const int32_t sstar = d.path[tl];
    if (dl == post_ninf()) {
        post_fail(d, res, kStatusZeroMass);
        return;
    }
    const double Z = cbl + (double)dl;
    __syncthreads();

    // ---- backward ----
    int64_t nlo = plo, nhi = phi;
    double *gn = A0, *gc = A1, *vn = V0, *vc = V1;
    const double nT = (double)d.lp[(size_t)tl * (size_t)d.ld + fb_lab(d, sstar)] * kLog2e64;
    for (int64_t p = nlo + tid; p < nhi; p += 256) {
        const double g = (p == sstar) ? nT : NINF;
        gn[p] = g;
        vn[p] = fb_lab(d, p) == 0 ? NINF : g;
    }
    double nprev = nT;
    double D = nT;
    if (tid == 0) d.post[tl] = 1.0f;
    bw.prev();   // bw was one frame past the end
    bw.prev();   // frame T-2
    __syncthreads();
    for (int64_t t = T - 2; t >= 0; --t) {
        int64_t lo, hi;
        bw.band(lo, hi);
        const float *lrow = d.lp + (size_t)t * (size_t)d.ld;
        const int32_t pt = d.path[t];
        const float dt = d.post[t];
        const double cb = d.ck[t / kPostCk];
        __syncthreads();   // (every thread has read post[t] before its owner overwrites it)
        const double mymax = fb_gen_bwd(d, lrow, lo, hi, nlo, nhi, gn, vn, gc, vc, nprev, false, 0, [&](int64_t p, int32_t, double w) {
            if (p == pt) d.post[t] = post_value(cb, dt, D, w, Z);
        });
        if (tid == 0 && !(pt >= lo && pt < hi)) d.post[t] = 0.0f;
        double n = post_block_max(mymax, red[t & 1]);
        n = (n == NINF) ? 0.0 : n;
        D += n;
        nprev = n;
        { double *x = gn; gn = gc; gc = x; }
        { double *x = vn; vn = vc; vc = x; }
        nlo = lo;
        nhi = hi;
        bw.prev();
    }
    if (tid == 0) {
        res[d.idx].status = kStatusOk;
        res[d.idx].log_likelihood = Z * kLn2;
    }
}

}  // namespace ka
