// ka_posterior.hpp — forward-backward over the band of align.py:64-65: the posterior of the caller's best path at every frame
// and the lattice log-likelihood.  Included by ka_posterior.hip and ka_posterior_banded.hip.
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
// One pass, posterior_lattice<Form, Band>, behind one kernel, posterior_kernel<Form, Band> (BandWalk: the reference's diagonal
// band; BandTable: a caller's table, on Banded<PostLattice> descriptors), over the form policy of ka_fb_form.hpp on a PostLattice: the fast form with the label
// ring (PostFast<M>) and the generic form (PostGen).  The form brings the threads, the columns, the row, the labels and the
// frame recurrences; the kernel brings the band walk, the path prefetches and what happens at the path.
#pragma once
#include "ka_fb_form.hpp"

namespace ka {

// a lattice without a result: NaN posteriors, and the status and log-likelihood of fb_fail_result
__device__ __forceinline__ void post_fail(const PostLattice &d, PostResult *res, int status)
{
    uint32_t *post = reinterpret_cast<uint32_t *>(d.post);
    for (int t = threadIdx.x; t < d.T; t += blockDim.x) post[t] = 0x7fc00000u;
    fb_fail_result(d, res, status);
}

template <int M>
using PostFast = FbFast<M, PostLattice, LabRing>;
using PostGen = FbGen<PostLattice>;

// One workgroup per lattice.  Global loads (the next row, the next path value, the next stored alpha, the labels entering the
// ring) are issued a frame before their use.
// Band: the band (BandWalk, or BandTable of ka_posterior_common.hpp on `tab`, the caller's table).
template <class Form, class Band>
__device__ __forceinline__ void posterior_lattice(const PostLattice &d, typename Form::template Shared<4> &sh, const int32_t *tab, PostResult *res)
{
    Form f(d, sh);
    const int tid = threadIdx.x;
    const int64_t T = d.T, L = d.L;
    const double NINF = post_dninf();
    if (fb_labels_bad(d)) {
        post_fail(d, res, kStatusBadLabel);
        return;
    }

    // ---- forward ----
    f.lab.fill();
    double *prev = f.col(0), *cur = f.col(1);
    if (tid == 0) prev[0] = 0.0;   // virtual state before frame 0
    int64_t plo = 0, phi = 1;
    Band bw(L, d.beam, T, tab);
    if (!bw.start()) {   // (a caller's table that is no band: before any of its values places a cell)
        post_fail(d, res, kStatusBadArgs);
        return;
    }
    double C = 0.0, Cb = 0.0, mprev = 0.0;
    int flags = 0;
    f.row_prefetch(0);
    int32_t ptn = d.path[0];
    f.sync();
    for (int64_t t = 0; t < T; ++t) {
        int64_t lo, hi, lon, hin;
        bw.band(lo, hi);
        bw.next();
        bw.band(lon, hin);
        f.lab.fwd_request(lon);
        flags |= f.row(t, t + 1, t + 1 < T, true);
        const int32_t pt = ptn;
        if (t + 1 < T) ptn = d.path[t + 1];
        flags |= (pt < 0 || pt >= L) ? 4 : 0;
        if (t % kPostCk == 0) {
            Cb = C;
            if (tid == 0) d.ck[t / kPostCk] = C;
        }
        f.fence();
        const double mymax = f.fwd(lo, hi, plo, phi, prev, cur, mprev, [&](int64_t p, double val) {
            if (p == pt) d.post[t] = (float)((C - Cb) + val);
        });
        if (tid == 0 && !(pt >= lo && pt < hi)) d.post[t] = post_ninf();
        double m = f.max(mymax);
        m = (m == NINF) ? 0.0 : m;
        C += m;
        mprev = m;
        { double *x = prev; prev = cur; cur = x; }
        plo = lo;
        phi = hi;
        f.lab.fwd_commit();
        f.fence();
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
    f.sync();   // every thread has read post[T-1] before post_fail or frame T-1 overwrites it
    if (dl == post_ninf()) {
        post_fail(d, res, kStatusZeroMass);
        return;
    }
    const double Z = cbl + (double)dl;

    // ---- backward ----
    // Frame T-1 runs as `last`: w = 0 at s*, so its posterior is 2^((cbl + dl) + (0 + 0) - Z) = 1 exactly.
    // post[t] is read a frame ahead (dtn), before the barrier of frame t+1's reduction in the generic form (post[T-1] before the
    // one above), and overwritten by the cell's owner or by thread 0 behind that barrier: the writers need no barrier of their own.
    double *gn = f.col(0), *gc = f.col(1), *vn = f.col(2), *vc = f.col(3);   // G_{t+1} and its vetoable copy; frame t's
    int64_t nlo = 0, nhi = 0;
    double D = 0.0, nprev = 0.0;   // D_T = 0: beta_{T-1} = {s*: 0}
    bw.prev();                     // bw was one frame past the end
    f.lab.turn(plo);
    f.row_prefetch(tl);
    ptn = sstar;
    float dtn = dl;
    f.sync();
    for (int64_t t = tl; t >= 0; --t) {
        int64_t lo, hi, lon = 0, hin = 0;
        bw.band(lo, hi);
        bw.prev();
        if (t >= 1) bw.band(lon, hin);
        f.lab.bwd_request(lon, t >= 1);
        f.row(t, t - 1, t >= 1);
        const int32_t pt = ptn;
        const float dt = dtn;
        if (t >= 1) {
            ptn = d.path[t - 1];
            dtn = d.post[t - 1];
        }
        const double cb = d.ck[t / kPostCk];
        f.fence();
        auto cell = [&](int64_t p, int32_t, double w) {
            if (p == pt) d.post[t] = post_value(cb, dt, D, w, Z);
        };
        // (two calls, so that `last` is a constant of the cell loop: as a variable it costs every cell two scalar branches)
        const double mymax = (t == tl) ? f.bwd(lo, hi, nlo, nhi, gn, vn, gc, vc, nprev, true, sstar, cell)
                                       : f.bwd(lo, hi, nlo, nhi, gn, vn, gc, vc, nprev, false, sstar, cell);
        if (tid == 0 && !(pt >= lo && pt < hi)) d.post[t] = 0.0f;
        double n = f.max(mymax);
        n = (n == NINF) ? 0.0 : n;
        D += n;
        nprev = n;
        { double *x = gn; gn = gc; gc = x; }
        { double *x = vn; vn = vc; vc = x; }
        nlo = lo;
        nhi = hi;
        f.lab.bwd_commit();
        f.fence();
    }
    if (tid == 0) {
        res[d.idx].status = kStatusOk;
        res[d.idx].log_likelihood = Z * kLn2;
    }
}

template <class Form, class Band>
__global__ __launch_bounds__(Form::NT) void posterior_kernel(const BandDesc<PostLattice, Band> *__restrict__ lats, PostResult *res)
{
    const BandDesc<PostLattice, Band> &d = lats[blockIdx.x];
    __shared__ typename Form::template Shared<4> sh;
    posterior_lattice<Form, Band>(d, sh, fb_table(d), res);
}

// descriptors [0, n_fast) in the fast form (fast[M - 1], M = max_move, 4 above 3), then n_generic in the generic form; one
// workgroup per lattice
template <class Band>
void launch_posteriors(const BandDesc<PostLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    using Kernel = void (*)(const BandDesc<PostLattice, Band> *, PostResult *);
    static constexpr Kernel fast[4] = {posterior_kernel<PostFast<1>, Band>, posterior_kernel<PostFast<2>, Band>, posterior_kernel<PostFast<3>, Band>,
                                       posterior_kernel<PostFast<4>, Band>};
    if (n_fast > 0)
        hipLaunchKernelGGL(fast[(max_move >= 1 && max_move <= 3 ? max_move : 4) - 1], dim3(n_fast), dim3(PostFast<1>::NT), 0, s, lats, res);
    if (n_generic > 0) hipLaunchKernelGGL((posterior_kernel<PostGen, Band>), dim3(n_generic), dim3(PostGen::NT), 0, s, lats + n_fast, res);
}

}  // namespace ka
