// ka_fb_ck.hpp — the checkpointed forward-backward that ka_occupancy.hpp (label occupancy), ka_state_posterior.hpp (state
// posteriors at chosen frames) and ka_duration.hpp (expected state durations) share, and whose forward half ka_sample.hpp
// (sampled alignments) reuses: one driver per form (fb_ck_fast<M, Out>, fb_ck_gen<Out>) and their launch.
//
// The posterior kernels keep alpha only at the path; these calls need it at band cells, so the forward pass checkpoints the
// whole column before the first frame of every 32-frame block (with the offset C and the frame maximum m it runs on), and the
// backward pass, last block first, recomputes a block's alpha from its checkpoint into a per-slot slab with the forward
// pass's own frame function (fb_fast_fwd / fb_gen_fwd of ka_posterior_common.hpp), then steps beta back through the block
// (fb_fast_bwd / fb_gen_bwd).  The recompute runs the same instructions on the same operands: its alpha is the forward
// pass's bit for bit, so gamma at (T-1, s*) is 2^0 exactly.  A cell's gamma is 2^arg, arg = ((ca + alpha) + (D + w)) - Z.
//
// The kernel's policy Out holds its outputs and has a hook for each place where the two calls differ:
//   fail(res, status)            a lattice without a result: fill the outputs with NaN, then fb_fail_result
//   recompute(t0)                recompute the block that starts at t0?  (if not, the walk is re-seated at t1, where the
//                                recompute would have left it; beta is still stepped through every frame)
//   cells(t, lo)                 frame t's action on a cell's gamma: a callable (p, lab, arg), arg() the log2 argument, formed
//                                only when called (asked for once a frame, before the frame's first cell and the fence in front of it)
//   cells_done(), frame_end(t, lo, hi)   after the frame's cells (before its reduction), and after its bookkeeping (before the
//                                fast form's end-of-frame fence); a hook owns any barrier or fence that only its kernel needs
// The forward pass and the recompute of a block are functions of their own (fb_ck_fast_forward / fb_ck_fast_recompute,
// fb_ck_gen_forward / fb_ck_gen_recompute): the drivers here call them, and so does the path sampler (ka_sample.hpp), which
// needs alpha and no beta.
// Storage: lattices walk slots (launch grid = slots, lattice i on slot i mod grid), so the workspace is bounded by the slots,
// not by the batch.
#pragma once
#include "ka_posterior_common.hpp"

namespace ka {

// one cell's gamma as a float from its log2 argument (occ_fix of ka_occupancy.hpp before the fixed-point step): what the state
// posteriors write and the state durations add
__device__ __forceinline__ float fb_gamma(double arg)
{
    const float g = __builtin_amdgcn_exp2f((float)arg);
    return g < 1.0f ? g : 1.0f;
}

// ---------------------------------------------------------------------------------------
// fast form: one wavefront per lattice, band <= kFastMaxBand, V <= 64, M = max_move <= 4; the cell layout of
// posterior_fast_kernel (position p at slot p & 1023 of an LDS column; lane l owns lo + l + 64 k).  The forward pass and
// the recompute both run fb_fast_fwd with the same label source, so the two produce the same bits.
// ---------------------------------------------------------------------------------------
// The forward pass of the fast form: label check, alpha through every frame with a checkpoint before every block, the flag,
// terminal and zero-mass checks, Z (log2 alpha_{T-1}(s*), the expression gamma's alpha is formed with) and Zr (fb_reported_z).
// Returns kStatusOk or the status the lattice fails with; col[0] / col[1] are its working columns, bw ends at frame T.
template <int M, class LabOf>
__device__ __forceinline__ int fb_ck_fast_forward(const FbCkLattice &d, double (*col)[1024], double *row, BandWalk &bw, LabOf lab_of,
                                                  double &Z, double &Zr)
{
    const int lane = threadIdx.x;
    const int64_t T = d.T, L = d.L, V = d.V;
    const size_t ld = (size_t)d.ld;
    const double NINF = post_dninf();
    if (fb_labels_bad(d)) return kStatusBadLabel;
    auto no_cell = [](int64_t, double) {};
    double *prev = col[0], *cur = col[1];
    if (lane == 0) prev[0] = 0.0;   // virtual state before frame 0
    int64_t plo = 0, phi = 1;
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
    if (flags) return post_status_of(flags);
    const double us = (sstar >= plo && sstar < phi) ? prev[sstar & 1023] : NINF;
    if ((float)((Ca - Cb) + us) == post_ninf()) return kStatusZeroMass;
    Z = Ca + us;
    Zr = fb_reported_z(Cb, Ca, us);
    post_wave_sync();
    return kStatusOk;
}

// The recompute of block k = [t0, t1): alpha from the block's checkpoint into the slab (row t - t0, slot = position & 1023) with
// the forward pass's frame function on the forward pass's operands, pv / cu the working columns; note(t - t0, C) is handed
// every frame's offset before the frame runs.  bw ends at frame t1.  A cell's slab entry is written by the lane that owns
// the cell in that frame (lane (p - lo_t) & 63).
template <int M, class LabOf, class Note>
__device__ __forceinline__ void fb_ck_fast_recompute(const FbCkLattice &d, int64_t k, int64_t t0, int64_t t1, BandWalk &bw, double *pv,
                                                     double *cu, double *row, LabOf lab_of, Note note)
{
    const int lane = threadIdx.x;
    const int64_t V = d.V;
    const size_t ld = (size_t)d.ld;
    const double NINF = post_dninf();
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
        note(t - t0, C2);
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
}

template <int M, class Out>
__device__ __forceinline__ void fb_ck_fast(const FbCkLattice &d, PostResult *res, double (*col)[1024], double *row, double *cav, Out &out)
{
    const int lane = threadIdx.x;
    const int64_t T = d.T, V = d.V;
    const size_t ld = (size_t)d.ld;
    const double NINF = post_dninf();
    auto lab_of = [&](int64_t p) { return fb_lab(d, p); };

    // ---- forward: Z, and a checkpoint before every block ----
    BandWalk bw(d.L, d.beam, T);
    double Z, Zr;
    const int status = fb_ck_fast_forward<M>(d, col, row, bw, lab_of, Z, Zr);
    if (status != kStatusOk) {
        out.fail(res, status);
        return;
    }
    const int64_t sstar = d.terminal;

    // ---- backward, a block at a time ----
    double *gn = col[0], *vn = col[1], *gc = col[2], *vc = col[3];   // G_{t+1} and its vetoable copy; scratch
    int64_t nlo = 0, nhi = 0;
    double D = 0.0, nprev = 0.0;   // D_T = 0: beta_{T-1} = {s*: 0}
    for (int64_t k = (T - 1) / kPostCk; k >= 0; --k) {
        const int64_t t0 = k * kPostCk, t1 = (t0 + kPostCk < T) ? t0 + kPostCk : T;
        if (out.recompute(t0)) {   // alpha over [t0, t1) into the slab, gc / vc as the working columns
            fb_ck_fast_recompute<M>(d, k, t0, t1, bw, gc, vc, row, lab_of, [&](int64_t f, double c) {
                if (lane == 0) cav[f] = c;
            });
        } else {
            bw.seek(t1);
        }
        // beta back through the block (bw walks back from t1)
        float rv3 = lane < V ? d.lp[(size_t)(t1 - 1) * ld + lane] : 0.0f;
        for (int64_t t = t1 - 1; t >= t0; --t) {
            bw.prev();
            int64_t lo, hi;
            bw.band(lo, hi);
            if (lane < V) row[lane] = (double)rv3 * kLog2e64;
            if (t > t0 && lane < V) rv3 = d.lp[(size_t)(t - 1) * ld + lane];
            const double ca = cav[t - t0];
            const double *al = d.slab + (t - t0) * 1024;
            auto cell = out.cells(t, lo);
            post_wave_sync();
            const double mymax = fb_fast_bwd<M>(lo, hi, nlo, nhi, gn, vn, gc, vc, row, nprev, t == T - 1, sstar, lab_of,
                                                [&](int64_t p, int32_t lab, double w) {
                                                    cell(p, lab, [&] { return ((ca + al[p & 1023]) + (D + w)) - Z; });
                                                });
            out.cells_done();
            double n = post_wave_max(mymax);
            n = (n == NINF) ? 0.0 : n;
            D += n;
            nprev = n;
            { double *x = gn; gn = gc; gc = x; }
            { double *x = vn; vn = vc; vc = x; }
            nlo = lo;
            nhi = hi;
            out.frame_end(t, lo, hi);
            post_wave_sync();
        }
    }
    if (lane == 0) {
        res[d.idx].status = kStatusOk;
        res[d.idx].log_likelihood = Zr;
    }
}

// ---------------------------------------------------------------------------------------
// generic form: any band, any V, max_move <= 255.  One 256-thread workgroup per lattice, working columns at absolute
// positions in global memory, checkpoints and slab relative to the band's low end.  A correctness path, not tuned.
// ---------------------------------------------------------------------------------------
// The generic form's forward pass and block recompute: the contracts of fb_ck_fast_forward / fb_ck_fast_recompute, with the
// working columns (prev / cur, pv / cu) at absolute positions in global memory, ph the parity of the reduction slots, and the
// slab relative to each frame's low end.  The forward pass ends behind a barrier, and so does the recompute.
__device__ __forceinline__ int fb_ck_gen_forward(const FbCkLattice &d, double *prev, double *cur, double (*red)[4], int &ph, BandWalk &bw,
                                                 double &Z, double &Zr)
{
    const int tid = threadIdx.x;
    const int64_t T = d.T, L = d.L, V = d.V;
    const int64_t cw = d.cw;
    const size_t ld = (size_t)d.ld;
    const double NINF = post_dninf();
    if (fb_labels_bad(d)) return kStatusBadLabel;
    auto no_cell = [](int64_t, double) {};
    if (tid == 0) prev[0] = 0.0;
    int64_t plo = 0, phi = 1;
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
    if (flags) return post_status_of(flags);
    const double us = (sstar >= plo && sstar < phi) ? prev[sstar] : NINF;
    if ((float)((Ca - Cb) + us) == post_ninf()) return kStatusZeroMass;
    Z = Ca + us;
    Zr = fb_reported_z(Cb, Ca, us);
    __syncthreads();
    return kStatusOk;
}

template <class Note>
__device__ __forceinline__ void fb_ck_gen_recompute(const FbCkLattice &d, int64_t k, int64_t t0, int64_t t1, BandWalk &bw, double *pv,
                                                    double *cu, double (*red)[4], int &ph, Note note)
{
    const int tid = threadIdx.x;
    const int64_t cw = d.cw;
    const size_t ld = (size_t)d.ld;
    const double NINF = post_dninf();
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
        note(t - t0, C2);
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
}

template <class Out>
__device__ __forceinline__ void fb_ck_gen(const FbCkLattice &d, PostResult *res, double (*red)[4], double *cav, Out &out)
{
    const int tid = threadIdx.x;
    const int64_t T = d.T, L = d.L;
    const int64_t cw = d.cw;
    const size_t ld = (size_t)d.ld;
    const double NINF = post_dninf();
    double *A[4] = {d.col, d.col + L, d.col + 2 * L, d.col + 3 * L};
    int ph = 0;   // parity of the reduction slots

    // ---- forward ----
    BandWalk bw(L, d.beam, T);
    double Z, Zr;
    const int status = fb_ck_gen_forward(d, A[0], A[1], red, ph, bw, Z, Zr);
    if (status != kStatusOk) {
        out.fail(res, status);
        return;
    }
    const int64_t sstar = d.terminal;

    // ---- backward, a block at a time ----
    double *gn = A[0], *vn = A[1], *gc = A[2], *vc = A[3];
    int64_t nlo = 0, nhi = 0;
    double D = 0.0, nprev = 0.0;
    for (int64_t k = (T - 1) / kPostCk; k >= 0; --k) {
        const int64_t t0 = k * kPostCk, t1 = (t0 + kPostCk < T) ? t0 + kPostCk : T;
        if (out.recompute(t0)) {
            fb_ck_gen_recompute(d, k, t0, t1, bw, gc, vc, red, ph, [&](int64_t f, double c) {
                if (tid == 0) cav[f] = c;
            });
        } else {
            bw.seek(t1);
        }
        for (int64_t t = t1 - 1; t >= t0; --t) {
            bw.prev();
            int64_t lo, hi;
            bw.band(lo, hi);
            const double ca = cav[t - t0];
            const double *al = d.slab + (t - t0) * cw;
            auto cell = out.cells(t, lo);
            const double mymax = fb_gen_bwd(d, d.lp + (size_t)t * ld, lo, hi, nlo, nhi, gn, vn, gc, vc, nprev, t == T - 1, sstar,
                                            [&](int64_t p, int32_t lab, double w) {
                                                cell(p, lab, [&] { return ((ca + al[p - lo]) + (D + w)) - Z; });
                                            });
            out.cells_done();
            double n = post_block_max(mymax, red[ph]);   // (its barrier also closes the frame's cells before frame_end)
            ph ^= 1;
            n = (n == NINF) ? 0.0 : n;
            D += n;
            nprev = n;
            { double *x = gn; gn = gc; gc = x; }
            { double *x = vn; vn = vc; vc = x; }
            nlo = lo;
            nhi = hi;
            out.frame_end(t, lo, hi);
        }
    }
    if (tid == 0) {
        res[d.idx].status = kStatusOk;
        res[d.idx].log_likelihood = Zr;
    }
}

// the launch of either call: descriptors [0, n_fast) on min(n_fast, kOccFastSlots) one-wavefront workgroups (fast[M - 1],
// M = max_move, 4 above 3), lattice i on workgroup i mod grid (its slot); then [n_fast, n_fast + n_generic) on
// min(n_generic, kOccGenericSlots) 256-thread workgroups
template <class Desc>
using FbCkKernel = void (*)(const Desc *, int, PostResult *);
template <class Desc>
void launch_fb_ck(const FbCkKernel<Desc> (&fast)[4], FbCkKernel<Desc> generic, const Desc *lats, int n_fast, int n_generic, int max_move,
                  PostResult *res, hipStream_t s)
{
    if (n_fast > 0) {
        const dim3 grid(n_fast < kOccFastSlots ? n_fast : kOccFastSlots);
        hipLaunchKernelGGL(fast[(max_move >= 1 && max_move <= 3 ? max_move : 4) - 1], grid, dim3(64), 0, s, lats, n_fast, res);
    }
    if (n_generic > 0) {
        const dim3 grid(n_generic < kOccGenericSlots ? n_generic : kOccGenericSlots);
        hipLaunchKernelGGL(generic, grid, dim3(256), 0, s, lats + n_fast, n_generic, res);
    }
}

}  // namespace ka
