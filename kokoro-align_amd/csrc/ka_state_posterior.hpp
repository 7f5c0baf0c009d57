// ka_state_posterior.hpp — state posteriors at chosen frames: for every query frame f_k the posterior gamma_{f_k}(s) of every
// band position, over the band's paths that end at a caller-given terminal s*, and Z = alpha_{T-1}(s*).  Included by
// ka_state_posterior.hip and ka_state_posterior_banded.hip.
//
// Same lattice, band, moves, veto, statuses and form split as ka_occupancy.hpp (DESIGN.md sections 4.18 and 4.19): the
// driver of ka_fb_ck.hpp with StOut, which differs from the occupancy's policy in two ways:
//   - the backward pass recomputes alpha only for the 32-frame blocks that hold a query frame; beta is still stepped
//     through every frame (it carries from block to block), so a call costs the two passes of the path posterior plus one
//     recomputed block per query block;
//   - a query frame's cells are written, not binned: gamma_t(s) = min(1, exp2f((float)(((ca + alpha) + (D + w)) - Z))), the
//     expression and hardware exp2 that occ_fix of ka_occupancy.hpp bins, so gamma_{T-1}(s*) = 1.0 exactly and gamma summed
//     by label agrees with the occupancy to its 32.32 truncation.  Row k holds gamma_{f_k}(lo_k + j) for j in
//     [0, hi_k - lo_k) from the lanes that own the cells (coalesced), then 0.0 up to W = min(beam, L).
// Frames are ascending; the backward pass walks them from the last (kq = K-1) down.
#pragma once
#include "ka_fb_ck.hpp"

namespace ka {

// the query frame at index kq, or -1 below the first
__device__ __forceinline__ int64_t st_frame(const StateLattice &d, int64_t kq) { return kq >= 0 ? d.frames[kq] : -1; }

// fb_ck's policy; the same in both forms but for the threads a row's tail is zeroed with
template <class Form_, class Band>
struct StOut {
    using Form = Form_;
    using Desc = StateLattice;
    struct Lds {};
    static constexpr int NT = Form::NT;
    const StateLattice &d;
    int64_t kq, fq;   // the next query frame down: its index and frame
    __device__ __forceinline__ StOut(const StateLattice &d_, Form &, Lds &) : d(d_), kq((int64_t)d_.K - 1), fq(st_frame(d_, (int64_t)d_.K - 1)) {}
    // a lattice without a result: NaN rows over [0, W), band_lo -1, and the status and log-likelihood of fb_fail_result
    __device__ __forceinline__ void fail(PostResult *res, int status)
    {
        const int64_t n = (int64_t)d.K * d.W;
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
            const int64_t k = i / d.W, j = i - k * d.W;
            reinterpret_cast<uint32_t *>(d.gamma)[k * d.ld_out + j] = 0x7fc00000u;
        }
        for (int64_t k = threadIdx.x; k < d.K; k += blockDim.x) d.band_lo[k] = -1;
        fb_fail_result(d, res, status);
    }
    __device__ __forceinline__ bool recompute(int64_t t0) const { return fq >= t0; }   // (every frame above t1 is done: fq < t1)
    __device__ __forceinline__ auto cells(int64_t t, int64_t lo) const   // gamma written at a query frame, else nothing
    {
        const bool hit = fq == t;
        float *grow = d.gamma + (size_t)(hit ? kq : 0) * (size_t)d.ld_out;
        return [=](int64_t p, int32_t, auto arg) {
            if (hit) grow[p - lo] = fb_gamma(arg());
        };
    }
    __device__ __forceinline__ void cells_done() {}
    __device__ __forceinline__ void frame_end(int64_t t, int64_t lo, int64_t hi)
    {
        if (fq != t) return;
        float *grow = d.gamma + (size_t)kq * (size_t)d.ld_out;
        for (int64_t j = (hi - lo) + threadIdx.x; j < d.W; j += NT) grow[j] = 0.0f;
        if (threadIdx.x == 0) d.band_lo[kq] = lo;
        fq = st_frame(d, --kq);
    }
};

// (over a caller's table, band_lo[k] is the table's value at f_k)
template <class Band>
void launch_state_posteriors(const BandDesc<StateLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<StOut, Band>(lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
