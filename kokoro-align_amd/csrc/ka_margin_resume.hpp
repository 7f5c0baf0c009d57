// ka_margin_resume.hpp — best-path margins under the caller's boundary conditions, and rows of max-marginals at chosen frames
// (ka_ctc_margins_resume_*).  Included by ka_margin_resume.hip only.
//
// margin_lattice (ka_margin.hpp) with the policy MgResume on a MarginResumeLattice: the row before frame 0 (d_in = D_{-1}) and
// the row at frame T-1 (e_in = E_{T-1}) come from the caller, and the two rows a neighbouring chunk needs go back (d_out =
// D_{T-1} over band T-1; e_out = the E of the row before frame 0).  The max-plus recurrence composes across a cut exactly: with
// chunk B's d_in = chunk A's d_out and A's e_in = B's e_out, every D, E and m of either chunk has the uncut lattice's bits,
// because every value is formed by the same adds and maxima of the same operands.
//   place     d_in over [lo_0 - (M-1), hi_0) into the column (no band applies to the row before frame 0; at most 1009 + 3 cells,
//             which fit the fast form's 1024 slots), or the virtual state {0: 0.0}.  Called by the forward pass and again by the
//             recompute of block 0, which therefore has no checkpoint.
//   finish    the rows' bits (a NaN or +inf anywhere in either row, read or not, is kStatusBadArgs), the terminal, the score
//             max over band T-1 of D + E (D at the terminal without e_in: the sibling's value), d_out
//   stores, block   which blocks keep a checkpoint and have their D recomputed: all of them if through, alt or runner_up is
//             asked for, else those that hold a query frame
//   query, row_done   rows[k] = m_{f_k} over band f_k from column 0, -inf behind it up to W; rows_lo[k] = lo
//   before    behind frame 0: e_out[p] = max_j G_0(p+j), p+j in band 0, a skip into a label VALUE 0 barred (the vetoable copy)
// Nothing here is read by ka_ctc_path_margins' kernels: MgPlain keeps their lines.
#pragma once
#include "ka_fb_resume.hpp"
#include "ka_margin.hpp"

namespace ka {

template <class Form>
struct MgResume {
    static constexpr bool kPlain = false;
    static constexpr int NT = Form::NT;
    const MarginResumeLattice &d;
    int32_t qf, qb;   // the query cursors: the first frame not yet passed by the forward pass, the last not yet met going back
    __device__ __forceinline__ explicit MgResume(const MarginResumeLattice &d_) : d(d_), qf(0), qb(d_.K - 1) {}

    __device__ __forceinline__ int moves() const
    {
        if constexpr (Form::kWave) return Form::kMoves;
        else return d.max_move;
    }
    __device__ __forceinline__ bool path_out() const { return d.through || d.alt || d.runner; }
    __device__ __forceinline__ bool backward() const { return path_out() || d.K > 0 || d.e_out; }
    // going back: nothing is left to do once the earliest query frame is behind, unless a value of every frame is asked for
    __device__ __forceinline__ bool done() const { return !path_out() && !d.e_out && qb < 0; }

    // a lattice without a result: NaN over every requested float output, rows included; -1 over runner_up and rows_lo
    __device__ __forceinline__ void fail(PostResult *res, int status) const
    {
        uint64_t *th = reinterpret_cast<uint64_t *>(d.through), *al = reinterpret_cast<uint64_t *>(d.alt);
        for (int64_t t = threadIdx.x; t < d.T; t += blockDim.x) {
            if (th) th[t] = kNaN64;
            if (al) al[t] = kNaN64;
            if (d.runner) d.runner[t] = -1;
        }
        for (int64_t k = 0; k < d.K; ++k) {
            fb_nan_row(d.rows + k * d.ld_rows, d.W);
            if (threadIdx.x == 0) d.rows_lo[k] = -1;
        }
        fb_nan_row(d.d_out, d.L);
        fb_nan_row(d.e_out, d.L);
        fb_fail_result(d, res, status);
    }

    // the row before frame 0 into `col` over [plo, phi); bw stands at frame 0.  Ends in no barrier: both callers synchronise
    // before frame 0
    template <class Band>
    __device__ __forceinline__ void place(const Band &bw, double *col, int64_t &plo, int64_t &phi) const
    {
        plo = 0;
        phi = 1;
        if (!d.d_in) {
            if (threadIdx.x == 0) col[0] = 0.0;
            return;
        }
        int64_t lo, hi;
        bw.band(lo, hi);
        const int64_t wlo = lo - (moves() - 1) > 0 ? lo - (moves() - 1) : 0;
        for (int64_t p = wlo + threadIdx.x; p < hi; p += NT) col[Form::cslot(p)] = d.d_in[p];
        plo = wlo;
        phi = hi;
    }

    // does the forward pass keep the column before block k?
    __device__ __forceinline__ bool stores(int64_t k)
    {
        if (k == 0) return false;
        if (path_out()) return true;
        while (qf < d.K && d.frames[qf] < k * kPostCk) ++qf;
        return qf < d.K && d.frames[qf] < (k + 1) * kPostCk;
    }
    // going back: is the D of block [t0, t1) asked for?
    __device__ __forceinline__ bool block(int64_t t0, int64_t) const { return path_out() || (qb >= 0 && d.frames[qb] >= t0); }
    __device__ __forceinline__ double *query(int64_t t) const { return (qb >= 0 && d.frames[qb] == t) ? d.rows + (int64_t)qb * d.ld_rows : nullptr; }
    __device__ __forceinline__ void row_done(double *row, int64_t lo, int64_t hi)
    {
        const double NINF = post_dninf();
        for (int64_t j = hi - lo + threadIdx.x; j < d.W; j += NT) row[j] = NINF;
        if (threadIdx.x == 0) d.rows_lo[qb] = lo;
        --qb;
    }

    // the end of the forward pass, prev = D_{T-1} over band T-1 = [plo, phi)
    template <class Red>
    __device__ __forceinline__ int finish(Form &f, Red &red, const double *prev, int64_t plo, int64_t phi, int flags, int64_t &sstar,
                                          double &score) const
    {
        const double NINF = post_dninf();
        const int64_t L = d.L;
        int bad = 0;
        for (int64_t p = threadIdx.x; p < L; p += NT) bad |= (d.d_in ? fb_bad_bits64(d.d_in[p]) : 0) | (d.e_in ? fb_bad_bits64(d.e_in[p]) : 0);
        flags |= bad ? 4 : 0;
        sstar = -1;
        if (!d.e_in) {
            sstar = d.terminal >= 0 ? (int64_t)d.terminal : d.path ? (int64_t)d.path[d.T - 1] : -1;
            flags |= (sstar < 0 || sstar >= L) ? 4 : 0;
        }
        flags = post_block_flags(flags);
        if (flags) return post_status_of(flags);
        if (d.e_in) {
            double m = NINF;
            int32_t at = -1;
            for (int64_t p = plo + threadIdx.x; p < phi; p += NT) margin_take(m, at, prev[Form::cslot(p)] + d.e_in[p], (int32_t)p);
            f.best(m, at, red);
            score = m;
        } else {
            score = (sstar >= plo && sstar < phi) ? prev[Form::cslot(sstar)] : NINF;
        }
        if (score != NINF && d.d_out)
            for (int64_t p = threadIdx.x; p < L; p += NT) d.d_out[p] = (p >= plo && p < phi) ? prev[Form::cslot(p)] : NINF;
        f.sync();   // (every thread has read the last column before a column is written again)
        return score == NINF ? kStatusZeroMass : kStatusOk;
    }

    // behind frame 0 of the backward pass: gn / vn hold G_0 and its vetoable copy over band 0 = [nlo, nhi)
    __device__ __forceinline__ void before(const double *gn, const double *vn, int64_t nlo, int64_t nhi) const
    {
        if (!d.e_out) return;
        const double NINF = post_dninf();
        const int M = moves();
        const int64_t wlo = nlo - (M - 1) > 0 ? nlo - (M - 1) : 0;
        for (int64_t p = threadIdx.x; p < d.L; p += NT) {
            double out = NINF;
            if (p >= wlo && p < nhi)
                for (int j = 0; j < M; ++j)
                    if (p + j >= nlo && p + j < nhi) out = __builtin_fmax(out, fb_skip(j) ? vn[Form::cslot(p + j)] : gn[Form::cslot(p + j)]);
            d.e_out[p] = out;
        }
    }
};

template <class Form>
__global__ __launch_bounds__(Form::NT) void margin_resume_kernel(const MarginResumeLattice *__restrict__ lats, int n, PostResult *res)
{
    __shared__ typename Form::template Shared<4> sh;
    __shared__ MarginRed red;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        Form f(lats[i], sh);
        if (lats[i].band_lo)
            margin_lattice<Form, BandTable, MgResume<Form>>(f, res, red);
        else
            margin_lattice<Form, BandWalk, MgResume<Form>>(f, res, red);
        f.sync();
    }
}

}  // namespace ka
