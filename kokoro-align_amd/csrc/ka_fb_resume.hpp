// ka_fb_resume.hpp — forward-backward posteriors under the caller's boundary conditions (ka_ctc_posteriors_resume, DESIGN.md
// section 4.37): the checkpointed pass of ka_fb_ck.hpp over a caller's table with the row before frame 0 (alpha_in) and the row
// at frame T-1 (beta_in) given, and the two rows a neighbouring chunk needs handed back (alpha_out: frame T-1's alpha; beta_out:
// the beta of the row before frame 0).  Included by ka_fb_resume.hip.
//
// The sum-product recurrence composes across a cut as the max-plus one does (ka_banded.hpp's BandResume): with chunk B's
// alpha_in = chunk A's alpha_out and A's beta_in = B's beta_out, every cell's gamma and either chunk's Z are the uncut
// lattice's.  All rows are [L] doubles in nats, absolute; -inf is no mass.  Inside, a row is turned to log2 units and its maximum
// is carried in the pass's offset (C forward, D backward), so that the columns stay relative as they are everywhere else.
//   FbCallerBound<Form>   ka_fb_ck.hpp's boundary policy: places alpha_in (no band applies to it: frame 0 reads [lo_0 - (M-1),
//                         hi_0), which may be kFastMaxBand + 3 = 1012 wide and still fits the fast form's 1024 slots), forms Z as
//                         a float64 log-sum-exp over band T-1 (a NULL beta_in keeps fb_ck_forward's expressions and bits), seeds
//                         w_{T-1} through fb_end_w, and runs the emission-free step behind frame 0 for beta_out
//   ResumeOut<Form, Band> the Out: OccOut's bins (held, not copied) where the occupancy is asked for, and gamma at the path cell
// A NaN or +inf anywhere in either row (all 2S+1 cells, read or not) is kStatusBadArgs, found on the bits as post_bad_bits finds
// a log-prob's.  An output row may not overlap an input row: the recompute of block 0 reads alpha_in again behind the store of
// alpha_out, and the backward pass reads beta_in behind it (the host rejects such a call).
#pragma once
#include "ka_occupancy.hpp"

namespace ka {

// post_bad_bits for a double of a row: NaN or +inf (-inf is no mass)
__device__ __forceinline__ int fb_bad_bits64(double x)
{
    uint32_t hi = (uint32_t)(__builtin_bit_cast(uint64_t, x) >> 32), lo = (uint32_t)__builtin_bit_cast(uint64_t, x);
    asm volatile("" : "+v"(hi), "+v"(lo));
    const uint32_t mag = hi & 0x7fffffffu;
    return ((mag > 0x7ff00000u || (mag == 0x7ff00000u && lo != 0u)) ? 1 : 0) | ((hi == 0x7ff00000u && lo == 0u) ? 1 : 0);
}
// a row of NaN bits (vector stores; the library is built with -fno-honor-nans, so the value is never a constant)
__device__ __forceinline__ void fb_nan_row(double *row, int64_t n)
{
    if (!row) return;
    for (int64_t p = threadIdx.x; p < n; p += blockDim.x) reinterpret_cast<uint64_t *>(row)[p] = kNaN64;
}

template <class Form>
struct FbCallerBound {
    static constexpr bool kVirtual = false;
    static constexpr int NT = Form::NT;
    const ResumeFbLattice &d;
    double dz;   // the maximum of beta_in over band T-1 in log2 units: the offset D the backward pass starts from
    __device__ __forceinline__ explicit FbCallerBound(const ResumeFbLattice &d_) : d(d_), dz(0.0) {}

    __device__ __forceinline__ int moves() const
    {
        if constexpr (Form::kWave) return Form::kMoves;
        else return d.max_move;
    }
    __device__ __forceinline__ bool stores() const { return d.occ || d.path_post; }
    __device__ __forceinline__ bool backward() const { return d.occ || d.path_post || d.beta_out; }
    __device__ __forceinline__ double d0() const { return dz; }
    __device__ __forceinline__ FbEndRow end(int64_t sstar) const { return FbEndRow{d.beta_in, dz, sstar}; }

    // the row before frame 0 (bw stands at frame 0): the virtual state, or alpha_in over [lo_0 - (M-1), hi_0) relative to its
    // maximum, which becomes the offset.  The row's bits are checked once, in finish(): a NaN that runs through the frames
    // places no cell.  Ends in no barrier: both callers synchronise before frame 0.
    template <class Band>
    __device__ __forceinline__ void place(Form &f, Band &bw, double *prev, int64_t &plo, int64_t &phi, double &C, int &) const
    {
        const double NINF = post_dninf();
        plo = 0;
        phi = 1;
        C = 0.0;
        if (!d.alpha_in) {
            if (threadIdx.x == 0) prev[0] = 0.0;
            return;
        }
        int64_t lo, hi;
        bw.band(lo, hi);
        const int64_t wlo = lo - (moves() - 1) > 0 ? lo - (moves() - 1) : 0;
        double mymax = NINF;
        for (int64_t p = wlo + threadIdx.x; p < hi; p += NT) mymax = fmax(mymax, d.alpha_in[p] * kLog2e64);
        double m = f.max(mymax);
        m = (m == NINF) ? 0.0 : m;
        for (int64_t p = wlo + threadIdx.x; p < hi; p += NT) prev[Form::cslot(p)] = d.alpha_in[p] * kLog2e64 - m;
        plo = wlo;
        phi = hi;
        C = m;
    }

    // the end of the forward pass, prev = u_{T-1} over band T-1 = [plo, phi), alpha_{T-1}(p) = Ca + u: the flags and their status,
    // Z and the reported Z, then alpha_out
    __device__ __forceinline__ int finish(Form &f, const double *prev, int64_t plo, int64_t phi, double Cb, double Ca, int flags, double &Z,
                                          double &Zr)
    {
        const double NINF = post_dninf();
        const int64_t L = d.L, sstar = d.terminal;
        const double *bin = d.beta_in;
        double mx = NINF, mb = NINF;
        if (!bin) {
            flags |= (sstar < 0 || sstar >= L) ? 4 : 0;
        } else {
            for (int64_t p = plo + threadIdx.x; p < phi; p += NT) {
                const double b = bin[p];
                mb = fmax(mb, b * kLog2e64);
                mx = fmax(mx, prev[Form::cslot(p)] + b * kLog2e64);
            }
        }
        int bad = 0;   // a NaN or +inf anywhere in either row, whether or not a frame reads the cell
        for (int64_t p = threadIdx.x; p < L; p += NT) bad |= (d.alpha_in ? fb_bad_bits64(d.alpha_in[p]) : 0) | (bin ? fb_bad_bits64(bin[p]) : 0);
        flags |= bad ? 4 : 0;
        flags = post_block_flags(flags);
        if (flags) return post_status_of(flags);
        if (!bin) {   // the sibling's expressions, and so its bits (its zero-mass test on the float Z is reported from included)
            const double us = (sstar >= plo && sstar < phi) ? prev[Form::cslot(sstar)] : NINF;
            if ((float)((Ca - Cb) + us) == post_ninf()) return kStatusZeroMass;
            Z = Ca + us;
            Zr = fb_reported_z(Cb, Ca, us);
            dz = 0.0;
        } else {
            mx = f.max(mx);
            mb = f.max(mb);
            if (mx == NINF) return kStatusZeroMass;
            double s = 0.0;
            for (int64_t p = plo + threadIdx.x; p < phi; p += NT) s += exp2((prev[Form::cslot(p)] + bin[p] * kLog2e64) - mx);
            s = f.sum(s);
            Z = Ca + (mx + log2(s));
            Zr = Z * kLn2;
            dz = mb;
        }
        if (d.alpha_out)
            for (int64_t p = threadIdx.x; p < L; p += NT) d.alpha_out[p] = (p >= plo && p < phi) ? (Ca + prev[Form::cslot(p)]) * kLn2 : NINF;
        f.sync();
        return kStatusOk;
    }

    // behind frame 0 of the backward pass: gn / vn hold G_0 and its vetoable copy over band 0 = [nlo, nhi), nprev their maximum,
    // beta_0(p) + e_0(p) = (D - nprev) + G_0(p).  One more step without an emission, over the moves into band 0 (a skip into a
    // cell whose label value is 0 reads the vetoable copy: -inf), is the beta of the row before frame 0.
    __device__ __forceinline__ void before(Form &, const double *gn, const double *vn, int64_t nlo, int64_t nhi, double nprev, double D) const
    {
        if (!d.beta_out) return;
        const double NINF = post_dninf();
        const int M = moves();
        const int64_t L = d.L;
        const int64_t wlo = nlo - (M - 1) > 0 ? nlo - (M - 1) : 0;
        for (int64_t p = threadIdx.x; p < L; p += NT) {
            double out = NINF;
            if (p >= wlo && p < nhi) {
                auto g = [&](int j) { return fb_skip(j) ? vn[Form::cslot(p + j)] : gn[Form::cslot(p + j)]; };
                double mx = NINF;
                for (int j = 0; j < M; ++j)
                    if (p + j >= nlo && p + j < nhi) mx = fmax(mx, g(j));
                double s = 0.0;
                for (int j = 0; j < M; ++j)
                    if (p + j >= nlo && p + j < nhi) s += exp2(g(j) - mx);
                if (mx != NINF) out = (D + ((mx + log2(s)) - nprev)) * kLn2;
            }
            d.beta_out[p] = out;
        }
    }
};

// fb_ck's policy: OccOut's binning where the occupancy is asked for, gamma at the path cell where path_post is; a block is
// recomputed only if either is
template <class Form_, class Band>
struct ResumeOut {
    using Form = Form_;
    using Desc = ResumeFbLattice;
    using Bound = FbCallerBound<Form>;
    using Occ = OccOut<Form, Band>;
    using Lds = typename Occ::Lds;
    const ResumeFbLattice &d;
    Occ occ;
    Bound bd;
    int64_t pt;   // the frame's path cell, -1 where none is asked for
    __device__ __forceinline__ ResumeOut(const ResumeFbLattice &d_, Form &f, Lds &lds) : d(d_), occ(d_, f, lds), bd(d_), pt(-1) {}
    __device__ __forceinline__ Bound &bound() { return bd; }

    // a lattice without a result: every requested output NaN, rows included
    __device__ __forceinline__ void fail(PostResult *res, int status)
    {
        if (d.path_post)
            for (int64_t t = threadIdx.x; t < d.T; t += blockDim.x) reinterpret_cast<uint32_t *>(d.path_post)[t] = 0x7fc00000u;
        fb_nan_row(d.alpha_out, d.L);
        fb_nan_row(d.beta_out, d.L);
        if (d.occ) occ.fail(res, status);
        else fb_fail_result(d, res, status);
    }
    __device__ __forceinline__ bool recompute(int64_t) const { return d.occ || d.path_post; }
    __device__ __forceinline__ auto cells(int64_t t, int64_t lo)
    {
        pt = d.path_post ? d.path[t] : -1;
        return [this, t, bin = occ.cells(t, lo)](int64_t p, int32_t lab, auto arg) {
            if (d.occ) bin(p, lab, arg);
            if (p == pt) d.path_post[t] = fb_gamma(arg());
        };
    }
    __device__ __forceinline__ void cells_done()
    {
        if (d.occ) occ.cells_done();
    }
    __device__ __forceinline__ void frame_end(int64_t t, int64_t lo, int64_t hi)
    {
        if (d.occ) occ.frame_end(t, lo, hi);
        if (d.path_post && threadIdx.x == 0 && !(pt >= lo && pt < hi)) d.path_post[t] = 0.0f;   // a path cell outside band t
    }
};

template <class Band>
void launch_posteriors_resume(const BandDesc<ResumeFbLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res,
                              hipStream_t s)
{
    launch_fb_ck<ResumeOut, Band>(lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
