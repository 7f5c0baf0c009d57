// ka_fb_ck.hpp — the checkpointed forward-backward that ka_occupancy.hpp (label occupancy), ka_state_posterior.hpp (state
// posteriors at chosen frames), ka_duration.hpp (expected state durations), ka_mea.hpp (the MEA path) and ka_visit.hpp (state
// visit probabilities) share, and whose forward half ka_sample.hpp (sampled alignments) reuses: fb_ck_forward<Form>,
// fb_ck_recompute<Form> and the driver fb_ck<Form, Out>, each written once over three policies (the form, the call's Out and
// the band: BandWalk, the reference's diagonal, or BandTable, a caller's table), and the one kernel and the one launch of
// the calls (fb_ck_kernel, launch_fb_ck).
//
// The posterior kernels keep alpha only at the path; these calls need it at band cells, so the forward pass checkpoints the
// whole column before the first frame of every 32-frame block (with the offset C and the frame maximum m it runs on), and the
// backward pass, last block first, recomputes a block's alpha from its checkpoint into a per-slot slab with the forward
// pass's own frame function (Form::fwd), then steps beta back through the block (Form::bwd).  The recompute runs the same
// instructions on the same operands: its alpha is the forward pass's bit for bit, so gamma at (T-1, s*) is 2^0 exactly.  A
// cell's gamma is 2^arg, arg = ((ca + alpha) + (D + w)) - Z.
//
// Form (FbFast<M> or FbGen of ka_fb_form.hpp, built per lattice) owns how a lattice is run: the threads and how they
// synchronise, the frame maximum, where a position lives in a column, a checkpoint and the slab, how the frame's log-prob
// row reaches a cell, and the frame recurrences.  Its table is at the head of ka_fb_form.hpp.
// Out (the driver's only) owns what a call does with gamma.  It is a template <class Form, class Band> (every call's, so that
// one launch can name the kernels of all five forms; the band is used where the call needs it), names
//   Form, Desc                   its form and the call's descriptor
//   Lds                          what its kernel holds in LDS beyond the form's Shared and the driver's cav: bins, rings, a
//                                tile.  Sized per form (a ring is the fast form's only and takes none of the generic kernel's
//                                LDS); empty where a call needs none
// is built per lattice as Out(descriptor, form, lds), holds the call's outputs and has a hook for each place where the calls
// differ:
//   fail(res, status)            a lattice without a result: fill the outputs with NaN, then fb_fail_result
//   begin()                      opt-in, once a lattice behind the forward pass (the band is accepted, Z is known) and before the
//                                first block: for what an Out may place only by an accepted band's values
//   recompute(t0)                recompute the block that starts at t0?  (if not, the walk is re-seated at t1, where the
//                                recompute would have left it; beta is still stepped through every frame)
//   cells(t, lo)                 frame t's action on a cell's gamma: a callable (p, lab, arg), arg() the log2 argument, formed
//                                only when called (asked for once a frame, before the frame's first cell and the fence in front of it)
//   kNextColumn, next_column(gn, vn, nprev, last)   opt-in, for a call that looks at a pair of frames: an Out that declares
//                                kNextColumn is handed, before cells(t, lo), the column of frame t + 1 as the recurrence is about
//                                to read it (G_{t+1}, its vetoable copy, the maximum taken off its log-sum-exp; last: t = T-1, no
//                                such column), and its cells are called as (p, lab, w, arg), w the recurrence's value
//   cells_done(), frame_end(t, lo, hi)   after the frame's cells (before its reduction), and after its bookkeeping (before the
//                                fast form's end-of-frame fence); a hook owns any barrier or fence that only its kernel needs
// An Out branches on Form::kWave where the forms really differ (an LDS ring or the outputs themselves as accumulators, a
// register sum or atomics) and takes slots and strides from the form everywhere else.
// One kernel, fb_ck_kernel<Out, Band>, runs every call: it takes BandDesc<Out::Desc, Band> descriptors (Banded<Desc> under
// BandTable), and fb_table() is the only place where its body meets the band.  One launch, launch_fb_ck<Out, Band>, names the
// five kernels of a call and a band; a call's header wraps it in the function ka_launch.hpp declares, and a translation unit
// holds that function's explicit instantiation for its band.
// The path sampler (ka_sample.hpp) needs alpha and no beta: it calls fb_ck_forward and fb_ck_recompute and has no Out.
// Storage: lattices walk slots (launch grid = slots, lattice i on slot i mod grid), so the workspace is bounded by the slots,
// not by the batch.
#pragma once
#include <type_traits>

#include "ka_fb_form.hpp"

namespace ka {

// does an Out opt into the next column (kNextColumn, above)?
template <class Out, class = void>
struct fb_next_column : std::false_type {};
template <class Out>
struct fb_next_column<Out, std::void_t<decltype(Out::kNextColumn)>> : std::true_type {};

// does an Out opt into begin() (above)?
template <class Out, class = void>
struct fb_begin : std::false_type {};
template <class Out>
struct fb_begin<Out, std::void_t<decltype(&Out::begin)>> : std::true_type {};

// The boundary policy of the passes below: what stands before frame 0 and at frame T-1.  FbVirtualBound, the default, is the
// virtual state {0: 0} and one terminal s*: every `if constexpr (Bound::kVirtual)` below keeps the lines the calls have always
// run.  A caller's boundary conditions (FbCallerBound of ka_fb_resume.hpp, the only other one) are named by an Out as its
// member type Bound and handed over by its bound(); such a policy brings
//   place(f, bw, prev, plo, phi, C, flags)   the row before frame 0 into prev over [plo, phi), its maximum into the offset C (bw
//                                stands at frame 0); the forward pass and the recompute of block 0 both call it, so block 0 has no
//                                checkpoint of its own
//   stores()                     does the forward pass store checkpoints (is any gamma asked for)?
//   finish(f, prev, plo, phi, Cb, Ca, flags, Z, Zr)   the end of the forward pass: the status, Z, and what the call keeps of the last row
//   backward()                   does the backward pass run?
//   d0(), end(sstar)             the offset D the backward pass starts from and the End its frame T-1 is seeded with (fb_end_w)
//   before(f, gn, vn, nlo, nhi, nprev, D)   behind frame 0 of the backward pass: what the call keeps of the row before frame 0
struct FbVirtualBound {
    static constexpr bool kVirtual = true;
    __device__ __forceinline__ static double d0() { return 0.0; }   // D_T = 0: beta_{T-1} = {s*: 0}
    __device__ __forceinline__ static int64_t end(int64_t sstar) { return sstar; }
};
template <class Out, class = void>
struct fb_bound_of {
    using type = FbVirtualBound;
    __device__ __forceinline__ static FbVirtualBound get(Out &) { return {}; }
};
template <class Out>
struct fb_bound_of<Out, std::void_t<typename Out::Bound>> {
    using type = typename Out::Bound;
    __device__ __forceinline__ static type &get(Out &out) { return out.bound(); }
};

// one cell's gamma as a float from its log2 argument (occ_fix of ka_occupancy.hpp before the fixed-point step): what the state
// posteriors write and the state durations add
__device__ __forceinline__ float fb_gamma(double arg)
{
    const float g = __builtin_amdgcn_exp2f((float)arg);
    return g < 1.0f ? g : 1.0f;
}

// The forward pass: label check, alpha through every frame with a checkpoint before every block, the flag, terminal and
// zero-mass checks, Z (log2 alpha_{T-1}(s*), the expression gamma's alpha is formed with) and Zr (fb_reported_z).  Returns
// kStatusOk or the status the lattice fails with; col(0) / col(1) are its working columns, bw ends at frame T.  It ends behind
// f.sync(): in the generic form a barrier, which also orders the sampler's first slab.
template <class Form, class Band, class Bound>
__device__ __forceinline__ int fb_ck_forward(Form &f, Band &bw, double &Z, double &Zr, Bound &bd)
{
    const FbCkLattice &d = f.d;
    const int tid = threadIdx.x;
    const int64_t T = d.T, L = d.L;
    const double NINF = post_dninf();
    if (fb_labels_bad(d)) return kStatusBadLabel;
    if (!bw.start()) return kStatusBadArgs;   // (a caller's table that is no band: before any of its values places a cell)
    auto no_cell = [](int64_t, double) {};
    double *prev = f.col(0), *cur = f.col(1);
    if constexpr (Bound::kVirtual)
        if (tid == 0) prev[0] = 0.0;   // virtual state before frame 0
    int64_t plo = 0, phi = 1;
    double C = 0.0, Cb = 0.0, Ca = 0.0, mprev = 0.0;
    int flags = 0;
    if constexpr (!Bound::kVirtual) bd.place(f, bw, prev, plo, phi, C, flags);
    f.row_prefetch(0);
    f.sync();
    for (int64_t t = 0; t < T; ++t) {
        int64_t lo, hi;
        bw.band(lo, hi);
        flags |= f.row(t, t + 1, t + 1 < T, true);
        if (t % kPostCk == 0) {
            const int64_t k = t / kPostCk;
            Cb = C;
            bool store = true;
            if constexpr (!Bound::kVirtual) store = k > 0 && bd.stores();
            if (store) {
                if (tid == 0) {
                    d.ck[2 * k] = C;
                    d.ck[2 * k + 1] = mprev;
                }
                f.ck_store(k, prev, plo, phi);
            }
        }
        f.fence();
        double m = f.max(f.fwd(lo, hi, plo, phi, prev, cur, mprev, no_cell));
        m = (m == NINF) ? 0.0 : m;
        Ca = C;
        C += m;
        mprev = m;
        { double *x = prev; prev = cur; cur = x; }
        plo = lo;
        phi = hi;
        bw.next();
        f.fence();
    }
    if constexpr (!Bound::kVirtual) return bd.finish(f, prev, plo, phi, Cb, Ca, flags, Z, Zr);
    const int64_t sstar = d.terminal;
    flags |= (sstar < 0 || sstar >= L) ? 4 : 0;
    flags = post_block_flags(flags);
    if (flags) return post_status_of(flags);
    const double us = (sstar >= plo && sstar < phi) ? prev[Form::cslot(sstar)] : NINF;
    // (tested on the float Z is reported from, as the path call tests its stored float: a terminal beyond float32's range below
    //  its block's offset is zero mass in every call alike - include/kokoro_align_amd.h, KA_ERR_ZERO_MASS)
    if ((float)((Ca - Cb) + us) == post_ninf()) return kStatusZeroMass;
    Z = Ca + us;
    Zr = fb_reported_z(Cb, Ca, us);
    f.sync();
    return kStatusOk;
}
template <class Form, class Band>
__device__ __forceinline__ int fb_ck_forward(Form &f, Band &bw, double &Z, double &Zr)
{
    FbVirtualBound bd;
    return fb_ck_forward(f, bw, Z, Zr, bd);
}

// The recompute of block k = [t0, t1): alpha from the block's checkpoint into the slab (row t - t0, slot Form::slot) with the
// forward pass's frame function on the forward pass's operands, pv / cu the working columns; note(t - t0, C) is handed every
// frame's offset before the frame runs.  bw ends at frame t1.  A cell's slab entry is written by the thread that owns the
// cell in that frame.  The generic form ends behind a barrier; the fast form's last frame ends in its fence.
template <class Form, class Band, class Note, class Bound>
__device__ __forceinline__ void fb_ck_recompute(Form &f, int64_t k, int64_t t0, int64_t t1, Band &bw, double *pv, double *cu, Note note, Bound &bd)
{
    const FbCkLattice &d = f.d;
    const double NINF = post_dninf();
    int64_t rlo = 0, rhi = 1;
    double C2, mp;
    auto load = [&] {
        f.ck_load(k, pv, rlo, rhi);
        C2 = d.ck[2 * k];
        mp = d.ck[2 * k + 1];
    };
    const bool placed = !Bound::kVirtual && k == 0;   // block 0 under a caller's start row: placed again, not loaded
    if (Form::kWave && !placed) load();   // (all of the column's slots, whatever the band: issued before the seek's division)
    bw.seek(t0);
    if (t0 > 0) {
        bw.prev();
        bw.band(rlo, rhi);
        bw.next();
    }
    if (!Form::kWave && !placed) load();
    if constexpr (!Bound::kVirtual)
        if (placed) {
            int none = 0;
            mp = 0.0;
            bd.place(f, bw, pv, rlo, rhi, C2, none);
        }
    f.row_prefetch(t0);
    f.sync();
    for (int64_t t = t0; t < t1; ++t) {
        int64_t lo, hi;
        bw.band(lo, hi);
        f.row(t, t + 1, t + 1 < t1);
        note(t - t0, C2);
        f.fence();
        double *al = d.slab + (t - t0) * f.cw();
        double m = f.max(f.fwd(lo, hi, rlo, rhi, pv, cu, mp, [&](int64_t p, double val) { al[Form::slot(p, lo)] = val; }));
        m = (m == NINF) ? 0.0 : m;
        C2 += m;
        mp = m;
        { double *x = pv; pv = cu; cu = x; }
        rlo = lo;
        rhi = hi;
        bw.next();
        f.fence();
    }
    if (!Form::kWave) f.sync();
}
template <class Form, class Band, class Note>
__device__ __forceinline__ void fb_ck_recompute(Form &f, int64_t k, int64_t t0, int64_t t1, Band &bw, double *pv, double *cu, Note note)
{
    FbVirtualBound bd;
    fb_ck_recompute(f, k, t0, t1, bw, pv, cu, note, bd);
}

// The driver of the calls that need gamma; cav: kPostCk doubles of LDS, the offsets of the block's frames; Band: the band
// (BandWalk, or BandTable of ka_posterior_common.hpp on `tab`, the caller's table).
template <class Form, class Out, class Band = BandWalk>
__device__ __forceinline__ void fb_ck(Form &f, PostResult *res, double *cav, Out &out, const int32_t *tab = nullptr)
{
    const FbCkLattice &d = f.d;
    const int tid = threadIdx.x;
    const int64_t T = d.T;
    const double NINF = post_dninf();

    // ---- forward: Z, and a checkpoint before every block ----
    using Bound = typename fb_bound_of<Out>::type;
    decltype(auto) bd = fb_bound_of<Out>::get(out);
    Band bw(d.L, d.beam, T, tab);
    double Z, Zr;
    const int status = fb_ck_forward(f, bw, Z, Zr, bd);
    if (status != kStatusOk) {
        out.fail(res, status);
        return;
    }
    const int64_t sstar = d.terminal;
    if constexpr (fb_begin<Out>::value) out.begin();
    if constexpr (!Bound::kVirtual)
        if (!bd.backward()) {   // a forward pass alone
            if (tid == 0) {
                res[d.idx].status = kStatusOk;
                res[d.idx].log_likelihood = Zr;
            }
            return;
        }

    // ---- backward, a block at a time ----
    double *gn = f.col(0), *vn = f.col(1), *gc = f.col(2), *vc = f.col(3);   // G_{t+1} and its vetoable copy; scratch
    int64_t nlo = 0, nhi = 0;
    double D = bd.d0(), nprev = 0.0;   // D_T = 0: beta_{T-1} = {s*: 0}; a caller's row: its maximum
    for (int64_t k = (T - 1) / kPostCk; k >= 0; --k) {
        const int64_t t0 = k * kPostCk, t1 = (t0 + kPostCk < T) ? t0 + kPostCk : T;
        if (out.recompute(t0)) {   // alpha over [t0, t1) into the slab, gc / vc as the working columns
            fb_ck_recompute(f, k, t0, t1, bw, gc, vc, [&](int64_t fr, double c) {
                if (tid == 0) cav[fr] = c;
            }, bd);
        } else {
            bw.seek(t1);
        }
        // beta back through the block (bw walks back from t1)
        f.row_prefetch(t1 - 1);
        for (int64_t t = t1 - 1; t >= t0; --t) {
            bw.prev();
            int64_t lo, hi;
            bw.band(lo, hi);
            f.row(t, t - 1, t > t0);
            const double ca = cav[t - t0];
            const double *al = d.slab + (t - t0) * f.cw();
            if constexpr (fb_next_column<Out>::value) out.next_column(gn, vn, nprev, t == T - 1);
            auto cell = out.cells(t, lo);
            f.fence();
            const double mymax = f.bwd(lo, hi, nlo, nhi, gn, vn, gc, vc, nprev, t == T - 1, bd.end(sstar), [&](int64_t p, int32_t lab, double w) {
                auto arg = [&] { return ((ca + al[Form::slot(p, lo)]) + (D + w)) - Z; };
                if constexpr (fb_next_column<Out>::value)
                    cell(p, lab, w, arg);
                else
                    cell(p, lab, arg);
            });
            out.cells_done();
            double n = f.max(mymax);   // (the generic form's barrier also closes the frame's cells before frame_end)
            n = (n == NINF) ? 0.0 : n;
            D += n;
            nprev = n;
            { double *x = gn; gn = gc; gc = x; }
            { double *x = vn; vn = vc; vc = x; }
            nlo = lo;
            nhi = hi;
            out.frame_end(t, lo, hi);
            f.fence();
        }
    }
    if constexpr (!Bound::kVirtual) bd.before(f, gn, vn, nlo, nhi, nprev, D);
    if (tid == 0) {
        res[d.idx].status = kStatusOk;
        res[d.idx].log_likelihood = Zr;
    }
}

// two rings of 1024 doubles (a position at the form's column slot) for an Out's Lds: the fast form's only, and no byte of the
// generic kernel's LDS
template <bool kWave>
struct FbRings {
    double r[2][1024];
    __device__ __forceinline__ double *ring(int i) { return r[i]; }
};
template <>
struct FbRings<false> {
    __device__ __forceinline__ double *ring(int) { return nullptr; }
};

// The kernel of every call that goes through fb_ck: lattices walk slots (lattice i on workgroup i mod grid).
template <class Out, class Band>
__global__ __launch_bounds__(Out::Form::NT) void fb_ck_kernel(const BandDesc<typename Out::Desc, Band> *__restrict__ lats, int n, PostResult *res)
{
    using Form = typename Out::Form;
    __shared__ typename Form::template Shared<4> sh;
    __shared__ double cav[kPostCk];
    __shared__ typename Out::Lds lds;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        Form f(lats[i], sh);
        Out out(lats[i], f, lds);
        fb_ck<Form, Out, Band>(f, res, cav, out, fb_table(lats[i]));
        f.sync();
    }
}

// the launch of kernels that walk slots: descriptors [0, n_fast) on min(n_fast, kOccFastSlots) one-wavefront workgroups (fast[M - 1],
// M = max_move, 4 above 3), lattice i on workgroup i mod grid (its slot); then [n_fast, n_fast + n_generic) on
// min(n_generic, kOccGenericSlots) 256-thread workgroups
template <class Desc>
using FbCkKernel = void (*)(const Desc *, int, PostResult *);
template <class Desc>
void launch_fb_slots(const FbCkKernel<Desc> (&fast)[4], FbCkKernel<Desc> generic, const Desc *lats, int n_fast, int n_generic, int max_move,
                     PostResult *res, hipStream_t s)
{
    if (n_fast > 0) {
        const dim3 grid(n_fast < kOccFastSlots ? n_fast : kOccFastSlots);
        hipLaunchKernelGGL(fast[(max_move >= 1 && max_move <= 3 ? max_move : 4) - 1], grid, dim3(FbFast<1>::NT), 0, s, lats, n_fast, res);
    }
    if (n_generic > 0) {
        const dim3 grid(n_generic < kOccGenericSlots ? n_generic : kOccGenericSlots);
        hipLaunchKernelGGL(generic, grid, dim3(FbGen<>::NT), 0, s, lats + n_fast, n_generic, res);
    }
}
// ... of a call's Out over a band: the five kernels are fb_ck_kernel's
template <template <class, class> class Out, class Band>
void launch_fb_ck(const BandDesc<typename Out<FbGen<>, Band>::Desc, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res,
                  hipStream_t s)
{
    using Desc = BandDesc<typename Out<FbGen<>, Band>::Desc, Band>;
    launch_fb_slots<Desc>({fb_ck_kernel<Out<FbFast<1>, Band>, Band>, fb_ck_kernel<Out<FbFast<2>, Band>, Band>, fb_ck_kernel<Out<FbFast<3>, Band>, Band>,
                           fb_ck_kernel<Out<FbFast<4>, Band>, Band>},
                          fb_ck_kernel<Out<FbGen<>, Band>, Band>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
