// ka_margin.hpp — best-path margins from max-marginals (ka_ctc_path_margins_*).  Included by
// ka_margin.hip and, through ka_margin_resume.hpp, by ka_margin_resume.hip.
//
// The best path's own recurrence, run forwards (D) and backwards (E) in max-plus arithmetic, over the lattice of
// ka_ctc_best_path_banded (lab' the blank-expanded labels, L = 2S+1, band [lo_t, hi_t) from the caller's table or, without one,
// the reference's diagonal, moves j in [0, max_move), an even j >= 2 may not land on a label VALUE 0, virtual state {0: 0.0}
// before frame 0, terminal s* = path[T-1]):
//   D_t(p) = max_j D_{t-1}(p-j) + lp[t, lab'[p]]                 p-j in band t-1, veto on lab'[p]
//   E_{T-1} = {s*: 0},  E_t(p) = max_j G_{t+1}(p+j),  G_t(p) = E_t(p) + lp[t, lab'[p]]     p+j in band t+1, veto on lab'[p+j]
//   m_t(p) = D_t(p) + E_t(p)        the score of the best complete path that is at p in frame t
//   through[t] = m_t(path[t]) (-inf outside band t);  alt[t] = max of m_t over the cells of another group (p >> unit);
//   runner_up[t] = the lowest p attaining alt[t], -1 where alt[t] is -inf;  score = D_{T-1}(s*)
// Every value is a float64, every log-prob widened exactly, every + one IEEE add, every max exact: the outputs are defined bit
// for bit, in natural units (no scaling of the row as FbFast::row does, which is inexact), with no offsets and no
// transcendental.
//
// The pass has ka_fb_ck.hpp's shape and its storage (FbCkLattice's slot: ckcol, slab, col; ck goes unused): the forward pass
// stores the D column before every kPostCk-frame block; the backward pass, last block first, recomputes a block's D into the
// slab with the forward pass's frame function and steps E back through the block, reducing (m, position) over the band per
// frame.  fb_ck<Form, Out> itself is built around offsets and gamma, so the driver here (margin_lattice) is a sibling; the forms
// are the family's with the row and the two recurrences replaced:
//   MgFast<M>  FbFast<M, MarginLattice, LabRing>: one wavefront, columns in LDS at p & 1023, labels from the ring (re-seated at
//              a block's first frame, turned at its last), the row prefetched a frame ahead, frames handed over by a fence
//   MgGen      FbGen<MarginLattice>: 256 threads, columns in global memory, a barrier per frame.  Plain, not tuned.
// The band is BandWalk or BandTable, chosen per lattice by MarginLattice::band_lo (NULL: the diagonal, no table in memory).
// The frame's reduction is lexicographic on (m, position): a float64 and a position do not fit one 64-bit key, so the
// cross-lane step carries the pair (three 32-bit exchanges) and takes the other lane's on a larger m or an equal m at a lower p.
#pragma once
#include "ka_fb_ck.hpp"

namespace ka {

// a lattice without a result: NaN over through and alt (stored as bits: -fno-honor-nans), -1 over runner_up, fb_fail_result
__device__ __forceinline__ void margin_fail(const MarginLattice &d, PostResult *res, int status)
{
    uint64_t *th = reinterpret_cast<uint64_t *>(d.through), *al = reinterpret_cast<uint64_t *>(d.alt);
    for (int64_t t = threadIdx.x; t < d.T; t += blockDim.x) {
        th[t] = kNaN64;
        al[t] = kNaN64;
        if (d.runner) d.runner[t] = -1;
    }
    fb_fail_result(d, res, status);
}

// (m, p) of two cells: the larger m, the lower p on a tie; p = -1 (no cell, m = -inf) loses to any cell
__device__ __forceinline__ void margin_take(double &m, int32_t &p, double om, int32_t op)
{
    const bool take = om > m || (om == m && (uint32_t)op < (uint32_t)p);
    m = take ? om : m;
    p = take ? op : p;
}
__device__ __forceinline__ void margin_wave_best(double &m, int32_t &p)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double om = __shfl_xor(m, off);
        const int32_t op = __shfl_xor(p, off);
        margin_take(m, p, om, op);
    }
}
// the generic form's four wavefronts meet here; the frame's closing barrier (MgGen::fence) frees it for the next frame
struct MarginRed {
    double m[4];
    int32_t p[4];
};

// The forms are written over the descriptor type (MgFastOn, MgGenOn): MarginLattice for ka_ctc_path_margins (MgFast<M>, MgGen
// below), MarginResumeLattice for the resumed call (ka_margin_resume.hpp).
template <int M, class Desc>
struct MgFastOn : FbFast<M, Desc, LabRing> {
    using Base = FbFast<M, Desc, LabRing>;
    template <class Sh>
    __device__ __forceinline__ MgFastOn(const Desc &d_, Sh &sh) : Base(d_, sh) {}

    // the row in natural units: a float widens exactly
    __device__ __forceinline__ int row(int64_t, int64_t tn, bool more, bool check = false)
    {
        const int lane = threadIdx.x;
        const int64_t V = this->d.V;
        int bad = 0;
        if (lane < V) {
            if (check) bad = post_bad_bits(this->rv);
            this->lds_row[lane] = (double)this->rv;
        }
        if (more && lane < V) this->rv = this->d.lp[(size_t)tn * (size_t)this->d.ld + lane];
        return bad;
    }
    // the ring over [lo, lo + 1024): before a block's first frame, whichever way the ring ran last
    __device__ __forceinline__ void reseat(int64_t lo)
    {
        const int64_t end = (lo + 1024 < this->d.L) ? lo + 1024 : (int64_t)this->d.L;
        for (int64_t p = lo + threadIdx.x; p < end; p += 64) this->lab.ring[p & 1023] = fb_lab(this->d, p);
        this->lab.lfill = end;
    }
    // ... for a backward walk that starts at a frame whose band begins at lo, with no forward walk before it
    __device__ __forceinline__ void reseat_bwd(int64_t lo)
    {
        reseat(lo);
        this->lab.lbot = lo;
    }
    __device__ __forceinline__ void best(double &m, int32_t &p, MarginRed &) const { margin_wave_best(m, p); }

    // A lane's cells are taken kCells at a time, every load of the group (labels, row entries, the neighbours' column values
    // and what `pre` fetches) issued before the first of its stores: a cell's chain of dependent LDS reads (label -> row entry)
    // and a slab read from global memory then overlap with the other cells' instead of queueing behind a store that might alias.
    // One cell at a time measured 811 / 1085 ms (one / 1024 cfg2 lattices), four 567 / 652, eight 564 / 623; the
    // registers are free, the kernel's LDS holds a SIMD to one wavefront.
    static constexpr int kCells = 8;

    // D_t over [lo, hi) from D_{t-1} (prev) over [plo, phi) into cur; cell(p, D_t(p))
    template <class Cell>
    __device__ __forceinline__ void fwd(int64_t lo_, int64_t hi_, int64_t plo_, int64_t phi_, const double *prev, double *cur, Cell cell) const
    {
        const double NINF = post_dninf();
        const int32_t hi = (int32_t)hi_, plo = (int32_t)plo_, phi = (int32_t)phi_;
        for (int32_t b = (int32_t)lo_ + (int32_t)threadIdx.x; b < hi; b += 64 * kCells) {
            int32_t lab[kCells];
            double e[kCells], mx[kCells];
#pragma unroll
            for (int k = 0; k < kCells; ++k) {
                const int32_t p = b + 64 * k;
                lab[k] = p < hi ? this->lab(p) : 0;
            }
#pragma unroll
            for (int k = 0; k < kCells; ++k) {
                const int32_t p = b + 64 * k;
                e[k] = this->lds_row[lab[k]];
                mx[k] = NINF;
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    const int32_t u = p - j;
                    const bool ok = u >= plo && u < phi && !fb_vetoed(j, lab[k]);
                    const double x = prev[u & 1023];
                    mx[k] = __builtin_fmax(mx[k], ok ? x : NINF);
                }
            }
#pragma unroll
            for (int k = 0; k < kCells; ++k) {
                const int32_t p = b + 64 * k;
                if (p < hi) {
                    const double val = mx[k] + e[k];
                    cur[p & 1023] = val;
                    cell(p, val);
                }
            }
        }
    }
    // G_t over [lo, hi) from G_{t+1} (gn, its vetoable copy vn) over [nlo, nhi) into gc / vc; cell(p, E_t(p), pre(p)), pre(p)
    // fetched with the group's loads.  kLast: t = T-1, E_{T-1} = {sstar: 0}, or the caller's row ein where there is one
    template <bool kLast, class Pre, class Cell>
    __device__ __forceinline__ void bwd(int64_t lo_, int64_t hi_, int64_t nlo_, int64_t nhi_, const double *gn, const double *vn, double *gc,
                                        double *vc, int64_t sstar, Pre pre, Cell cell, const double *ein = nullptr) const
    {
        const double NINF = post_dninf();
        const int32_t hi = (int32_t)hi_, nlo = (int32_t)nlo_, nhi = (int32_t)nhi_;
        for (int32_t b = (int32_t)lo_ + (int32_t)threadIdx.x; b < hi; b += 64 * kCells) {
            int32_t lab[kCells];
            double e[kCells], w[kCells], a[kCells];
#pragma unroll
            for (int k = 0; k < kCells; ++k) {
                const int32_t p = b + 64 * k;
                lab[k] = p < hi ? this->lab(p) : 0;
                a[k] = p < hi ? pre(p) : 0.0;
            }
#pragma unroll
            for (int k = 0; k < kCells; ++k) {
                const int32_t p = b + 64 * k;
                e[k] = this->lds_row[lab[k]];
                if (kLast) {
                    w[k] = ein ? (p < hi ? ein[p] : NINF) : (p == sstar) ? 0.0 : NINF;
                } else {
                    w[k] = NINF;
#pragma unroll
                    for (int j = 0; j < M; ++j) {
                        const int32_t u = p + j;
                        const bool ok = u >= nlo && u < nhi;
                        const double g = fb_skip(j) ? vn[u & 1023] : gn[u & 1023];
                        w[k] = __builtin_fmax(w[k], ok ? g : NINF);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kCells; ++k) {
                const int32_t p = b + 64 * k;
                if (p < hi) {
                    const double g = w[k] + e[k];
                    gc[p & 1023] = g;
                    vc[p & 1023] = lab[k] == 0 ? NINF : g;
                    cell(p, w[k], a[k]);
                }
            }
        }
    }
};

template <int M>
struct MgFast : MgFastOn<M, MarginLattice> {
    template <class Sh>
    __device__ __forceinline__ MgFast(const MarginLattice &d_, Sh &sh) : MgFastOn<M, MarginLattice>(d_, sh) {}
};

template <class Desc>
struct MgGenOn : FbGen<Desc> {
    using Base = FbGen<Desc>;
    using Base::d;
    using Base::lrow;
    template <class Sh>
    __device__ __forceinline__ MgGenOn(const Desc &d_, Sh &sh) : Base(d_, sh) {}

    __device__ __forceinline__ void fence() const { __syncthreads(); }   // (no frame maximum here whose barrier would order the frames)
    __device__ __forceinline__ void reseat(int64_t) {}
    __device__ __forceinline__ void reseat_bwd(int64_t) {}
    __device__ __forceinline__ void best(double &m, int32_t &p, MarginRed &red) const
    {
        margin_wave_best(m, p);
        if ((threadIdx.x & 63) == 0) {
            red.m[threadIdx.x >> 6] = m;
            red.p[threadIdx.x >> 6] = p;
        }
        __syncthreads();
        m = red.m[0];
        p = red.p[0];
        for (int w = 1; w < 4; ++w) margin_take(m, p, red.m[w], red.p[w]);
    }

    template <class Cell>
    __device__ __forceinline__ void fwd(int64_t lo, int64_t hi, int64_t plo, int64_t phi, const double *prev, double *cur, Cell cell) const
    {
        const int M = d.max_move;
        const double NINF = post_dninf();
        for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
            const int32_t lab = fb_lab(d, p);
            const double e = (double)lrow[lab];
            double mx = NINF;
            for (int j = 0; j < M && j <= p; ++j) {
                const int64_t u = p - j;
                if (u >= plo && u < phi && !fb_vetoed(j, lab)) mx = __builtin_fmax(mx, prev[u]);
            }
            const double val = mx + e;
            cur[p] = val;
            cell(p, val);
        }
    }
    template <bool kLast, class Pre, class Cell>
    __device__ __forceinline__ void bwd(int64_t lo, int64_t hi, int64_t nlo, int64_t nhi, const double *gn, const double *vn, double *gc,
                                        double *vc, int64_t sstar, Pre pre, Cell cell, const double *ein = nullptr) const
    {
        const int M = d.max_move;
        const double NINF = post_dninf();
        for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
            const int32_t lab = fb_lab(d, p);
            double w;
            if (kLast) {
                w = ein ? ein[p] : (p == sstar) ? 0.0 : NINF;
            } else {
                w = NINF;
                for (int j = 0; j < M && p + j < nhi; ++j)
                    if (p + j >= nlo) w = __builtin_fmax(w, fb_skip(j) ? vn[p + j] : gn[p + j]);
            }
            const double g = w + (double)lrow[lab];
            gc[p] = g;
            vc[p] = lab == 0 ? NINF : g;
            cell(p, w, pre(p));
        }
    }
};
struct MgGen : MgGenOn<MarginLattice> {
    template <class Sh>
    __device__ __forceinline__ MgGen(const MarginLattice &d_, Sh &sh) : MgGenOn<MarginLattice>(d_, sh) {}
};

// What stands before frame 0 and at frame T-1, and what is read out of m: a policy of margin_lattice.  MgPlain, the default,
// is ka_ctc_path_margins: the virtual start {0: 0.0}, E_{T-1} = {path[T-1]: 0}, through / alt / runner_up of every frame; every
// `if constexpr (Pol::kPlain)` below keeps the lines that call has always run.  The one other policy, MgResume
// (ka_margin_resume.hpp), takes the two rows from the caller, hands two back and reads rows of m out at chosen frames.
struct MgPlain {
    static constexpr bool kPlain = true;
    const MarginLattice &d;
    __device__ __forceinline__ explicit MgPlain(const MarginLattice &d_) : d(d_) {}
    __device__ __forceinline__ void fail(PostResult *res, int status) const { margin_fail(d, res, status); }
};

// One lattice: the forward pass with its checkpoints and checks, then the blocks backwards.
template <class Form, class Band, class Pol = MgPlain>
__device__ __forceinline__ void margin_lattice(Form &f, PostResult *res, MarginRed &red)
{
    const auto &d = f.d;
    Pol pol(d);
    const int tid = threadIdx.x;
    const int64_t T = d.T, L = d.L;
    const double NINF = post_dninf();
    if (fb_labels_bad(d)) return pol.fail(res, kStatusBadLabel);
    Band bw(L, d.beam, T, d.band_lo);
    if (!bw.start()) return pol.fail(res, kStatusBadArgs);   // (a caller's table that is no band: before any of its values places a cell)
    int flags = 0;
    if (Pol::kPlain || d.path)
        for (int64_t t = tid; t < T; t += Form::NT) {
            const int32_t pv = d.path[t];
            flags |= (pv < 0 || pv >= L) ? 4 : 0;
        }

    // ---- forward: D through every frame, a checkpoint before every block ----
    auto no_cell = [](int64_t, double) {};
    f.lab.fill();
    double *prev = f.col(0), *cur = f.col(1);
    int64_t plo = 0, phi = 1;
    if constexpr (Pol::kPlain) {
        if (tid == 0) prev[0] = 0.0;   // virtual state before frame 0
    } else {
        pol.place(bw, prev, plo, phi);
    }
    f.row_prefetch(0);
    f.sync();
    for (int64_t t = 0; t < T; ++t) {
        int64_t lo, hi, lon, hin;
        bw.band(lo, hi);
        bw.next();
        bw.band(lon, hin);
        const bool more = t + 1 < T;
        if (more) f.lab.fwd_request(lon);
        flags |= f.row(t, t + 1, more, true);
        if (t % kPostCk == 0) {
            bool store = true;
            if constexpr (!Pol::kPlain) store = pol.stores(t / kPostCk);
            if (store) f.ck_store(t / kPostCk, prev, plo, phi);
        }
        f.fence();
        f.fwd(lo, hi, plo, phi, prev, cur, no_cell);
        { double *x = prev; prev = cur; cur = x; }
        plo = lo;
        phi = hi;
        if (more) f.lab.fwd_commit();
        f.fence();
    }
    int64_t sstar;
    double score;
    if constexpr (Pol::kPlain) {
        flags = post_block_flags(flags);
        if (flags) return pol.fail(res, post_status_of(flags));
        sstar = d.path[T - 1];
        score = (sstar >= plo && sstar < phi) ? prev[Form::cslot(sstar)] : NINF;
        f.sync();   // (every thread has read the score before a column is written again)
        if (score == NINF) return pol.fail(res, kStatusZeroMass);
    } else {
        const int status = pol.finish(f, red, prev, plo, phi, flags, sstar, score);
        if (status != kStatusOk) return pol.fail(res, status);
        if (!pol.backward()) {   // a forward pass alone
            if (tid == 0) {
                res[d.idx].status = kStatusOk;
                res[d.idx].log_likelihood = score;
            }
            return;
        }
    }

    // ---- backward, a block at a time ----
    double *gn = f.col(0), *vn = f.col(1), *gc = f.col(2), *vc = f.col(3);   // G_{t+1} and its vetoable copy; frame t's, and scratch
    int64_t nlo = 0, nhi = 0;
    const int unit = d.unit;
    for (int64_t k = (T - 1) / kPostCk; k >= 0; --k) {
        const int64_t t0 = k * kPostCk, t1 = (t0 + kPostCk < T) ? t0 + kPostCk : T;
        bool with_d = true;   // is the block's D asked for?  (a resumed call may want E alone)
        if constexpr (!Pol::kPlain) {
            if (pol.done()) break;
            with_d = pol.block(t0, t1);
        }
        int64_t rlo = 0, rhi = 1;
        if (with_d) {
            // D over [t0, t1) from the block's checkpoint into the slab, gc / vc as the working columns
            bw.seek(t0);
            if (t0 > 0) {
                bw.prev();
                bw.band(rlo, rhi);
                bw.next();
            }
            double *pv = gc, *cu = vc;
            if (Pol::kPlain || k > 0) {
                f.ck_load(k, pv, rlo, rhi);
            } else {
                if constexpr (!Pol::kPlain) pol.place(bw, pv, rlo, rhi);   // (block 0 has no checkpoint: its start row is placed again)
            }
            {
                int64_t lo, hi;
                bw.band(lo, hi);
                f.reseat(lo);
            }
            f.row_prefetch(t0);
            f.sync();
            for (int64_t t = t0; t < t1; ++t) {
                int64_t lo, hi, lon, hin;
                bw.band(lo, hi);
                bw.next();
                bw.band(lon, hin);
                const bool more = t + 1 < t1;
                if (more) f.lab.fwd_request(lon);
                f.row(t, t + 1, more);
                f.fence();
                double *al = d.slab + (t - t0) * f.cw();
                f.fwd(lo, hi, rlo, rhi, pv, cu, [&](int64_t p, double val) { al[Form::slot(p, lo)] = val; });
                { double *x = pv; pv = cu; cu = x; }
                rlo = lo;
                rhi = hi;
                if (more) f.lab.fwd_commit();
                f.fence();
            }
            // E back through the block; bw stands at t1, and is kept a frame ahead (below) of the frame at work
            f.lab.turn(rlo);
        } else {
            bw.seek(t1 - 1);
            bw.band(rlo, rhi);
            bw.next();
            f.reseat_bwd(rlo);
        }
        f.row_prefetch(t1 - 1);
        int32_t ptn = (Pol::kPlain || d.path) ? d.path[t1 - 1] : -1;
        bw.prev();
        f.sync();
        for (int64_t t = t1 - 1; t >= t0; --t) {
            int64_t lo, hi, lon = 0, hin = 0;
            bw.band(lo, hi);
            bw.prev();
            const bool more = t > t0;
            if (more) bw.band(lon, hin);
            f.lab.bwd_request(lon, more);
            f.row(t, t - 1, more);
            const int32_t pt = ptn;
            if (more && (Pol::kPlain || d.path)) ptn = d.path[t - 1];
            f.fence();
            const double *al = d.slab + (t - t0) * f.cw();
            double bm = NINF;
            int32_t bp = -1;
            if constexpr (Pol::kPlain) {
                auto pre = [&](int64_t p) { return al[Form::slot(p, lo)]; };   // D_t(p), from the slab
                auto cell = [&](int64_t p, double w, double dt) {
                    const double m = dt + w;
                    if ((p >> unit) == ((int64_t)pt >> unit)) {
                        if (p == pt) d.through[t] = m;
                    } else if (m > bm) {   // (a lane's cells ascend: the first of equal m stays)
                        bm = m;
                        bp = (int32_t)p;
                    }
                };
                if (t == T - 1)
                    f.template bwd<true>(lo, hi, nlo, nhi, gn, vn, gc, vc, sstar, pre, cell);
                else
                    f.template bwd<false>(lo, hi, nlo, nhi, gn, vn, gc, vc, sstar, pre, cell);
                f.best(bm, bp, red);
                if (tid == 0) {
                    if (!(pt >= lo && pt < hi)) d.through[t] = NINF;
                    d.alt[t] = bm;
                    if (d.runner) d.runner[t] = bp;
                }
            } else {
                // the frame in two instantiations, chosen per block: with D (from the slab, with every read-out of m) and without (E
                // alone: no slab load, no cell work), so that neither carries the other's branches in its cells
                auto frame = [&](auto with) {
                    constexpr bool kD = decltype(with)::value;
                    double *row = nullptr;   // where m_t goes, if the frame is asked for
                    if constexpr (kD) row = pol.query(t);
                    const bool paths = kD && pol.path_out();
                    auto pre = [&](int64_t p) {
                        if constexpr (kD) return al[Form::slot(p, lo)];
                        else return 0.0;
                    };
                    auto cell = [&](int64_t p, double w, double dt) {
                        if constexpr (kD) {
                            const double m = dt + w;
                            if (row) row[p - lo] = m;
                            if (!paths) return;
                            if ((p >> unit) == ((int64_t)pt >> unit)) {
                                if (p == pt && d.through) d.through[t] = m;
                            } else if (m > bm) {
                                bm = m;
                                bp = (int32_t)p;
                            }
                        }
                    };
                    if (t == T - 1)
                        f.template bwd<true>(lo, hi, nlo, nhi, gn, vn, gc, vc, sstar, pre, cell, d.e_in);
                    else
                        f.template bwd<false>(lo, hi, nlo, nhi, gn, vn, gc, vc, sstar, pre, cell);
                    if constexpr (kD) {
                        if (d.alt || d.runner) f.best(bm, bp, red);
                        if (tid == 0 && paths) {
                            if (d.through && !(pt >= lo && pt < hi)) d.through[t] = NINF;
                            if (d.alt) d.alt[t] = bm;
                            if (d.runner) d.runner[t] = bp;
                        }
                        if (row) pol.row_done(row, lo, hi);
                    }
                };
                if (with_d)
                    frame(std::true_type{});
                else
                    frame(std::false_type{});
            }
            { double *x = gn; gn = gc; gc = x; }
            { double *x = vn; vn = vc; vc = x; }
            nlo = lo;
            nhi = hi;
            f.lab.bwd_commit();
            f.fence();
        }
    }
    if constexpr (!Pol::kPlain) pol.before(gn, vn, nlo, nhi);
    if (tid == 0) {
        res[d.idx].status = kStatusOk;
        res[d.idx].log_likelihood = score;
    }
}

// lattices walk slots (lattice i on workgroup i mod grid), as fb_ck_kernel's do
template <class Form>
__global__ __launch_bounds__(Form::NT) void margin_kernel(const MarginLattice *__restrict__ lats, int n, PostResult *res)
{
    __shared__ typename Form::template Shared<4> sh;
    __shared__ MarginRed red;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        Form f(lats[i], sh);
        if (lats[i].band_lo)
            margin_lattice<Form, BandTable>(f, res, red);
        else
            margin_lattice<Form, BandWalk>(f, res, red);
        f.sync();
    }
}

}  // namespace ka
