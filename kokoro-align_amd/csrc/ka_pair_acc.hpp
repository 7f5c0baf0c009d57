// ka_pair_acc.hpp — the pair accumulator of the expected state durations (ka_duration.hpp) and the state visit probabilities
// (ka_visit.hpp): both add a value e_t(s) of every band cell, and t e_t(s), to two float64 sums of the cell's position, and
// write the sums to two [L] outputs (PairLattice: sum, and tsum, which may be NULL).  PairAcc is the part of fb_ck's Out policy
// that the two calls share - every hook but cells(), which says what e is.
//
// The backward pass visits the frames T-1 ... 0, so a position receives one add per frame whose band holds it, in descending
// frame order: the sums are those of a sequential float64 loop over the frames, bit for bit.
//
// Where the sums live.  Fast form: lane l owns lo + l + 64 k, so a position's owner changes whenever lo moves; the sums are
// two LDS rings (position p at the form's column slot, p & 1023), which one wavefront reads and writes in program order.
// Going back the band slides down: before frame t's cells the positions [hi_t, hi_{t+1}) have left the band for good and are
// retired - written to the outputs, their slots zeroed - so a live position (the band is at most 1009 wide) never shares a
// slot with a sum that is still held.  After frame 0, [lo_0, hi_0) is written, and under a caller's table, whose lo_0 may lie
// above 0, zeros below it.  Positions no band holds get 0: the retiring loop runs over all of [hi_t, hi_{t+1}), however far a
// table's band jumped, and tells what frame t + 1 held from what it jumped over.
// Generic form: the outputs themselves at absolute positions, zeroed first, ordered from frame to frame by the barrier of
// the frame's reduction (as the working columns are).
#pragma once
#include "ka_fb_ck.hpp"

namespace ka {

template <class Form_, class Band>
struct PairAcc {
    using Form = Form_;
    using Lds = FbRings<Form::kWave>;
    static constexpr int NT = Form::NT;
    const PairLattice &d;
    double *acc0, *acc1;   // fast form: the LDS rings; generic: the outputs (acc1 NULL without a tsum)
    int64_t nlo, nhi;      // the band of frame t + 1 ([L, L) above the last frame)
    __device__ __forceinline__ PairAcc(const PairLattice &d_, Form &, Lds &lds)
        : d(d_), acc0(Form::kWave ? lds.ring(0) : d_.sum), acc1(Form::kWave ? lds.ring(1) : d_.tsum), nlo(d_.L), nhi(d_.L)
    {
        if (Form::kWave) {   // (whatever the slot's last lattice left)
            for (int s = threadIdx.x; s < 1024; s += NT) {
                acc0[s] = 0.0;
                acc1[s] = 0.0;
            }
        } else {
            for (int64_t p = threadIdx.x; p < d.L; p += NT) {
                acc0[p] = 0.0;
                if (acc1) acc1[p] = 0.0;
            }
        }
    }
    // a lattice without a result: NaN over [0, L), and the status and log-likelihood of fb_fail_result
    __device__ __forceinline__ void fail(PostResult *res, int status)
    {
        for (int64_t p = threadIdx.x; p < d.L; p += NT) {
            reinterpret_cast<uint64_t *>(d.sum)[p] = kNaN64;
            if (d.tsum) reinterpret_cast<uint64_t *>(d.tsum)[p] = kNaN64;
        }
        fb_fail_result(d, res, status);
    }
    __device__ __forceinline__ bool recompute(int64_t) const { return true; }
    // before frame t's cells, lo = lo_t.  Fast form: the positions [hi_t, hi_{t+1}) go to the outputs - the sums of those
    // frame t + 1 held, 0 for those the band jumped over - and their slots are zeroed.  Either form: frame t's band is kept.
    __device__ __forceinline__ void retire(int64_t lo)
    {
        const int64_t hi = (d.L - lo < d.beam) ? (int64_t)d.L : lo + d.beam;   // hi_t from lo_t, as post_band forms it
        if (Form::kWave)
            for (int64_t p = hi + threadIdx.x; p < nhi; p += NT) {
                const bool held = p >= nlo;
                const int s = (int)Form::cslot(p);
                d.sum[p] = held ? acc0[s] : 0.0;
                if (d.tsum) d.tsum[p] = held ? acc1[s] : 0.0;
                if (held) {
                    acc0[s] = 0.0;
                    acc1[s] = 0.0;
                }
            }
        nlo = lo;
        nhi = hi;
    }
    // frame t's adds: a callable (p, e)
    __device__ __forceinline__ auto adder(int64_t t) const
    {
        const double tt = (double)t;
        double *a0 = acc0, *a1 = acc1;
        return [=](int64_t p, double e) {
            const int64_t s = Form::cslot(p);
            a0[s] += e;
            if (Form::kWave || a1) a1[s] += tt * e;
        };
    }
    __device__ __forceinline__ void cells_done() {}
    __device__ __forceinline__ void frame_end(int64_t t, int64_t lo, int64_t hi)
    {
        if (!Form::kWave || t != 0) return;
        post_wave_sync();   // frame 0's adds, made by the lanes that own the cells, before the lanes that write them out
        for (int64_t p = lo + threadIdx.x; p < hi; p += NT) {
            d.sum[p] = acc0[Form::cslot(p)];
            if (d.tsum) d.tsum[p] = acc1[Form::cslot(p)];
        }
        if constexpr (Band::kTable)   // a table may start above 0: no band holds [0, lo_0)
            for (int64_t p = threadIdx.x; p < lo; p += NT) {
                d.sum[p] = 0.0;
                if (d.tsum) d.tsum[p] = 0.0;
            }
    }
};

}  // namespace ka
