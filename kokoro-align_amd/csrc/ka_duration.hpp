// ka_duration.hpp — expected state durations: for every position s of the blank-expanded labels the time-marginal of the
// posterior gamma_t(s) and its first time moment, over the band's paths that end at a caller-given terminal s*, and
// Z = alpha_{T-1}(s*).  Included by ka_duration.hip and ka_duration_banded.hip.
//   D(s) = sum over t of gamma_t(s)       expected number of frames spent in s
//   B(s) = sum over t of t gamma_t(s)     (B / D: the expected centre frame of s)
//
// Same lattice, band, moves, veto, statuses and form split as ka_occupancy.hpp (DESIGN.md sections 4.18 and 4.22): the
// driver of ka_fb_ck.hpp with DurOut, which recomputes every block as the occupancy does and adds every cell's gamma - the
// float the state posteriors write (fb_gamma) - to two float64 accumulators of its position.  The backward pass visits the
// frames T-1 ... 0, so a position receives one add per frame whose band holds it, in descending frame order: the sums are those
// of a sequential float64 loop over the rows of ka_ctc_state_posteriors, bit for bit.
//
// Where the accumulators live.  Fast form: lane l owns lo + l + 64 k, so a position's owner changes whenever lo moves; the
// accumulators are two more LDS rings (position p at the form's column slot, p & 1023), which one wavefront reads and writes in
// program order.  Going back the band slides down: before frame t's cells the positions [hi_t, hi_{t+1}) have left the band
// for good and are retired - written to the outputs, their slots zeroed - so a live position (the band is at most 1009 wide)
// never shares a slot with a sum that is still held.  After frame 0, [lo_0, hi_0) is written, and under a caller's table, whose
// lo_0 may lie above 0, zeros below it.  Positions no band holds get 0: the retiring loop runs over all of [hi_t, hi_{t+1}),
// however far a table's band jumped, and tells what frame t + 1 held from what it jumped over.
// Generic form: the outputs themselves at absolute positions, zeroed first, ordered from frame to frame by the barrier of
// the frame's reduction (as the working columns are).
#pragma once
#include "ka_fb_ck.hpp"

namespace ka {

// fb_ck's policy.  The forms differ in where the accumulators live (above); a position's place in them is the form's column slot.
template <class Form, class Band = BandWalk>
struct DurOut {
    static constexpr int NT = Form::NT;
    const DurLattice &d;
    double *accD, *accB;   // fast form: the LDS rings; generic: the outputs (accB NULL without a time_sum)
    int64_t nlo, nhi;      // fast form: the band of frame t + 1 ([L, L) above the last frame)
    __device__ __forceinline__ DurOut(const DurLattice &d_, double *ringD, double *ringB)
        : d(d_), accD(Form::kWave ? ringD : d_.dur), accB(Form::kWave ? ringB : d_.tsum), nlo(d_.L), nhi(d_.L)
    {
        if (Form::kWave) {   // (whatever the slot's last lattice left)
            for (int s = threadIdx.x; s < 1024; s += NT) {
                accD[s] = 0.0;
                accB[s] = 0.0;
            }
        } else {
            for (int64_t p = threadIdx.x; p < d.L; p += NT) {
                accD[p] = 0.0;
                if (accB) accB[p] = 0.0;
            }
        }
    }
    // a lattice without a result: NaN over [0, L), and the status and log-likelihood of fb_fail_result
    __device__ __forceinline__ void fail(PostResult *res, int status)
    {
        for (int64_t p = threadIdx.x; p < d.L; p += NT) {
            reinterpret_cast<uint64_t *>(d.dur)[p] = kNaN64;
            if (d.tsum) reinterpret_cast<uint64_t *>(d.tsum)[p] = kNaN64;
        }
        fb_fail_result(d, res, status);
    }
    __device__ __forceinline__ bool recompute(int64_t) const { return true; }
    // fast form, before frame t's cells: the positions [hi_t, hi_{t+1}) go to the outputs - the sums of those frame t + 1
    // held, 0 for those the band jumped over - and their slots are zeroed
    __device__ __forceinline__ void retire(int64_t lo, int64_t hi)
    {
        for (int64_t p = hi + threadIdx.x; p < nhi; p += NT) {
            const bool held = p >= nlo;
            const int s = (int)Form::cslot(p);
            d.dur[p] = held ? accD[s] : 0.0;
            if (d.tsum) d.tsum[p] = held ? accB[s] : 0.0;
            if (held) {
                accD[s] = 0.0;
                accB[s] = 0.0;
            }
        }
        nlo = lo;
        nhi = hi;
    }
    __device__ __forceinline__ auto cells(int64_t t, int64_t lo)
    {
        if (Form::kWave) {
            const int64_t hi = (d.L - lo < d.beam) ? (int64_t)d.L : lo + d.beam;   // hi_t from lo_t, as post_band forms it
            retire(lo, hi);
        }
        const double tt = (double)t;
        double *aD = accD, *aB = accB;
        return [=](int64_t p, int32_t, auto arg) {
            const double g = (double)fb_gamma(arg());
            const int64_t s = Form::cslot(p);
            aD[s] += g;
            if (Form::kWave || aB) aB[s] += tt * g;
        };
    }
    __device__ __forceinline__ void cells_done() {}
    __device__ __forceinline__ void frame_end(int64_t t, int64_t lo, int64_t hi)
    {
        if (!Form::kWave || t != 0) return;
        post_wave_sync();   // frame 0's adds, made by the lanes that own the cells, before the lanes that write them out
        for (int64_t p = lo + threadIdx.x; p < hi; p += NT) {
            d.dur[p] = accD[Form::cslot(p)];
            if (d.tsum) d.tsum[p] = accB[Form::cslot(p)];
        }
        if constexpr (Band::kTable)   // a table may start above 0: no band holds [0, lo_0)
            for (int64_t p = threadIdx.x; p < lo; p += NT) {
                d.dur[p] = 0.0;
                if (d.tsum) d.tsum[p] = 0.0;
            }
    }
};

template <class Form>
__global__ __launch_bounds__(Form::NT) void duration_kernel(const DurLattice *__restrict__ lats, int n, PostResult *res)
{
    __shared__ typename Form::template Shared<4> sh;
    __shared__ double cav[kPostCk];
    __shared__ double ringD[1024];   // (the rings are the fast form's: the generic kernel never names them, and they take none
    __shared__ double ringB[1024];   //  of its LDS)
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        Form f(lats[i], sh);
        DurOut<Form> out(lats[i], ringD, ringB);
        fb_ck(f, res, cav, out);
        f.sync();
    }
}
// ... over the caller's table (ka_duration_banded.hip)
template <class Form>
__global__ __launch_bounds__(Form::NT) void duration_banded_kernel(const Banded<DurLattice> *__restrict__ lats, int n, PostResult *res)
{
    __shared__ typename Form::template Shared<4> sh;
    __shared__ double cav[kPostCk];
    __shared__ double ringD[1024];
    __shared__ double ringB[1024];
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        Form f(lats[i], sh);
        DurOut<Form, BandTable> out(lats[i], ringD, ringB);
        fb_ck<Form, DurOut<Form, BandTable>, BandTable>(f, res, cav, out, lats[i].band_lo);
        f.sync();
    }
}

}  // namespace ka
