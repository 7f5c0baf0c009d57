// ka_visit.hpp — state visit probabilities: for every position s of the blank-expanded labels the probability that the path
// passes through s at all and the first time moment of the frame at which it leaves s, over the band's paths that end at a
// caller-given terminal s*, and Z = alpha_{T-1}(s*).  Included by ka_visit.hip only.
//   exit_t(s) = P(state_t = s and (t = T-1 or state_{t+1} != s)) = gamma_t(s) r_t(s)
//   V(s) = sum over t of exit_t(s)        paths only move up, so a position is left once or never: V(s) in [0, 1]
//   X(s) = sum over t of t exit_t(s)      (X / V: the expected last frame of s, given that it is visited)
//
// Same lattice, band, moves, veto, statuses and form split as ka_duration.hpp (DESIGN.md sections 4.22 and 4.27): the driver of
// ka_fb_ck.hpp with VisitOut, which recomputes every block and adds gamma r of every cell - gamma the float the state posteriors
// write (fb_gamma), widened - to two float64 accumulators of its position, one add per frame whose band holds the position, in
// descending frame order.
//
// r_t(s) is the share of the backward recurrence's log-sum-exp at (t, s) that does not come from the stay j = 0.  With x_j the
// recurrence's terms (G_{t+1}(s + j), or -inf outside band t+1 or for a vetoed move), read from the next column that the driver
// hands over (next_column, the driver's opt-in hook):
//   t = T-1: r = 1;   x_0 = -inf: r = 1;   no x_j, j >= 1, finite: r = 0;
//   otherwise r = 1 - 2^(x_0 - (w + n)), clamped to [0, 1]: w + n is the recurrence's log-sum-exp again, w what the cell is
//   handed and n the next frame's maximum that the recurrence took off it.
// A cell with gamma = 0 adds exactly 0.0.  r <= 1 and the operand is the duration call's float, so V <= D and X <= B hold bit
// for bit, and a position that one frame's band holds has D's bits.
//
// Where the accumulators live: as in ka_duration.hpp.  Fast form: two LDS rings at the form's column slot, positions
// [hi_t, hi_{t+1}) retired before frame t's cells; generic form: the outputs themselves, zeroed first.
#pragma once
#include "ka_fb_ck.hpp"

namespace ka {

template <class Form>
struct VisitOut {
    static constexpr int NT = Form::NT;
    static constexpr bool kNextColumn = true;   // fb_ck hands next_column() the column of frame t + 1 before frame t's cells
    const VisitLattice &d;
    double *accV, *accX;   // fast form: the LDS rings; generic: the outputs (accX NULL without an exit_time)
    int64_t nlo, nhi;      // the band of frame t + 1 ([L, L) above the last frame)
    const double *gn, *vn;   // G_{t+1} and its vetoable copy
    double nprev;            // the maximum the recurrence takes off frame t + 1's log-sum-exp
    bool last;               // t = T-1: no frame above
    __device__ __forceinline__ VisitOut(const VisitLattice &d_, double *ringV, double *ringX)
        : d(d_), accV(Form::kWave ? ringV : d_.visit), accX(Form::kWave ? ringX : d_.xtime), nlo(d_.L), nhi(d_.L), gn(nullptr), vn(nullptr),
          nprev(0.0), last(true)
    {
        if (Form::kWave) {   // (whatever the slot's last lattice left)
            for (int s = threadIdx.x; s < 1024; s += NT) {
                accV[s] = 0.0;
                accX[s] = 0.0;
            }
        } else {
            for (int64_t p = threadIdx.x; p < d.L; p += NT) {
                accV[p] = 0.0;
                if (accX) accX[p] = 0.0;
            }
        }
    }
    // a lattice without a result: NaN over [0, L), and the status and log-likelihood of fb_fail_result
    __device__ __forceinline__ void fail(PostResult *res, int status)
    {
        for (int64_t p = threadIdx.x; p < d.L; p += NT) {
            reinterpret_cast<uint64_t *>(d.visit)[p] = kNaN64;
            if (d.xtime) reinterpret_cast<uint64_t *>(d.xtime)[p] = kNaN64;
        }
        fb_fail_result(d, res, status);
    }
    __device__ __forceinline__ bool recompute(int64_t) const { return true; }
    // the driver's hook, once a frame before cells(t, lo): frame t + 1's column and maximum (its band is kept here, as the
    // retire rule needs it)
    __device__ __forceinline__ void next_column(const double *gn_, const double *vn_, double nprev_, bool last_)
    {
        gn = gn_;
        vn = vn_;
        nprev = nprev_;
        last = last_;
    }
    // fast form, before frame t's cells: the positions [hi_t, hi_{t+1}) go to the outputs - the sums of those frame t + 1
    // held, 0 for those the band jumped over - and their slots are zeroed
    __device__ __forceinline__ void retire(int64_t hi)
    {
        for (int64_t p = hi + threadIdx.x; p < nhi; p += NT) {
            const bool held = p >= nlo;
            const int s = (int)Form::cslot(p);
            d.visit[p] = held ? accV[s] : 0.0;
            if (d.xtime) d.xtime[p] = held ? accX[s] : 0.0;
            if (held) {
                accV[s] = 0.0;
                accX[s] = 0.0;
            }
        }
    }
    __device__ __forceinline__ auto cells(int64_t t, int64_t lo)
    {
        const int64_t hi = (d.L - lo < d.beam) ? (int64_t)d.L : lo + d.beam;   // hi_t from lo_t, as post_band forms it
        if (Form::kWave) retire(hi);
        const int64_t blo = nlo, bhi = nhi;   // band t + 1, which the cells' terms lie in
        nlo = lo;
        nhi = hi;
        const double tt = (double)t, np = nprev, NINF = post_dninf();
        const bool top = last;
        const double *g1 = gn, *v1 = vn;
        double *aV = accV, *aX = accX;
        int M = d.max_move;
        if constexpr (Form::kWave) M = Form::kMoves;
        return [=](int64_t p, int32_t, double w, auto arg) {
            const double g = (double)fb_gamma(arg());
            double e = 0.0;
            if (g != 0.0) {   // (w is finite, and so is every sum below)
                double r = 1.0;
                const double x0 = (!top && p >= blo && p < bhi) ? g1[Form::cslot(p)] : NINF;
                if (x0 != NINF) {
                    bool other = false;
                    for (int j = 1; j < M; ++j) {
                        const int64_t u = p + j;
                        other = other || (u >= blo && u < bhi && (fb_skip(j) ? v1 : g1)[Form::cslot(u)] != NINF);
                    }
                    r = 1.0 - exp2(x0 - (w + np));
                    r = r < 1.0 ? r : 1.0;
                    r = (other && r > 0.0) ? r : 0.0;
                }
                e = g * r;
            }
            const int64_t s = Form::cslot(p);
            aV[s] += e;
            if (Form::kWave || aX) aX[s] += tt * e;
        };
    }
    __device__ __forceinline__ void cells_done() {}
    __device__ __forceinline__ void frame_end(int64_t t, int64_t lo, int64_t hi)
    {
        if (!Form::kWave || t != 0) return;
        post_wave_sync();   // frame 0's adds, made by the lanes that own the cells, before the lanes that write them out
        for (int64_t p = lo + threadIdx.x; p < hi; p += NT) {
            d.visit[p] = accV[Form::cslot(p)];
            if (d.xtime) d.xtime[p] = accX[Form::cslot(p)];
        }
    }
};

template <class Form>
__global__ __launch_bounds__(Form::NT) void visit_kernel(const VisitLattice *__restrict__ lats, int n, PostResult *res)
{
    __shared__ typename Form::template Shared<4> sh;
    __shared__ double cav[kPostCk];
    __shared__ double ringV[1024];   // (the rings are the fast form's: the generic kernel never names them, and they take none
    __shared__ double ringX[1024];   //  of its LDS)
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        Form f(lats[i], sh);
        VisitOut<Form> out(lats[i], ringV, ringX);
        fb_ck(f, res, cav, out);
        f.sync();
    }
}

}  // namespace ka
