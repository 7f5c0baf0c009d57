// ka_visit.hpp — state visit probabilities: for every position s of the blank-expanded labels the probability that the path
// passes through s at all and the first time moment of the frame at which it leaves s, over the band's paths that end at a
// caller-given terminal s*, and Z = alpha_{T-1}(s*).  Included by ka_visit.hip and ka_visit_banded.hip only.
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
// Where the accumulators live, how positions retire from them and what no band holds: PairAcc (ka_pair_acc.hpp), as for the
// durations.
#pragma once
#include "ka_pair_acc.hpp"

namespace ka {

// fb_ck's policy: PairAcc's hooks, the next column, and the value added per cell, gamma r
template <class Form, class Band>
struct VisitOut : PairAcc<Form, Band> {
    using Desc = VisitLattice;
    static constexpr bool kNextColumn = true;   // fb_ck hands next_column() the column of frame t + 1 before frame t's cells
    const double *gn = nullptr, *vn = nullptr;   // G_{t+1} and its vetoable copy
    double nprev = 0.0;                           // the maximum the recurrence takes off frame t + 1's log-sum-exp
    bool last = true;                             // t = T-1: no frame above
    using PairAcc<Form, Band>::PairAcc;
    // the driver's hook, once a frame before cells(t, lo): frame t + 1's column and maximum (PairAcc keeps its band)
    __device__ __forceinline__ void next_column(const double *gn_, const double *vn_, double nprev_, bool last_)
    {
        gn = gn_;
        vn = vn_;
        nprev = nprev_;
        last = last_;
    }
    __device__ __forceinline__ auto cells(int64_t t, int64_t lo)
    {
        const int64_t blo = this->nlo, bhi = this->nhi;   // band t + 1, which the cells' terms lie in: what the driver's walk handed
                                                          // retire() a frame ago, so a stepping table's own value of t + 1
        this->retire(lo);
        const auto add = this->adder(t);
        const double np = nprev, NINF = post_dninf();
        const bool top = last;
        const double *g1 = gn, *v1 = vn;
        int M = this->d.max_move;
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
            add(p, e);
        };
    }
};

template <class Band>
void launch_state_visits(const BandDesc<VisitLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<VisitOut, Band>(lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
