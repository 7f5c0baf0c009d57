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
// Where the accumulators live, how positions retire from them and what no band holds: PairAcc (ka_pair_acc.hpp), which the
// state visits share.
#pragma once
#include "ka_pair_acc.hpp"

namespace ka {

// fb_ck's policy: PairAcc's hooks, and the value added per cell, gamma
template <class Form, class Band>
struct DurOut : PairAcc<Form, Band> {
    using Desc = DurLattice;
    using PairAcc<Form, Band>::PairAcc;
    __device__ __forceinline__ auto cells(int64_t t, int64_t lo)
    {
        this->retire(lo);
        const auto add = this->adder(t);
        return [=](int64_t p, int32_t, auto arg) { add(p, (double)fb_gamma(arg())); };
    }
};

template <class Band>
void launch_state_durations(const BandDesc<DurLattice, Band> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<DurOut, Band>(lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
