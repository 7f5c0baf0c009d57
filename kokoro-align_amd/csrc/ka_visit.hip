// ka_visit.hip — translation unit of the state visit kernels (ka_visit.hpp): the probability that the path passes through
// every position, the first time moment of the frame it leaves it at, and the lattice log-likelihood of a caller-given terminal.
#include "ka_launch.hpp"
#include "ka_visit.hpp"

namespace ka {

void launch_state_visits(const VisitLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<VisitLattice>({visit_kernel<FbFast<1>>, visit_kernel<FbFast<2>>, visit_kernel<FbFast<3>>, visit_kernel<FbFast<4>>},
                             visit_kernel<FbGen<>>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
