// ka_duration.hip — translation unit of the state duration kernels (ka_duration.hpp): the expected number of frames spent in
// every position, its first time moment, and the lattice log-likelihood of a caller-given terminal.
#include "ka_launch.hpp"
#include "ka_duration.hpp"

namespace ka {

void launch_state_durations(const DurLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<DurLattice>({duration_kernel<FbFast<1>>, duration_kernel<FbFast<2>>, duration_kernel<FbFast<3>>, duration_kernel<FbFast<4>>},
                           duration_kernel<FbGen<>>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
