// ka_occupancy.hip — translation unit of the label occupancy kernels (ka_occupancy.hpp): per-frame label posteriors and the
// lattice log-likelihood of a caller-given terminal.
#include "ka_launch.hpp"
#include "ka_occupancy.hpp"

namespace ka {

void launch_label_posteriors(const OccLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<OccLattice>({occupancy_kernel<FbFast<1>>, occupancy_kernel<FbFast<2>>, occupancy_kernel<FbFast<3>>, occupancy_kernel<FbFast<4>>},
                           occupancy_kernel<FbGen<>>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
