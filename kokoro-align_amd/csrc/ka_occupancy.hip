// ka_occupancy.hip — translation unit of the label occupancy kernels (ka_occupancy.hpp): per-frame label posteriors and the
// lattice log-likelihood of a caller-given terminal.
#include "ka_launch.hpp"
#include "ka_occupancy.hpp"

namespace ka {

void launch_label_posteriors(const OccLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<OccLattice>({occupancy_fast_kernel<1>, occupancy_fast_kernel<2>, occupancy_fast_kernel<3>, occupancy_fast_kernel<4>},
                           occupancy_generic_kernel, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
