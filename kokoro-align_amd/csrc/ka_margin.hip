// ka_margin.hip — translation unit of the best-path margin kernels (ka_margin.hpp): the four one-wavefront kernels, the generic
// kernel and their launch.  One unit for both bands: a kernel chooses per lattice.
#include "ka_launch.hpp"
#include "ka_margin.hpp"

namespace ka {

void launch_path_margins(const MarginLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_slots<MarginLattice>({margin_kernel<MgFast<1>>, margin_kernel<MgFast<2>>, margin_kernel<MgFast<3>>, margin_kernel<MgFast<4>>},
                                   margin_kernel<MgGen>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
