// ka_quantile.hip — translation unit of the boundary-quantile kernels (ka_quantile.hpp): for every cut position and level the
// first frame at which the posterior mass at or above the cut reaches the level, and the lattice log-likelihood of a
// caller-given terminal.
#include "ka_launch.hpp"
#include "ka_quantile.hpp"

namespace ka {

void launch_boundary_quantiles(const QuantLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<QuantLattice>({quantile_kernel<FbFast<1>>, quantile_kernel<FbFast<2>>, quantile_kernel<FbFast<3>>, quantile_kernel<FbFast<4>>},
                               quantile_kernel<FbGen<>>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
