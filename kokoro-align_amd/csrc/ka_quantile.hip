// ka_quantile.hip — translation unit of the boundary-quantile kernels (ka_quantile.hpp): for every cut position and level the
// first frame at which the posterior mass at or above the cut reaches the level, and the lattice log-likelihood of a
// caller-given terminal.
#include "ka_launch.hpp"
#include "ka_quantile.hpp"

namespace ka {

template void launch_boundary_quantiles<BandWalk>(const QuantLattice *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
