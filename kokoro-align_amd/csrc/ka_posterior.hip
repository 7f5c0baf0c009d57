// ka_posterior.hip — translation unit of the forward-backward kernels (ka_posterior.hpp): best-path posteriors and the
// lattice log-likelihood.
#include "ka_launch.hpp"
#include "ka_posterior.hpp"

namespace ka {

template void launch_posteriors<BandWalk>(const PostLattice *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
