// ka_state_posterior.hip — translation unit of the state posterior kernels (ka_state_posterior.hpp): the posterior of every
// band position at chosen frames and the lattice log-likelihood of a caller-given terminal.
#include "ka_launch.hpp"
#include "ka_state_posterior.hpp"

namespace ka {

template void launch_state_posteriors<BandWalk>(const StateLattice *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
