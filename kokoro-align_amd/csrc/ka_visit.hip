// ka_visit.hip — translation unit of the state visit kernels (ka_visit.hpp): the probability that the path passes through
// every position, the first time moment of the frame it leaves it at, and the lattice log-likelihood of a caller-given terminal.
#include "ka_launch.hpp"
#include "ka_visit.hpp"

namespace ka {

template void launch_state_visits<BandWalk>(const VisitLattice *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
