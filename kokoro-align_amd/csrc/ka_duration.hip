// ka_duration.hip — translation unit of the state duration kernels (ka_duration.hpp): the expected number of frames spent in
// every position, its first time moment, and the lattice log-likelihood of a caller-given terminal.
#include "ka_launch.hpp"
#include "ka_duration.hpp"

namespace ka {

template void launch_state_durations<BandWalk>(const DurLattice *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
