// ka_occupancy.hip — translation unit of the label occupancy kernels (ka_occupancy.hpp): per-frame label posteriors and the
// lattice log-likelihood of a caller-given terminal.
#include "ka_launch.hpp"
#include "ka_occupancy.hpp"

namespace ka {

template void launch_label_posteriors<BandWalk>(const OccLattice *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
