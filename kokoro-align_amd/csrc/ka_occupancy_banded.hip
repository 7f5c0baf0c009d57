// ka_occupancy_banded.hip — translation unit of the label-occupancy kernels over a caller-given band (ka_occupancy.hpp): the
// sibling unit's kernels and launch with BandTable in place of BandWalk.
#include "ka_launch.hpp"
#include "ka_occupancy.hpp"

namespace ka {

template void launch_label_posteriors<BandTable>(const Banded<OccLattice> *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
