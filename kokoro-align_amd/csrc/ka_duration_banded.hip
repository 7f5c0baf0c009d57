// ka_duration_banded.hip — translation unit of the state-duration kernels over a caller-given band (ka_duration.hpp): the
// sibling unit's kernels and launch with BandTable in place of BandWalk.
#include "ka_launch.hpp"
#include "ka_duration.hpp"

namespace ka {

template void launch_state_durations<BandTable>(const Banded<DurLattice> *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
