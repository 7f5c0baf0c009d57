// ka_visit_banded.hip — translation unit of the state visit kernels over a caller-given band (ka_visit.hpp): the sibling
// unit's kernels and launch with BandTable in place of BandWalk.
#include "ka_launch.hpp"
#include "ka_visit.hpp"

namespace ka {

template void launch_state_visits<BandTable>(const Banded<VisitLattice> *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
