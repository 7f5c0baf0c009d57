// ka_quantile_banded.hip — translation unit of the boundary-quantile kernels over a caller-given band (ka_quantile.hpp): the
// sibling unit's kernels and launch with BandTable in place of BandWalk; a cut's start frame comes from the accepted table
// (QuantOut::begin), not from the host.
#include "ka_launch.hpp"
#include "ka_quantile.hpp"

namespace ka {

template void launch_boundary_quantiles<BandTable>(const Banded<QuantLattice> *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
