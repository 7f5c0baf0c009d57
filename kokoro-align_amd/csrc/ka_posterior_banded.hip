// ka_posterior_banded.hip — translation unit of the path-posterior kernels over a caller-given band (ka_posterior.hpp):
// ka_posterior.hip's kernels and launch with BandTable in place of BandWalk.
#include "ka_launch.hpp"
#include "ka_posterior.hpp"

namespace ka {

template void launch_posteriors<BandTable>(const Banded<PostLattice> *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
