// ka_state_posterior_banded.hip — translation unit of the state-posterior kernels over a caller-given band
// (ka_state_posterior.hpp): the sibling unit's kernels and launch with BandTable in place of BandWalk.
#include "ka_launch.hpp"
#include "ka_state_posterior.hpp"

namespace ka {

template void launch_state_posteriors<BandTable>(const Banded<StateLattice> *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
