// ka_sample_banded.hip — translation unit of the path sampling kernels over a caller-given band (ka_sample.hpp): the sibling
// unit's kernels and launch with BandTable in place of BandWalk.
#include "ka_launch.hpp"
#include "ka_sample.hpp"

namespace ka {

template void launch_sample_paths<BandTable>(const Banded<SampleLattice> *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
