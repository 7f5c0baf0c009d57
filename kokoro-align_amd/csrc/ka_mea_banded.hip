// ka_mea_banded.hip — translation unit of the MEA path kernels over a caller-given band (ka_mea.hpp): the sibling unit's
// kernels and launch with BandTable in place of BandWalk; the forward walk steps the table the backward pass stored its codes
// under.
#include "ka_launch.hpp"
#include "ka_mea.hpp"

namespace ka {

template void launch_mea_path<BandTable>(const Banded<MeaLattice> *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
