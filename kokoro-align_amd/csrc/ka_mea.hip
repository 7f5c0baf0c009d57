// ka_mea.hip — translation unit of the maximum-expected-accuracy alignment kernels (ka_mea.hpp): the band path that ends at a
// caller-given terminal and has the most frames at the right state in expectation, that expectation, and the lattice
// log-likelihood of the terminal.
#include "ka_launch.hpp"
#include "ka_mea.hpp"

namespace ka {

template void launch_mea_path<BandWalk>(const MeaLattice *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
