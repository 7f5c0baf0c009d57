// ka_sample.hip — translation unit of the path sampling kernels (ka_sample.hpp): whole alignments drawn from the posterior over
// the band's paths that end at a caller-given terminal, and the lattice log-likelihood of that terminal.
#include "ka_launch.hpp"
#include "ka_sample.hpp"

namespace ka {

template void launch_sample_paths<BandWalk>(const SampleLattice *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
