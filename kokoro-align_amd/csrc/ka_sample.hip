// ka_sample.hip — translation unit of the path sampling kernels (ka_sample.hpp): whole alignments drawn from the posterior over
// the band's paths that end at a caller-given terminal, and the lattice log-likelihood of that terminal.
#include "ka_launch.hpp"
#include "ka_sample.hpp"

namespace ka {

void launch_sample_paths(const SampleLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_slots<SampleLattice>({sample_kernel<FbFast<1>>, sample_kernel<FbFast<2>>, sample_kernel<FbFast<3>>, sample_kernel<FbFast<4>>},
                                   sample_kernel<FbGen<>>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
