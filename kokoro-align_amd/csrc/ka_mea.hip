// ka_mea.hip — translation unit of the maximum-expected-accuracy alignment kernels (ka_mea.hpp): the band path that ends at a
// caller-given terminal and has the most frames at the right state in expectation, that expectation, and the lattice
// log-likelihood of the terminal.
#include "ka_launch.hpp"
#include "ka_mea.hpp"

namespace ka {

void launch_mea_path(const MeaLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<MeaLattice>({mea_kernel<FbFast<1>>, mea_kernel<FbFast<2>>, mea_kernel<FbFast<3>>, mea_kernel<FbFast<4>>}, mea_kernel<FbGen<>>,
                             lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
