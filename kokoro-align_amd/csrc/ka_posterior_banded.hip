// ka_posterior_banded.hip — translation unit of the path-posterior kernels over a caller-given band (ka_posterior.hpp,
// posterior_banded_kernel): ka_posterior.hip's pass with BandTable in place of BandWalk.
#include "ka_launch.hpp"
#include "ka_posterior.hpp"

namespace ka {

// launch_posteriors' split and grid
void launch_posteriors_banded(const Banded<PostLattice> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    using Kernel = void (*)(const Banded<PostLattice> *, PostResult *);
    static constexpr Kernel fast[4] = {posterior_banded_kernel<PostFast<1>>, posterior_banded_kernel<PostFast<2>>,
                                       posterior_banded_kernel<PostFast<3>>, posterior_banded_kernel<PostFast<4>>};
    if (n_fast > 0)
        hipLaunchKernelGGL(fast[(max_move >= 1 && max_move <= 3 ? max_move : 4) - 1], dim3(n_fast), dim3(PostFast<1>::NT), 0, s, lats, res);
    if (n_generic > 0) hipLaunchKernelGGL(posterior_banded_kernel<PostGen>, dim3(n_generic), dim3(PostGen::NT), 0, s, lats + n_fast, res);
}

}  // namespace ka
