// ka_posterior.hip — translation unit of the forward-backward kernels (ka_posterior.hpp): best-path posteriors and the
// lattice log-likelihood.
#include "ka_launch.hpp"
#include "ka_posterior.hpp"

namespace ka {

// descriptors [0, n_fast) in the fast form (fast[M - 1], M = max_move, 4 above 3), then n_generic in the generic form; one
// workgroup per lattice
void launch_posteriors(const PostLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    using Kernel = void (*)(const PostLattice *, PostResult *);
    static constexpr Kernel fast[4] = {posterior_kernel<PostFast<1>>, posterior_kernel<PostFast<2>>, posterior_kernel<PostFast<3>>,
                                       posterior_kernel<PostFast<4>>};
    if (n_fast > 0)
        hipLaunchKernelGGL(fast[(max_move >= 1 && max_move <= 3 ? max_move : 4) - 1], dim3(n_fast), dim3(PostFast<1>::NT), 0, s, lats, res);
    if (n_generic > 0) hipLaunchKernelGGL(posterior_kernel<PostGen>, dim3(n_generic), dim3(PostGen::NT), 0, s, lats + n_fast, res);
}

}  // namespace ka
