// ka_posterior.hip — translation unit of the forward-backward kernels (ka_posterior.hpp): best-path posteriors and the
// lattice log-likelihood.
#include "ka_launch.hpp"
#include "ka_posterior.hpp"

namespace ka {

void launch_posteriors(const PostLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    if (n_fast > 0) {
        switch (max_move) {
        case 1: hipLaunchKernelGGL(posterior_fast_kernel<1>, dim3(n_fast), dim3(64), 0, s, lats, res); break;
        case 2: hipLaunchKernelGGL(posterior_fast_kernel<2>, dim3(n_fast), dim3(64), 0, s, lats, res); break;
        case 3: hipLaunchKernelGGL(posterior_fast_kernel<3>, dim3(n_fast), dim3(64), 0, s, lats, res); break;
        default: hipLaunchKernelGGL(posterior_fast_kernel<4>, dim3(n_fast), dim3(64), 0, s, lats, res); break;
        }
    }
    if (n_generic > 0) hipLaunchKernelGGL(posterior_generic_kernel, dim3(n_generic), dim3(256), 0, s, lats + n_fast, res);
}

}  // namespace ka
