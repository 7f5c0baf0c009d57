// ka_state_posterior.hip — translation unit of the state posterior kernels (ka_state_posterior.hpp): the posterior of every
// band position at chosen frames and the lattice log-likelihood of a caller-given terminal.
#include "ka_launch.hpp"
#include "ka_state_posterior.hpp"

namespace ka {

void launch_state_posteriors(const StateLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    if (n_fast > 0) {
        const dim3 grid(n_fast < kOccFastSlots ? n_fast : kOccFastSlots);
        switch (max_move) {
        case 1: hipLaunchKernelGGL(state_posterior_fast_kernel<1>, grid, dim3(64), 0, s, lats, n_fast, res); break;
        case 2: hipLaunchKernelGGL(state_posterior_fast_kernel<2>, grid, dim3(64), 0, s, lats, n_fast, res); break;
        case 3: hipLaunchKernelGGL(state_posterior_fast_kernel<3>, grid, dim3(64), 0, s, lats, n_fast, res); break;
        default: hipLaunchKernelGGL(state_posterior_fast_kernel<4>, grid, dim3(64), 0, s, lats, n_fast, res); break;
        }
    }
    if (n_generic > 0) {
        const dim3 grid(n_generic < kOccGenericSlots ? n_generic : kOccGenericSlots);
        hipLaunchKernelGGL(state_posterior_generic_kernel, grid, dim3(256), 0, s, lats + n_fast, n_generic, res);
    }
}

}  // namespace ka
