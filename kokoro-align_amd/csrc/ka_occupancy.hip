// ka_occupancy.hip — translation unit of the label occupancy kernels (ka_occupancy.hpp): per-frame label posteriors and the
// lattice log-likelihood of a caller-given terminal.
#include "ka_launch.hpp"
#include "ka_occupancy.hpp"

namespace ka {

void launch_label_posteriors(const OccLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    if (n_fast > 0) {
        const dim3 grid(n_fast < kOccFastSlots ? n_fast : kOccFastSlots);
        switch (max_move) {
        case 1: hipLaunchKernelGGL(occupancy_fast_kernel<1>, grid, dim3(64), 0, s, lats, n_fast, res); break;
        case 2: hipLaunchKernelGGL(occupancy_fast_kernel<2>, grid, dim3(64), 0, s, lats, n_fast, res); break;
        case 3: hipLaunchKernelGGL(occupancy_fast_kernel<3>, grid, dim3(64), 0, s, lats, n_fast, res); break;
        default: hipLaunchKernelGGL(occupancy_fast_kernel<4>, grid, dim3(64), 0, s, lats, n_fast, res); break;
        }
    }
    if (n_generic > 0) {
        const dim3 grid(n_generic < kOccGenericSlots ? n_generic : kOccGenericSlots);
        hipLaunchKernelGGL(occupancy_generic_kernel, grid, dim3(256), 0, s, lats + n_fast, n_generic, res);
    }
}

}  // namespace ka
