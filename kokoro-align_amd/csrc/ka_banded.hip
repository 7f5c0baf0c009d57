// ka_banded.hip — translation unit of the kernels of the best path over a caller-given band (ka_banded.hpp): table and label
// preparation, the one-wavefront forward pass and walk back, the generic pair.
#include "ka_launch.hpp"
#include "ka_banded.hpp"

namespace ka {

template <int M>
static void launch_forward_banded_wave(const BandLattice *lats, int n, int32_t *meta, hipStream_t s)
{
    forward_banded_wave_kernel<M, false><<<dim3(n), dim3(64), 0, s>>>(lats, meta);
    forward_banded_wave_kernel<M, true><<<dim3(n), dim3(64), 0, s>>>(lats, meta);
}

void launch_best_path_banded(const BandLattice *lats, int n_fast, int n_generic, int max_move, int32_t *meta, hipStream_t s)
{
    prep_banded_kernel<<<dim3(n_fast + n_generic), dim3(256), 0, s>>>(lats, meta);
    if (n_fast > 0) {
        switch (max_move) {
        case 1: launch_forward_banded_wave<1>(lats, n_fast, meta, s); break;
        case 2: launch_forward_banded_wave<2>(lats, n_fast, meta, s); break;
        case 3: launch_forward_banded_wave<3>(lats, n_fast, meta, s); break;
        default: launch_forward_banded_wave<4>(lats, n_fast, meta, s); break;
        }
        backtrace_banded_wave_kernel<<<dim3(n_fast), dim3(64), 0, s>>>(lats, meta);
    }
    if (n_generic > 0) {
        forward_banded_generic_kernel<<<dim3(n_generic), dim3(256), 0, s>>>(lats + n_fast, meta);
        backtrace_banded_generic_kernel<<<dim3(n_generic), dim3(64), 0, s>>>(lats + n_fast, meta);
    }
}

}  // namespace ka
