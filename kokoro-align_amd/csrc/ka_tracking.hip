// ka_tracking.hip — translation unit of the kernels of the best path over a self-steering band (ka_ctc_best_path_tracking,
// DESIGN.md section 4.32): ka_banded.hpp's frame loops over the tracking band source, label preparation without a table.  The
// walk back is ka_banded.hip's, over the table the forward kernels wrote.
#include "ka_launch.hpp"
#include "ka_banded.hpp"

namespace ka {

// the labels alone, for the self-steering band, whose table is an output
__global__ __launch_bounds__(256) void prep_tracking_kernel(const BandLattice *__restrict__ lats, int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    int32_t *m = meta_of(meta, d.idx);
    prep_labels(d, m);
}

__global__ __launch_bounds__(256) void forward_tracking_generic_kernel(const BandLattice *__restrict__ lats, int32_t *meta, int period,
                                                                              int end_rule)
{
    forward_banded_generic<true>(lats[blockIdx.x], meta, period, end_rule);
}

template <int M>
static void launch_forward_tracking_wave(const BandLattice *lats, int n, int32_t *meta, int period, int end_rule, hipStream_t s)
{
    forward_tracking_wave_kernel<M, false><<<dim3(n), dim3(64), 0, s>>>(lats, meta, (uint32_t)period, end_rule);
    forward_tracking_wave_kernel<M, true><<<dim3(n), dim3(64), 0, s>>>(lats, meta, (uint32_t)period, end_rule);
}

void launch_best_path_tracking(const BandLattice *lats, int n_fast, int n_generic, int max_move, int period, int end_rule, int32_t *meta,
                               hipStream_t s)
{
    prep_tracking_kernel<<<dim3(n_fast + n_generic), dim3(256), 0, s>>>(lats, meta);
    if (n_fast > 0) {
        switch (max_move) {
        case 1: launch_forward_tracking_wave<1>(lats, n_fast, meta, period, end_rule, s); break;
        case 2: launch_forward_tracking_wave<2>(lats, n_fast, meta, period, end_rule, s); break;
        case 3: launch_forward_tracking_wave<3>(lats, n_fast, meta, period, end_rule, s); break;
        default: launch_forward_tracking_wave<4>(lats, n_fast, meta, period, end_rule, s); break;
        }
    }
    if (n_generic > 0) forward_tracking_generic_kernel<<<dim3(n_generic), dim3(256), 0, s>>>(lats + n_fast, meta, period, end_rule);
    launch_backtrace_banded(lats, n_fast, n_generic, meta, s);
}

}  // namespace ka
