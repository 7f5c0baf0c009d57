// ka_banded.hip — translation unit of the kernels of the best path over a caller-given band (ka_banded.hpp): table and label
// preparation, the one-wavefront forward pass and walk back, the generic pair.  The walks back also serve ka_tracking.hip;
// their bodies are ka_banded.hpp's, which ka_resume.hip's walks share.
#include "ka_launch.hpp"
#include "ka_banded.hpp"

namespace ka {

// ---------------------------------------------------------------------------------------
// preparation: labels (validate, scale by 4, zero-pad), the band table (validate, shift, pad)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_banded_kernel(const BandLattice *__restrict__ lats, int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    int32_t *m = meta_of(meta, d.idx);
    prep_labels(d, m);
    prep_band_table(d, m);
}
// ---------------------------------------------------------------------------------------
// the walks back (ka_banded.hpp)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void backtrace_banded_wave_kernel(const BandLattice *__restrict__ lats, const int32_t *meta)
{
    backtrace_banded_wave(lats[blockIdx.x], meta);
}

// ---------------------------------------------------------------------------------------
// generic form: the forward kernel over the table, the walk back
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void forward_banded_generic_kernel(const BandLattice *__restrict__ lats, int32_t *meta)
{
    forward_banded_generic<false>(lats[blockIdx.x], meta, 0, 0);
}

__global__ __launch_bounds__(64) void backtrace_banded_generic_kernel(const BandLattice *__restrict__ lats, const int32_t *meta)
{
    backtrace_banded_generic(lats[blockIdx.x], meta);
}

template <int M>
static void launch_forward_banded_wave(const BandLattice *lats, int n, int32_t *meta, hipStream_t s)
{
    forward_banded_wave_kernel<M, false><<<dim3(n), dim3(64), 0, s>>>(lats, meta);
    forward_banded_wave_kernel<M, true><<<dim3(n), dim3(64), 0, s>>>(lats, meta);
}

void launch_backtrace_banded(const BandLattice *lats, int n_fast, int n_generic, const int32_t *meta, hipStream_t s)
{
    if (n_fast > 0) backtrace_banded_wave_kernel<<<dim3(n_fast), dim3(64), 0, s>>>(lats, meta);
    if (n_generic > 0) backtrace_banded_generic_kernel<<<dim3(n_generic), dim3(64), 0, s>>>(lats + n_fast, meta);
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
    }
    if (n_generic > 0) forward_banded_generic_kernel<<<dim3(n_generic), dim3(256), 0, s>>>(lats + n_fast, meta);
    launch_backtrace_banded(lats, n_fast, n_generic, meta, s);
}

}  // namespace ka
