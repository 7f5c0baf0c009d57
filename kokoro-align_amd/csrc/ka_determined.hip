// ka_determined.hip — translation unit of the walk that finds a resumed best path's determined prefix
// (ka_ctc_best_path_determined, ka_ctc_best_path_tracking_determined): launched behind the forward
// kernels and the walks back of ka_resume.hip / ka_tracking_resume.hip, over the move codes and the last row they left.
#include "ka_launch.hpp"
#include "ka_determined.hpp"

namespace ka {

// `det`: one int32 per lattice of the batch, in the caller's order (one lane, a vector store)
__global__ __launch_bounds__(64) void determined_wave_kernel(const BandLattice *__restrict__ lats, const ResumeRows *__restrict__ rows,
                                                             const int32_t *meta, int32_t *det)
{
    const BandLattice &d = lats[blockIdx.x];
    const int v = determined_wave(d, rows[blockIdx.x].fin, meta);
    if (threadIdx.x == 0) det[d.idx] = v;
}

__global__ __launch_bounds__(256) void determined_generic_kernel(const BandLattice *__restrict__ lats, const ResumeRows *__restrict__ rows,
                                                                 const int32_t *meta, int32_t *det)
{
    const BandLattice &d = lats[blockIdx.x];
    const int v = determined_generic(d, rows[blockIdx.x].fin, meta);
    if (threadIdx.x == 0) det[d.idx] = v;
}

void launch_determined(const BandLattice *lats, const ResumeRows *rows, int n_fast, int n_generic, const int32_t *meta, int32_t *det,
                       hipStream_t s)
{
    if (n_fast > 0) determined_wave_kernel<<<dim3(n_fast), dim3(64), 0, s>>>(lats, rows, meta, det);
    if (n_generic > 0) determined_generic_kernel<<<dim3(n_generic), dim3(256), 0, s>>>(lats + n_fast, rows + n_fast, meta, det);
}

}  // namespace ka
