// ka_tracking_resume.hip — translation unit of the kernels of the resumable tracking best path
// (ka_ctc_best_path_tracking_resume): ka_banded.hpp's frame loops over the self-steering band under the
// caller's boundary conditions (BandTrackingResume), a preparation without a table, and ka_resume.hip's walks back over the
// table the forward kernels wrote.
#include "ka_launch.hpp"
#include "ka_banded.hpp"

namespace ka {

// prep_resume_kernel without a table to check: the labels, the last row all dead, the lattice's two cells (the entry and the low
// end of frame T) -1, and the start row's +inf check
__global__ __launch_bounds__(256) void prep_tracking_resume_kernel(const BandLattice *__restrict__ lats, const ResumeRows *__restrict__ rows,
                                                                   int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    const ResumeRows &r = rows[blockIdx.x];
    int32_t *m = meta_of(meta, d.idx);
    if (r.fin)
        for (int p = threadIdx.x; p < d.L; p += blockDim.x) reinterpret_cast<uint32_t *>(r.fin)[p] = kDeadScoreBits;
    if (threadIdx.x < 2) r.entry[threadIdx.x] = -1;
    prep_labels(d, m);
    int inf = 0;
    if (r.init)
        for (int p = threadIdx.x; p < d.L; p += blockDim.x)
            if (reinterpret_cast<const uint32_t *>(r.init)[p] == 0x7f800000u) inf = 1;
    if (__syncthreads_or(inf) && threadIdx.x == 0) {
        atomicMin(&m[0], kStatusBadArgs);
        atomicOr(&m[2], kBandFlagBadTable);
        m[1] = -1;
    }
}

template <int M, bool ZL>
__global__ __launch_bounds__(64, kBandMinWaves) void forward_tracking_resume_wave_kernel(const BandLattice *__restrict__ lats,
                                                                                         const ResumeRows *__restrict__ rows, int32_t *meta,
                                                                                         uint32_t period)
{
    const BandLattice &d = lats[blockIdx.x];
    const int flags = __builtin_amdgcn_readfirstlane(meta_of(meta, d.idx)[2]);
    if (flags & kBandFlagBadTable) return;   // a +inf cell in the start row
    if (((flags & kFlagZeroLabel) != 0) != ZL) return;
    const ResumeRows &r = rows[blockIdx.x];
    BandTrackingResume src;
    src.period = period;
    src.end_rule = 0;   // (the end is the rows')
    src.init = (gcu32_t)r.init;
    src.fin = (gf32_t)r.fin;
    src.end = __builtin_amdgcn_readfirstlane(r.end);
    src.lo0 = (uint32_t)__builtin_amdgcn_readfirstlane(r.first_lo);
    src.lo_T = src.lo0;
    src.next = (gi32_t)(r.entry + 1);
    forward_banded_wave<M, ZL>(d, meta, src);
}

__global__ __launch_bounds__(256) void forward_tracking_resume_generic_kernel(const BandLattice *__restrict__ lats,
                                                                              const ResumeRows *__restrict__ rows, int32_t *meta, int period)
{
    forward_banded_generic<true, true>(lats[blockIdx.x], meta, period, 0, &rows[blockIdx.x]);
}

template <int M>
static void launch_forward_tracking_resume_wave(const BandLattice *lats, const ResumeRows *rows, int n, int32_t *meta, int period, hipStream_t s)
{
    forward_tracking_resume_wave_kernel<M, false><<<dim3(n), dim3(64), 0, s>>>(lats, rows, meta, (uint32_t)period);
    forward_tracking_resume_wave_kernel<M, true><<<dim3(n), dim3(64), 0, s>>>(lats, rows, meta, (uint32_t)period);
}

void launch_best_path_tracking_resume(const BandLattice *lats, const ResumeRows *rows, int n_fast, int n_generic, int max_move, int period,
                                      int32_t *meta, hipStream_t s)
{
    prep_tracking_resume_kernel<<<dim3(n_fast + n_generic), dim3(256), 0, s>>>(lats, rows, meta);
    if (n_fast > 0) {
        switch (max_move) {
        case 1: launch_forward_tracking_resume_wave<1>(lats, rows, n_fast, meta, period, s); break;
        case 2: launch_forward_tracking_resume_wave<2>(lats, rows, n_fast, meta, period, s); break;
        case 3: launch_forward_tracking_resume_wave<3>(lats, rows, n_fast, meta, period, s); break;
        default: launch_forward_tracking_resume_wave<4>(lats, rows, n_fast, meta, period, s); break;
        }
    }
    if (n_generic > 0)
        forward_tracking_resume_generic_kernel<<<dim3(n_generic), dim3(256), 0, s>>>(lats + n_fast, rows + n_fast, meta, period);
    launch_backtrace_resume(lats, rows, n_fast, n_generic, meta, s);
}

}  // namespace ka
