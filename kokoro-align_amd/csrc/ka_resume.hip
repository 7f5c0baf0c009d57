// ka_resume.hip — translation unit of the kernels of the resumable best path (ka_ctc_best_path_resume, DESIGN.md section
// 4.34): ka_banded.hpp's frame loops over the table with the caller's boundary conditions (BandResume), a preparation that
// also checks the start row and presets the last row, and the walks back of ka_banded.hpp, which here report the cell of the
// start row they end on.
#include "ka_launch.hpp"
#include "ka_banded.hpp"

namespace ka {

// labels and table as prep_banded_kernel; the last row all dead until a forward pass has live cells to put there (so a lattice
// that fails keeps a row from which nothing resumes); a +inf cell in the start row is the lattice's KA_ERR_BAD_ARGS, and the
// kernels behind skip it like a lattice with a bad table
__global__ __launch_bounds__(256) void prep_resume_kernel(const BandLattice *__restrict__ lats, const ResumeRows *__restrict__ rows,
                                                          int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    const ResumeRows &r = rows[blockIdx.x];
    int32_t *m = meta_of(meta, d.idx);
    if (r.fin)
        for (int p = threadIdx.x; p < d.L; p += blockDim.x) reinterpret_cast<uint32_t *>(r.fin)[p] = kDeadScoreBits;
    if (threadIdx.x == 0) *r.entry = -1;
    prep_labels(d, m);
    if (!prep_band_table(d, m)) return;
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
__global__ __launch_bounds__(64, kBandMinWaves) void forward_resume_wave_kernel(const BandLattice *__restrict__ lats,
                                                                                const ResumeRows *__restrict__ rows, int32_t *meta)
{
    const BandLattice &d = lats[blockIdx.x];
    const int flags = __builtin_amdgcn_readfirstlane(meta_of(meta, d.idx)[2]);
    if (flags & kBandFlagBadTable) return;
    if (((flags & kFlagZeroLabel) != 0) != ZL) return;
    const ResumeRows &r = rows[blockIdx.x];
    BandResume src;
    src.init = (gcu32_t)r.init;
    src.fin = (gf32_t)r.fin;
    src.end = __builtin_amdgcn_readfirstlane(r.end);
    forward_banded_wave<M, ZL>(d, meta, src);
}

__global__ __launch_bounds__(256) void forward_resume_generic_kernel(const BandLattice *__restrict__ lats, const ResumeRows *__restrict__ rows,
                                                                     int32_t *meta)
{
    forward_banded_generic<false, true>(lats[blockIdx.x], meta, 0, 0, &rows[blockIdx.x]);
}

// the walks back: the position before frame 0 is the cell of the start row the path left from (one lane, a vector store)
__global__ __launch_bounds__(64) void backtrace_resume_wave_kernel(const BandLattice *__restrict__ lats, const ResumeRows *__restrict__ rows,
                                                                   const int32_t *meta)
{
    const int entry = backtrace_banded_wave(lats[blockIdx.x], meta);
    if (threadIdx.x == 0 && entry >= 0) *rows[blockIdx.x].entry = entry;
}

__global__ __launch_bounds__(64) void backtrace_resume_generic_kernel(const BandLattice *__restrict__ lats, const ResumeRows *__restrict__ rows,
                                                                      const int32_t *meta)
{
    const int64_t entry = backtrace_banded_generic(lats[blockIdx.x], meta);
    if (threadIdx.x == 0 && entry >= 0) *rows[blockIdx.x].entry = (int32_t)entry;
}

template <int M>
static void launch_forward_resume_wave(const BandLattice *lats, const ResumeRows *rows, int n, int32_t *meta, hipStream_t s)
{
    forward_resume_wave_kernel<M, false><<<dim3(n), dim3(64), 0, s>>>(lats, rows, meta);
    forward_resume_wave_kernel<M, true><<<dim3(n), dim3(64), 0, s>>>(lats, rows, meta);
}

void launch_backtrace_resume(const BandLattice *lats, const ResumeRows *rows, int n_fast, int n_generic, const int32_t *meta, hipStream_t s)
{
    if (n_fast > 0) backtrace_resume_wave_kernel<<<dim3(n_fast), dim3(64), 0, s>>>(lats, rows, meta);
    if (n_generic > 0) backtrace_resume_generic_kernel<<<dim3(n_generic), dim3(64), 0, s>>>(lats + n_fast, rows + n_fast, meta);
}

void launch_best_path_resume(const BandLattice *lats, const ResumeRows *rows, int n_fast, int n_generic, int max_move, int32_t *meta,
                             hipStream_t s)
{
    prep_resume_kernel<<<dim3(n_fast + n_generic), dim3(256), 0, s>>>(lats, rows, meta);
    if (n_fast > 0) {
        switch (max_move) {
        case 1: launch_forward_resume_wave<1>(lats, rows, n_fast, meta, s); break;
        case 2: launch_forward_resume_wave<2>(lats, rows, n_fast, meta, s); break;
        case 3: launch_forward_resume_wave<3>(lats, rows, n_fast, meta, s); break;
        default: launch_forward_resume_wave<4>(lats, rows, n_fast, meta, s); break;
        }
    }
    if (n_generic > 0) forward_resume_generic_kernel<<<dim3(n_generic), dim3(256), 0, s>>>(lats + n_fast, rows + n_fast, meta);
    launch_backtrace_resume(lats, rows, n_fast, n_generic, meta, s);
}

}  // namespace ka
