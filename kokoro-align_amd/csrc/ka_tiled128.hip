// ka_tiled128.hip — translation unit of the 128-position tile pipeline (ka_tiled128.hpp): a workgroup of three wavefronts
// per tile - compute, emission look-up, feeder.
#include "ka_launch.hpp"
#include "ka_tiled128.hpp"

#include <algorithm>

namespace ka {

template <int M, int PITCH, bool CONTIG>
struct Tiled128 {
    static void launch(const TileLaunch &a, hipStream_t s)
    {
        const unsigned need = (unsigned)TsLds<PITCH, CONTIG>::kTotal;
        hipLaunchKernelGGL((forward_ts_kernel<M, PITCH, CONTIG>), dim3((unsigned)a.n_tasks), dim3(192), std::max(need, a.lds), s, a.lats, a.tasks, a.n_tasks, a.meta,
                           a.halo, a.aux, a.ticket, a.verify, a.stats, a.cu_rank);
    }
};

void launch_forward_tiled128(const TileLaunch &a, hipStream_t s) { launch_tile_instance<Tiled128>(a, s); }

}  // namespace ka
