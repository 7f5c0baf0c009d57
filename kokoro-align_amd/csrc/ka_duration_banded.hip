// ka_duration_banded.hip — translation unit of the state-duration kernels over a caller-given band (ka_duration.hpp,
// duration_banded_kernel): the sibling unit's driver with BandTable in place of BandWalk.
#include "ka_launch.hpp"
#include "ka_duration.hpp"

namespace ka {

void launch_state_durations_banded(const Banded<DurLattice> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<Banded<DurLattice>>({duration_banded_kernel<FbFast<1>>, duration_banded_kernel<FbFast<2>>, duration_banded_kernel<FbFast<3>>, duration_banded_kernel<FbFast<4>>},
                                 duration_banded_kernel<FbGen<>>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
