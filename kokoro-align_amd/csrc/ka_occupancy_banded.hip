// ka_occupancy_banded.hip — translation unit of the label occupancy kernels over a caller-given band (ka_occupancy.hpp,
// occupancy_banded_kernel): the sibling unit's driver with BandTable in place of BandWalk.
#include "ka_launch.hpp"
#include "ka_occupancy.hpp"

namespace ka {

void launch_label_posteriors_banded(const Banded<OccLattice> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<Banded<OccLattice>>({occupancy_banded_kernel<FbFast<1>>, occupancy_banded_kernel<FbFast<2>>, occupancy_banded_kernel<FbFast<3>>, occupancy_banded_kernel<FbFast<4>>},
                                 occupancy_banded_kernel<FbGen<>>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
