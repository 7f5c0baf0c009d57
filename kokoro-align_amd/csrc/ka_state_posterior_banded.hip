// ka_state_posterior_banded.hip — translation unit of the state-posterior kernels over a caller-given band (ka_state_posterior.hpp,
// state_posterior_banded_kernel): the sibling unit's driver with BandTable in place of BandWalk.
#include "ka_launch.hpp"
#include "ka_state_posterior.hpp"

namespace ka {

void launch_state_posteriors_banded(const Banded<StateLattice> *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<Banded<StateLattice>>({state_posterior_banded_kernel<FbFast<1>>, state_posterior_banded_kernel<FbFast<2>>, state_posterior_banded_kernel<FbFast<3>>, state_posterior_banded_kernel<FbFast<4>>},
                                 state_posterior_banded_kernel<FbGen<>>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
