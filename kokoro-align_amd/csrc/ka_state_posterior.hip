// ka_state_posterior.hip — translation unit of the state posterior kernels (ka_state_posterior.hpp): the posterior of every
// band position at chosen frames and the lattice log-likelihood of a caller-given terminal.
#include "ka_launch.hpp"
#include "ka_state_posterior.hpp"

namespace ka {

void launch_state_posteriors(const StateLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    launch_fb_ck<StateLattice>({state_posterior_kernel<FbFast<1>>, state_posterior_kernel<FbFast<2>>, state_posterior_kernel<FbFast<3>>,
                                state_posterior_kernel<FbFast<4>>},
                               state_posterior_kernel<FbGen<>>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
