// ka_margin_resume.hip — translation unit of the resumed best-path margin kernels (ka_margin_resume.hpp): the four one-wavefront
// kernels, the generic kernel and their launch.  One unit for both bands: a kernel chooses per lattice.
#include "ka_launch.hpp"
#include "ka_margin_resume.hpp"

namespace ka {

void launch_margins_resume(const MarginResumeLattice *lats, int n_fast, int n_generic, int max_move, PostResult *res, hipStream_t s)
{
    using D = MarginResumeLattice;
    launch_fb_slots<D>({margin_resume_kernel<MgFastOn<1, D>>, margin_resume_kernel<MgFastOn<2, D>>, margin_resume_kernel<MgFastOn<3, D>>,
                        margin_resume_kernel<MgFastOn<4, D>>},
                       margin_resume_kernel<MgGenOn<D>>, lats, n_fast, n_generic, max_move, res, s);
}

}  // namespace ka
