// ka_fb_resume.hip — translation unit of the forward-backward kernels under the caller's boundary conditions
// (ka_fb_resume.hpp): the checkpointed driver with FbCallerBound and ResumeOut, over a caller's table (the call has no diagonal form).
#include "ka_launch.hpp"
#include "ka_fb_resume.hpp"

namespace ka {

template void launch_posteriors_resume<BandTable>(const Banded<ResumeFbLattice> *, int, int, int, PostResult *, hipStream_t);

}  // namespace ka
