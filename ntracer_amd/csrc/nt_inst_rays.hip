// nt_inst_rays.hip -- instantiates the ray-colour kernels of nt_rays.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 24, in parallel with the render units): BoxScene's kernel at every one of them, CompositeScene's up to 10.
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_rays.hpp"
#include "nt_dispatch.hpp"

#if NT_INST_N <= NT_DEV_MAX_FIXED
template <> int nt_rays_fixed<NT_INST_N>(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtRayJob &job, const NtTarget &tg) {
    return launch_rays_fixed<NT_INST_N>(li, sc, job, tg);
}
#endif
template <> int nt_rays_box_fixed<NT_INST_N>(const NtLaunchInfo &li, const NtRayJob &job, const NtTarget &tg) {
    return launch_rays_box_fixed<NT_INST_N>(li, job, tg);
}
