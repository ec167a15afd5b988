// nt_inst_rays.hip -- instantiates the ray-colour kernels of nt_rays.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 24, in parallel with the render units): BoxScene's kernel at every one of them, CompositeScene's up to 10;
// without the macro every dimension is instantiated here.
#include "nt_rays.hpp"

#define NT_DEFINE_RAYS(N)                                                                                              \
    int nt_rays_fixed_##N(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtRayJob &job, const NtTarget &tg) { \
        return launch_rays_fixed<N>(li, sc, job, tg);                                                                  \
    }
#define NT_DEFINE_RAYS_BOX(N)                                                                    \
    int nt_rays_box_fixed_##N(const NtLaunchInfo &li, const NtRayJob &job, const NtTarget &tg) { \
        return launch_rays_box_fixed<N>(li, job, tg);                                            \
    }
#define NT_DEFINE_RAYS_(N) NT_DEFINE_RAYS(N)
#define NT_DEFINE_RAYS_BOX_(N) NT_DEFINE_RAYS_BOX(N)

#ifdef NT_INST_N
#if NT_INST_N <= NT_DEV_MAX_FIXED
NT_DEFINE_RAYS_(NT_INST_N)
#endif
NT_DEFINE_RAYS_BOX_(NT_INST_N)
#else
NT_DEFINE_RAYS(3) NT_DEFINE_RAYS(4) NT_DEFINE_RAYS(5) NT_DEFINE_RAYS(6)
NT_DEFINE_RAYS(7) NT_DEFINE_RAYS(8) NT_DEFINE_RAYS(9) NT_DEFINE_RAYS(10)
NT_DEFINE_RAYS_BOX(3) NT_DEFINE_RAYS_BOX(4) NT_DEFINE_RAYS_BOX(5) NT_DEFINE_RAYS_BOX(6) NT_DEFINE_RAYS_BOX(7) NT_DEFINE_RAYS_BOX(8)
NT_DEFINE_RAYS_BOX(9) NT_DEFINE_RAYS_BOX(10) NT_DEFINE_RAYS_BOX(11) NT_DEFINE_RAYS_BOX(12) NT_DEFINE_RAYS_BOX(13) NT_DEFINE_RAYS_BOX(14)
NT_DEFINE_RAYS_BOX(15) NT_DEFINE_RAYS_BOX(16) NT_DEFINE_RAYS_BOX(17) NT_DEFINE_RAYS_BOX(18) NT_DEFINE_RAYS_BOX(19) NT_DEFINE_RAYS_BOX(20)
NT_DEFINE_RAYS_BOX(21) NT_DEFINE_RAYS_BOX(22) NT_DEFINE_RAYS_BOX(23) NT_DEFINE_RAYS_BOX(24)
#endif
