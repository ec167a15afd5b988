// nt_inst_adaptive.hip -- instantiates the refine kernels of nt_adaptive.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 24, in parallel with the render units): BoxScene's kernel at every one of them, CompositeScene's up to 10;
// without the macro every dimension is instantiated here.
#include "nt_adaptive.hpp"

#define NT_DEFINE_REFINE(N)                                                                                             \
    int nt_refine_fixed_##N(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtRefine &rf, const NtTarget &tg) { \
        return launch_refine_fixed<N>(li, sc, rf, tg);                                                                  \
    }
#define NT_DEFINE_REFINE_BOX(N)                                                                   \
    int nt_refine_box_fixed_##N(const NtLaunchInfo &li, const NtRefine &rf, const NtTarget &tg) { \
        return launch_refine_box_fixed<N>(li, rf, tg);                                            \
    }
#define NT_DEFINE_REFINE_(N) NT_DEFINE_REFINE(N)
#define NT_DEFINE_REFINE_BOX_(N) NT_DEFINE_REFINE_BOX(N)

#ifdef NT_INST_N
#if NT_INST_N <= NT_DEV_MAX_FIXED
NT_DEFINE_REFINE_(NT_INST_N)
#endif
NT_DEFINE_REFINE_BOX_(NT_INST_N)
#else
NT_DEFINE_REFINE(3) NT_DEFINE_REFINE(4) NT_DEFINE_REFINE(5) NT_DEFINE_REFINE(6)
NT_DEFINE_REFINE(7) NT_DEFINE_REFINE(8) NT_DEFINE_REFINE(9) NT_DEFINE_REFINE(10)
NT_DEFINE_REFINE_BOX(3) NT_DEFINE_REFINE_BOX(4) NT_DEFINE_REFINE_BOX(5) NT_DEFINE_REFINE_BOX(6) NT_DEFINE_REFINE_BOX(7) NT_DEFINE_REFINE_BOX(8)
NT_DEFINE_REFINE_BOX(9) NT_DEFINE_REFINE_BOX(10) NT_DEFINE_REFINE_BOX(11) NT_DEFINE_REFINE_BOX(12) NT_DEFINE_REFINE_BOX(13) NT_DEFINE_REFINE_BOX(14)
NT_DEFINE_REFINE_BOX(15) NT_DEFINE_REFINE_BOX(16) NT_DEFINE_REFINE_BOX(17) NT_DEFINE_REFINE_BOX(18) NT_DEFINE_REFINE_BOX(19) NT_DEFINE_REFINE_BOX(20)
NT_DEFINE_REFINE_BOX(21) NT_DEFINE_REFINE_BOX(22) NT_DEFINE_REFINE_BOX(23) NT_DEFINE_REFINE_BOX(24)
#endif
