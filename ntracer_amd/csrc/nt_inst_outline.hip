// nt_inst_outline.hip -- instantiates the outline kernels of nt_outline.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 10, in parallel with the render units); without the macro every dimension is instantiated here.
#include "nt_outline.hpp"

#define NT_DEFINE_OUTLINE(N)                                                                                                        \
    int nt_outline_fixed_##N(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtOutline &ol, bool draw) { \
        return launch_outline_fixed<N>(li, sc, tg, ol, draw);                                                                       \
    }
#define NT_DEFINE_OUTLINE_(N) NT_DEFINE_OUTLINE(N)

#ifdef NT_INST_N
NT_DEFINE_OUTLINE_(NT_INST_N)
#else
NT_DEFINE_OUTLINE(3) NT_DEFINE_OUTLINE(4) NT_DEFINE_OUTLINE(5) NT_DEFINE_OUTLINE(6) NT_DEFINE_OUTLINE(7) NT_DEFINE_OUTLINE(8) NT_DEFINE_OUTLINE(9) NT_DEFINE_OUTLINE(10)
#endif
