// nt_inst_ao.hip -- instantiates the ambient occlusion kernel of nt_ao.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 10, in parallel with the render units); without the macro every dimension is instantiated here.
#include "nt_ao.hpp"

#define NT_DEFINE_AO(N)                                                                                        \
    int nt_ao_fixed_##N(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtAo &ao) { \
        return launch_ao_fixed<N>(li, sc, tg, ao);                                                             \
    }
#define NT_DEFINE_AO_(N) NT_DEFINE_AO(N)

#ifdef NT_INST_N
NT_DEFINE_AO_(NT_INST_N)
#else
NT_DEFINE_AO(3) NT_DEFINE_AO(4) NT_DEFINE_AO(5) NT_DEFINE_AO(6) NT_DEFINE_AO(7) NT_DEFINE_AO(8) NT_DEFINE_AO(9) NT_DEFINE_AO(10)
#endif
