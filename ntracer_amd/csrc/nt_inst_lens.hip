// nt_inst_lens.hip -- instantiates the packet route of a render through a lens (nt_lens.hpp).  The build compiles this file once
// per dimension (-DNT_INST_N=3 .. 10, in parallel with the render units); without the macro every dimension is instantiated here.
#include "nt_lens.hpp"

#define NT_DEFINE_LENS(N)                                                                                              \
    int nt_lens_fixed_##N(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtLens &ln) {    \
        return launch_lens_fixed<N>(li, sc, tg, ln);                                                                   \
    }
#define NT_DEFINE_LENS_(N) NT_DEFINE_LENS(N)

#ifdef NT_INST_N
NT_DEFINE_LENS_(NT_INST_N)
#else
NT_DEFINE_LENS(3) NT_DEFINE_LENS(4) NT_DEFINE_LENS(5) NT_DEFINE_LENS(6)
NT_DEFINE_LENS(7) NT_DEFINE_LENS(8) NT_DEFINE_LENS(9) NT_DEFINE_LENS(10)
#endif
