// nt_inst_parallel.hip -- instantiates the packet route of a render under the parallel projection (nt_parallel.hpp).  The build
// compiles this file once per dimension (-DNT_INST_N=3 .. 10, in parallel with the render units); without the macro every
// dimension is instantiated here.
#include "nt_parallel.hpp"

#define NT_DEFINE_PARALLEL(N)                                                                                                  \
    int nt_parallel_fixed_##N(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtParallel &pl) {    \
        return launch_parallel_fixed<N>(li, sc, tg, pl);                                                                       \
    }
#define NT_DEFINE_PARALLEL_(N) NT_DEFINE_PARALLEL(N)

#ifdef NT_INST_N
NT_DEFINE_PARALLEL_(NT_INST_N)
#else
NT_DEFINE_PARALLEL(3) NT_DEFINE_PARALLEL(4) NT_DEFINE_PARALLEL(5) NT_DEFINE_PARALLEL(6)
NT_DEFINE_PARALLEL(7) NT_DEFINE_PARALLEL(8) NT_DEFINE_PARALLEL(9) NT_DEFINE_PARALLEL(10)
#endif
