// nt_inst_query.hip -- instantiates the ray-query kernels of nt_query.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 10, in parallel with the render units); without the macro every dimension is instantiated here.
#include "nt_query.hpp"

#define NT_DEFINE_QUERY(N)                                                                          \
    int nt_query_fixed_##N(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtQuery &q) {   \
        return launch_query_fixed<N>(li, sc, q);                                                    \
    }
#define NT_DEFINE_QUERY_(N) NT_DEFINE_QUERY(N)

#ifdef NT_INST_N
NT_DEFINE_QUERY_(NT_INST_N)
#else
NT_DEFINE_QUERY(3) NT_DEFINE_QUERY(4) NT_DEFINE_QUERY(5) NT_DEFINE_QUERY(6)
NT_DEFINE_QUERY(7) NT_DEFINE_QUERY(8) NT_DEFINE_QUERY(9) NT_DEFINE_QUERY(10)
#endif
