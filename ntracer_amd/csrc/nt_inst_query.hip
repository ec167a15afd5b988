// nt_inst_query.hip -- instantiates the ray-query kernels of nt_query.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 10, in parallel with the render units).
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_query.hpp"
#include "nt_dispatch.hpp"

template <> int nt_query_fixed<NT_INST_N>(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtQuery &q) {
    return launch_query_fixed<NT_INST_N>(li, sc, q);
}
