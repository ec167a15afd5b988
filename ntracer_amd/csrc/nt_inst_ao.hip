// nt_inst_ao.hip -- instantiates the ambient occlusion kernel of nt_ao.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 10, in parallel with the render units).
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_ao.hpp"
#include "nt_dispatch.hpp"

template <> int nt_ao_fixed<NT_INST_N>(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtAo &ao) {
    return launch_ao_fixed<NT_INST_N>(li, sc, tg, ao);
}
