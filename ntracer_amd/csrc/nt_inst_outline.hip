// nt_inst_outline.hip -- instantiates the outline kernels of nt_outline.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 10, in parallel with the render units).
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_outline.hpp"
#include "nt_dispatch.hpp"

template <> int nt_outline_fixed<NT_INST_N>(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtOutline &ol, bool draw) {
    return launch_outline_fixed<NT_INST_N>(li, sc, tg, ol, draw);
}
