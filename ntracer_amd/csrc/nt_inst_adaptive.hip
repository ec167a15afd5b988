// nt_inst_adaptive.hip -- instantiates the refine kernels of nt_adaptive.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 24, in parallel with the render units): BoxScene's kernel at every one of them, CompositeScene's up to 10.
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_adaptive.hpp"
#include "nt_dispatch.hpp"

#if NT_INST_N <= NT_DEV_MAX_FIXED
template <> int nt_refine_fixed<NT_INST_N>(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtRefine &rf, const NtTarget &tg) {
    return launch_refine_fixed<NT_INST_N>(li, sc, rf, tg);
}
#endif
template <> int nt_refine_box_fixed<NT_INST_N>(const NtLaunchInfo &li, const NtRefine &rf, const NtTarget &tg) {
    return launch_refine_box_fixed<NT_INST_N>(li, rf, tg);
}
