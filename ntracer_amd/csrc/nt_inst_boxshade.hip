// nt_inst_boxshade.hip -- instantiates the BoxScene face-shading kernels of nt_boxshade.hpp.  The build compiles this file once
// per dimension (-DNT_INST_N=3 .. 24, in parallel with the render units).
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_boxshade.hpp"
#include "nt_dispatch.hpp"

template <> int nt_box_shade<NT_INST_N>(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg, const NtBoxShade &bs) {
    return launch_box_shade<NT_INST_N>(li, cam, tg, bs);
}
