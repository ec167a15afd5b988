// nt_inst_boxhits.hip -- instantiates the BoxScene hit-buffer kernel of nt_boxhits.hpp.  The build compiles this file once per
// dimension (-DNT_INST_N=3 .. 24, in parallel with the render units).
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_boxhits.hpp"
#include "nt_dispatch.hpp"

template <> int nt_box_faces<NT_INST_N>(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg, const NtBoxFaces &bf) {
    return launch_box_faces<NT_INST_N>(li, cam, tg, bf);
}
