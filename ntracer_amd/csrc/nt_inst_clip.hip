// nt_inst_clip.hip -- instantiates the clip-plane kernels of nt_clip.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 10, in parallel with the render units).
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_clip.hpp"
#include "nt_dispatch.hpp"

template <> int nt_clip_packet<NT_INST_N>(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtClip &cl, bool draw) {
    return launch_clip_fixed<NT_INST_N>(li, sc, tg, cl, draw);
}
