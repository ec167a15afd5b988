// nt_inst_cue.hip -- instantiates the depth cue kernels of nt_cue.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 10, in parallel with the render units).
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_cue.hpp"
#include "nt_dispatch.hpp"

template <> int nt_cue_packet<NT_INST_N>(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtCue &cu, bool draw) {
    return launch_cue_fixed<NT_INST_N>(li, sc, tg, cu, draw);
}
