// nt_inst_lens.hip -- instantiates the packet route of a render through a lens (nt_lens.hpp).  The build compiles this file once
// per dimension (-DNT_INST_N=3 .. 10, in parallel with the render units).
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_lens.hpp"
#include "nt_dispatch.hpp"

template <> int nt_lens_fixed<NT_INST_N>(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtLens &ln) {
    return launch_lens_fixed<NT_INST_N>(li, sc, tg, ln);
}
