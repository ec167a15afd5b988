// nt_inst_layers.hip -- instantiates the hit-layer kernels of nt_layers.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 10, in parallel with the render units).
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_layers.hpp"
#include "nt_dispatch.hpp"

template <> int nt_layers_packet<NT_INST_N>(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtLayers &ly) {
    return launch_layers_fixed<NT_INST_N>(li, sc, tg, ly);
}
