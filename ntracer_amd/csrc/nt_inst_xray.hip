// nt_inst_xray.hip -- instantiates the X-ray kernels of nt_xray.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 10, in parallel with the render units).
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#include "nt_xray.hpp"
#include "nt_dispatch.hpp"

template <> int nt_xray_packet<NT_INST_N>(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtXray &xr) {
    return launch_xray_fixed<NT_INST_N>(li, sc, tg, xr);
}
