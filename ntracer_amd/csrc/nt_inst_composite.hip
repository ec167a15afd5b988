// nt_inst_composite.hip -- instantiates the CompositeScene kernels of nt_composite.hpp.  The build compiles this file
// once per dimension (-DNT_INST_N=3 .. 10, in parallel).
// The lean packet kernel up to four dimensions: seven waves a SIMD instead of six.  It has registers to spare (40 VGPRs) and
// waits on scalar loads 38 % of the time, but its 106 SGPRs admit only six 256-thread blocks a CU (MI355X_MICROARCH.md,
// "Residency"): a budget of 96 admits seven -- 120-cell 1.11 -> 1.04 ms a 1080p frame, 600-cell 0.355 -> 0.339 (eight waves
// with 80 SGPRs: 1.09 / 0.36, the spills to VGPR lanes eat the gain).  The attribute is per translation unit because it takes
// no template arguments; the build compiles one unit per dimension.
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#if NT_INST_N <= 4 && !defined(NT_PACKET_WAVES4)
#define NT_PACKET_WAVES4 7
#define NT_PACKET_ATTR __attribute__((amdgpu_num_sgpr(96)))
#endif
#include "nt_composite.hpp"
#include "nt_dispatch.hpp"

template <> int nt_composite_fixed<NT_INST_N>(const NtLaunchInfo &li, const NtCamera &cam, const NtCompositeDev &sc, const NtTarget &tg) {
    return launch_composite_fixed<NT_INST_N>(li, cam, sc, tg);
}
