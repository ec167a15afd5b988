// nt_inst_hits.hip -- instantiates the primary-hit kernels of nt_hits.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 10, in parallel with the render and query units).
// The packet walk up to four dimensions gets what nt_inst_composite.hip gives the render's: seven waves a SIMD and the scalar
// register budget that admits them (the reasons and the figures are there).
#ifndef NT_INST_N
#error "one dimension a translation unit: compile with -DNT_INST_N=<N> (build.py)"
#endif
#if NT_INST_N <= 4 && !defined(NT_PACKET_WAVES4)
#define NT_PACKET_WAVES4 7
#define NT_PACKET_ATTR __attribute__((amdgpu_num_sgpr(96)))
#endif
#include "nt_hits.hpp"
#include "nt_dispatch.hpp"

template <> int nt_hits_fixed<NT_INST_N>(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtHits &h) {
    return launch_hits_fixed<NT_INST_N>(li, sc, tg, h);
}
