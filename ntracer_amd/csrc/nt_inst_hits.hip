// nt_inst_hits.hip -- instantiates the primary-hit kernels of nt_hits.hpp.  The build compiles this file once per dimension
// (-DNT_INST_N=3 .. 10, in parallel with the render and query units); without the macro every dimension is instantiated here.
// The packet walk up to four dimensions gets what nt_inst_composite.hip gives the render's: seven waves a SIMD and the scalar
// register budget that admits them (the reasons and the figures are there).
#if defined(NT_INST_N) && NT_INST_N <= 4 && !defined(NT_PACKET_WAVES4)
#define NT_PACKET_WAVES4 7
#define NT_PACKET_ATTR __attribute__((amdgpu_num_sgpr(96)))
#endif
#include "nt_hits.hpp"

#define NT_DEFINE_HITS(N)                                                                                                \
    int nt_hits_fixed_##N(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtHits &h) {      \
        return launch_hits_fixed<N>(li, sc, tg, h);                                                                      \
    }
#define NT_DEFINE_HITS_(N) NT_DEFINE_HITS(N)

#ifdef NT_INST_N
NT_DEFINE_HITS_(NT_INST_N)
#else
NT_DEFINE_HITS(3) NT_DEFINE_HITS(4) NT_DEFINE_HITS(5) NT_DEFINE_HITS(6)
NT_DEFINE_HITS(7) NT_DEFINE_HITS(8) NT_DEFINE_HITS(9) NT_DEFINE_HITS(10)
#endif
