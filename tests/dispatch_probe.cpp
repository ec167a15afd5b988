// nt_dispatch_dim (csrc/nt_dispatch.hpp) over both ranges the launchers use, for every n from -5 to 70: one line
// "HI n in_range r calls calls_of_n" each, for tests/test_dispatch.py.  The callee of N counts its calls and returns 1000 + N.
#include <cstdio>

#include "nt_device.hpp"
#include "nt_dispatch.hpp"

static int calls[128];

template <int N>
static int callee() {
    ++calls[N];
    return 1000 + N;
}

template <int LO, int HI>
static void sweep() {
    for (int n = -5; n <= 70; ++n) {
        for (int &c : calls) c = 0;
        int r = -77;
        const bool in = nt_dispatch_dim<LO, HI>(n, r, [](auto N) { return callee<decltype(N)::value>(); });
        int total = 0;
        for (int c : calls) total += c;
        std::printf("%d %d %d %d %d %d\n", HI, n, in ? 1 : 0, r, total, n >= 0 && n < 128 ? calls[n] : 0);
    }
}

int main() {
    sweep<3, NT_DEV_MAX_FIXED>();
    sweep<3, NT_DEV_MAX_FIXED_BOX>();
    return 0;
}
