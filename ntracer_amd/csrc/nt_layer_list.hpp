// nt_layer_list.hpp -- the sorted list of a lane's nearest crossings and its record stores, shared by the two hit-layer routes:
// layers_packet (nt_layers.hpp) and layers_var (nt_var.hip).  DESIGN.md 4.18; the rule in full: ntracer_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

namespace {

// A key is (bits of t, id) as one unsigned 64-bit value: t > 0, so its bits order as t does, and id = (item << 3) | (lane + 1)
// orders as the rule's (item, lane).  The all-ones key is "nothing": it sorts behind every crossing and is what a lane that did
// not accept hands to the insertion.
#define NT_LAYER_NONE 0xffffffffffffffffull
__device__ __forceinline__ unsigned long long layer_key(bool ok, float t, int item, int lane) {
    const unsigned long long k = ((unsigned long long)(unsigned int)__float_as_int(t) << 32) | (unsigned int)((item << 3) | (lane + 1));
    return ok ? k : NT_LAYER_NONE;
}

// The KCAP smallest keys of a lane, ascending.  Every index below is a constant of a fully unrolled loop, so the list is KCAP
// register pairs and never a run-time-indexed array (which would go to scratch).
template <int KCAP>
struct LayerList {
    unsigned long long k[KCAP];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < KCAP; ++j) k[j] = NT_LAYER_NONE;
    }
    // one pass of compare-and-exchange from slot 0 up, the displaced key carried along (keys are distinct: a primitive is met once)
    __device__ __forceinline__ void insert(unsigned long long c) {
#pragma unroll
        for (int j = 0; j < KCAP; ++j) {
            const unsigned long long e = k[j];
            const bool lt = c < e;
            k[j] = lt ? c : e;
            c = lt ? e : c;
        }
    }
};

// The entering distance of a Solid sphere that the Solid's own fp32 test has accepted at `t32`, evaluated again in float64 and
// rounded to fp32 once.  The sphere's quadratic b^2 - 4ac cancels nearly all of its digits when the origin is many radii away
// (fp32: up to 2.5e-5 of t at sixteen dimensions), which a nearest-hit render tolerates and an ordered list with
// distances to subtract does not; the cube's quotient (s - lo_i) / ld_i has no such cancellation and keeps its fp32 value.
// `rec` is the Solid's record [orientation n x n][inverse n x n][position n]; o(k), d(k) the ray.  Sums run in ascending k and i,
// no fma, so both routes give the same bits.  Where float64 finds no entering root (a ray within rounding of the surface) the
// fp32 distance stays.
template <typename O, typename D>
__device__ __forceinline__ float layer_sphere_t(const float *__restrict__ rec, int n, float t32, O o, D d) {
    const float *inv = rec + n * n;
    const float *pos = inv + n * n;
    double a = 0.0, b = 0.0, c = 0.0;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {         // (rolled: few lanes come here, and unrolled it took the packet walk's registers)
        double so = 0.0, sd = 0.0;
#pragma unroll 1
        for (int k = 0; k < n; ++k) {
            const double m = (double)inv[i * n + k];
            const double po = m * (double)o(k), pd = m * (double)d(k);
            so = k == 0 ? po : so + po;
            sd = k == 0 ? pd : sd + pd;
        }
        so = so - (double)pos[i];
        const double pa = sd * sd, pb = sd * so, pc = so * so;
        a = i == 0 ? pa : a + pa;
        b = i == 0 ? pb : b + pb;
        c = i == 0 ? pc : c + pc;
    }
    b = 2.0 * b;
    c = c - 1.0;
    const double disc = b * b - 4.0 * a * c;
    if (!(disc >= 0.0)) return t32;
    const double t = (-b - sqrt(disc)) / (2.0 * a);
    const float tf = (float)t;
    return tf > 0.0f && tf < FLT_MAX ? tf : t32;
}

// the `layers` records of one pixel: plane l at recs[l * px + at]; slots past the pixel's count say "none"
template <int KCAP>
__device__ __forceinline__ void layers_store(void *recs, long long at, long long px, int layers, const LayerList<KCAP> &ls, int count) {
#pragma unroll
    for (int l = 0; l < KCAP; ++l) {
        if (l >= layers) break;
        const unsigned long long e = ls.k[l];
        const unsigned int id = (unsigned int)e;
        const bool there = l < count;
        reinterpret_cast<int4 *>(recs)[(long long)l * px + at] =
            make_int4(there ? (int)(unsigned int)(e >> 32) : __float_as_int(FLT_MAX), there ? (int)(id >> 3) : -1, there ? (int)(id & 7u) - 1 : -1, count);
    }
}

}  // namespace
