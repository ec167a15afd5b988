// nt_box.hpp -- BoxScene kernels for compile-time N (fixed_geometry.hpp -> registers), box_scene::calculate_color
// (src/tracer.hpp:101-152) fused with process_pixel's conversion and packing (nt_pixel.hpp), so the only HBM traffic of a
// frame is the packed framebuffer.  Two routes (launch_box_fixed):
//   packed RGB of <= 10 bits a channel, three fp32 channels:  box_tile_kernel (-> box_redo_kernel for packed RGB, N > 8)
//   every other format, probe mode:                           box_cull_kernel -> box_kernel
// Instantiated per N by nt_inst_box.hip.
#pragma once
#include <type_traits>
#include "nt_pixel.hpp"
#include "nt_box_span.hpp"

namespace {

// box_scene::calculate_color + hypercube_intersects (tracer.hpp:101-152).
//
// The reference tries the entry face of every axis i in ascending order; face i is the hit when
// dist_i = (s_i - o_i)/d_i > 0 and |o_j + d_j*dist_i| <= 1+FUZZ for all j != i.  That predicate is evaluated
// here bit for bit, but only for the faces that can satisfy it:
//   1. a ray whose distance from the centre exceeds the cube's circumradius (0.1 % margin) satisfies it for
//      no face: such waves skip everything;
//   2. let K be the candidate face reached LAST (largest dist; found by cross-multiplication, no division).
//      A candidate i reached earlier than K by more than a sliver is still outside slab K at t = dist_i:
//      |o_K + d_K*dist_i| = 1 + |d_K|*(dist_K - dist_i) > 1 + FUZZ, so it fails the reference's own j = K check.
//      With a = |s - o|, b = |d| (dist = a/b), "more than a sliver" is  a_i*b_K < b_i*(a_K - mu),
//      mu = 1e-4*(1+|o_K|) -- ~100x the rounding error of the quantities compared and of the reference's
//      check.  Only the remaining near-ties (normally just K) get the division and the N-1 checks, in
//      ascending order, exactly as the reference computes them.
// Step 1 of the pruning above, on the UNNORMALISED direction v (|v|^2 = sq): the ray passes within the
// circumradius unless |o|^2 - (o.v)^2/|v|^2 > rad2.  Conservative (0.1 % on the radius, 1e-4 on the product),
// not bit-exact -- it only decides whether the exact predicate is evaluated at all.  Waves in which no lane
// may hit never normalise more than dir[0], the one component the background colour needs: that saves N-1 of
// the N IEEE divisions for ~85 % of the rays of the 6-D benchmark frames.
// dots: |o|^2, o.right, o.up, o.forward (host); v = forward + right*sx - up*sy, so o.v follows from three of them
__device__ __forceinline__ bool box_may_hit(int n, const float *dots, float sx, float sy, float sq) {
    const float osq = dots[0];
    const float ov = fmaf(-dots[2], sy, fmaf(dots[1], sx, dots[3]));
    const float rad2 = (float)n * (1.0f + NT_FUZZ) * (1.0f + NT_FUZZ) * 1.001f;
#ifdef NT_EXP_SKIP_SLABS
    return false;
#else
    return !((osq - rad2) * sq > ov * ov * 1.0001f);         // NaN -> maybe
#endif
}

__device__ __forceinline__ void box_background(float in, float &r, float &g, float &b) {
    // miss: i = dir[0]; i > 0 ? (i,i,i) : (0,-i,-i)   (tracer.hpp:109-113)
    if (in > 0.0f) { r = in; g = in; b = in; }
    else { r = 0.0f; g = -in; b = -in; }
}

template <int N>
__device__ __forceinline__ void box_color(const float (&o)[N], const float (&dir)[N], bool maybe, float &r, float &g, float &b) {
    bool done = false;     // a face passed the slab test (hit, or dist >= cutoff)
    float shade = 0.0f;

    {
        float num[N];
        bool pre[N];
        // candidates: dist > 0 needs a non-zero numerator with the sign of d_i; track the last-reached one
        float aK = 0.0f, bK = 1.0f, oK = 0.0f;
        bool any = false;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float di = dir[i];
            const float s = di < 0.0f ? 1.0f : -1.0f;
            num[i] = s - o[i];
            pre[i] = maybe && ((num[i] > 0.0f && di > 0.0f) || (num[i] < 0.0f && di < 0.0f));
            const float a = fabsf(num[i]), bb = fabsf(di);
            // a/bb > aK/bK  <=>  a*bK > aK*bb   (all positive)
            if (pre[i] && (!any || a * bK > aK * bb)) { aK = a; bK = bb; oK = o[i]; any = true; }
        }
        const float mu = 1e-4f * (1.0f + fabsf(oK));
        const float aKm = (aK - mu) * (1.0f - 1e-6f);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            // near-tie with the last-reached face (always true for that face itself); NaN-safe: !(x < y)
            const bool tie = pre[i] && !done && !(fabsf(num[i]) * bK < fabsf(dir[i]) * aKm);
            if (__builtin_amdgcn_ballot_w64(tie) != 0ull) {
                const float di = dir[i];
                const float dist = num[i] / di;
                bool ok = tie && dist > 0.0f;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    if (j != i) {
                        const float p = dir[j] * dist + o[j];
                        ok = ok && !(fabsf(p) > (1.0f + NT_FUZZ));
                    }
                }
                if (ok) {
                    done = true;
                    // `if(dist >= cutoff) return 0` with cutoff = FLT_MAX (tracer.hpp:142): a miss
                    if (dist >= FLT_MAX) shade = -1.0f;
                    else {
                        const float sine = di * (di < 0.0f ? 1.0f : -1.0f);   // dot(dir, s*e_i)
                        shade = sine <= 0.0f ? -sine : 0.0f;
                    }
                }
            }
        }
    }
    if (done && shade >= 0.0f) {
        r = shade * 1.0f;
        g = shade * 0.5f;
        b = shade * 0.5f;
    } else {
        box_background(dir[0], r, g, b);
    }
}

// m of box_classify / box_resolve / box_cull_kernel, per unit of 1 + max|o_j|.  What it has to dominate:
// ROUNDING_FUZZ (1.2e-6), the reference's own rounding in p_j (<= (5|o_j| + 6)*2^-24) and the v_rcp_f32 arithmetic
// here (~2^-22*(1 + |o_j|)): under 2e-6*(1 + max|o_j|) together, 5x below this.  (Rounds 1 and most of 2 ran with 3e-5; the
// narrower band sends a third fewer stretches to box_redo_kernel.  Builds with -DNT_BOX_MARGIN=2e-6f, the bound itself, and
// 5e-6f render the 440 full frames of tools/box_soak.py byte for byte like the oracle; at 5e-7f frames start to differ.)
// box_tile_kernel renders everything itself -- no box_redo_kernel after it -- up to this dimension (packed RGB; fp32x3: always)
#ifndef NT_BOX_INLINE_MAX_N
#define NT_BOX_INLINE_MAX_N 8
#endif
// ... which is as far as the codes wave works out tie sets (bits 0..9 and 10..19 of a dword: at most 10)
#ifndef NT_BOX_SETS_MAX_N
#define NT_BOX_SETS_MAX_N NT_BOX_INLINE_MAX_N
#endif
// (NT_BOX_MARGIN itself: nt_box_span.hpp, which the host's span of a camera shares it with; -DNT_BOX_MARGIN=... reaches both)
// Which rays need the exact evaluation at all?  Everything below works on the UNNORMALISED direction v
// (p_j(tau) = o_j + v_j*tau; the reference's dist is tau*|v|), with reciprocals from v_rcp_f32, and sorts a lane
// that may hit into one of three classes.  m = NT_BOX_MARGIN*(1 + max|o_j|) dominates the sum of ROUNDING_FUZZ and
// every rounding error involved (see NT_BOX_MARGIN).
//   miss      the ray (tau > 0) stays outside the cube grown to 1+m.  Every point the reference accepts has
//             |p_i| = 1, |p_j| <= 1+FUZZ at a dist > 0, so the reference finds no face either.
//   hit at K  K = the entry face reached last, at tau_K; tau_K is clearly positive; at tau_K every other
//             coordinate is inside 1-m/2 (the reference's test for K passes); and every other entry plane is
//             crossed while p_K is still outside 1+m ((tau_K - tau_i)*|v_K| > m), so no face before K in the
//             reference's ascending order can pass its j = K check.  The reference returns face K: shade |d_K|.
//   unclear   anything else (edges, grazing rays, origins on or inside the cube, NaN): the wave takes the exact,
//             reference-ordered evaluation in box_color.
// x = the component the colour is made of: v_K for a hit, v_0 for the background.
template <int N>
__device__ __forceinline__ void box_classify(const float (&o)[N], const float (&v)[N], float m, bool maybe, bool &hit, bool &unclear,
                                             float &x, float (&near)[N], float &tn, float &vK) {
    float tn2 = -INFINITY;                                 // tn, tn2: last and second-to-last entry, unit cube
    tn = -INFINITY;
    vK = 0.0f;
    float tnp = -INFINITY, tfp = INFINITY;                 // last entry / first exit, cube grown by m
    const float m1p = 1.0f + m;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        // slab j: (+-1 - o_j)/v_j = c -+ |1/v_j| with c = -o_j/v_j; grown by m: c -+ (1 + m)|1/v_j|.  (v_j = 0: inf - inf
        // is a NaN, which drops out of fmaxf / fminf -- right for an origin inside the slab; one outside it goes
        // undetected here and ends up unclear, but box_stretch_code culls such stretches before anyone looks at a ray)
        const float inv = __builtin_amdgcn_rcpf(v[j]);
        const float c0 = -o[j] * inv;
        const float nr = c0 - fabsf(inv);
        near[j] = nr;
        tnp = fmaxf(tnp, fmaf(-fabsf(inv), m1p, c0));
        tfp = fminf(tfp, fmaf(fabsf(inv), m1p, c0));
        const bool later = nr > tn;
        tn2 = __builtin_amdgcn_fmed3f(tn, tn2, nr);
        vK = later ? v[j] : vK;
        tn = fmaxf(tn, nr);
    }
    const bool miss = tnp > tfp || tfp < 0.0f;
    const float c = 1.0f - m;
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < N; ++j) sum = sum + fmaxf(fabsf(fmaf(v[j], tn, o[j])), c);
    // face K itself contributes 1 - c = m; the others nothing unless they are within m of their planes
    const bool inside = sum - (float)N * c <= 1.5f * m;
    const bool sole = (tn - tn2) * fabsf(vK) > m;
    const bool front = tn > 1e-3f && tn < 1e30f;
    hit = maybe && !miss && inside && sole && front;
    unclear = maybe && !miss && !hit;
#ifdef NT_EXP_NOUNCLEAR
    unclear = false;
#endif
    x = hit ? vK : v[0];
}

// v_max_f32 / v_min_f32 as they are (box_stretch_code2, box_classify_sets): fmaxf / fminf on a value that reaches them from another basic block come with a
// canonicalising `v_max_f32 x, x, x` per operand (the compiler cannot see that the value is the result of arithmetic), and
// these instructions run at half the rate of a multiply: an eighth of box_stretch_code2's instructions were such no-ops.
// Quiet NaNs drop out of the hardware's max / min as they do out of fmaxf / fminf; every operand here is the result of
// arithmetic or an infinity.
__device__ __forceinline__ float nt_vmax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float nt_vmin(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float nt_vmax3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float nt_vmin3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float nt_vmed3(float a, float b, float c) { float r; asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float nt_vmax_abs(float a, float b) { float r; asm("v_max_f32 %0, |%1|, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }   // max(|a|, b)
__device__ __forceinline__ float nt_vmax3_abs(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }   // max(a, |b|, |c|)
__device__ __forceinline__ float nt_vmin_abs(float a, float b) { float r; asm("v_min_f32 %0, |%1|, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }   // min(|a|, b)

// The "sure hit" bit of a stretch's sets word (box_stretch_code2; bit 24: bits 20..23 hold the code where code and sets share a
// register): every ray of the stretch is a hit for the reference, at a face of T -- which one is the business of its rounding,
// but the packed pixel rarely depends on it (box_pixel's sure_hit_row).  Packed RGB, N = NT_BOX_TIE_SHORTCUT_MIN_N.._MAX_N, the 64 x 1
// shape in launches of NT_BOX_TIE_SHORTCUT_MIN_WAVES waves or more;
// -DNT_BOX_TIE_SHORTCUT=0: neither the bit nor the branch, the build to measure and to test against (and N = 7's, nt_inst_box.hip).
//
// The reference's ray is (o, d) with the float d = v/|v|, u = 2^-24.  Face i (entry plane s_i = -+1) has
// dist_i = fl(fl(s_i - o_i)/d_i) = tau_i (1 + e1)(1 + e2), |e| <= u, tau_i = (s_i - o_i)/d_i exactly; it passes iff dist_i > 0
// and |p_j| <= 1 + FUZZ = 1 + 20u for every j != i, p_j = fl(fl(d_j dist_i) + o_j).  A stretch with valid sets (T, C) has
// (1) no face outside T passing and (2) no coordinate outside C failing for a face of T, at any tau of [t_lo, t_hi], which
// holds every such test (box_stretch_code2).  The bit is set when, besides,
//   * C == T;
//   * no slab is left inside the window: (t_hi - t_lo) * max_j (|vc_j| + g_j) <= 1 (T's axes are what the argument needs);
//   * |o_j| <= NT_BOX_TIE_SURE_MAX_ORIGIN on every axis j of T.
// Then the face K* of T with the largest float dist passes.  A coordinate outside T = C passes by (2).  For j in T, j != K*:
// dist_K* >= dist_j, so the exact P_j = o_j + d_j dist_K* lies on the inner side of
//   o_j + d_j dist_j = s_j + (s_j - o_j)(e1 + e2 + e1 e2),   at most (1 + |o_j|) 2u (and u^2 of that) outside the slab:
// it has entered, or is that far short of entering; and it has not left: both entries lie in the window, across which no
// coordinate of T moves by more than 1 of the slab's width of 2.  So |P_j| <= 1 + (1 + |o_j|) 2u.  The product's rounding adds
// at most |d_j dist_K*| u <= (1 + |o_j|) u (P_j is between o_j and the far plane), the sum's -- a result next to 1 -- at most u:
//   |p_j| <= 1 + (4 + 3|o_j|) u  <=  1 + 17.5 u  <  1 + 20u     at |o_j| = 4.5    (16.5 u at the bench's 4.17; 5.33 is the break-even).
// K* passes, faces outside T do not (1), every face of T has dist > 0 (t_lo > 1e-3) and below FLT_MAX (t_hi < 1e30): the
// reference returns a hit at the first passing face of T.
#ifndef NT_BOX_TIE_SHORTCUT
#define NT_BOX_TIE_SHORTCUT 1
#endif
#ifndef NT_BOX_TIE_SHORTCUT_MIN_N
#define NT_BOX_TIE_SHORTCUT_MIN_N 6
#endif
#ifndef NT_BOX_TIE_SHORTCUT_MAX_N
#define NT_BOX_TIE_SHORTCUT_MAX_N 8
#endif
#ifndef NT_BOX_TIE_SURE_MAX_ORIGIN
#define NT_BOX_TIE_SURE_MAX_ORIGIN 4.5f
#endif
// The kernel with the bit and the branch in it (box_tile_kernel<N, false, 64, 1, true>) is a launch's kernel only from this many
// 64-row waves on: having them costs a launch a nearly fixed time whether any row takes the branch -- with a bit that is never set
// the headline call (81 600 waves) measured 308.2 -> 312.4 us and a rank's eighth of it in the same shape (14 400 waves) 75.0 ->
// 77.3 us -- and what the stored rows save grows with the rows: 9.2 us of the headline call, 1.0 us of the eighth.  Those figures
// meet at about 24 000 waves.  Smaller launches, and the 16- and 8-row shapes, which are small launches by
// construction, run the kernel without.
#ifndef NT_BOX_TIE_SHORTCUT_MIN_WAVES
#define NT_BOX_TIE_SHORTCUT_MIN_WAVES 32768
#endif
#define NT_BOX_SETS_SURE 0x01000000u
// The span of a frame (NtCamera::span, nt_box_span.hpp: a camera table's frames have one): no ray with sx outside [lo, hi] can
// come within h of the cube at a tau > 0, whatever its row.  A wave whose column strip lies outside it -- the strip's sx runs
// from its first pixel's to its last one's, the row phase's own fp32 expressions, which are monotonic in x -- goes around
// box_stretch_code2 with code 0 and no sets for every lane: about 155 vector instructions, two v_rcp_f32 an axis among them,
// that more than half of the headline call's waves spent on finding out what the camera alone decides.
// The bytes cannot change.  A skipped strip's rows are culled rows: culled_row / put_quick behind their guard, with the
// reference's arithmetic (box_pixel) where the guard fails -- the path of every code-0 row.  Code 0 itself only ever meant "no
// ray of the stretch can be a hit for the reference", and that is what the span states of the whole strip, from the premise
// box_stretch_code2 works from (with the same m and h), in double and with a slack of a sixth of a pixel.  A stretch that the
// looser per-stretch cull used to keep and the span clears was classified ray by ray or went through box_pixel, and every ray
// came out a miss: background, the same bytes as the culled path's (which is what the guard is for).
// -DNT_BOX_STRIP_SPAN=0: without the test, the device code as it was: the build to measure and to test against.
#ifndef NT_BOX_STRIP_SPAN
#define NT_BOX_STRIP_SPAN 1
#endif
// (Measured with it and not taken: a counted loop of sixteen groups of four, the next group's table entries loaded ahead, for
// waves all of whose 64 slots are culled rows.  Rotating the sixteen scalar registers of the entries costs nine s_mov_b64 a
// group -- two sets that swap roles do not fit the scalar registers -- and the kernel ran 4 % MORE scalar instructions, at the
// same time or 0.2 % slower: DESIGN.md 4.1.)
template <int N>
constexpr bool nt_box_tie_shortcut() { return NT_BOX_TIE_SHORTCUT != 0 && N >= NT_BOX_TIE_SHORTCUT_MIN_N && N <= NT_BOX_TIE_SHORTCUT_MAX_N && N <= NT_BOX_SETS_MAX_N; }

// box_classify for a row sorted ray by ray (code 15) whose stretch has valid sets (box_stretch_code2: T in bits 0..9, C in bits
// 10..19, wave-uniform): the same three verdicts from T's entry planes and C's coordinates alone -- |C| reciprocals, slab updates
// and inside terms instead of N (BoxScene(6)'s bench cameras: |T| = 1.6, |C| = 2.8 on average; in 60 % of these rows T is one
// face).  Axes are picked by scalar tests on `sets`; there is nothing per lane.  Why nothing is lost, with A_j <= near_j <= B_j
// the range of slab j's entry over the stretch, TN = max A_j, M >= m/|v_K| (see box_stretch_code2) and tn, tn2, vK, tnp, tfp
// as in box_classify:
//   last axis     a ray's last entry axis K has B_K >= near_K = tn >= TN, so K is in T: tn and vK over T are tn and vK over
//                 all axes.
//   second entry  an axis outside T has near_j <= B_j < TN - M <= tn - m/|v_K| (M carries 1 + 1e-5 for the arithmetic): it is
//                 neither within the `sole` margin of tn nor -- its grown entry lies before the unit one -- the grown cube's
//                 last entry.  `sole` and tnp over T are the full ones (tn2 = -inf for a single face: sole).
//   inside sum    a coordinate outside C stays inside 1 - m - 1e-4 < c over [t_lo, t_hi], which holds every ray's tn: its term
//                 of box_classify's sum is exactly c, and the sum over C against |C|*c is the full sum against N*c.
//   miss          tfp over C is at least the full tfp and tnp over T at most the full tnp: a miss here is a miss there, never
//                 the other way round.  (A ray that does miss leaves through a slab whose coordinate is outside 1 at tn: one of C.)
// So "hit at K" and "miss" are verdicts box_classify gives too, and everything else is unclear.  There are no entry times of
// all N axes for box_resolve afterwards: a wave with an unclear lane takes the reference's arithmetic on the stretch's T and C
// (box_pixel's sets branch), which is right for every ray of the stretch, and keeps its answer for every lane.
// For N = 6 and 7 (-DNT_BOX_CLASSIFY_SETS_MAX_N=0: nowhere, the build to measure against).  Measured against the build without it,
// alternately on one box, 160 frames of 1080p a call: BoxScene(6), the bench's cameras, 338.5 -> 331.3 us a call;
// BoxScene(7), random cameras, +0.8 % rays a second; BoxScene(5) even; BoxScene(3) and (4) 4-5 % SLOWER -- with three or four
// slabs there is little to restrict, and the unclear lanes' route through the stretch's sets costs more than box_resolve's
// per-lane ones.  Every tile kernel it is in needs one to four more VGPRs, which at N = 6 and 7 stays on the occupancy step the
// kernel is on (n = 6, 64 x 1: 71 -> 72, seven waves).  At N = 8 it does not: 79 -> 83 (16-row shapes) and 80 -> 82 (fp32,
// 64 x 1) cross 80, six waves a SIMD to five.
#ifndef NT_BOX_CLASSIFY_SETS_MIN_N
#define NT_BOX_CLASSIFY_SETS_MIN_N 6
#endif
#ifndef NT_BOX_CLASSIFY_SETS_MAX_N
#define NT_BOX_CLASSIFY_SETS_MAX_N 7
#endif
// FIXED != 0 (box_tile_kernel's edge rows, NT_BOX_EDGE_ROWS): the sets word is that compile-time constant, whatever `sets` says, and
// the per-axis tests fold away.
template <int N, uint32_t FIXED = 0u>
__device__ __forceinline__ void box_classify_sets(const float (&o)[N], const float (&v)[N], float m, uint32_t sets, bool &hit, bool &unclear,
                                                  float &x) {
    if constexpr (FIXED != 0u) sets = FIXED;
    // (nt_vmax & co.: these values cross basic blocks -- see there; the empty asm keeps the compiler from turning a skipped axis
    // into computed-and-discarded)
    float tn = -INFINITY, tn2 = -INFINITY, vK = 0.0f;
    float tnp = -INFINITY, tfp = INFINITY;
    const float m1p = 1.0f + m;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (((sets >> (10 + j)) & 1u) != 0u) {
            const float inv = __builtin_amdgcn_rcpf(v[j]);
            const float c0 = -o[j] * inv;
            tfp = nt_vmin(tfp, fmaf(fabsf(inv), m1p, c0));
            if (((sets >> j) & 1u) != 0u) {
                const float nr = c0 - fabsf(inv);
                tnp = nt_vmax(tnp, fmaf(-fabsf(inv), m1p, c0));
                const bool later = nr > tn;
                tn2 = nt_vmed3(tn, tn2, nr);
                vK = later ? v[j] : vK;
                tn = nt_vmax(tn, nr);
            }
        }
    }
    const bool miss = tnp > tfp || tfp < 0.0f;
    const float c = 1.0f - m;
    float sum = 0.0f;
    // (the second loop tests the bits of `sets` again: left to itself the compiler keeps the first loop's six outcomes as lane
    // masks -- five scalar instructions a test instead of a bit test and a branch, and six register pairs held across the loops
    // of a kernel that already parks scalar registers in a vector one; -DNT_EXP_SETS_MASKS: without, the build to measure against)
#ifndef NT_EXP_SETS_MASKS
    if constexpr (FIXED == 0u) asm volatile("" : "+s"(sets));
#endif
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (((sets >> (10 + j)) & 1u) != 0u) {
            asm volatile("" : "+v"(sum));
            sum = sum + nt_vmax_abs(fmaf(v[j], tn, o[j]), c);
        }
    }
    const bool inside = sum - (float)__builtin_popcount((sets >> 10) & 0x3ffu) * c <= 1.5f * m;
    const bool sole = (tn - tn2) * fabsf(vK) > m;
    const bool front = tn > 1e-3f && tn < 1e30f;
    hit = !miss && inside && sole && front;
    unclear = !miss && !hit;
    x = hit ? vK : v[0];
}

// The part of box_classify that box_resolve needs: entry times into the unit cube, the last of them, its axis.
template <int N>
__device__ __forceinline__ void box_entries(const float (&o)[N], const float (&v)[N], float (&near)[N], float &tn, float &vK) {
    tn = -INFINITY;
    vK = 0.0f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float inv = __builtin_amdgcn_rcpf(v[j]);
        const float nr = fmaf(-o[j], inv, -fabsf(inv));          // (+-1 - o_j)/v_j, the earlier of the two
        near[j] = nr;
        vK = nr > tn ? v[j] : vK;
        tn = fmaxf(tn, nr);
    }
}

// The unclear lanes of a wave, resolved with the reference's own arithmetic -- but only the part of it that can
// matter.  With near[], tn, vK from box_classify (approximate; the margins absorb that):
//   T = { i : (tn - near_i)*|v_K| <= m }   the faces that can still be the reference's answer: any other face is
//       entered while p_K is outside 1+m and fails its j = K check (box_classify);
//   C = { j : |p_j(tn)| + |v_j|*m/|v_K| > 1 - m/2 }   the coordinates whose test some face of T could fail: every
//       face of T is entered within m/|v_K| of tn, so a coordinate outside C is inside 1-m/2 at all of them.
//       T is a subset of C (p_i(tn) is within |v_i|*m/|v_K| of +-1 for i in T).
// The faces of T are tried in ascending order exactly as hypercube_intersects does (tracer.hpp:126-152): dist from the
// IEEE quotient, then d_j*dist + o_j against 1+FUZZ for the j in C; d_j = v_j/len is computed for the axes of C only.
// A lane whose tn is not a usable number gets T = C = everything, i.e. the reference's full loop.
template <int N>
__device__ __forceinline__ void box_resolve(const float (&o)[N], const float (&v)[N], float len, float m, const float (&near)[N], float tn,
                                            float vK, bool unclear, bool &hit, float &x) {
    const float aK = fabsf(vK);
    const float slack = m * __builtin_amdgcn_rcpf(aK), lim = 1.0f - 0.5f * m;
    bool inT[N], inC[N];
    float d[N];
    uint32_t anyC = 0u;                       // coordinates in some lane's C (uniform): the others are not looked at below
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const bool early = (tn - near[j]) * aK > m;                                     // false for a NaN
        const bool robust = fmaf(fabsf(v[j]), slack, fabsf(fmaf(v[j], tn, o[j]))) <= lim;  // false for a NaN
        inT[j] = unclear && !early;
        inC[j] = unclear && !(robust && early);
        d[j] = 0.0f;
        if (__builtin_amdgcn_ballot_w64(inC[j]) != 0ull) {
            d[j] = v[j] / len;
            anyC |= 1u << j;
        }
    }
    bool done = false, found = false;
    float xs = v[0];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const bool cand = inT[i] && !done;
        if (__builtin_amdgcn_ballot_w64(cand) != 0ull) {
            const float di = d[i];
            const float dist = ((di < 0.0f ? 1.0f : -1.0f) - o[i]) / di;
            bool ok = cand && di != 0.0f && dist > 0.0f;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                if (j != i && ((anyC >> j) & 1u) != 0u) {
                    const float p = d[j] * dist + o[j];
                    ok = ok && !(inC[j] && fabsf(p) > (1.0f + NT_FUZZ));
                }
            }
            if (ok) {
                done = true;
                // `if(dist >= cutoff) return 0` with cutoff = FLT_MAX (tracer.hpp:142): a miss
                if (!(dist >= FLT_MAX)) { found = true; xs = v[i]; }
            }
        }
    }
    if (unclear) {
        hit = found;
        x = xs;
    }
}

// a pointer into global memory every lane agrees on, pinned to scalar registers (and so kept apart from the per-lane
// offset added to it): base of a global_store with an SGPR address
typedef __attribute__((address_space(1))) uint8_t *nt_gptr;
__device__ __forceinline__ nt_gptr uniform_ptr(uint8_t *p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (nt_gptr)(((unsigned long long)hi << 32) | lo);
}
#define NT_G32(p) (*(__attribute__((address_space(1))) uint32_t *)(p))

// Three fp32 channels that are plain components (tg.plain_f32, 12-byte pixels on 4-byte-aligned rows), BoxScene colours
// (g == b): the bytes emit_pixel writes for this layout -- clamp, big-endian floats or the reversed pixel -- as one
// 12-byte store.
template <typename P>
__device__ __forceinline__ void emit_f32x3_at(const NtTarget &tg, P p, float r, float gb) {
    r = r > 0.0f ? r : 0.0f;          // simd::clamp, as in channel_value
    r = r < 1.0f ? r : 1.0f;
    gb = gb > 0.0f ? gb : 0.0f;
    gb = gb < 1.0f ? gb : 1.0f;
    uint32_t vr = __float_as_uint(r), vgb = __float_as_uint(gb);
    uint3 w;
    if (tg.plain_f32[0] == 0 && tg.plain_f32[1] == 1 && tg.plain_f32[2] == 2 && !tg.reversed) {       // (uniform) R, G, B in order
        w.x = bswap32(vr);
        w.y = bswap32(vgb);
        w.z = w.y;
    } else {
        if (!tg.reversed) { vr = bswap32(vr); vgb = bswap32(vgb); }
        w.x = tg.plain_f32[tg.reversed ? 2 : 0] == 0 ? vr : vgb;
        w.y = tg.plain_f32[1] == 0 ? vr : vgb;
        w.z = tg.plain_f32[tg.reversed ? 0 : 2] == 0 ? vr : vgb;
    }
    if constexpr (std::is_same<P, nt_gptr>::value) {
        typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
        u32x3 v;
        v.x = w.x; v.y = w.y; v.z = w.z;
        *(__attribute__((address_space(1))) u32x3 *)(p) = v;
    } else {
        *reinterpret_cast<uint3 *>(p) = w;
    }
}
__device__ __forceinline__ void emit_f32x3(const NtTarget &tg, long long offset, float r, float gb) { emit_f32x3_at(tg, tg.dest + offset, r, gb); }

// sqrtf(x) for x in [2^-96, 2^96): hipcc's correctly rounded square root is v_sqrt_f32 followed by a choice among the
// result and its two neighbours (two fma residuals), wrapped in a rescaling for x < 2^-96 and a pass-through for 0 and
// infinity; inside that range the wrapping does nothing, and this is the rest -- the same operations, hence the same float.
__device__ __forceinline__ float sqrt_in_range(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float s_dn = __uint_as_float(__float_as_uint(s) - 1u), s_up = __uint_as_float(__float_as_uint(s) + 1u);
    const float vp = fmaf(-s_dn, s, x), vs = fmaf(-s_up, s, x);
    float r = vp <= 0.0f ? s_dn : s;
    r = vs > 0.0f ? s_up : r;
    return r;
}
// ... for a whole wave: the plain sqrtf unless every lane is inside the range (NaN included in "outside")
__device__ __forceinline__ float sqrt_wave(float x) {
    if (__builtin_amdgcn_ballot_w64(!(x >= 0x1p-96f && x < 0x1p96f)) == 0ull) return sqrt_in_range(x);
    return sqrtf(x);
}

// One pixel of BoxScene from the unnormalised direction `dir` (|dir|^2 = sq), sx / sy as in the ray source.
// PLAIN: the format is known to be plain_rgb with at most 10 bits per channel (the launcher checks).
// DEFER: a wave with an unclear lane writes nothing and returns false (the caller hands the stretch to box_redo_kernel),
// which keeps the resolving code -- and its registers -- out of the kernel every other wave runs.
// REDO (box_redo_kernel): no sorting into clear and unclear -- box_resolve is complete by itself (a clear hit is T = C =
// {K}; a clear miss fails at a coordinate of C), and in a stretch that is here because of its unclear lanes the
// sorting of the others saves nothing.
template <int N, bool PLAIN, bool DEFER = false, bool REDO = false, bool F32 = false, bool TIE = false>
__device__ __forceinline__ bool box_pixel(const NtTarget &tg, const PixelRef &pr, const float (&org)[N], float (&dir)[N], float sq,
                                          const float (&dots)[4], float sx, float sy, float margin, bool rowhit = true, int face = -1,
                                          uint32_t sets = 0u, bool noclass = false) {
    // noclass (wave-uniform; box_tile_kernel where it has no second kernel: F32, or N <= 8): a near-tie stretch (code 14) --
    // as in box_redo_kernel, no sorting into clear and unclear first
    constexpr bool INL = (F32 || PLAIN) && !REDO && !DEFER;
    const bool redo = REDO || (INL && noclass);
    // rowhit (wave-uniform): the culling bit of this 64-pixel stretch of the row, see box_cull_kernel
    // face (wave-uniform) >= 0: every ray of the stretch is known to hit that face (a one-face row of box_tile_kernel whose
    // cheap quantisation came too close to a rounding boundary): nothing to sort, only the exact colour is wanted
    // (DEFER: box_tile_kernel passes the code of the stretch as rowhit -- a stretch that survived the codes wave is next to the
    // cube, where the circumsphere test rarely spares a wave the classification and costs eight instructions every time)
    const bool maybe = redo || (rowhit && (DEFER || INL || box_may_hit(N, dots, sx, sy, sq)));
    float r, g, b;
    bool hit = false, unclear = false;
    float x = dir[0];
#ifndef NT_EXP_NOCLASSIFY
    float near[N], tn = 0.0f, vK = 0.0f;
    // sets (wave-uniform, box_tile_kernel): T and C of the whole stretch from the codes wave (box_stretch_code2, through LDS).
    // A near-tie stretch goes straight to the reference's arithmetic on them; a stretch sorted ray by ray is sorted on them
    // (box_classify_sets) and goes there only with an unclear lane.
    constexpr bool CSETS = INL && N >= NT_BOX_CLASSIFY_SETS_MIN_N && N <= NT_BOX_CLASSIFY_SETS_MAX_N;
    // the reference's arithmetic on T and C, as in box_resolve, without the entry times
    auto exact_on_sets = [&]() {
        const float len = sqrt_wave(sq);
        float d[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            d[j] = 0.0f;
            if ((sets >> (10 + j)) & 1u) d[j] = dir[j] / len;
        }
        bool done = false;
        x = dir[0];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (((sets >> i) & 1u) != 0u && __builtin_amdgcn_ballot_w64(!done) != 0ull) {
                const float di = d[i];
                const float dist = ((di < 0.0f ? 1.0f : -1.0f) - org[i]) / di;
                bool ok = !done && di != 0.0f && dist > 0.0f;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    if (j != i && ((sets >> (10 + j)) & 1u) != 0u) {
                        const float p = d[j] * dist + org[j];
                        ok = ok && !(fabsf(p) > (1.0f + NT_FUZZ));
                    }
                }
                if (ok) {
                    done = true;
                    // `if(dist >= cutoff) return 0` with cutoff = FLT_MAX (tracer.hpp:142): a miss
                    if (!(dist >= FLT_MAX)) { hit = true; x = dir[i]; }
                }
            }
        }
    };
    // A stretch whose sets carry the "sure hit" bit (NT_BOX_SETS_SURE: every ray hits a face of T): the pixel without the
    // reference's arithmetic.  Its colour is |d_i| (1, 1/2, 1/2) for the face i of T the reference's rounding picks, and
    // t(x) = |x| rsq(sq) maxval -- the clear path's quotient below, with its guard of 2^-20 (1 + t) -- is monotone in |x|, as is
    // t - guard(t): when t and t/2 of the smallest and of the largest |dir_i| over T are clear of every k + 1/2 and round to the
    // same two integers, those of every face of T lie between them, are clear, and round likewise.  Those are the bytes; a wave
    // with a lane that is not so takes exact_on_sets as before.  (Axes picked by scalar tests on `sets`; wave-uniform result.)
    constexpr bool SURE = TIE && nt_box_tie_shortcut<N>() && INL && PLAIN && !F32;
    auto sure_hit_row = [&]() -> bool {
        float lo = INFINITY, hi = 0.0f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if (((sets >> j) & 1u) != 0u) {
                asm volatile("" : "+v"(lo), "+v"(hi));
                lo = nt_vmin_abs(dir[j], lo);
                hi = nt_vmax_abs(dir[j], hi);
            }
        }
        const float maxv = (float)tg.plain_maxval;
        const float rs = __builtin_amdgcn_rsqf(sq);
        const float t0 = (lo * rs) * maxv, t1 = (hi * rs) * maxv;
        const float h0 = t0 * 0.5f, h1 = t1 * 0.5f;
        auto clear = [](float t) { return fabsf(__builtin_amdgcn_fractf(t) - 0.5f) > fmaf(t, 0x1p-20f, 0x1p-20f); };
        // t + 2^23 holds round(t) in its low mantissa bits (t <= 1023.5: plain_bits <= 10)
        const uint32_t r0 = __float_as_uint(t0 + 8388608.0f), r1 = __float_as_uint(t1 + 8388608.0f);
        const uint32_t g0 = __float_as_uint(h0 + 8388608.0f), g1 = __float_as_uint(h1 + 8388608.0f);
        const bool same = clear(t0) && clear(t1) && clear(h0) && clear(h1) && r0 == r1 && g0 == g1;      // (a NaN fails)
        if (__builtin_amdgcn_ballot_w64(!same) != 0ull) return false;
        if (tg.plain_sel != 0u) {
            *reinterpret_cast<uint32_t *>(tg.dest + pr.offset) = __builtin_amdgcn_perm(r1, g1, tg.plain_sel);
            return true;
        }
        uint32_t qgb = (uint32_t)(h1 + 0.5f), qr = (uint32_t)(t1 + 0.5f);
        qgb = qgb < tg.plain_maxval ? qgb : tg.plain_maxval;
        qr = qr < tg.plain_maxval ? qr : tg.plain_maxval;
        emit_plain(tg, pr, qr, qgb);
        return true;
    };
    if constexpr (CSETS) {
        const bool have_sets = face < 0 && (sets & 0x80000000u) != 0u;
        bool on_sets = have_sets && redo;
        bool sorted = face >= 0;                   // (wave-uniform) nothing left to classify
        if (face >= 0) {
            hit = true;
#pragma unroll
            for (int j = 1; j < N; ++j) x = face == j ? dir[j] : x;
        } else if (have_sets && !redo && __builtin_amdgcn_ballot_w64(maybe) != 0ull) {
            box_classify_sets<N>(org, dir, margin, sets, hit, unclear, x);
            on_sets = __builtin_amdgcn_ballot_w64(unclear) != 0ull;
            unclear = false;
            sorted = true;
        }
        if (on_sets) {
            if constexpr (SURE) {
                if ((sets & NT_BOX_SETS_SURE) != 0u && redo && sure_hit_row()) return true;
            }
            hit = false;
            exact_on_sets();
        } else if (sorted) {
        } else if (redo) {
            box_entries<N>(org, dir, near, tn, vK);
            unclear = true;
        } else if (__builtin_amdgcn_ballot_w64(maybe) != 0ull) {
            box_classify<N>(org, dir, margin, maybe, hit, unclear, x, near, tn, vK);
        }
    } else {
        // (as it was before there was a box_classify_sets)
        if (face >= 0) {
            hit = true;
#pragma unroll
            for (int j = 1; j < N; ++j) x = face == j ? dir[j] : x;
        } else if ((REDO || INL) && redo && (sets & 0x80000000u) != 0u) {
            if constexpr (SURE) {
                if ((sets & NT_BOX_SETS_SURE) != 0u && sure_hit_row()) return true;
            }
            exact_on_sets();
        } else if (redo) {
            box_entries<N>(org, dir, near, tn, vK);
            unclear = true;
        } else if (__builtin_amdgcn_ballot_w64(maybe) != 0ull) {
            box_classify<N>(org, dir, margin, maybe, hit, unclear, x, near, tn, vK);
        }
    }
    // unclear lanes: the reference's arithmetic on the faces and coordinates still in question; a lane without a
    // usable entry time (origin on or inside the cube, NaN) keeps the whole wave on box_color's full evaluation
    if (DEFER) {
        if (__builtin_amdgcn_ballot_w64(unclear) != 0ull) return false;
    } else {
        const bool hard = unclear && !(tn > 1e-3f && tn < 1e30f);
        if (__builtin_amdgcn_ballot_w64(unclear) != 0ull && __builtin_amdgcn_ballot_w64(hard) == 0ull) {
            box_resolve<N>(org, dir, sqrt_wave(sq), margin, near, tn, vK, unclear, hit, x);
            unclear = false;
        }
    }
#else
    unclear = maybe;
#endif
    if (__builtin_amdgcn_ballot_w64(unclear) == 0ull) {
        // every lane's colour is |x|/len times (1,.5,.5) (hit) or (1,1,1) / (0,1,1) (background, by the sign of x)
        if (PLAIN || (plain_rgb(tg) && tg.plain_bits <= 10u)) {
            // Only round(value * maxval) is stored.  |x| * rsq(sq) is within 3*2^-23 of the reference's twice-rounded
            // |x/len| (v_rsq_f32: 1 ulp; two multiplications here; sqrt and division there), so whenever
            // t = that * maxval keeps 2^-20*(1+t) clear of every k + 1/2 the two round to the same integer: no
            // sqrt, no division.  (A hit also stores round(t/2).)  A wave with a lane inside a guard band (a few
            // per cent of them at 8 bits), or with a NaN / infinity, takes the exact division below.
            const float maxv = (float)tg.plain_maxval;
            const float t = (fabsf(x) * __builtin_amdgcn_rsqf(sq)) * maxv;
            const float tgb = hit ? t * 0.5f : t;
            const bool clear_gb = fabsf(__builtin_amdgcn_fractf(tgb) - 0.5f) > fmaf(tgb, 0x1p-20f, 0x1p-20f);
            const bool clear_r = fabsf(__builtin_amdgcn_fractf(t) - 0.5f) > fmaf(t, 0x1p-20f, 0x1p-20f);
            if (__builtin_amdgcn_ballot_w64(!(clear_gb && (clear_r || !hit))) == 0ull) {
                if (tg.plain_sel != 0u) {
                    // 8-bit fields: t + 2^23 holds round(t) in its low mantissa byte (see box_tile_kernel), the byte v_perm_b32 picks
                    const uint32_t q8gb = __float_as_uint(tgb + 8388608.0f), q8r = __float_as_uint(t + 8388608.0f);
                    *reinterpret_cast<uint32_t *>(tg.dest + pr.offset) = __builtin_amdgcn_perm((hit || x > 0.0f) ? q8r : 0u, q8gb, tg.plain_sel);
                    return true;
                }
                uint32_t qgb = (uint32_t)(tgb + 0.5f), qr = (uint32_t)(t + 0.5f);
                qgb = qgb < tg.plain_maxval ? qgb : tg.plain_maxval;    // the value may round to just above 1: clamped
                qr = qr < tg.plain_maxval ? qr : tg.plain_maxval;
                emit_plain(tg, pr, (hit || x > 0.0f) ? qr : 0u, qgb);
                return true;
            }
        }
        const float in = x / sqrtf(sq);
        if (hit) {
            // sine = d_K * (-sign d_K) <= 0, shade = -sine (tracer.hpp:105-107)
            const float shade = fabsf(in);
            r = shade * 1.0f;
            g = shade * 0.5f;
            b = shade * 0.5f;
        } else {
            box_background(in, r, g, b);
        }
    } else if (!DEFER) {
        const float len = sqrtf(sq);
#pragma unroll
        for (int j = 0; j < N; ++j) dir[j] = dir[j] / len;
        box_color<N>(org, dir, maybe, r, g, b);
    } else {
        return false;
    }
    if (F32) {
        emit_f32x3(tg, pr.offset, r, g);                                        // g == b
        return true;
    }
    if (PLAIN || plain_rgb(tg)) {
        emit_plain(tg, pr, plain_quantize(tg, r), plain_quantize(tg, g));       // g == b
        return true;
    }
    emit_pixel(tg, pr, r, g, b);
    return true;
}

// The general kernel: every format, and probe mode.  A lane renders R = NT_BOXROWS (8) pixels of one image column (a block:
// 64 columns x 4*R rows; a wave still writes 64 consecutive pixels of a row at a time): forward + right*sx and the wave's
// set-up are shared by all of them.  Probe mode (listed pixels) is one pixel per lane.
#ifndef NT_BOXROWS
#define NT_BOXROWS 8
#endif
template <int N>
__global__ __launch_bounds__(256) void box_kernel(NtCameraFixed cam, NtTarget tg) {
    const int tid = (int)threadIdx.x;
    float org[N], right[N], up[N], fwd[N], dir[N];
    load_camera<N>(cam, org, right, up, fwd);
    float margin = fabsf(org[0]);
#pragma unroll
    for (int j = 1; j < N; ++j) margin = fmaxf(margin, fabsf(org[j]));
    margin = NT_BOX_MARGIN * (1.0f + margin);
    float dots[4];
    if (cam.buf) {
        const float *dp = cam.dots + (size_t)blockIdx.z * 4;
        dots[0] = dp[0]; dots[1] = dp[1]; dots[2] = dp[2]; dots[3] = dp[3];
    } else {
        dots[0] = cam.odots[0]; dots[1] = cam.odots[1]; dots[2] = cam.odots[2]; dots[3] = cam.odots[3];
    }
    if (tg.colors_out) {
        // one pixel per lane: probe mode (listed pixels)
        const PixelRef pr = locate_pixel<64, 4>(tg, tid & 63, tid >> 6, tid);
        if (!pr.valid) return;
        // flat_origin_ray_source::operator() (tracer.hpp:71-75), as primary_dir, with the normalisation split off
        const float sx = tg.fovI * ((float)pr.x - tg.half_w);
        const float sy = tg.fovI * ((float)pr.y - tg.half_h);
#pragma unroll
        for (int j = 0; j < N; ++j) dir[j] = (fwd[j] + right[j] * sx) - up[j] * sy;
        float sq = dir[0] * dir[0];
#pragma unroll
        for (int j = 1; j < N; ++j) sq = sq + dir[j] * dir[j];
        box_pixel<N, false>(tg, pr, org, dir, sq, dots, sx, sy, margin);
        return;
    }
    // the wave's number as a scalar: everything that depends on the row alone stays on the scalar unit
    constexpr int R = NT_BOXROWS;
    const int row0 = ((int)blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(tid >> 6)) * R;
    const int x = (int)blockIdx.x * 64 + (tid & 63);
    if (x >= tg.width) return;
    const float sx = tg.fovI * ((float)x - tg.half_w);
    float base[N];
#pragma unroll
    for (int j = 0; j < N; ++j) base[j] = fwd[j] + right[j] * sx;
    // the stretch codes of the wave's rows, fetched together ahead of the loop (only "culled or not" is used here)
    uint32_t live = ~0u;
    if (tg.cull) {
        if (row0 >= tg.row_count) return;               // (keeps the reads inside the table's padding)
        const uint32_t *cp = tg.cull + ((size_t)blockIdx.z * tg.row_count + row0) * tg.cull_words + (blockIdx.x >> 3);
        live = 0u;
#pragma unroll
        for (int rr = 0; rr < R; ++rr) live |= (((cp[rr * tg.cull_words] >> (4 * (blockIdx.x & 7))) & 15u) != 0u ? 1u : 0u) << rr;
    }
    for (int rr = 0; rr < R; ++rr) {
        const int row = row0 + rr;                      // relative to row_begin; the same for the whole wave
        if (row >= tg.row_count) return;
        const bool rowhit = (live >> rr) & 1u;
        const int orow = tg.row_begin + row;
        const int y = nt_image_row(tg, orow);
        if (y >= tg.height) continue;
        PixelRef pr;
        pr.x = x;
        pr.y = y;
        pr.offset = (long long)blockIdx.z * tg.frame_stride + (long long)(tg.compact ? orow : y) * tg.pitch + (long long)x * tg.bpp;
        pr.hit_index = 0;
        pr.valid = true;
        const float sy = tg.fovI * ((float)y - tg.half_h);
#pragma unroll
        for (int j = 0; j < N; ++j) dir[j] = base[j] - up[j] * sy;
        float sq = dir[0] * dir[0];
#pragma unroll
        for (int j = 1; j < N; ++j) sq = sq + dir[j] * dir[j];
        box_pixel<N, false>(tg, pr, org, dir, sq, dots, sx, sy, margin, rowhit);
    }
}

// The stretches box_tile_kernel<N, false> left behind in the redo bitmap (tg.redo; packed RGB, N > 8): one wave per (frame,
// row, word of 32 stretches), every set bit rendered with the complete box_pixel -- classification, box_resolve, box_color.
// The wave hands its bits back zeroed: the tile kernel marks the bitmap with atomic ORs, and it must be clean when the next
// launch starts.
// SPLIT (small launches): 2 or 4 waves per word, wave k for the stretches k, k + SPLIT, ... -- the marked stretches
// of a row come in runs, and with few rows in flight a run of ten is a long tail for one wave.
template <int N, int SPLIT>
__global__ __launch_bounds__(256) void box_redo_kernel(NtCameraFixed cam, NtTarget tg) {
    const int tid = (int)threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    static_assert(SPLIT == 1 || SPLIT == 2 || SPLIT == 4, "waves per redo word");
    const int row = (int)blockIdx.y * (4 / SPLIT) + wv / SPLIT;
    if (row >= tg.row_count) return;
    uint32_t *word = tg.redo + ((size_t)blockIdx.z * tg.row_count + row) * tg.redo_words + blockIdx.x;
    const uint32_t mine = (SPLIT == 1 ? 0xffffffffu : SPLIT == 2 ? 0x55555555u : 0x11111111u) << (wv % SPLIT);
    uint32_t todo = *word & mine;
    if (todo == 0u) return;
    if ((tid & 63) == 0) {
        if (SPLIT > 1) atomicAnd(word, ~mine);  // (the other waves may not have read the word yet: each needs its own bits only)
        else *word = 0u;
    }
    float org[N], right[N], up[N], fwd[N], dir[N];
    load_camera<N>(cam, org, right, up, fwd);
    float margin = fabsf(org[0]);
#pragma unroll
    for (int j = 1; j < N; ++j) margin = fmaxf(margin, fabsf(org[j]));
    margin = NT_BOX_MARGIN * (1.0f + margin);
    float dots[4];
    if (cam.buf) {
        const float *dp = cam.dots + (size_t)blockIdx.z * 4;
        dots[0] = dp[0]; dots[1] = dp[1]; dots[2] = dp[2]; dots[3] = dp[3];
    } else {
        dots[0] = cam.odots[0]; dots[1] = cam.odots[1]; dots[2] = cam.odots[2]; dots[3] = cam.odots[3];
    }
    const int orow = tg.row_begin + row;
    const int y = nt_image_row(tg, orow);
    if (y >= tg.height) return;
    const float sy = tg.fovI * ((float)y - tg.half_h);
    while (todo != 0u) {
        const int bit = __builtin_ctz(todo);
        todo &= todo - 1u;
        int x = ((int)blockIdx.x * 32 + bit) * 64 + (tid & 63);
        x = x < tg.width ? x : tg.width - 1;            // as in box_tile_kernel
        PixelRef pr;
        pr.x = x;
        pr.y = y;
        pr.offset = (long long)blockIdx.z * tg.frame_stride + (long long)(tg.compact ? orow : y) * tg.pitch + (long long)x * tg.bpp;
        pr.hit_index = 0;
        pr.valid = true;
        const float sx = tg.fovI * ((float)x - tg.half_w);
#pragma unroll
        for (int j = 0; j < N; ++j) dir[j] = (fwd[j] + right[j] * sx) - up[j] * sy;
        float sq = dir[0] * dir[0];
#pragma unroll
        for (int j = 1; j < N; ++j) sq = sq + dir[j] * dir[j];
        box_pixel<N, true, false, true>(tg, pr, org, dir, sq, dots, sx, sy, margin);
    }
}

// What can be said about a whole 64-pixel stretch of a row?  One thread per stretch.  Its rays are v = vc + right*e
// with vc the direction through its middle and |e| <= 32*fovI: v_j lies in [vc_j - g_j, vc_j + g_j],
// g_j = 32*fovI*|right_j| (+1e-6 for the rounding of v itself).
//  * code 0 -- no ray can reach the cube.  A ray that comes within h = 1 + 2m + 1e-3 of the cube in every coordinate
//    at some tau > 0 (every ray the reference could call a hit does, see box_classify) satisfies
//        (vc_j + g_j)*tau >= -h - o_j     and     (vc_j - g_j)*tau <= h - o_j         for every j:
//    2n half-lines in tau; an empty intersection clears the stretch, and the kernels paint background there without
//    looking further.  Convexity makes this sharp: what is left is within half a stretch of the cube's silhouette.
//  * code K+1 -- every ray clearly hits face K, K = the face the middle ray enters last.  With v_K of one sign over
//    the stretch, tau_K = (s_K - o_K)/v_K ranges over [tlo, thi]; if for every other j the extremes of
//    o_j + v_j*tau over that box stay inside 1 - m*(1 + |v_j|max/|v_K|min) (less 1e-4 for the arithmetic here), then for
//    each ray the reference's test of face K passes with room to spare, and every other slab was entered at least
//    m/|v_K| earlier, i.e. while p_K was outside 1+m, so no face before K can pass its j = K check (the argument of
//    box_classify).  box_tile_kernel shades such rows from v_K alone.
//  * code 15 -- anything else: the rays are classified one by one;  code 14 -- a near-tie stretch (the middle ray's last two
//    entries are within m/|v_K| of each other): box_tile_kernel goes straight to the reference's arithmetic there, or leaves
//    the stretch to box_redo_kernel (packed RGB, N > 8).
//  box_kernel<N> only asks whether a stretch is culled (code 0) and classifies every ray of the others.
// Reciprocals are approximate (v_rcp_f32); the slacks above are ~1000x their error.
// The code of one 64-pixel stretch (see the comment above): row y of the image, stretch `col` of the row.
// `sets` (box_tile_kernel): for a stretch of code 14 or 15, what box_resolve works out ray by ray from entry times -- the faces T that
// can still be the reference's answer and the coordinates C one of them could fail at -- as supersets valid for EVERY ray
// of the stretch (bits 0..9: T, bits 10..19: C, bit 31: valid, bit 24: every ray hits a face of T -- NT_BOX_SETS_SURE), so that box_tile_kernel goes straight to the reference's
// arithmetic on them in its near-tie stretches.  With [A_j, B_j] the range of slab j's entry time over the stretch's directions: every ray's last
// entry is at or after TN = max_j A_j; M = m / (the smallest |v_j| of an axis that can be last, B_j >= TN) is at least the
// ray's m/|v_K|; so a face within m/|v_K| of a ray's last entry has B_j >= TN - M: that is T.  The entries of T's faces,
// for any ray, lie in [min_{T} A_j, max_j B_j]; a coordinate that stays inside 1 - m over that span of tau, for all the
// stretch's directions, passes every test made there: the others, and T itself, are C.  (A face of T that a given ray
// enters long before its last entry fails at that ray's last axis, which is in T, hence in C.)  No valid sets when a candidate's v_j
// changes sign in the stretch or TN - M is not clearly positive (rays starting on or in the cube: box_color's business).
template <int N, bool SETS = false, bool SURE = false>
__device__ __forceinline__ unsigned long long box_stretch_code2(const float (&org)[N], const float (&right)[N], const float (&up)[N],
                                                                const float (&fwd)[N], const NtTarget &tg, int y, int col) {
    // returns the code in the low dword and, SETS, the sets in the high one
    uint32_t sets_value = 0u;
    uint32_t *const sets = SETS ? &sets_value : nullptr;
    uint32_t code = 0u;
    float omax = fabsf(org[0]);
#pragma unroll
    for (int j = 1; j < N; ++j) omax = fmaxf(omax, fabsf(org[j]));
    const float m = NT_BOX_MARGIN * (1.0f + omax);
    const float h = 1.0f + 2.0f * m + 1e-3f;
    const float sxc = tg.fovI * (((float)(col * 64) + 31.5f) - tg.half_w);
    const float sy = tg.fovI * ((float)y - tg.half_h);
    const float spread = 32.0f * tg.fovI;
    float tlo = 0.0f, thi = INFINITY;
    float vc[N], g[N];
    float tn = -INFINITY, tn2 = -INFINITY, vK = 0.0f, gK = 0.0f, oK = 0.0f;
    int K = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        vc[j] = (fwd[j] + right[j] * sxc) - up[j] * sy;
        g[j] = fmaf(spread, fabsf(right[j]), 1e-6f);
        const float pa = vc[j] + g[j], qa = -h - org[j];
        const float pb = vc[j] - g[j], qb = h - org[j];
        const float ra = qa * __builtin_amdgcn_rcpf(pa), rb = qb * __builtin_amdgcn_rcpf(pb);
        // pa*tau >= qa bounds tau from below when pa > 0, from above when pa < 0; pb*tau <= qb the other way round.  A zero
        // (always +0: g > 0, and x + y is -0 only for two negative zeros) goes with the positive side: ra is then
        // -inf (no bound), +inf (qa > 0: no tau at all -- tlo = inf) or a NaN, 0*inf, which drops out of max / min
        const bool ap = pa >= 0.0f, bp = pb >= 0.0f;
        const float lo_a = ap ? ra : -INFINITY, hi_a = ap ? INFINITY : ra;
        const float hi_b = bp ? rb : INFINITY, lo_b = bp ? -INFINITY : rb;
        tlo = nt_vmax3(tlo, lo_a, lo_b);
        thi = nt_vmin3(thi, hi_a, hi_b);
    }
    if (!(tlo > thi)) {                              // a NaN keeps the stretch
        code = 15u;
        // the middle ray's entries into the slabs: the last one, K, and the one before it (any K is verified below, so
        // accuracy only matters for the yield).  Only for stretches that survive: most tiles have none.
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float nr = ((vc[j] < 0.0f ? 1.0f : -1.0f) - org[j]) * __builtin_amdgcn_rcpf(vc[j]);
            tn2 = nt_vmed3(tn, tn2, nr);                        // second-to-last entry
            const bool later = nr > tn;
            vK = later ? vc[j] : vK;
            gK = later ? g[j] : gK;
            oK = later ? org[j] : oK;
            K = later ? j : K;
            tn = nt_vmax(tn, nr);
        }
        const float vKa = vK - gK, vKb = vK + gK;
        if (K < 13 && vKa * vKb > 0.0f) {            // (the code of a one-face stretch is K + 1 <= 13: 14 and 15 are taken; faces 13..15 of N > 13 go without)
            const float num = (vK < 0.0f ? 1.0f : -1.0f) - oK;
            const float t1 = num * __builtin_amdgcn_rcpf(vKa), t2 = num * __builtin_amdgcn_rcpf(vKb);
            const float t_lo = nt_vmin(t1, t2) * (1.0f - 1e-6f), t_hi = nt_vmax(t1, t2) * (1.0f + 1e-6f);
            // (the smaller of |vKa|, |vKb| with both of one sign: |vK| - gK, rounded the same way)
            const float rK = m * __builtin_amdgcn_rcpf(fabsf(vK) - gK) * (1.0f + 1e-6f);
            bool ok = t_lo > 1e-3f && t_hi < 1e30f;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float va = vc[j] - g[j], vb = vc[j] + g[j];
                const float pmax = org[j] + nt_vmax(vb * t_lo, vb * t_hi);
                const float pmin = org[j] + nt_vmin(va * t_lo, va * t_hi);
                // (the larger of |va|, |vb| is |vc| + g, rounded the same way)
                const float lim = (1.0f - m - 1e-4f) - (fabsf(vc[j]) + g[j]) * rK;
                ok = ok && (j == K || (pmax <= lim && pmin >= -lim));
            }
            if (ok) code = (uint32_t)K + 1u;
        }
        // The middle ray enters two slabs within m/|v_K| of each other: box_classify would call the rays around it
        // unclear and box_kernel would hand the stretch to box_redo_kernel after classifying all of it -- send it
        // there directly (code 14; only a prediction: box_redo_kernel is right for any stretch).
        if (code == 15u && !((tn - tn2) * fabsf(vK) > m)) code = 14u;
        if (code >= 14u) {
            if (sets != nullptr && N <= 10) {
                auto range = [&](int j, float &A, float &B, float &vabs) {
                    const float va = vc[j] - g[j], vb = vc[j] + g[j];
                    const float num = (vc[j] < 0.0f ? 1.0f : -1.0f) - org[j];
                    const float e1 = num * __builtin_amdgcn_rcpf(va), e2 = num * __builtin_amdgcn_rcpf(vb);
                    const float lo = nt_vmin(e1, e2), hi = nt_vmax(e1, e2);
                    const bool same = va * vb > 0.0f;
                    A = same ? lo - fabsf(lo) * 1e-6f : -INFINITY;             // (v_rcp_f32: 1 ulp)
                    B = same ? hi + fabsf(hi) * 1e-6f : INFINITY;
                    vabs = same ? fabsf(vc[j]) - g[j] : 0.0f;                  // (the smaller of |va|, |vb|)
                };
                // (the ranges are kept for the two passes that follow: with interleaved rows nearly every wave of the middle strips
                // has a stretch that needs its sets, so this is no longer a rare path -- and working each range out three times, two
                // v_rcp_f32 each, was a twentieth of the kernel's vector instructions; 3N registers that are dead again before
                // the row loops begin)
                float rA[N], rB[N], rV[N];
                float TN = -INFINITY, TH = -INFINITY;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    range(j, rA[j], rB[j], rV[j]);
                    TN = nt_vmax(TN, rA[j]);
                    TH = nt_vmax(TH, rB[j]);
                }
                float vmin = INFINITY;                  // the smallest |v_j| an axis that can be last has anywhere in the stretch
#pragma unroll
                for (int j = 0; j < N; ++j) vmin = rB[j] >= TN ? nt_vmin(vmin, rV[j]) : vmin;
                const float M = m * __builtin_amdgcn_rcpf(vmin) * (1.0f + 1e-5f);
                // T, and the earliest entry of any of its faces for any ray: every test the redo kernel makes is made at a
                // tau in [t_lo, t_hi]
                uint32_t T = 0u, C = 0u;
                float t_lo = INFINITY;
                const float t_hi = TH;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const bool inT = rB[j] >= TN - M;
                    T |= inT ? 1u << j : 0u;
                    t_lo = inT ? nt_vmin(t_lo, rA[j]) : t_lo;
                }
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const float va = vc[j] - g[j], vb = vc[j] + g[j];
                    const float pmax = org[j] + nt_vmax(vb * t_lo, vb * t_hi);
                    const float pmin = org[j] + nt_vmin(va * t_lo, va * t_hi);
                    const float lim = 1.0f - m - 1e-4f;
                    const bool inC = ((T >> j) & 1u) != 0u || !(pmax <= lim && pmin >= -lim);
                    C |= inC ? 1u << j : 0u;
                }
                const bool valid = vmin > 0.0f && t_lo > 1e-3f && t_hi < 1e30f;         // (a NaN fails)
                *sets = valid ? (0x80000000u | (C << 10) | T) : 0u;
                if constexpr (SURE) {
                    // the "sure hit" bit (NT_BOX_SETS_SURE, see there): C == T, no slab left inside the window, no axis of T
                    // further out than the bound on the reference's rounding allows.  One vector instruction an axis: the
                    // largest |v_j| is taken over all axes, not T's alone (of the bench's cameras' stretches that costs none its
                    // bit, tools/box_sets_census.py), and which axes are too far out is the same for every stretch of a frame:
                    // an integer compare of |o_j|'s bits -- a NaN counts as too far -- on the scalar unit.
                    float wmax = 0.0f;
                    uint32_t far_axes = 0u;
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        wmax = nt_vmax3_abs(wmax, vc[j] - g[j], vc[j] + g[j]);            // (the larger is |vc_j| + g_j)
                        far_axes |= (__float_as_uint(org[j]) & 0x7fffffffu) > __float_as_uint(NT_BOX_TIE_SURE_MAX_ORIGIN) ? 1u << j : 0u;
                    }
                    const bool sure = valid && C == T && (T & far_axes) == 0u && (t_hi - t_lo) * wmax <= 1.0f;      // (a NaN fails)
                    *sets |= sure ? NT_BOX_SETS_SURE : 0u;
                }
            }
        }
    }
    return (unsigned long long)code | ((unsigned long long)sets_value << 32);
}
template <int N>
__device__ __forceinline__ uint32_t box_stretch_code(const float (&org)[N], const float (&right)[N], const float (&up)[N], const float (&fwd)[N],
                                                     const NtTarget &tg, int y, int col) {
    return (uint32_t)box_stretch_code2<N, false>(org, right, up, fwd, tg, y, col);
}

template <int N>
__global__ __launch_bounds__(256) void box_cull_kernel(NtCameraFixed cam, NtTarget tg, uint32_t *out, int ncols) {
    float org[N], right[N], up[N], fwd[N];
    load_camera<N>(cam, org, right, up, fwd);
    // a half-wave = 32 stretches of one row: blockIdx.x = which 32, blockIdx.y = which 8 rows
    const int word = (int)blockIdx.x, row = (int)blockIdx.y * 8 + (int)(threadIdx.x >> 5);
    const int col = word * 32 + (int)(threadIdx.x & 31);
    uint32_t code = 0u;
    if (row < tg.row_count && col < ncols) {
        const int orow = tg.row_begin + row;
        const int y = nt_image_row(tg, orow);
        code = box_stretch_code<N>(org, right, up, fwd, tg, y, col);
    }
    // eight stretches to a dword
    uint32_t packed = code << (4 * (threadIdx.x & 7));
    packed |= (uint32_t)__shfl_xor((int)packed, 1, 64);
    packed |= (uint32_t)__shfl_xor((int)packed, 2, 64);
    packed |= (uint32_t)__shfl_xor((int)packed, 4, 64);
    if (row < tg.row_count && (threadIdx.x & 7) == 0) out[((size_t)blockIdx.z * tg.row_count + row) * tg.cull_words + (col >> 3)] = packed;
}

// --------------------------------------------------------------------------------------
// The fused path for the two formats the reference's scripts render into (packed plain RGB of <= 10 bits a channel in
// one aligned dword -- RGBX8 & co.: F32 = false; three plain fp32 channels, 12-byte pixels: F32 = true):
//
//   box_tile_kernel<N, F32, ROWS, WAVES>   a block = 64 columns x WAVES*ROWS rows (at most 64: one row per lane of the wave
//                                   that works out the stretch codes, box_stretch_code, and leaves them in LDS); after the
//                                   barrier every wave renders its ROWS rows from them with the lean loops, all of them in
//                                   one pass (one wave a block, 64 rows: no LDS, no barrier -- the codes stay in the lanes
//                                   that worked them out).  Per-row parameters come from the host's row table through
//                                   scalar loads (NtTarget::rowtab).  Packed RGB at N > 8: a row it cannot settle (code 14,
//                                   or a lane that needs the reference's face-by-face arithmetic) gets its bit set in the
//                                   redo bitmap, [frame][row][word of 32 stretches], with an atomic OR.
//   box_redo_kernel<N, SPLIT>       one wave per (frame, row, word): the marked stretches with box_pixel<REDO>; it hands the
//                                   word back zeroed, so the bitmap is clean for the next launch (the host zeroes it once).
// No pre-kernel; the only scratch is the bitmap (one bit per 64 pixels).
// --------------------------------------------------------------------------------------
// ROWS x WAVES: 64 x 1 for launches of 512 rows or more with waves to spare (what depends on the column alone is set up once
// for 64 rows); otherwise 16 (8 in small launches) x 4, or x 3 when that leaves fewer idle waves below the last row of the
// launch (a rank's 136 rows of a 1080-row frame: three tiles of 48 rows instead of three of 64).
// (experiment switch: -DNT_EXP_NOSTORE times the tile kernel's lean loops without their stores)
#ifdef NT_EXP_NOSTORE
#define NT_EXP_STORE_IF if (tg.width < 0)
#else
#define NT_EXP_STORE_IF
#endif
// Occupancy (-DNT_TILE_OCC=..., set per dimension in nt_inst_box.hip).  The waves a SIMD are decided by BOTH register files:
// 512 / VGPRs and floor(800 / (ceil(SGPRs / 16) * 16 + 16)) -- with 106 SGPRs that is six, whatever `amdgpu_waves_per_eu` says
// about the vector registers (round 2 "held the kernel to 64 VGPRs for eight waves" and saw 1 % for six spilled dwords a lane:
// it was still running six).  Up to n = 6 the kernels are given an SGPR budget of 96, which admits seven.
#ifndef NT_TILE_OCC
#define NT_TILE_OCC
#endif
#ifndef NT_BOX_PIN_UP
#define NT_BOX_PIN_UP 1
#endif
// The packed-RGB lean loops take aligned groups of four slots at once where all four rows are culled, or all four are the one
// face K0: one scalar load and one wait for the four table entries, one branch on the four guards, one instruction to clear the
// four bits -- the vector arithmetic of every row is the one-row loop's.  Groups of four up to this N (0: nowhere, the build to
// measure against); beyond 20 the tile kernels are held to 168 VGPRs and already spill to scratch, and the group body's sixteen
// live values a lane would spill more.
#ifndef NT_BOX_LEAN_GROUPS_MAX_N
#define NT_BOX_LEAN_GROUPS_MAX_N 20
#endif
// The lean rows' guard: t keeps G * (1 + t) clear of every k + 1/2, so that the cheap quotient and the reference's round to
// the same integer (box_tile_kernel, packed RGB).  G is sized per dimension from the distance between the two quotients.
//
// The budget, in units of u = 2^-24 (one fp32 rounding, relative), first order in u; everything is relative to the exact
// T = |d| maxval / sqrt(S), S = sum_j (base_j - up_j sy)^2 = BB - 2 BU sy + UU sy^2 over the fp32 values base_j, up_j, sy that
// both sides start from, and d = dir[K] is the same fp32 number on both sides.  Write a = BB, b = UU sy^2, X = 2 |BU sy|.
// fastsq (bu^2 <= bb uu / 16) gives X <= sqrt(ab) / 2, hence S >= a + b - sqrt(ab) / 2 >= 3/4 (a + b), and b <= 16/15 S.
//   lean_quotient
//     bb, uu: N fma each, sums of squares: N a, N b.   bu: N fma, by Cauchy-Schwarz N sqrt(BB UU), times 2 |sy|: 2N sqrt(ab).
//     The three products with 1/maxval^2: a, b and X.   Without the X: (N + 1)(a + b) + 2N sqrt(ab), which over S grows with
//     sqrt(ab) / (a + b) and is largest at a = b:                                 (8N + 4) / 3
//     the two fma of the evaluation: |sy| |sy uu + m2bu| <= b + X, and S; with the X above (2X + b) / S + 1 <=    2.52
//     (2X <= sqrt(ab); over S that is largest near a = b / 3, 1.51)
//     1/maxval^2 itself (a square and a reciprocal, common to the three):         2
//     rsq halves the sum: (4N + 2) / 3 + 2.26; v_rsq_f32 at 1 ulp: 2; |d| * rsq: 1 (the half of a hit's t is exact)
//                                                                            =>   4N/3 + 5.93
//   the reference
//     dir_j = fl(base_j - fl(up_j sy)) is off by (|up_j sy| + |dir_j|) u, its square's sum by 2 (sqrt(S b) + S) <= 4.07 S;
//     N products and N - 1 additions left to right: N.   sqrtf halves the sum: N/2 + 2.04; sqrtf: 1; the division: 1; the
//     product with maxval is exact (quantize multiplies the mantissa as an integer)
//                                                                            =>   N/2 + 4.04
// Sum: 11N/6 + 9.97 <= 11N/6 + 10 -- 21 at N = 6, 54 at N = 24.  (The worst cases above do not meet: over the
// culled and one-face pixels of tests/test_box_lean_guard_host.py's cameras, which it holds to the budget one by one, the largest
// distance is 6.7 at N = 8.)
constexpr double nt_lean_budget_ulps(int n) { return 11.0 * n / 6.0 + 10.0; }
// The width: the smallest power of two that leaves 1.5 times the budget, not below 2^-20 (box_pixel's guard for an exact sq) and
// not above 2^-18, the one width every kernel had: 2^-19 for N = 3..6, 2^-18 beyond.  At the cap the factor is less than 1.5 from
// N = 18 on (1.19 at N = 24), as it always was; the budget itself fits at every N.
// -DNT_BOX_LEAN_GUARD_LOG2=18: that width everywhere, the device code as it was -- the build to measure and to test against.
constexpr int nt_lean_guard_log2(int n) {
#ifdef NT_BOX_LEAN_GUARD_LOG2
    return NT_BOX_LEAN_GUARD_LOG2;
#else
    for (int k = 20; k > 18; --k)
        if ((double)(1 << (24 - k)) >= 1.5 * nt_lean_budget_ulps(n)) return k;
    return 18;
#endif
}
template <int N>
__device__ __forceinline__ bool guard_clear(float t) {
    constexpr int K = nt_lean_guard_log2(N);
    static_assert(K >= 18 && K <= 20, "the lean rows' guard: 2^-20 .. 2^-18");
    static_assert((double)(1 << (24 - K)) >= (K == 18 ? 1.0 : 1.5) * nt_lean_budget_ulps(N), "the lean rows' guard holds 1.5 times the budget below the cap, the budget at it");
    constexpr float G = 1.0f / (float)(1 << K);
    return fabsf(__builtin_amdgcn_fractf(t) - 0.5f) > fmaf(t, G, G);
}
// ... and their quotient |d| * maxval / |dir| from the quadratic in sy (uu, m2bu, bb: |dir|^2 / maxval^2 = bb + m2bu sy + uu sy^2)
__device__ __forceinline__ float lean_quotient(float d, float sy, float uu, float m2bu, float bb) {
    return fabsf(d) * __builtin_amdgcn_rsqf(fmaf(sy, fmaf(sy, uu, m2bu), bb));
}
// component K (wave-uniform) of `base` and of `up`, by selects: the arrays stay in registers
template <int N>
__device__ __forceinline__ void pick_component(uint32_t K, const float (&base)[N], const float (&upv)[N], float &bK, float &uK) {
    bK = base[0];
    uK = upv[0];
#pragma unroll
    for (int j = 1; j < N; ++j) {
        bK = K == (uint32_t)j ? base[j] : bK;
        uK = K == (uint32_t)j ? upv[j] : uK;
    }
}
// dir = base - up * sy and its |dir|^2, in the reference's order of operations
template <int N>
__device__ __forceinline__ float row_dir(const float (&base)[N], const float (&upv)[N], float sy, float (&dir)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) dir[j] = base[j] - upv[j] * sy;
    float sq = dir[0] * dir[0];
#pragma unroll
    for (int j = 1; j < N; ++j) sq = sq + dir[j] * dir[j];
    return sq;
}
// Edge rows (packed RGB, N = 6, the 64 x 1 kernel of launches of NT_BOX_TIE_SHORTCUT_MIN_WAVES waves or more -- the one with TIE;
// why only there: below): a row sorted ray by ray whose stretch has valid sets with two coordinates in C -- a < b -- and T = C or one of the two: the cube's outline, or an edge between two faces
// (63 % of the code-15 rows of the bench's cameras, tools/box_sets_census.py).  Set by set, as the one-face rows go face by face:
// the first such row's sets word is read, one vector compare finds the rows that share it, the components a, b of `base`, `up`
// and the origin are picked once, and a row of the set computes dir[a], dir[b], dir[0] alone -- the mul and sub of row_dir, bit
// for bit its values -- and asks box_classify_sets<2> on those two axes, its sets word a compile-time constant (three cases: T =
// {a}, {b}, {a, b}).  The verdicts are the N-axis call's, lane for lane: the argument above box_classify_sets (last axis, second
// entry, inside sum, miss) carries over unchanged on one added premise -- the two arrays hold exactly the axes of C, in ascending
// order, so that every max, min and sum runs over the same values in the same order, and the sum is set against 2 c = |C| c.
// A row with an unclear lane stores nothing here and stays with the general loop.  A clear row is x = v_K (hit) or dir[0]
// (background) through the lean rows' quotient behind their guard (guard_clear<N>, 2^-19 at N = 6: t, and t/2 of a hit), whose error
// budget holds for any component (face_row uses it for dir[K], culled_row for dir[0]); a row with a lane inside the guard stays
// with the general loop as well.  No floating-point operation that reaches a pixel is new.
// (No cap on the sets a wave takes: picking the components costs about thirty vector instructions a set, so even a set of one
// row is cheaper here than in the general loop; of the bench's cameras and of 3000 random ones no wave held more than four.)
// Where.  The code needs box_classify_sets (N = 6 and 7) and is in the kernel that launch_box_fixed takes for large launches
// only, as the near-tie short cut is and for its reason: built into box_tile_kernel<6, false, 64, 1, false> as well it cost a
// rank's eighth of the headline call (14 400 waves) 67.97 -> 68.67 us, spreads 0.05 and 0.15, while the headline call (81 600
// waves, the kernel with TIE) gained 292.4 -> 288.0 us.  N = 7 has no such kernel (nt_inst_box.hip) and goes without.
// -DNT_BOX_EDGE_ROWS=0: without, the device code as it was: the build to measure and to test against.
#ifndef NT_BOX_EDGE_ROWS
#define NT_BOX_EDGE_ROWS 1
#endif
// (the dimensions whose kernels sort a row on its stretch's sets; which of their kernels: EDGE in box_tile_kernel)
template <int N>
constexpr bool nt_box_edge_rows() {
    return NT_BOX_EDGE_ROWS != 0 && N >= NT_BOX_CLASSIFY_SETS_MIN_N && N <= NT_BOX_CLASSIFY_SETS_MAX_N && N <= NT_BOX_SETS_MAX_N && N <= NT_BOX_INLINE_MAX_N;
}
// Rows a pass of the row phase covers in the 64 x 1 shape: all 64 (masks of 64 row bits in scalar register pairs), or 16 -- the
// sixteen-row passes the kernel had while its codes went through a qword of LDS, four a wave, each with its own header: the build
// to measure against.  The 16- and 8-row shapes take their rows in one pass either way.
#ifndef NT_BOX_PASS_ROWS
#define NT_BOX_PASS_ROWS 64
#endif
// masks of row bits, 32 or 64 of them: the lowest set bit, and mask &= ~(1 << bit) / mask |= 1 << bit as ONE scalar instruction
// (the compiler writes mask & (mask - 1) as an add and an and): the lean loops run about as many scalar instructions a row as
// vector ones
__device__ __forceinline__ int nt_low_bit(uint32_t m) { return __builtin_ctz(m); }
__device__ __forceinline__ int nt_low_bit(unsigned long long m) { return __builtin_ctzll(m); }
__device__ __forceinline__ int nt_count_bits(uint32_t m) { return __builtin_popcount(m); }
__device__ __forceinline__ int nt_count_bits(unsigned long long m) { return __builtin_popcountll(m); }
__device__ __forceinline__ void nt_clear_bit(uint32_t &m, int bit) { asm("s_bitset0_b32 %0, %1" : "+s"(m) : "s"(bit)); }
__device__ __forceinline__ void nt_clear_bit(unsigned long long &m, int bit) { asm("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(bit)); }
__device__ __forceinline__ void nt_set_bit(uint32_t &m, int bit) { asm("s_bitset1_b32 %0, %1" : "+s"(m) : "s"(bit)); }
__device__ __forceinline__ void nt_set_bit(unsigned long long &m, int bit) { asm("s_bitset1_b64 %0, %1" : "+s"(m) : "s"(bit)); }
// ... and without its lowest set bit (`bit`), as the loops outside the lean ones always stepped: 32 bits, the compiler's add and
// and; 64 bits, where that is an add, an add with carry and an and, the one instruction
__device__ __forceinline__ void nt_drop_low_bit(uint32_t &m, int) { m &= m - 1u; }
__device__ __forceinline__ void nt_drop_low_bit(unsigned long long &m, int bit) { nt_clear_bit(m, bit); }
// TIE: the near-tie rows' short cut (NT_BOX_SETS_SURE) is in this kernel -- launch_box_fixed says for which launches
template <int N, bool F32, int ROWS, int WAVES, bool TIE = false>
__global__ __launch_bounds__(64 * WAVES) NT_TILE_OCC void box_tile_kernel(NtCameraFixed cam, NtTarget tg) {
    static_assert(!TIE || (!F32 && ROWS == 64 && nt_box_tie_shortcut<N>()), "the short cut: packed RGB, 64 x 1, the dimensions it is built for");
    static_assert(ROWS == 8 || ROWS == 16 || ROWS == 64, "a wave's rows: a qword of sixteen codes in LDS or fewer, or one row a lane");
    static_assert(WAVES >= 1 && WAVES <= 4 && WAVES * ROWS <= 64, "the codes of a tile are the work of one wave, a row per lane");
    static_assert(WAVES == 1 ? ROWS == 64 : ROWS <= 16, "one wave a block renders the 64 rows whose codes it worked out itself");
    constexpr int R = ROWS;
    // One wave a block: the wave that works out the codes is the one that renders their rows.  Code and tie sets of slot s stay in
    // lane s, in one register (sets: bits 0..19, 24 and 31 as box_stretch_code2 leaves them; code: bits 20..23), and the row phase
    // fetches them with v_readlane_b32 on the slot's scalar index: no LDS, no barrier.  More waves a block: another wave's codes
    // come through LDS.
    constexpr bool REG = WAVES == 1;
    constexpr int LDS_N = REG ? 1 : 64;
    __shared__ uint32_t s_code[LDS_N];
    // ... and the same as one bit per tile row and class (culled / one face / ray by ray / near-tie): the row loops are driven by
    // masks of row bits -- two scalar instructions to step, one to index the row table (masks of nibble positions in a
    // qword cost five and two; the scalar unit is as busy as the vector units in these loops)
    __shared__ unsigned long long s_rows[REG ? 1 : 4];
    // F32: this kernel is bound by its stores (12 bytes a pixel), not by vector instructions, and renders the near-tie and
    // unclear stretches itself -- no second kernel; the tie sets of its rows stay in LDS
    // ... and so does the packed format up to eight dimensions, where the codes wave's tie sets (LDS) give the near-tie
    // stretches their short cut: the second kernel's work costs this kernel a tenth of its time and saves a third of it
    // (BoxScene(6): 423 -> 410 us a call; 75 VGPRs instead of 70).  Beyond eight -- no tie sets -- it loses: BoxScene(10) 4096^2
    // 6-12 % slower without box_redo_kernel, BoxScene(16) 15 %.
    constexpr bool ALLIN = F32 || N <= NT_BOX_INLINE_MAX_N;
    constexpr bool SETS_LDS = ALLIN && N <= NT_BOX_SETS_MAX_N;
    constexpr uint32_t SETS_MASK = 0x800fffffu | (TIE ? NT_BOX_SETS_SURE : 0u);       // what of a sets word lane_cs keeps
    __shared__ uint32_t s_sets[SETS_LDS ? LDS_N : 1];
    __shared__ int s_abort;                  // the codes wave's reading of NtTarget::abort_word: one answer for the whole block
    uint32_t lane_cs = 0u;                   // REG: code and tie sets of the slot that is this lane
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
#ifdef NT_EXP_TRACE
    const unsigned long long trace_t0 = wall_clock64();          // ablation builds: per-wave residency record (tools/box_wave_trace.py)
    unsigned trace_rows = 0u;                                    // rows by class: culled | one face << 8 | ray by ray << 16 | near-tie << 24
    unsigned long long trace_t1 = 0ull;                          // end of the codes phase
#endif
    // Work order.  Blocks start in grid order -- column, tile row, then z -- and a wave with sixty-four rows to sort ray by ray
    // lives ten times as long as one with none: with z = frame the long waves of the last frames were still running, almost
    // alone, 60 us after the grid had been handed out (tools/box_wave_trace.py).  The long waves are in the middle columns of
    // the image (the scripts' cameras look at the cube), so those columns run tg.lead_frames frames ahead of the outer ones: z
    // counts lead_frames + nframes slots, slot z holds the middle columns of frame z and the outer columns of frame
    // z - lead_frames; the grid ends on short waves only.  (A block whose frame does not exist leaves at once.)
    const unsigned nframes = gridDim.z - (unsigned)tg.lead_frames;
    unsigned frame = blockIdx.z;
    if (tg.lead_frames > 0) {
        const unsigned cols = gridDim.x, q = cols / 4u;
        const bool middle = blockIdx.x >= q && blockIdx.x < cols - q;
        if (!middle) frame -= (unsigned)tg.lead_frames;          // (wraps for the first slots: >= nframes)
        if (frame >= nframes) return;
    }
    float org[N], right[N], up[N], fwd[N], dir[N];
    load_camera<N>(cam, frame, org, right, up, fwd);
    float margin = fabsf(org[0]);
#pragma unroll
    for (int j = 1; j < N; ++j) margin = fmaxf(margin, fabsf(org[j]));
    margin = NT_BOX_MARGIN * (1.0f + margin);
    float dots[4];
    if (cam.buf) {
        const float *dp = cam.dots + (size_t)frame * 4;
        dots[0] = dp[0]; dots[1] = dp[1]; dots[2] = dp[2]; dots[3] = dp[3];
    } else {
        dots[0] = cam.odots[0]; dots[1] = cam.odots[1]; dots[2] = cam.odots[2]; dots[3] = cam.odots[3];
    }
    const int tile_row0 = (int)blockIdx.y * WAVES * R;
    // the strip against the frame's span (NT_BOX_STRIP_SPAN, see there): wave-uniform, two scalar loads; +-inf and NaN compare
    // as they should (no statement: never outside; the empty interval: always)
    // (dimensions beyond NT_BOX_SPAN_MAX_N never get a statement: their kernels go without the test)
    bool strip_out = false;
    if constexpr (NT_BOX_STRIP_SPAN != 0 && N <= NT_BOX_SPAN_MAX_N) {
      if (cam.span != nullptr) {
        const float *sp = cam.span + (size_t)frame * 2;
        const float span_lo = sp[0], span_hi = sp[1];
        const int x_first = (int)blockIdx.x * 64;
        const int x_last = x_first + 63 < tg.width ? x_first + 63 : tg.width - 1;
        // (the smaller and the larger of the two: a negative fovI turns the strip round)
        const float sx_a = tg.fovI * ((float)x_first - tg.half_w), sx_b = tg.fovI * ((float)x_last - tg.half_w);
        strip_out = fmaxf(sx_a, sx_b) < span_lo || fminf(sx_a, sx_b) > span_hi;
      }
    }
    // ---- phase 1: the tile's stretch codes, one row per lane of one wave -- a different one from block to block, so that
    // the extra work does not always land on the same SIMD of a CU
    if (REG || wv == (int)((blockIdx.x + blockIdx.y + frame) % (unsigned)WAVES)) {
        if (tg.abort_word != nullptr) {
            const bool ab = nt_aborted(tg);
            if constexpr (REG) { if (ab) return; }
            else { if (lane == 0) s_abort = ab ? 1 : 0; }
        }
        uint32_t code = 0u;
        uint32_t row_sets = 0u;
        // lane <-> slot tile_row0 + lane = row rr of wave w; interleaved: that wave's rr-th row is w + W * rr (NtTarget::row_il)
        const int trow = tg.row_il > 0 ? ((int)blockIdx.y * WAVES + lane / R) + tg.row_il * (lane % R) : tile_row0 + lane;
        if (!strip_out && lane < WAVES * R && trow < tg.row_count) {
            const int orow = tg.row_begin + trow;
            const int y = nt_image_row(tg, orow);
            if (y < tg.height) {
                // (N > 8: the sets' arithmetic would raise the kernel's register allocation -- 124 VGPRs and spills at N = 10 --
                // for every row; those dimensions go without)
                const unsigned long long cs = box_stretch_code2<N, (N <= NT_BOX_SETS_MAX_N), TIE>(org, right, up, fwd, tg, y, (int)blockIdx.x);
                code = (uint32_t)cs;
                row_sets = (uint32_t)(cs >> 32);
            }
        }
        if constexpr (REG) {
            lane_cs = (SETS_LDS ? row_sets & SETS_MASK : 0u) | (code << 20);
        } else {
            if (SETS_LDS) s_sets[lane] = row_sets;
            {
                const unsigned long long m0 = __builtin_amdgcn_ballot_w64(code == 0u), m1 = __builtin_amdgcn_ballot_w64(code >= 1u && code <= 13u),
                                         m2 = __builtin_amdgcn_ballot_w64(code == 15u), m3 = __builtin_amdgcn_ballot_w64(code == 14u);
                if (lane == 0) {
                    s_rows[0] = m0;
                    s_rows[1] = m1;
                    s_rows[2] = m2;
                    s_rows[3] = m3;
                }
            }
            // rows of wave w in nibbles of s_code[2w] (rows 0..7) and s_code[2w + 1] (rows 8..15)
            uint32_t packed = code << (4 * (lane & 7));
            packed |= (uint32_t)__shfl_xor((int)packed, 1, 64);
            packed |= (uint32_t)__shfl_xor((int)packed, 2, 64);
            packed |= (uint32_t)__shfl_xor((int)packed, 4, 64);
            if ((lane & 7) == 0) {
                const int grp = lane >> 3;                                   // eight rows each
                const int slot = R == 8 ? 2 * grp : grp;                     // R == 8: wave w's rows are group w
                s_code[slot] = packed;
                if (R == 8) s_code[slot + 1] = 0u;
            }
        }
    }
    if constexpr (!REG) {
        __syncthreads();
        if (tg.abort_word != nullptr && s_abort != 0) return;
    }
#ifdef NT_EXP_TRACE
    trace_t1 = wall_clock64();
#endif
    // The row phase takes PASS rows a pass: all the wave's rows at once, driven by masks of one bit a row (64 bits in the 64 x 1
    // shape) -- or, -DNT_BOX_PASS_ROWS=16, that shape's rows sixteen at a time, the same driver run four times.  What depends on
    // the column alone (forward + right*sx, the quadratic for |dir|^2) is set up once for all the wave's rows.
    constexpr int PASS = R == 64 ? NT_BOX_PASS_ROWS : R;
    static_assert(PASS == R || (R == 64 && PASS == 16), "NT_BOX_PASS_ROWS: 64 or 16");
    typedef typename std::conditional<PASS == 64, unsigned long long, uint32_t>::type mask_t;
    const int wrow0 = tile_row0 + wv * R;                     // the wave's first slot (its first row when rows are not interleaved)
    const int il = tg.row_il;                                 // (scalar) 0, or the stride between a wave's rows
    const int wfirst = il > 0 ? (int)blockIdx.y * WAVES + wv : wrow0;
    if (wfirst < tg.row_count) {
        typedef uint32_t nt_u32x4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(4))) const nt_u32x4 *nt_rowtab;
        // four entries in a row (the table is in slot order): one s_load_dwordx16
        typedef uint32_t nt_u32x16 __attribute__((ext_vector_type(16), aligned(16)));
        typedef __attribute__((address_space(4))) const nt_u32x16 *nt_rowtab4;
        constexpr bool GROUPS = !F32 && N <= NT_BOX_LEAN_GROUPS_MAX_N;
        constexpr bool EDGE = TIE && !F32 && REG && PASS == 64 && nt_box_edge_rows<N>();
        uint8_t *const frame_base = tg.dest + (long long)frame * tg.frame_stride;
        // What a row loop needs to know about its row -- sy of the ray source and the row's byte offset in a frame -- comes
        // from a table the host wrote (NtTarget::rowtab, 16 bytes per owned row: sy, -, offset), read through the scalar
        // data cache (constant address space: s_load_dwordx4): no vector instruction, nothing per lane
#define NT_ROW_LOAD(rr)                     \
        const nt_u32x4 row_e = tab[(rr)];   \
        const float sy = __uint_as_float(row_e.x)
#define NT_ROW_OFF() ((long long)(((unsigned long long)row_e.w << 32) | row_e.z) + (long long)frame * tg.frame_stride)
        // a store goes to (row pointer: scalar registers) + (the lane's byte offset in the row: 32 bits) -- the addressing
        // mode of global_store with an SGPR base, no vector arithmetic on addresses
#define NT_ROW_PTR() uniform_ptr(frame_base + (long long)(((unsigned long long)row_e.w << 32) | row_e.z))
        // ... of row k of a group of four (grp_e: its four entries)
#define NT_GROUP_PTR(k) uniform_ptr(frame_base + (long long)(((unsigned long long)grp_e[4 * (k) + 3] << 32) | grp_e[4 * (k) + 2]))
        // (instruction selection works block by block and only recognises base + zero-extended 32-bit offset when it sees the
        // extension: the empty asm keeps it from being hoisted out of the row loops)
#define NT_LANE_OFF() ({ asm volatile("" : "+v"(xoff)); xoff; })
        // (one scalar instruction each, on 32 or 64 row bits: nt_clear_bit)
#define NT_CLEAR_BIT(mask, bit) nt_clear_bit(mask, bit)
#define NT_SET_BIT(mask, bit) nt_set_bit(mask, bit)
        int x = (int)blockIdx.x * 64 + lane;
        x = x < tg.width ? x : tg.width - 1;
        uint32_t xoff = (uint32_t)x * (uint32_t)tg.bpp;
        const float sx = tg.fovI * ((float)x - tg.half_w);
        float base[N];
#pragma unroll
        for (int j = 0; j < N; ++j) base[j] = fwd[j] + right[j] * sx;
        // `up` in vector registers: up[j] * sy has the scalar sy as its one scalar operand
        float upv[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            upv[j] = up[j];
            // (NT_BOX_PIN_UP = 0: only up[0], the one the culled rows' loop multiplies -- the others stay in scalar registers and
            // are moved over where a row needs them, which is what lets the n = 6 kernel fit seven waves' registers unspilled)
            // (the fp32 kernel, bound by its stores, keeps them pinned: unpinned it executes 8 % more instructions for nothing)
            if (NT_BOX_PIN_UP || F32 || j == 0) asm volatile("" : "+v"(upv[j]));
        }
        // packed RGB: rows that are background or one face throughout need |dir|^2 only to ~2^-19 (see the guard below): as a
        // quadratic in sy, |base - up*sy|^2 = bb - 2 bu sy + uu sy^2 (bb = base.base, bu = base.up, uu = up.up), it costs two fma a
        // row instead of the N-1 other components and their squares.  Its absolute error is ~2.7n*2^-24*(bb + sy^2 uu), and that
        // is relative to the result as long as the cross term cannot cancel the squares: lanes check bu^2 <= bb*uu/16 (any sane
        // camera: up is orthogonal to forward and right), and a wave with a lane that fails it never takes the shortcut (fastsq).
        float bb = 0.0f, bu = 0.0f, uu = 0.0f;
        bool fastsq = true;
        if (!F32) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                bb = fmaf(base[j], base[j], bb);
                bu = fmaf(base[j], up[j], bu);
                uu = fmaf(up[j], up[j], uu);
            }
            fastsq = __builtin_amdgcn_ballot_w64(!(bu * bu <= bb * uu * 0.0625f)) == 0ull;
        }
        const float maxv = (float)tg.plain_maxval;
        // ... scaled by 1/maxval^2, so that rsq of it is maxval/|dir|: the multiplication by maxval costs three instructions a
        // wave instead of one a row (three more roundings of 2^-24 each, counted in the guard's budget: guard_clear)
        const float inv_maxv2 = 1.0f / (maxv * maxv);
        const float m2bu = (-2.0f * bu) * inv_maxv2;
        bb = bb * inv_maxv2;
        uu = uu * inv_maxv2;
        // the classes of the wave's rows, a bit per row
        const uint32_t lane_code = (lane_cs >> 20) & 15u;       // (REG)
        unsigned long long rows_culled, rows_face, rows_rays, rows_tie;
        if constexpr (REG) {
            // one wave a block: the ballots themselves
            rows_culled = __builtin_amdgcn_ballot_w64(lane_code == 0u);
            rows_face = __builtin_amdgcn_ballot_w64(lane_code >= 1u && lane_code <= 13u);
            rows_rays = __builtin_amdgcn_ballot_w64(lane_code == 15u);
            rows_tie = __builtin_amdgcn_ballot_w64(lane_code == 14u);
        } else {
            auto rows_of = [&](int k) {
                const unsigned long long m = s_rows[k];
                return (((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32) |
                        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m)) >> (wv * R);
            };
            rows_culled = rows_of(0);
            rows_face = rows_of(1);
            rows_rays = rows_of(2);
            rows_tie = rows_of(3);
        }
        // Which of the wave's rows exist: one slot per lane (lane l <-> slot wrow0 + l), once for all the wave's rows -- the
        // band arithmetic and the launch parameters it reads stay out of the row loops, whose scalar registers are short.
        // Every lane stays active in the row loops -- lanes past the right edge redo the last pixel (same bytes, same value)
        // instead of leaving
        const int lrow = il > 0 ? wfirst + il * lane : wrow0 + lane;
        const int ly = nt_image_row(tg, tg.row_begin + lrow);
        const unsigned long long rows_valid = __builtin_amdgcn_ballot_w64(lane < R && lrow < tg.row_count && ly < tg.height);
#pragma unroll 1
        for (int pass = 0; pass < R / PASS; ++pass) {
        const int slot0 = PASS * pass;                        // the pass's first slot among the wave's
        const int row0 = wrow0 + slot0;                       // ... among the launch's
        const int hfirst = il > 0 ? wfirst + il * slot0 : row0;            // ... and that row
        if (hfirst >= tg.row_count) break;
        mask_t redo_bits = 0u;                                // rows (bit rr) left to box_redo_kernel
        // Code and tie sets of slot rr of the pass.  REG: one v_readlane_b32 from the lane that worked them out; otherwise the
        // codes wave's qword of sixteen nibbles and its dword of sets, from LDS.
        unsigned long long rowcodes = 0ull;
        if constexpr (!REG) {
            rowcodes = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)s_code[2 * wv + 1]) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)s_code[2 * wv]);
        }
        auto slot_word = [&](int rr) { return (uint32_t)__builtin_amdgcn_readlane((int)lane_cs, slot0 + rr); };
        auto code_of = [&](int rr) {
            if constexpr (REG) return (slot_word(rr) >> 20) & 15u;
            else return (uint32_t)(rowcodes >> (4 * rr)) & 15u;
        };
        auto sets_of = [&](int rr) {
            if constexpr (!SETS_LDS) return 0u;
            else if constexpr (REG) return slot_word(rr) & SETS_MASK;
            else return (uint32_t)__builtin_amdgcn_readfirstlane((int)s_sets[wv * R + rr]);
        };
        // the rows of the pass whose code is c (a face's): one vector compare -- of the lane's own code, or of its nibble of the qword
        auto rows_with_code = [&](uint32_t c) {
            if constexpr (REG) return (mask_t)(__builtin_amdgcn_ballot_w64(lane_code == c) >> slot0);
            else return (mask_t)__builtin_amdgcn_ballot_w64(lane < PASS && ((uint32_t)(rowcodes >> (4 * (lane & 15))) & 15u) == c);
        };
        const mask_t valid = R > PASS ? (mask_t)(rows_valid >> slot0) & (mask_t)((1ull << (PASS & 63)) - 1ull) : (mask_t)rows_valid;
        // (interleaved rows: the table is in slot order and belongs to this launch's row range)
        const nt_rowtab tab = (nt_rowtab)tg.rowtab + (il > 0 ? row0 : tg.row_begin + row0);
        // (bit rr <-> row row0 + rr; code 14 -- a near-tie stretch -- is not looked at here unless this kernel is all there is)
        mask_t quick = (mask_t)(rows_culled >> slot0) & valid, inner = (mask_t)(rows_face >> slot0) & valid;
        mask_t todo = (mask_t)((ALLIN ? rows_rays | rows_tie : rows_rays) >> slot0) & valid;
        if (!ALLIN) redo_bits = (mask_t)(rows_tie >> slot0) & valid;
#ifdef NT_EXP_TRACE
        trace_rows += (unsigned)nt_count_bits(quick) | ((unsigned)nt_count_bits(inner) << 8) |
                      ((unsigned)nt_count_bits((mask_t)(rows_rays >> slot0) & valid) << 16) |
                      ((unsigned)nt_count_bits((mask_t)(rows_tie >> slot0) & valid) << 24);
#endif
        if (!F32) {
            // ---- packed RGB: guarded rsq quantisation.  round(|dir[K]|/len * maxval) (and its half for a hit), as in box_pixel,
            // with the guard widened for the quadratic |dir|^2: t is within nt_lean_budget_ulps(N) * 2^-24 (1 + t) of the
            // reference's quotient (derived at guard_clear: 21 at N = 6, 54 at N = 24), and the guard is sized from that per
            // dimension -- 2^-19 up to N = 6, 2^-18 beyond.  A wave with a lane inside it takes the row ray by ray.
            if (!fastsq) {
                todo |= quick | inner;
                quick = 0u;
                inner = 0u;
            }
            // (the two loops in two copies: 8-bit fields on byte boundaries -- v_perm_b32 packing, tg.plain_sel -- and the rest;
            // the test is made once here, not once a row)
            auto lean_rows = [&](auto sel8) {
            constexpr bool SEL8 = decltype(sel8)::value;
            // the packed pixel of a culled row (t: the guarded quotient, d0: dir[0]) and of a one-face row (t and its half)
            // (-DNT_EXP_RED_BY_SHIFT, measured and not taken, DESIGN.md 4.1: culled_row hands over -dir[0], and the red byte is
            // q AND the sign of that spread over the dword -- a shift and an AND, both full rate, for the compare and the select.
            // The same bytes: dir[0] = +-0 has t = 0 either way, and a NaN fails the guard before any store.)
#ifdef NT_EXP_RED_BY_SHIFT
#define NT_RED_OF(q, d0) ((q) & (uint32_t)((int32_t)__float_as_uint(d0) >> 31))
#else
#define NT_RED_OF(q, d0) ((d0) > 0.0f ? (q) : 0u)
#endif
            auto put_quick = [&](nt_gptr out, float t, float d0) {
                if (SEL8) {
                    // 8-bit fields: t + 2^23 has round(t) in its low mantissa byte (t < 255.5; the guard keeps t off the
                    // half-way points, so nearest-even is the reference's rounding), which is the byte v_perm_b32 picks
                    const uint32_t q = __float_as_uint(t + 8388608.0f);
                    // (the red byte is zero where dir[0] is not positive: a select on every row.  Until the end of round 3 the
                    // select sat behind a wave-uniform branch -- its sign rarely changes within a stretch -- but the branch and
                    // the jump around it are scalar instructions, and the scalar unit is the busier one in this loop: 1.4 % of
                    // the headline call)
                    NT_EXP_STORE_IF NT_G32(out) = __builtin_amdgcn_perm(NT_RED_OF(q, d0), q, tg.plain_sel);
                    return;
                }
                uint32_t q = (uint32_t)(t + 0.5f);
                q = q < tg.plain_maxval ? q : tg.plain_maxval;
                const uint32_t w = NT_RED_OF(q, d0) * tg.plain_mul[0] + q * (tg.plain_mul[1] + tg.plain_mul[2]);      // (emit_plain)
                NT_EXP_STORE_IF NT_G32(out) = tg.reversed ? w : bswap32(w);
            };
            auto put_face = [&](nt_gptr out, float t, float th) {
                if (SEL8) {
                    NT_EXP_STORE_IF NT_G32(out) = __builtin_amdgcn_perm(__float_as_uint(t + 8388608.0f), __float_as_uint(th + 8388608.0f), tg.plain_sel);
                    return;
                }
                uint32_t qr = (uint32_t)(t + 0.5f), qgb = (uint32_t)(th + 0.5f);
                qr = qr < tg.plain_maxval ? qr : tg.plain_maxval;
                qgb = qgb < tg.plain_maxval ? qgb : tg.plain_maxval;
                const uint32_t w = qr * tg.plain_mul[0] + qgb * (tg.plain_mul[1] + tg.plain_mul[2]);
                NT_EXP_STORE_IF NT_G32(out) = tg.reversed ? w : bswap32(w);
            };
            // bit 4k of the result: bits 4k .. 4k + 3 of the mask are all set
            auto full_groups = [](mask_t mask) { return mask & (mask >> 1) & (mask >> 2) & (mask >> 3) & (mask_t)(PASS == 64 ? 0x1111111111111111ull : 0x1111ull); };
            // The aligned group of four slots g .. g + 3.  row(sy, a, b): one row's arithmetic and its own guard as in the one-row
            // loops below (a, b: what `put` stores; returns "clear"), nothing shared between rows; the four guards' outcomes stay
            // scalar lane masks, and one branch decides for the four stores.  Otherwise the clear rows are stored one by one and the
            // others handed on -- on the spot: a few per cent of the rows fail their guard, so one group in ten has such a row, and a
            // build that sent those groups through the one-row loop again measured 1.2 % slower on the headline than one without groups.
            auto lean_group = [&](int g, auto row, auto put) {
                const nt_u32x16 grp_e = *(nt_rowtab4)(tab + g);
                float a[4], b[4];
                unsigned long long fail[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) fail[k] = __builtin_amdgcn_ballot_w64(!row(__uint_as_float(grp_e[4 * k]), a[k], b[k]));
                if (__builtin_expect(((fail[0] | fail[1]) | (fail[2] | fail[3])) == 0ull, 1)) {
                    const uint32_t xo = NT_LANE_OFF();
                    put(NT_GROUP_PTR(0) + xo, a[0], b[0]);
                    put(NT_GROUP_PTR(1) + xo, a[1], b[1]);
                    put(NT_GROUP_PTR(2) + xo, a[2], b[2]);
                    put(NT_GROUP_PTR(3) + xo, a[3], b[3]);
                } else {
                    // (rare) the rows with a lane too close to a rounding boundary go on to the ray-by-ray loop
                    todo |= (mask_t)((fail[0] != 0ull ? 1u : 0u) | (fail[1] != 0ull ? 2u : 0u) | (fail[2] != 0ull ? 4u : 0u) | (fail[3] != 0ull ? 8u : 0u)) << g;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (fail[k] == 0ull) {
                            uint32_t xo = xoff;
                            asm volatile("" : "+v"(xo));
                            put(NT_GROUP_PTR(k) + xo, a[k], b[k]);
                        }
                    }
                }
            };
            // a culled row: t and dir[0]
            auto culled_row = [&](float sy, float &t, float &d0) {
#ifdef NT_EXP_RED_BY_SHIFT
                d0 = upv[0] * sy - base[0];                               // -dir[0], exactly (the same product, the operands swapped)
#else
                d0 = base[0] - upv[0] * sy;                               // dir[0], bit for bit
#endif
                t = lean_quotient(d0, sy, uu, m2bu, bb);
                return guard_clear<N>(t);
            };
            // a row of one face, bK and uK its components of `base` and `up`: t and its half
            auto face_row = [&](float bK, float uK, float sy, float &t, float &th) {
                const float dK = bK - uK * sy;                            // dir[K], bit for bit
                t = lean_quotient(dK, sy, uu, m2bu, bb);
                th = t * 0.5f;
                return guard_clear<N>(t) && guard_clear<N>(th);
            };
            // ---- 1. aligned groups of four culled rows (groups that are mixed or cut by `valid` are left to 2.)
            if (GROUPS) {
                mask_t full = full_groups(quick);
                quick &= ~(full * 15u);
                while (full != 0u) {
                    const int g = nt_low_bit(full);
                    NT_CLEAR_BIT(full, g);
                    lean_group(g, culled_row, put_quick);
                }
            }
            // ---- 2. the remaining culled rows, one by one
            mask_t quick_stored = 0u;
            for (mask_t rest = quick; rest != 0u;) {
                const int rr = nt_low_bit(rest);
                NT_CLEAR_BIT(rest, rr);
                NT_ROW_LOAD(rr);
                float t, d0;
                // (a row with a lane too close to a rounding boundary stores nothing and is not marked: the clear row is the
                // straight path, one branch taken a row where an if / else was laid out with three)
                if (__builtin_expect(__builtin_amdgcn_ballot_w64(!culled_row(sy, t, d0)) == 0ull, 1)) {
                    put_quick(NT_ROW_PTR() + NT_LANE_OFF(), t, d0);
                    NT_SET_BIT(quick_stored, rr);
                }
            }
            todo |= quick & ~quick_stored;
            // The one-face rows, face by face (a wave has one to three): K0 is the face of the first row left, its components of
            // `base` and `up` are picked once, and one vector compare finds the rows that share it.
            while (inner != 0u) {
                const uint32_t code0 = code_of(nt_low_bit(inner));
                float bK0, uK0;
                pick_component<N>(code0 - 1u, base, upv, bK0, uK0);
                mask_t same = inner & rows_with_code(code0);
                inner &= ~same;
                // ---- 3. its aligned groups of four
                if (GROUPS) {
                    mask_t full = full_groups(same);
                    same &= ~(full * 15u);
                    while (full != 0u) {
                        const int g = nt_low_bit(full);
                        NT_CLEAR_BIT(full, g);
                        lean_group(g, [&](float sy, float &t, float &th) { return face_row(bK0, uK0, sy, t, th); }, put_face);
                    }
                }
                // ---- 4. its remaining rows, one by one
                mask_t same_stored = 0u;
                for (mask_t rest = same; rest != 0u;) {
                    const int rr = nt_low_bit(rest);
                    NT_CLEAR_BIT(rest, rr);
                    NT_ROW_LOAD(rr);
                    float t, th;
                    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!face_row(bK0, uK0, sy, t, th)) == 0ull, 1)) {
                        put_face(NT_ROW_PTR() + NT_LANE_OFF(), t, th);
                        NT_SET_BIT(same_stored, rr);
                    }
                }
                todo |= same & ~same_stored;
            }
            // ---- 5. the edge rows, set by set (NT_BOX_EDGE_ROWS, see there)
            if constexpr (EDGE) {
                mask_t edge = fastsq ? (mask_t)rows_rays & valid : (mask_t)0u;
                if (edge != 0u) {
                    // the lane's own word: valid, T inside C, |C| = 2, and T = C or |T| = 1
                    const uint32_t lT = lane_cs & 0x3ffu, lC = (lane_cs >> 10) & 0x3ffu;
                    const bool two = (lane_cs & 0x80000000u) != 0u && (lT & ~lC) == 0u && __builtin_popcount(lC) == 2 && (lT == lC || __builtin_popcount(lT) == 1);
                    edge &= (mask_t)__builtin_amdgcn_ballot_w64(two);
                }
                // the packed pixel of a clear row: t of x, tgb its half for a hit, red unless the background looks down dir[0]
                auto put_edge = [&](nt_gptr out, float t, float tgb, bool red) {
                    if (SEL8) {
                        const uint32_t q8r = __float_as_uint(t + 8388608.0f), q8gb = __float_as_uint(tgb + 8388608.0f);
                        NT_EXP_STORE_IF NT_G32(out) = __builtin_amdgcn_perm(red ? q8r : 0u, q8gb, tg.plain_sel);
                        return;
                    }
                    uint32_t qr = (uint32_t)(t + 0.5f), qgb = (uint32_t)(tgb + 0.5f);
                    qr = qr < tg.plain_maxval ? qr : tg.plain_maxval;
                    qgb = qgb < tg.plain_maxval ? qgb : tg.plain_maxval;
                    const uint32_t w = (red ? qr : 0u) * tg.plain_mul[0] + qgb * (tg.plain_mul[1] + tg.plain_mul[2]);
                    NT_EXP_STORE_IF NT_G32(out) = tg.reversed ? w : bswap32(w);
                };
                mask_t edge_stored = 0u;
                while (edge != 0u) {
                    const uint32_t w0 = slot_word(nt_low_bit(edge)) & 0x800fffffu;
                    const mask_t same = edge & (mask_t)__builtin_amdgcn_ballot_w64((lane_cs & 0x800fffffu) == w0);
                    edge &= ~same;
                    const uint32_t c0 = (w0 >> 10) & 0x3ffu;
                    const uint32_t ja = (uint32_t)__builtin_ctz(c0), jb = 31u - (uint32_t)__builtin_clz(c0);          // C = {ja < jb}
                    float bA, uA, bB, uB;
                    pick_component<N>(ja, base, upv, bA, uA);
                    pick_component<N>(jb, base, upv, bB, uB);
                    float oA = org[0], oB = org[0];
#pragma unroll
                    for (int j = 1; j < N; ++j) {
                        oA = ja == (uint32_t)j ? org[j] : oA;
                        oB = jb == (uint32_t)j ? org[j] : oB;
                    }
                    // the rows of the set; TSEL: which of the two axes are in T (bit 0: ja, bit 1: jb)
                    auto set_rows = [&](auto tsel) {
                        constexpr uint32_t WORD = 0x80000000u | (3u << 10) | decltype(tsel)::value;
                        for (mask_t rest = same; rest != 0u;) {
                            const int rr = nt_low_bit(rest);
                            NT_CLEAR_BIT(rest, rr);
                            NT_ROW_LOAD(rr);
                            const float o2[2] = {oA, oB};
                            const float v2[2] = {bA - uA * sy, bB - uB * sy};            // dir[ja], dir[jb], bit for bit
                            const float v0 = base[0] - upv[0] * sy;                     // dir[0]
                            bool hit, unclear;
                            float x;
                            box_classify_sets<2, WORD>(o2, v2, margin, WORD, hit, unclear, x);
                            x = hit ? x : v0;
                            const float t = lean_quotient(x, sy, uu, m2bu, bb);
                            const float tgb = hit ? t * 0.5f : t;
                            // (& on ints for &&: three lane masks and two scalar ands, where && was laid out as two branches on exec)
                            const bool ok = ((int)!unclear & (int)guard_clear<N>(t) & (int)guard_clear<N>(tgb)) != 0;
                            if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) == 0ull, 1)) {
                                put_edge(NT_ROW_PTR() + NT_LANE_OFF(), t, tgb, hit || x > 0.0f);
                                NT_SET_BIT(edge_stored, rr);
                            }
                        }
                    };
                    const bool inA = ((w0 >> ja) & 1u) != 0u, inB = ((w0 >> jb) & 1u) != 0u;
                    if (inA && inB) set_rows(std::integral_constant<uint32_t, 3u>{});
                    else if (inA) set_rows(std::integral_constant<uint32_t, 1u>{});
                    else set_rows(std::integral_constant<uint32_t, 2u>{});
                }
                todo &= ~edge_stored;
            }
            };
            if (tg.plain_sel != 0u) lean_rows(std::true_type{});
            else lean_rows(std::false_type{});
        } else {
            // ---- fp32 channels: the stored value IS x / sqrtf(sq), so the reference's sum, square root and division are
            // done as they stand -- but on rows whose code says which x it is, nothing else is
            while (quick != 0u) {
                // background rows: i = dir[0]; i > 0 ? (i,i,i) : (0,-i,-i) (tracer.hpp:109-113), clamped as channel_value does
                const int rr = nt_low_bit(quick);
                nt_drop_low_bit(quick, rr);
                NT_ROW_LOAD(rr);
                const float sq = row_dir<N>(base, upv, sy, dir);
                const float in = dir[0] / sqrt_wave(sq);
                float r, gb, b_;
                box_background(in, r, gb, b_);
                emit_f32x3_at(tg, NT_ROW_PTR() + NT_LANE_OFF(), r, gb);
            }
            // (face by face, as the packed formats' rows)
            while (inner != 0u) {
                const uint32_t code0 = code_of(nt_low_bit(inner));
                float bK0, uK0;
                pick_component<N>(code0 - 1u, base, upv, bK0, uK0);
                mask_t same = inner & rows_with_code(code0);
                inner &= ~same;
                while (same != 0u) {
                    // one face K throughout: sine = d_K * (-sign d_K) <= 0, shade = -sine (tracer.hpp:105-107)
                    const int rr = nt_low_bit(same);
                    nt_drop_low_bit(same, rr);
                    NT_ROW_LOAD(rr);
                    const float sq = row_dir<N>(base, upv, sy, dir);
                    const float xk = bK0 - uK0 * sy;                          // dir[K], bit for bit (the same two operations)
                    const float shade = fabsf(xk / sqrt_wave(sq));
                    emit_f32x3_at(tg, NT_ROW_PTR() + NT_LANE_OFF(), shade * 1.0f, shade * 0.5f);
                }
            }
        }
        while (todo != 0u) {
            const int rr = nt_low_bit(todo);
            nt_drop_low_bit(todo, rr);
            // (a row with a face code is here because its cheap quantisation failed: the face is known)
            const int rcode = (int)code_of(rr);
            const bool rowhit = rcode != 0;
            NT_ROW_LOAD(rr);
            PixelRef pr;
            pr.x = x;
            pr.y = 0;
            pr.offset = NT_ROW_OFF() + (long long)xoff;
            pr.hit_index = 0;
            pr.valid = true;
            const float sq = row_dir<N>(base, upv, sy, dir);
            if (ALLIN) {
                // everything here: classification, the reference's arithmetic on the faces in question (on the stretch's tie sets
                // for a near-tie stretch), box_color for rays that start on or in the cube
                box_pixel<N, !F32, false, false, F32, TIE>(tg, pr, org, dir, sq, dots, sx, sy, margin, rowhit, rcode >= 1 && rcode <= 13 ? rcode - 1 : -1,
                                                       sets_of(rr), rcode == 14);
            } else if (!box_pixel<N, true, true, false, false>(tg, pr, org, dir, sq, dots, sx, sy, margin, rowhit, rcode >= 1 && rcode <= 13 ? rcode - 1 : -1)) {
                redo_bits |= (mask_t)1u << rr;
            }
        }
        // mark the rows left over in the redo bitmap (clean on entry: box_redo_kernel zeroes what it has read)
        if (!ALLIN && lane == 0) {
            while (redo_bits != 0u) {
                const int rr = nt_low_bit(redo_bits);
                nt_drop_low_bit(redo_bits, rr);
                const int mrow = il > 0 ? hfirst + il * rr : row0 + rr;     // (hfirst, row0: of slot PASS * pass)
                atomicOr(tg.redo + ((size_t)frame * tg.row_count + mrow) * tg.redo_words + (blockIdx.x >> 5), 1u << (blockIdx.x & 31));
            }
        }
        }           // (a pass)
    }
#ifdef NT_EXP_TRACE
    if (lane == 0) {       // the records lie behind the last frame: [frame][tile row][column][wave] x 4 qwords
        unsigned long long *tr = reinterpret_cast<unsigned long long *>(tg.dest + (long long)nframes * tg.frame_stride) +
                                 ((((size_t)frame * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * WAVES + wv) * 4;
        tr[0] = trace_t0;
        tr[1] = wall_clock64();
        tr[2] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) | ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32);
        tr[3] = (unsigned long long)trace_rows | ((trace_t1 - trace_t0) << 32);
    }
#endif
#undef NT_ROW_LOAD
#undef NT_ROW_OFF
#undef NT_ROW_PTR
#undef NT_GROUP_PTR
#undef NT_LANE_OFF
#undef NT_CLEAR_BIT
#undef NT_SET_BIT
#undef NT_RED_OF
}

template <int N>
int launch_box_fixed(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg_in) {
    NtCameraFixed cf;
    cf.buf = cam.buf;
    cf.dots = cam.dots;
    cf.span = cam.buf ? cam.span : nullptr;
    for (int k = 0; k < 4; ++k) cf.odots[k] = cam.odots[k];
    cf.n = N;
    for (int k = 0; k < 4 * N; ++k) cf.inl[k] = cam.inl[k];
    NtTarget tg = tg_in;
    dim3 grid;
    grid_for(tg, 64, tg.colors_out ? 4 : 4 * NT_BOXROWS, li.nframes, grid);
    tg.cull = nullptr;
    tg.redo = nullptr;
    tg.cull_words = 0;
    tg.redo_words = 0;
    // the two formats of the reference's scripts take the fused kernels (no pre-kernel): packed plain RGB of at most 10 bits
    // a channel in one aligned dword, and three plain fp32 channels
    const bool fmt_rgb = tg.plain_bits != 0u && tg.plain_bits <= 10u && tg.bpp == 4 && tg.aligned4;
    const bool fmt_f32 = tg.plain_f32[0] >= 0 && tg.bpp == 12 && tg.aligned4;
    if (li.cull_buf && tg.rowtab && !tg.colors_out && (fmt_rgb || fmt_f32) && li.cull_clean) {
        hipStream_t st = (hipStream_t)li.stream;
        // rows a wave x waves a block (nt_box_tile_geom, nt_device.hpp -- the host's row table follows the same decision):
        // sixteen rows a lane once there are waves to spare (the per-wave set-up is a fifth of the work at eight), three waves a
        // block instead of four when that leaves fewer idle waves below the last row; sixty-four rows a lane, one wave a block
        // (the wave works out its own codes, and the set-up per column is shared by four times the rows) once the launch is tall
        // enough for such tiles to fit it well and has waves enough even so (four 4096 x 4096 frames are 16 384 such waves: 7 %
        // slower than with 16 rows a wave; sixteen frames: 9 % faster)
        NtBoxTileGeom geom;
        geom.rows = li.tile_rows;
        geom.waves = li.tile_waves;
        const bool r64 = geom.rows == 64, r16 = geom.rows == 16;
        const int wpb = geom.waves;
        const int tile_rows = geom.rows * geom.waves;
        dim3 tgrid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.row_count + tile_rows - 1) / tile_rows), (unsigned)li.nframes);
        tg.redo_words = ((tg.width + 63) / 64 + 31) / 32;
        tg.redo = li.cull_buf;                        // [frame][row][redo_words], all zero between launches
        // the middle columns 96 frames ahead of the outer ones (32 .. 96 measure alike on the 160-frame call: -4 %, and on
        // BoxScene(3): -3 %; a rank's eighth of the call: -3 % with 48, -6 % with 96; 16: half of it), in launches of 8 frames
        // or more (eight 4096 x 4096 frames of BoxScene(10): 621 -> 693 Grays/s; four: no difference)
        tg.lead_frames = li.nframes >= 8 ? (li.nframes < 96 ? li.nframes : 96) : 0;
        // ... with interleaved rows (round 3) a strip's waves are all alike and little is left for the lead to do: 160-frame call
        // 358 us without, 347 with 32, 354 with 96; 32- / 64- / 320-frame calls 1-2 % better with 8..16 than without and than
        // with more; sixteen 4096 x 4096 frames of BoxScene(10) 3 % WORSE with 16 than without (measured with the NTRACER_BOX_LEAD
        // override, since removed)
        if (tg.row_il > 0) tg.lead_frames = li.nframes >= 32 ? 16 : 0;
        if ((long long)li.nframes + tg.lead_frames > 65535) tg.lead_frames = 0;        // (grid z)
        tgrid.z += (unsigned)tg.lead_frames;
        if (fmt_rgb) {
            // (one 64-row wave a block; tgrid.z counts the lead slots too, hence li.nframes)
            bool tie = false;
            if constexpr (nt_box_tie_shortcut<N>()) tie = r64 && (unsigned long long)tgrid.x * tgrid.y * (unsigned)li.nframes >= (unsigned long long)NT_BOX_TIE_SHORTCUT_MIN_WAVES;
            if (tie) {
                if constexpr (nt_box_tie_shortcut<N>()) hipLaunchKernelGGL((box_tile_kernel<N, false, 64, 1, true>), tgrid, dim3(64), 0, st, cf, tg);
            } else if (r64) hipLaunchKernelGGL((box_tile_kernel<N, false, 64, 1>), tgrid, dim3(64), 0, st, cf, tg);
            else if (r16 && wpb == 3) hipLaunchKernelGGL((box_tile_kernel<N, false, 16, 3>), tgrid, dim3(192), 0, st, cf, tg);
            else if (r16) hipLaunchKernelGGL((box_tile_kernel<N, false, 16, 4>), tgrid, dim3(256), 0, st, cf, tg);
            else hipLaunchKernelGGL((box_tile_kernel<N, false, 8, 4>), tgrid, dim3(256), 0, st, cf, tg);
            if constexpr (N > NT_BOX_INLINE_MAX_N) {          // (up to there the tile kernel leaves nothing behind)
                // few rows in flight: two waves per redo word
                const long long rwords = (long long)tg.row_count * li.nframes * tg.redo_words;
                const int split = rwords < 48 * 1024 ? 2 : 1;   // (87k words: one wave 3 % faster; 44k: even; 22k: two waves 2 % faster;
                                                                //  four waves a word measured slower than two; NTRACER_BOX_SPLIT,
                                                                //  the override these were measured with, has been removed)
                const int rpb = 4 / split;              // rows per block
                const dim3 rgrid((unsigned)tg.redo_words, (unsigned)((tg.row_count + rpb - 1) / rpb), (unsigned)li.nframes);
                if (split == 2) hipLaunchKernelGGL((box_redo_kernel<N, 2>), rgrid, dim3(256), 0, st, cf, tg);
                else hipLaunchKernelGGL((box_redo_kernel<N, 1>), rgrid, dim3(256), 0, st, cf, tg);
            }
        } else {
            if (r64) hipLaunchKernelGGL((box_tile_kernel<N, true, 64, 1>), tgrid, dim3(64), 0, st, cf, tg);
            else if (r16 && wpb == 3) hipLaunchKernelGGL((box_tile_kernel<N, true, 16, 3>), tgrid, dim3(192), 0, st, cf, tg);
            else if (r16) hipLaunchKernelGGL((box_tile_kernel<N, true, 16, 4>), tgrid, dim3(256), 0, st, cf, tg);
            else hipLaunchKernelGGL((box_tile_kernel<N, true, 8, 4>), tgrid, dim3(256), 0, st, cf, tg);
            // (no second kernel: bound by its stores, the tile kernel has the vector instructions to spare)
        }
        return 0;
    }
    // every other format, and probe mode: the stretch codes (when there is a cull buffer), then the general kernel.  The codes
    // go to the start of the cull buffer, over the fused route's redo bitmap (plan_box's cull_clean accounts for that).
    if (li.cull_buf && !tg.colors_out) {
        const int ncols = (tg.width + 63) / 64;
        const int words = (ncols + 31) / 32;                    // 32 stretches of a row to a half-wave of box_cull_kernel
        tg.cull_words = 4 * words;
        hipLaunchKernelGGL(box_cull_kernel<N>, dim3((unsigned)words, (unsigned)((tg.row_count + 7) / 8), (unsigned)li.nframes), dim3(256), 0,
                           (hipStream_t)li.stream, cf, tg, li.cull_buf, ncols);
        tg.cull = li.cull_buf;
    }
    hipLaunchKernelGGL(box_kernel<N>, grid, dim3(256), 0, (hipStream_t)li.stream, cf, tg);
    return 0;
}

}  // namespace
