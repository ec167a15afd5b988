// nt_var.hip -- the run-time-n kernels (the reference's generic `tracern` / var_geometry.hpp path: n-vectors in LDS as
// [k][lane]), the small kernels around them (camera upload, lens / parallel / ambient occlusion expansion, outline marks, depth
// cues), and every nt_launch_* of nt_device.hpp: the dispatch over the dimension (nt_dispatch.hpp) to the compile-time-N launchers
// of the nt_inst_*.hip units, or to the run-time-n kernels here.
#include "nt_box.hpp"
#include "nt_composite.hpp"
#include "nt_query.hpp"
#include "nt_hits.hpp"
#include "nt_rays.hpp"
#include "nt_resolve.hpp"
#include "nt_adaptive.hpp"
#include "nt_outline.hpp"
#include "nt_cue.hpp"
#include "nt_boxhits.hpp"
#include "nt_boxshade.hpp"
#include "nt_layer_list.hpp"
#include "nt_dispatch.hpp"
#include <climits>

namespace {

// --------------------------------------------------------------------------------------
// BoxScene, run-time n (var_geometry.hpp -> per-lane n-vector in LDS, [j][lane] so that a
// wave's accesses to component j hit 64 consecutive banks)
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void box_kernel_var(NtCamera cam, NtTarget tg) {
    extern __shared__ float lds_dir[];    // [n][256] per-lane direction, then [4][n] camera rows (broadcast reads)
    const int tid = (int)threadIdx.x;
    const int n = cam.n;
    float *camrow = lds_dir + (size_t)n * 256;
    {
        // stage the camera rows once per block: run-time-indexed kernel arguments would be one scalar load each
        const float *src = cam.buf ? cam.buf + (size_t)blockIdx.z * 4 * n : nullptr;
        for (int k = tid; k < 4 * n; k += 256) camrow[k] = src ? src[k] : cam.inl[k];
    }
    __syncthreads();
    const PixelRef pr = locate_pixel<64, 4>(tg, tid & 63, tid >> 6, tid);
    if (!pr.valid) return;
    const float *c = camrow;              // origin, right, up, forward
    float *dir = lds_dir + tid;           // dir[j] at dir[j*256]
    const float sx = tg.fovI * ((float)pr.x - tg.half_w);
    const float sy = tg.fovI * ((float)pr.y - tg.half_h);
    float sq = 0.0f;
    for (int j = 0; j < n; ++j) {
        const float v = (c[3 * n + j] + c[n + j] * sx) - c[2 * n + j] * sy;
        dir[j * 256] = v;
        sq = j == 0 ? v * v : sq + v * v;
    }
    const float len = sqrtf(sq);

    bool done = false;
    float shade = 0.0f;
    // Same exact pruning as box_color<N> (see there): circumsphere rejection per wave on the unnormalised
    // direction (box_may_hit), then only the faces in a near-tie with the last-reached candidate K get the
    // division and the n-1 checks.  Waves that cannot hit normalise dir[0] only.
    float dots[4];
    if (cam.buf) {
        const float *dp = cam.dots + (size_t)blockIdx.z * 4;
        dots[0] = dp[0]; dots[1] = dp[1]; dots[2] = dp[2]; dots[3] = dp[3];
    } else {
        dots[0] = cam.odots[0]; dots[1] = cam.odots[1]; dots[2] = cam.odots[2]; dots[3] = cam.odots[3];
    }
    const float osq = dots[0];
    const float ov = fmaf(-dots[2], sy, fmaf(dots[1], sx, dots[3]));
    const float rad2 = (float)n * (1.0f + NT_FUZZ) * (1.0f + NT_FUZZ) * 1.001f;
    const bool maybe = !((osq - rad2 * 1.0001f - 1e-5f * osq) * sq > ov * ov * 1.0001f);   // FMA rounding covered by the margins
    const bool wave_maybe = __builtin_amdgcn_ballot_w64(maybe) != 0ull;
    if (wave_maybe) {
        for (int j = 0; j < n; ++j) dir[j * 256] = dir[j * 256] / len;
    } else {
        dir[0] = dir[0] / len;
    }
    if (wave_maybe) {
        float aK = 0.0f, bK = 1.0f, oK = 0.0f;
        bool any = false;
        for (int i = 0; i < n; ++i) {
            const float di = dir[i * 256];
            const float oi = c[i];
            const float num = (di < 0.0f ? 1.0f : -1.0f) - oi;
            const bool pre = maybe && ((num > 0.0f && di > 0.0f) || (num < 0.0f && di < 0.0f));
            const float a = fabsf(num), bb = fabsf(di);
            if (pre && (!any || a * bK > aK * bb)) { aK = a; bK = bb; oK = oi; any = true; }
        }
        const float mu = 1e-4f * (1.0f + fabsf(oK));
        const float aKm = (aK - mu) * (1.0f - 1e-6f);
        for (int i = 0; i < n; ++i) {
            const float di = dir[i * 256];
            const float oi = c[i];
            const float s = di < 0.0f ? 1.0f : -1.0f;
            const float num = s - oi;
            const bool pre = maybe && ((num > 0.0f && di > 0.0f) || (num < 0.0f && di < 0.0f));
            const bool tie = pre && !done && !(fabsf(num) * bK < fabsf(di) * aKm);
            if (__builtin_amdgcn_ballot_w64(tie) == 0ull) continue;
            const float dist = num / di;
            bool ok = tie && dist > 0.0f;
            for (int j = 0; j < n; ++j) {
                if (j != i) {
                    const float oj = c[j];
                    const float p = dir[j * 256] * dist + oj;
                    ok = ok && !(fabsf(p) > (1.0f + NT_FUZZ));
                }
            }
            if (ok) {
                done = true;
                if (dist >= FLT_MAX) shade = -1.0f;
                else {
                    const float sine = di * s;
                    shade = sine <= 0.0f ? -sine : 0.0f;
                }
            }
        }
    }
    float r, g, b;
    if (done && shade >= 0.0f) {
        r = shade * 1.0f;
        g = shade * 0.5f;
        b = shade * 0.5f;
    } else {
        const float in = dir[0];
        if (in > 0.0f) { r = in; g = in; b = in; }
        else { r = 0.0f; g = -in; b = -in; }
    }
    if (plain_rgb(tg)) {
        emit_plain(tg, pr, plain_quantize(tg, r), plain_quantize(tg, g));            // g == b
        return;
    }
    emit_pixel(tg, pr, r, g, b);
}

// --------------------------------------------------------------------------------------
// BoxScene, run-time n, packed plain RGB (RGBX8 & co.): the structure of box_tile_kernel (nt_box.hpp) with the n-vectors in
// LDS.  A block = 64 columns x 32 rows (four waves of eight rows); one wave works out the stretch codes of the tile
// (box_stretch_code_var: what box_stretch_code computes, with loops over n); then every lane works out the three dot products
// of forward + right*sx that give |dir|^2 as a quadratic in sy (the vector itself is recomputed where a row needs it), and
//   * rows the codes call background or one face throughout cost a handful of operations per pixel WHATEVER n is
//     (guarded rsq quantisation as in box_tile_kernel),
//   * the others are evaluated ray by ray like box_kernel_var does (the reference's arithmetic on the faces in a near-tie).
// --------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t box_stretch_code_var(int n, const float *camrow, const NtTarget &tg, int y, int col) {
    const float *org = camrow, *right = camrow + n, *up = camrow + 2 * n, *fwd = camrow + 3 * n;
    float omax = fabsf(org[0]);
    for (int j = 1; j < n; ++j) omax = fmaxf(omax, fabsf(org[j]));
    const float m = NT_BOX_MARGIN * (1.0f + omax);
    const float h = 1.0f + 2.0f * m + 1e-3f;
    const float sxc = tg.fovI * (((float)(col * 64) + 31.5f) - tg.half_w);
    const float sy = tg.fovI * ((float)y - tg.half_h);
    const float spread = 32.0f * tg.fovI;
    float tlo = 0.0f, thi = INFINITY;
    bool dead = false;
    float tn = -INFINITY, tn2 = -INFINITY, vK = 0.0f, gK = 0.0f, oK = 0.0f;
    int K = 0;
    for (int j = 0; j < n; ++j) {
        const float vc = (fwd[j] + right[j] * sxc) - up[j] * sy;
        const float g = fmaf(spread, fabsf(right[j]), 1e-6f);
        const float pa = vc + g, qa = -h - org[j];
        const float pb = vc - g, qb = h - org[j];
        const float ra = qa * __builtin_amdgcn_rcpf(pa), rb = qb * __builtin_amdgcn_rcpf(pb);
        const float lo_a = pa > 0.0f ? ra : -INFINITY, hi_a = pa < 0.0f ? ra : INFINITY;
        const float hi_b = pb > 0.0f ? rb : INFINITY, lo_b = pb < 0.0f ? rb : -INFINITY;
        tlo = fmaxf(tlo, fmaxf(lo_a, lo_b));
        thi = fminf(thi, fminf(hi_a, hi_b));
        dead = dead || (pa == 0.0f && qa > 0.0f) || (pb == 0.0f && qb < 0.0f);
        const float nr = ((vc < 0.0f ? 1.0f : -1.0f) - org[j]) * __builtin_amdgcn_rcpf(vc);
        tn2 = __builtin_amdgcn_fmed3f(tn, tn2, nr);
        const bool later = nr > tn;
        vK = later ? vc : vK;
        gK = later ? g : gK;
        oK = later ? org[j] : oK;
        K = later ? j : K;
        tn = fmaxf(tn, nr);
    }
    if (dead || tlo > thi) return 0u;                  // a NaN keeps the stretch
    uint32_t code = 15u;
    const float vKa = vK - gK, vKb = vK + gK;
    if (K <= 12 && vKa * vKb > 0.0f) {                 // (codes 1 .. 13 name the face)
        const float num = (vK < 0.0f ? 1.0f : -1.0f) - oK;
        const float t1 = num * __builtin_amdgcn_rcpf(vKa), t2 = num * __builtin_amdgcn_rcpf(vKb);
        const float t_lo = fminf(t1, t2) * (1.0f - 1e-6f), t_hi = fmaxf(t1, t2) * (1.0f + 1e-6f);
        const float rK = m * __builtin_amdgcn_rcpf(fminf(fabsf(vKa), fabsf(vKb))) * (1.0f + 1e-6f);
        bool ok = t_lo > 1e-3f && t_hi < 1e30f;
        for (int j = 0; j < n; ++j) {
            const float vc = (fwd[j] + right[j] * sxc) - up[j] * sy;
            const float g = fmaf(spread, fabsf(right[j]), 1e-6f);
            const float va = vc - g, vb = vc + g;
            const float pmax = org[j] + fmaxf(vb * t_lo, vb * t_hi);
            const float pmin = org[j] + fminf(va * t_lo, va * t_hi);
            const float lim = (1.0f - m - 1e-4f) - fmaxf(fabsf(va), fabsf(vb)) * rK;
            ok = ok && (j == K || (pmax <= lim && pmin >= -lim));
        }
        if (ok) code = (uint32_t)K + 1u;
    }
    return code;
}

__global__ __launch_bounds__(256) void box_rows_kernel_var(NtCamera cam, NtTarget tg) {
    constexpr int R = 8;
    // dirs [n][256], camera rows [4][n], codes [4].  (Until round 3 `forward + right*sx` sat in LDS as well, [n][256]: with it a
    // block needed 2n KB, and from n = 25 on it was LDS that set the occupancy -- two blocks a CU at n = 32, one at n = 64, where a
    // wave alone issues an instruction every 8.4 cycles.  The two operations are simply done again where the value is used.)
    extern __shared__ float lds_var[];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = cam.n;
    float *dirs = lds_var + tid;          // component j at [j * 256]
    float *camrow = lds_var + (size_t)n * 256;
    uint32_t *s_code = reinterpret_cast<uint32_t *>(camrow + 4 * n);
    {
        const float *src = cam.buf ? cam.buf + (size_t)blockIdx.z * 4 * n : nullptr;
        for (int k = tid; k < 4 * n; k += 256) camrow[k] = src ? src[k] : cam.inl[k];
    }
    __syncthreads();
    const float *org = camrow, *right = camrow + n, *up = camrow + 2 * n, *fwd = camrow + 3 * n;
    const int tile_row0 = (int)blockIdx.y * 4 * R;
    if (wv == (int)((blockIdx.x + blockIdx.y + blockIdx.z) & 3u)) {
        uint32_t code = 0u;
        const int trow = tile_row0 + lane;
        if (lane < 4 * R && trow < tg.row_count) {
            const int orow = tg.row_begin + trow;
            const int y = nt_image_row(tg, orow);
            if (y < tg.height) code = box_stretch_code_var(n, camrow, tg, y, (int)blockIdx.x);
        }
        uint32_t packed = code << (4 * (lane & 7));
        packed |= (uint32_t)__shfl_xor((int)packed, 1, 64);
        packed |= (uint32_t)__shfl_xor((int)packed, 2, 64);
        packed |= (uint32_t)__shfl_xor((int)packed, 4, 64);
        if ((lane & 7) == 0 && lane < 4 * R) s_code[lane >> 3] = packed;          // wave w's eight rows: s_code[w]
    }
    __syncthreads();
    const int row0 = tile_row0 + wv * R;
    if (row0 >= tg.row_count) return;
    const uint32_t rowcodes = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_code[wv]);
    // row bookkeeping: one row per lane, read back with v_readlane (see box_tile_kernel)
    const int lorow = tg.row_begin + row0 + lane;
    const int ly = nt_image_row(tg, lorow);
    const uint32_t valid = (uint32_t)__builtin_amdgcn_ballot_w64(lane < R && row0 + lane < tg.row_count && ly < tg.height);
    const float v_sy = tg.fovI * ((float)ly - tg.half_h);
    const long long v_off = (long long)blockIdx.z * tg.frame_stride + (long long)(tg.compact ? lorow : ly) * tg.pitch;
    const int v_off_lo = (int)v_off, v_off_hi = (int)(v_off >> 32);
    int x = (int)blockIdx.x * 64 + lane;
    x = x < tg.width ? x : tg.width - 1;                 // lanes past the right edge redo the last pixel
    const long long xoff = (long long)x * tg.bpp;
    const float sx = tg.fovI * ((float)x - tg.half_w);
    float bb = 0.0f, bu = 0.0f, uu = 0.0f;
    for (int j = 0; j < n; ++j) {
        const float b = fwd[j] + right[j] * sx;
        bb = fmaf(b, b, bb);
        bu = fmaf(b, up[j], bu);
        uu = fmaf(up[j], up[j], uu);
    }
    const float base0 = fwd[0] + right[0] * sx, up0 = up[0];
    const float m2bu = -2.0f * bu;
    // (the quadratic's error grows with n: (3.7n + 4) * 2^-24 relative -- the guard below is sized for it)
    const bool fastsq = __builtin_amdgcn_ballot_w64(!(bu * bu <= bb * uu * 0.0625f)) == 0ull;
    const float guard = (5.55f * (float)n + 21.0f) * 0x1p-24f;         // three times (1.85n + 7) * 2^-24: at every n more than 1.5 times nt_lean_budget_ulps(n) (nt_box.hpp, guard_clear)
    const float maxv = (float)tg.plain_maxval;
    float dots[4];
    if (cam.buf) {
        const float *dp = cam.dots + (size_t)blockIdx.z * 4;
        dots[0] = dp[0]; dots[1] = dp[1]; dots[2] = dp[2]; dots[3] = dp[3];
    } else {
        dots[0] = cam.odots[0]; dots[1] = cam.odots[1]; dots[2] = cam.odots[2]; dots[3] = cam.odots[3];
    }
    for (int rr = 0; rr < R; ++rr) {
        if (!((valid >> rr) & 1u)) continue;
        const uint32_t code = (rowcodes >> (4 * rr)) & 15u;
        const float sy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v_sy), rr));
        PixelRef pr;
        pr.x = x;
        pr.y = 0;
        pr.offset = (((long long)__builtin_amdgcn_readlane(v_off_hi, rr) << 32) | (unsigned)__builtin_amdgcn_readlane(v_off_lo, rr)) + xoff;
        pr.hit_index = 0;
        pr.valid = true;
        if (fastsq && code <= 13u) {
            // background (code 0) or face K = code - 1 throughout: |x| / |dir| from x = dir[0] or dir[K] alone
            const int K = code == 0u ? 0 : (int)code - 1;
            const float xk = (code == 0u ? base0 : fwd[K] + right[K] * sx) - (code == 0u ? up0 : up[K]) * sy;       // dir[K], bit for bit
            const float sqa = fmaf(sy, fmaf(sy, uu, m2bu), bb);
            const float t = (fabsf(xk) * __builtin_amdgcn_rsqf(sqa)) * maxv, th = t * 0.5f;
            const bool clear = fabsf(__builtin_amdgcn_fractf(t) - 0.5f) > fmaf(t, guard, guard) &&
                               (code == 0u || fabsf(__builtin_amdgcn_fractf(th) - 0.5f) > fmaf(th, guard, guard));
            if (__builtin_amdgcn_ballot_w64(!clear) == 0ull) {
                uint32_t q = (uint32_t)(t + 0.5f), qh = (uint32_t)(th + 0.5f);
                q = q < tg.plain_maxval ? q : tg.plain_maxval;
                qh = qh < tg.plain_maxval ? qh : tg.plain_maxval;
                if (code == 0u) emit_plain(tg, pr, xk > 0.0f ? q : 0u, q);
                else emit_plain(tg, pr, q, qh);
                continue;
            }
        }
        // ---- ray by ray: box_kernel_var's evaluation (the reference's arithmetic on the faces in a near-tie with the
        // last-reached one), with the direction in `dirs`
        float sq = 0.0f;
        for (int j = 0; j < n; ++j) {
            const float v = (fwd[j] + right[j] * sx) - up[j] * sy;
            dirs[j * 256] = v;
            sq = j == 0 ? v * v : sq + v * v;
        }
        const float len = sqrtf(sq);
        const float osq = dots[0];
        const float ov = fmaf(-dots[2], sy, fmaf(dots[1], sx, dots[3]));
        const float rad2 = (float)n * (1.0f + NT_FUZZ) * (1.0f + NT_FUZZ) * 1.001f;
        const bool maybe = code != 0u && !((osq - rad2 * 1.0001f - 1e-5f * osq) * sq > ov * ov * 1.0001f);
        const bool wave_maybe = __builtin_amdgcn_ballot_w64(maybe) != 0ull;
        bool done = false;
        float shade = 0.0f;
        if (wave_maybe) {
            for (int j = 0; j < n; ++j) dirs[j * 256] = dirs[j * 256] / len;
            float aK = 0.0f, bK = 1.0f, oK = 0.0f;
            bool any = false;
            for (int i = 0; i < n; ++i) {
                const float di = dirs[i * 256];
                const float oi = org[i];
                const float num = (di < 0.0f ? 1.0f : -1.0f) - oi;
                const bool pre = maybe && ((num > 0.0f && di > 0.0f) || (num < 0.0f && di < 0.0f));
                const float a = fabsf(num), bq = fabsf(di);
                if (pre && (!any || a * bK > aK * bq)) { aK = a; bK = bq; oK = oi; any = true; }
            }
            const float mu = 1e-4f * (1.0f + fabsf(oK));
            const float aKm = (aK - mu) * (1.0f - 1e-6f);
            for (int i = 0; i < n; ++i) {
                const float di = dirs[i * 256];
                const float oi = org[i];
                const float s_ = di < 0.0f ? 1.0f : -1.0f;
                const float num = s_ - oi;
                const bool pre = maybe && ((num > 0.0f && di > 0.0f) || (num < 0.0f && di < 0.0f));
                const bool tie = pre && !done && !(fabsf(num) * bK < fabsf(di) * aKm);
                if (__builtin_amdgcn_ballot_w64(tie) == 0ull) continue;
                const float dist = num / di;
                bool ok = tie && dist > 0.0f;
                for (int j = 0; j < n; ++j) {
                    if (j != i) {
                        const float pj = dirs[j * 256] * dist + org[j];
                        ok = ok && !(fabsf(pj) > (1.0f + NT_FUZZ));
                    }
                }
                if (ok) {
                    done = true;
                    if (dist >= FLT_MAX) shade = -1.0f;
                    else {
                        const float sine = di * s_;
                        shade = sine <= 0.0f ? -sine : 0.0f;
                    }
                }
            }
        } else {
            dirs[0] = dirs[0] / len;
        }
        float r, g, b;
        if (done && shade >= 0.0f) {
            r = shade * 1.0f;
            g = shade * 0.5f;
            b = shade * 0.5f;
        } else {
            const float in = dirs[0];
            if (in > 0.0f) { r = in; g = in; b = in; }
            else { r = 0.0f; g = -in; b = -in; }
        }
        (void)b;
        emit_plain(tg, pr, plain_quantize(tg, r), plain_quantize(tg, g));            // g == b
    }
}

// --------------------------------------------------------------------------------------
// CompositeScene, run-time n (up to 64): the reference's generic `tracern` module (var_geometry.hpp).  Per-lane
// kernel, the whole of composite_scene::calculate_color for opaque scenes: batches, unbatched triangles, Solids,
// point / global / camera lights, shadow rays (with _occludes' far-child rule), reflection.  The current ray's n-vectors
// (origin, 1/direction, direction, a scratch vector) live in LDS as [k][lane] -- every record component is applied to all
// of them in turn -- while the vectors shading needs once per hit (normal ray, light vector, the saved view direction,
// a Solid's local ray) sit in per-lane scratch memory.  Simplex and solid records are read component by component.
// Operation order is the oracle's, so results equal the compile-time-N kernels' where both exist (NTRACER_FORCE_VAR=1).
// Transparent materials, and the reference's o_hit.normal handling for scenes with Solids: composite_kernel_var_t below.
// --------------------------------------------------------------------------------------
struct VarLds {
    float2 *ray;     // [n][64] (origin, 1/direction; NaN marks direction == 0)
    float *dv;       // [n][64] direction
    float *ps;       // [n][64] scratch: pside
    int *stack;      // [depth][64]
    int *mbox;       // [NT_MBOX][64]
};

// The dynamic LDS of every walk kernel below, one wave a block: what var_lds_carve lays out, so the host sizes a launch by the
// expression the kernels carve by -- ray 8 n, dv 4 n, ps 4 n, stack 4 depth and mbox 4 NT_MBOX bytes a lane
__host__ __device__ __forceinline__ size_t var_lds_bytes(int depth, int n) {
    return (size_t)64 * ((size_t)n * 16 + (size_t)depth * 4 + (size_t)NT_MBOX * 4);
}
__device__ __forceinline__ void var_lds_carve(char *p, int n, int depth, VarLds &L, WaveLds &w) {
    L.ray = reinterpret_cast<float2 *>(p);
    L.dv = reinterpret_cast<float *>(p + (size_t)64 * n * 8);
    L.ps = L.dv + (size_t)64 * n;
    L.stack = reinterpret_cast<int *>(L.ps + (size_t)64 * n);
    L.mbox = L.stack + (size_t)64 * depth;
    w.ray = L.ray;
    w.stack = L.stack;
    w.mbox = L.mbox;
}

struct VarCtx {
    const NtCompositeDev &sc;
    VarLds L;
    WaveLds w;
    int n, lane;
};
// What the CLIP instantiations of the walks below are handed as their VarCtx (the four kernels nt_launch_clip launches make one):
// the planes and this lane's window travel behind the context, so no walk's signature changes and the instantiations without
// CLIP -- every call from before the setting -- are the parent commit's code
struct VarCtxClip : VarCtx {
    const float *clip;       // clip planes [clip_count][n + 1] (NtClipPlanes)
    int clip_count;
    float *cwin;             // this lane's {t0, t1} of the current ray (clip_window_var) and the candidates rejected of the item at hand
};

#define VO(k) (cx.L.ray[(k) * 64 + cx.lane].x)       // origin[k] of the current ray
#define VD(k) (cx.L.dv[(k) * 64 + cx.lane])          // direction[k]

// make (o, d) the current ray: origin, direction and invdir = 1/direction (tracer.hpp:1174)
__device__ __forceinline__ void var_set_ray(const VarCtx &cx, const float *o, const float *d) {
    for (int k = 0; k < cx.n; ++k) {
        const float dk = d[k];
        cx.L.dv[k * 64 + cx.lane] = dk;
        cx.L.ray[k * 64 + cx.lane] = make_float2(o[k], dk != 0.0f ? 1.0f / dk : __int_as_float(0x7fc00000));
    }
}

// Clip planes at run-time n (cx.clip, cx.clip_count; the rule in full: ntracer_hip.h, and clip_window in nt_composite.hpp): the
// window [t0, t1] of the current ray into cx.cwin, an empty one as t0 > t1.  Every walk forms it when it starts, so whatever
// made its ray the current one need not know of the setting.
__device__ __forceinline__ void clip_window_var(const VarCtx &cx_) {
    const VarCtxClip &cx = static_cast<const VarCtxClip &>(cx_);
    const int n = cx.n;
    float t0 = 0.0f, t1 = FLT_MAX;
    bool empty = false;
    for (int k = 0; k < cx.clip_count; ++k) {
        const float *a = cx.clip + (size_t)k * (n + 1);
        float p = 0.0f, r = 0.0f;
        for (int j = 0; j < n; ++j) {
            const float po = a[j] * VO(j), pd = a[j] * VD(j);
            p = j == 0 ? po : p + po;
            r = j == 0 ? pd : r + pd;
        }
        const float s = p - a[n];
        if (r > 0.0f) {
            const float q = (-s) / r;
            if (q < t1) t1 = q;
        } else if (r < 0.0f) {
            const float q = (-s) / r;
            if (q > t0) t0 = q;
        } else if (r == 0.0f && s > 0.0f) {
            empty = true;
        }
    }
    empty = empty || t0 > t1;
    cx.cwin[0] = empty ? 1.0f : t0;
    cx.cwin[1] = empty ? 0.0f : t1;
    cx.cwin[2] = 0.0f;
}

// a candidate t of the current ray under the planes: t itself, or 0 -- "no hit", as if the primitive had not been tested --
// outside the ray's window (cwin[2] counts the rejections; leaf_closest_var_t, its one reader, clears it before every item)
template <bool CLIP>
__device__ __forceinline__ float clip_keep_var(const VarCtx &cx_, float t) {
    if constexpr (CLIP) {
        const VarCtxClip &cx = static_cast<const VarCtxClip &>(cx_);
        if (t != 0.0f && !(t >= cx.cwin[0] && t <= cx.cwin[1])) {
            cx.cwin[2] += 1.0f;
            return 0.0f;
        }
    }
    return t;
}

// The root interval of a primary walk under the planes: from max(aabb entry, t0) to t1.  false: the window is empty.
__device__ __forceinline__ bool clip_primary_var(const VarCtx &cx_, float &t_near, RootWindow &root) {
    const VarCtxClip &cx = static_cast<const VarCtxClip &>(cx_);
    clip_window_var(cx);
    if (!(cx.cwin[0] <= cx.cwin[1])) return false;
    if (cx.cwin[0] > t_near) t_near = cx.cwin[0];
    root.tn = 0.0f;
    root.tf = cx.cwin[1];
    return true;
}

// triangle_batch::intersects lane / triangle::intersects with run-time n (tracer.hpp:411-440, 561-581)
__device__ __forceinline__ float simplex_var(const float *__restrict__ rec, int n, const VarLds &L, int lane, bool scalar_form, float cutoff) {
    float denom = 0.0f, no = 0.0f;
    for (int k = 0; k < n; ++k) {
        const float fn = rec[1 + k];
        const float pd = fn * L.dv[k * 64 + lane];
        const float po = fn * L.ray[k * 64 + lane].x;
        denom = k == 0 ? pd : denom + pd;
        no = k == 0 ? po : no + po;
    }
    if (scalar_form && denom == 0.0f) return 0.0f;
    const float t = -(no + rec[0]) / denom;
    if (scalar_form && (t <= 0.0f || t >= cutoff)) return 0.0f;
    bool ok = scalar_form ? true : (denom != 0.0f && t >= 0.0f);
    for (int k = 0; k < n; ++k) L.ps[k * 64 + lane] = rec[1 + n + k] - (L.ray[k * 64 + lane].x + t * L.dv[k * 64 + lane]);
    float tot = 0.0f;
    for (int e = 0; e < n - 1; ++e) {
        const float *en = rec + 1 + 2 * n + (size_t)e * n;
        float area = 0.0f;
        for (int k = 0; k < n; ++k) {
            const float p = en[k] * L.ps[k * 64 + lane];
            area = k == 0 ? p : area + p;
        }
        if (scalar_form) ok = ok && !(area < -NT_FUZZ || area > (1.0f + NT_FUZZ));
        else ok = ok && area >= -NT_FUZZ;
        tot += area;
    }
    ok = ok && tot <= (1.0f + NT_FUZZ);
    return ok ? t : 0.0f;
}

// solid::intersects (tracer.hpp:251-276) on the current ray, hypercube_intersects / hypersphere_intersects (:126-173) on
// the local ray.  want_normal: (no, nd) receive the world-space normal ray.
__device__ __noinline__ float solid_var(const VarCtx &cx, int idx, float cutoff, bool want_normal, float *no, float *nd) {
    const int n = cx.n;
    const float *orient = cx.sc.solid_recs + (size_t)idx * (2 * n * n + n);
    const float *inv = orient + n * n;
    const float *pos = inv + n * n;
    float lo[NT_DEV_MAX_DIM], ld[NT_DEV_MAX_DIM], ln_o[NT_DEV_MAX_DIM], ln_d[NT_DEV_MAX_DIM];
    for (int i = 0; i < n; ++i) {
        float so = 0.0f, sd = 0.0f;
        for (int k = 0; k < n; ++k) {
            const float m = inv[i * n + k];
            const float po = m * VO(k), pd = m * VD(k);
            so = k == 0 ? po : so + po;
            sd = k == 0 ? pd : sd + pd;
        }
        lo[i] = so - pos[i];
        ld[i] = sd;
    }
    float dist = 0.0f;
    if (cx.sc.solid_types[idx] == 1) {
        for (int i = 0; i < n; ++i) {
            const float di = ld[i];
            if (di == 0.0f) continue;
            const float s = di < 0.0f ? 1.0f : -1.0f;
            const float t = (s - lo[i]) / di;
            if (!(t > 0.0f)) continue;
            bool ok = true;
            for (int j = 0; j < n; ++j) {
                if (j != i) {
                    const float p = ld[j] * t + lo[j];
                    ln_o[j] = p;
                    if (fabsf(p) > (1.0f + NT_FUZZ)) { ok = false; break; }
                }
            }
            if (!ok) continue;
            if (t >= cutoff) return 0.0f;
            dist = t;
            ln_o[i] = s;
            for (int j = 0; j < n; ++j) ln_d[j] = j == i ? s : 0.0f;
            break;
        }
    } else {
        float a = 0.0f, b = 0.0f, c = 0.0f;
        for (int k = 0; k < n; ++k) {
            const float pa = ld[k] * ld[k], pb = ld[k] * lo[k], pc = lo[k] * lo[k];
            a = k == 0 ? pa : a + pa;
            b = k == 0 ? pb : b + pb;
            c = k == 0 ? pc : c + pc;
        }
        b = 2.0f * b;
        c = c - 1.0f;
        const float disc = b * b - 4.0f * a * c;
        if (disc < 0.0f) return 0.0f;
        const float t = (-b - sqrtf(disc)) / (2.0f * a);
        if (t <= 0.0f || t >= cutoff) return 0.0f;
        dist = t;
        for (int j = 0; j < n; ++j) { ln_o[j] = lo[j] + ld[j] * t; ln_d[j] = ln_o[j]; }
    }
    if (dist == 0.0f) return 0.0f;
    if (want_normal) {
        for (int i = 0; i < n; ++i) ln_o[i] = ln_o[i] + pos[i];
        for (int i = 0; i < n; ++i) {
            float so = 0.0f, sd = 0.0f;
            for (int k = 0; k < n; ++k) {
                const float m = orient[i * n + k];
                const float po = m * ln_o[k], pd = m * ln_d[k];
                so = k == 0 ? po : so + po;
                sd = k == 0 ? pd : sd + pd;
            }
            no[i] = so;
            nd[i] = sd;
        }
    }
    return dist;
}

// composite_scene::aabb_distance (tracer.hpp:1892-1918) for the current ray
__device__ __forceinline__ float aabb_distance_var(const VarCtx &cx) {
    const int n = cx.n;
    const float *aabb = cx.sc.aabb;
    for (int i = 0; i < n; ++i) {
        const float di = VD(i);
        if (di == 0.0f) continue;
        const float face = di > 0.0f ? aabb[i] : aabb[n + i];
        float dist = (face - VO(i)) / di;
        int skip = i;
        if (dist < 0.0f) { dist = 0.0f; skip = -1; }
        bool ok = true;
        for (int j = 0; j < n; ++j) {
            if (j != skip) {
                const float p = VD(j) * dist + VO(j);
                if (p >= aabb[n + j] || p <= aabb[j]) { ok = false; break; }
            }
        }
        if (ok) return dist;
    }
    return -1.0f;
}

// kd_leaf<Store,true>::intersects for all-opaque scenes (see leaf_closest in nt_composite.hpp)
template <bool CLIP = false>
__device__ __forceinline__ bool leaf_closest_var(const VarCtx &cx, int start, int count, int skip_item, int skip_lane, Hit &hit) {
    const NtCompositeDev &sc = cx.sc;
    bool improved = false;
    for (int i = 0; i < count; ++i) {
        const int item = sc.items[start + i];
        const int kind = item & 3, idx = item >> 2;
        if (mbox_seen(cx.w, cx.lane, item)) continue;
        if (kind == 0) {
            const int sl = item == skip_item ? skip_lane : -1;
            float min_t = hit.dist;
            int r = -1;
            for (int l = 0; l < NT_DEV_BATCH; ++l) {
                const float t = clip_keep_var<CLIP>(cx, simplex_var(sc.batch_recs + ((size_t)idx * NT_DEV_BATCH + l) * sc.rec_stride, cx.n, cx.L, cx.lane, false, 0.0f));
                if (l != sl && t != 0.0f && t < min_t) { min_t = t; r = l; }
            }
            if (r >= 0) { hit.dist = min_t; hit.item = item; hit.lane = r; improved = true; }
        } else if (item != skip_item) {
            float t;
            if (kind == 1) t = simplex_var(sc.tri_recs + (size_t)idx * sc.rec_stride, cx.n, cx.L, cx.lane, true, hit.dist);
            else t = solid_var(cx, idx, hit.dist, false, nullptr, nullptr);
            t = clip_keep_var<CLIP>(cx, t);
            if (t != 0.0f) { hit.dist = t; hit.item = item; hit.lane = -1; improved = true; }
        }
    }
    return improved;
}

// kd_node_intersection::operator() (tracer.hpp:1179-1243): the continuation stack of kd_descend / kd_resume_closest (nt_composite.hpp)
template <typename ROOT = RootWhole, bool CLIP = false>
__device__ __noinline__ bool trace_closest_var(const VarCtx &cx, float t_near, int skip_item, int skip_lane, Hit &hit, const ROOT root = ROOT()) {
    const NtCompositeDev &sc = cx.sc;
    const WaveLds &w = cx.w;
    const int lane = cx.lane;
    hit.dist = FLT_MAX;
    hit.item = -1;
    hit.lane = -1;
    mbox_reset(w, lane);
    if constexpr (CLIP) clip_window_var(cx);
    int node = sc.root, sp = 0, dirty = 0;
    float t_far = root.t_far();
    const int max_sp = sc.stack_depth;
    for (;;) {
        while (node >= 0) {
            if (sc.prune && nt_beyond_hit(hit.dist, t_near)) { node = -1; break; }
            const NtNode nd = sc.nodes[node];
            if (nd.axis < 0) {
                if (leaf_closest_var<CLIP>(cx, nd.left, nd.right, skip_item, skip_lane, hit)) dirty = sp;
                node = -1;
                break;
            }
            const KdStep s = kd_descend(w, lane, nd, node, sp, max_sp, t_near, t_far, 0u);
            if (s.crossed) t_near = s.t;
        }
        if (!kd_resume_closest(sc, w, lane, node, sp, dirty, hit.dist, t_near)) break;
        t_far = kd_t_far_below(sc, w, lane, sp, root.t_far());
    }
    return hit.item >= 0;
}

// kd_leaf::occludes (tracer.hpp:1088-1124), all-opaque scenes
template <bool CLIP = false>
__device__ __forceinline__ bool leaf_occludes_var(const VarCtx &cx, int start, int count, float ldistance, int skip_item, int skip_lane) {
    const NtCompositeDev &sc = cx.sc;
    for (int i = 0; i < count; ++i) {
        const int item = sc.items[start + i];
        const int kind = item & 3, idx = item >> 2;
        if (kind == 0) {
            const int sl = item == skip_item ? skip_lane : -1;
            bool any = false;
            for (int l = 0; l < NT_DEV_BATCH; ++l) {
                const float t = clip_keep_var<CLIP>(cx, simplex_var(sc.batch_recs + ((size_t)idx * NT_DEV_BATCH + l) * sc.rec_stride, cx.n, cx.L, cx.lane, false, 0.0f));
                any = any || (l != sl && t != 0.0f && t < ldistance);
            }
            if (any) return true;
        } else if (item != skip_item) {
            float t;
            if (kind == 1) t = simplex_var(sc.tri_recs + (size_t)idx * sc.rec_stride, cx.n, cx.L, cx.lane, true, ldistance);
            else t = solid_var(cx, idx, ldistance, false, nullptr, nullptr);
            if (clip_keep_var<CLIP>(cx, t) != 0.0f) return true;
        }
    }
    return false;
}

// _occludes (tracer.hpp:1258-1307) for the current ray on kd_descend / kd_resume_occluded (nt_composite.hpp),
// `if(t < ldistance) return false;` (:1298) included
template <typename ROOT = RootWhole, bool CLIP = false>
__device__ __noinline__ bool trace_occluded_var(const VarCtx &cx, float ldistance, int skip_item, int skip_lane, const ROOT root = ROOT()) {
    const NtCompositeDev &sc = cx.sc;
    const WaveLds &w = cx.w;
    const int lane = cx.lane;
    if constexpr (CLIP) clip_window_var(cx);
    int node = sc.root, sp = 0;
    float t_near = root.t_near(), t_far = root.t_far();
    const int max_sp = sc.stack_depth;
    for (;;) {
        while (node >= 0) {
            const NtNode nd = sc.nodes[node];
            if (nd.axis < 0) {
                if (leaf_occludes_var<CLIP>(cx, nd.left, nd.right, ldistance, skip_item, skip_lane)) return true;
                node = -1;
                break;
            }
            const KdStep s = kd_descend(w, lane, nd, node, sp, max_sp, t_near, t_far, 0u);
            if (s.crossed) {
                if (s.t < ldistance) { node = -1; break; }
                t_near = s.t;
            }
        }
        if (!kd_resume_occluded(sc, w, lane, node, sp, ldistance, t_near)) return false;
        t_far = kd_t_far_below(sc, w, lane, sp, root.t_far());
    }
}

__device__ __forceinline__ float dot_var(int n, const float *a, const float *b) {
    float s = 0.0f;
    for (int k = 0; k < n; ++k) {
        const float p = a[k] * b[k];
        s = k == 0 ? p : s + p;
    }
    return s;
}

// append_specular (tracer.hpp:1701-1707)
__device__ __forceinline__ void append_specular_var(int n, Color3 &c, float &a, const float *m, Color3 light_c, const float *target, const float *normal,
                                                    const float *light_dir) {
    float tmp[NT_DEV_MAX_DIM];
    for (int k = 0; k < n; ++k) tmp[k] = light_dir[k] - target[k];
    const float len = sqrtf(dot_var(n, tmp, tmp));
    for (int k = 0; k < n; ++k) tmp[k] = tmp[k] / len;
    const float base = powf(dot_var(n, normal, tmp), m[9]) * m[8];
    c = cadd(c, cscale(cscale(cmul(c3p(m + 3), light_c), base), (1.0f - a)));
    a += base * (1.0f - a);
    c = cscale(c, a);
}

// ray_color + base_color (tracer.hpp:1768-1883), the reflection recursion as a level stack (see composite_color).
// On entry the primary ray is the current ray.
template <bool CLIP = false>
__device__ __noinline__ Color3 composite_color_var(const VarCtx &cx) {
    const NtCompositeDev &sc = cx.sc;
    const int n = cx.n;
    Level levels[NT_DEV_MAX_REFLECT];
    Color3 deep_a = c3(0.0f, 0.0f, 0.0f), deep_b = c3(1.0f, 1.0f, 1.0f);
    int depth = 0;
    int skip_item = -1, skip_lane = -1;
    Color3 result;
    float dir[NT_DEV_MAX_DIM], no[NT_DEV_MAX_DIM], nd[NT_DEV_MAX_DIM], lv[NT_DEV_MAX_DIM];
    for (;;) {
        // ---- ray_color (tracer.hpp:1856-1883)
        Hit hit;
        hit.dist = FLT_MAX; hit.item = -1; hit.lane = -1;
        bool found = false;
        const float dist0 = aabb_distance_var(cx);
        if (dist0 >= 0.0f) {
            if constexpr (CLIP) {
                if (depth == 0) {
                    // the primary ray under clip planes: the walk starts at max(aabb entry, t0) and ends at t1
                    float tn = dist0;
                    RootWindow root;
                    if (clip_primary_var(cx, tn, root)) found = trace_closest_var<RootWindow, true>(cx, tn, skip_item, skip_lane, hit, root);
                } else {
                    found = trace_closest_var<RootWhole, true>(cx, dist0, skip_item, skip_lane, hit);
                }
            } else {
                found = trace_closest_var(cx, dist0, skip_item, skip_lane, hit);
            }
        }
        if (!found) {
            const float iv = VD(sc.bg_axis);
            result = iv >= 0.0f ? cadd(cscale(c3p(sc.bg1), iv), cscale(c3p(sc.bg2), 1.0f - iv))
                                : cadd(cscale(c3p(sc.bg3), -iv), cscale(c3p(sc.bg2), 1.0f + iv));
            break;
        }
        // ---- the hit's normal ray (what the reference's tests stored in o_hit.normal)
        const int kind = hit.item & 3, idx = hit.item >> 2;
        for (int k = 0; k < n; ++k) dir[k] = VD(k);
        if (kind != 2) {
            const float *rec = kind == 0 ? sc.batch_recs + ((size_t)idx * NT_DEV_BATCH + hit.lane) * sc.rec_stride
                                         : sc.tri_recs + (size_t)idx * sc.rec_stride;
            float denom = 0.0f, fsq = 0.0f;
            for (int k = 0; k < n; ++k) {
                const float fn = rec[1 + k];
                const float pd = fn * dir[k];
                denom = k == 0 ? pd : denom + pd;
                fsq = k == 0 ? fn * fn : fsq + fn * fn;
            }
            const float flen = sqrtf(fsq);
            for (int k = 0; k < n; ++k) {
                no[k] = VO(k) + hit.dist * dir[k];
                const float u = rec[1 + k] / flen;
                nd[k] = denom > 0.0f ? -u : u;
            }
        } else {
            solid_var(cx, idx, FLT_MAX, true, no, nd);
        }
        // ---- base_color (tracer.hpp:1768-1854)
        const float *m = material_of(sc, hit.item, hit.lane);
        Color3 light = c3(0.0f, 0.0f, 0.0f), specular = c3(0.0f, 0.0f, 0.0f);
        float spec_a = 0.0f;
        for (int li = 0; li < sc.n_point_lights; ++li) {
            const float *pos = sc.pl_pos + (size_t)li * n;
            const Color3 plc = c3p(sc.pl_color + 3 * li);
            for (int k = 0; k < n; ++k) lv[k] = no[k] - pos[k];
            const float ldist = sqrtf(dot_var(n, lv, lv));
            for (int k = 0; k < n; ++k) lv[k] = lv[k] / ldist;
            const float sine = dot_var(n, nd, lv);
            if (sine > 0.0f) {
                const float strength = nt_falloff(ldist, n - 1);
                if (sc.shadows) {
                    if (fmaxf(plc.r, fmaxf(plc.g, plc.b)) * strength * sine > NT_LIGHT_THRESHOLD) {
                        var_set_ray(cx, no, lv);
                        if (!trace_occluded_var<RootWhole, CLIP>(cx, ldist, hit.item, hit.lane)) {
                            const Color3 filtered = cscale(plc, strength);
                            light = cadd(light, cscale(filtered, sine));
                            if (m[8] != 0.0f) append_specular_var(n, specular, spec_a, m, filtered, dir, nd, lv);
                        }
                    }
                } else {
                    light = cadd(light, cscale(cscale(plc, strength), sine));
                }
            }
        }
        for (int li = 0; li < sc.n_global_lights; ++li) {
            const float *gd = sc.gl_dir + (size_t)li * n;
            const Color3 glc = c3p(sc.gl_color + 3 * li);
            const float sine = -dot_var(n, nd, gd);
            if (sine > 0.0f) {
                if (sc.shadows) {
                    for (int k = 0; k < n; ++k) lv[k] = -gd[k];
                    var_set_ray(cx, no, lv);
                    if (!trace_occluded_var<RootWhole, CLIP>(cx, FLT_MAX, hit.item, hit.lane)) {
                        light = cadd(light, cscale(glc, sine));
                        if (m[8] != 0.0f) append_specular_var(n, specular, spec_a, m, glc, dir, nd, lv);
                    }
                } else {
                    light = cadd(light, cscale(glc, sine));
                }
            }
        }
        const float sine = -dot_var(n, dir, nd);
        if (sc.camera_light && sine > 0.0f) {
            light = cadd(light, c3(sine, sine, sine));
            if (m[8] != 0.0f) {
                const float base = powf(sine, m[9]) * m[8];
                specular = cadd(specular, cscale(cscale(c3p(m + 3), base), (1.0f - spec_a)));
                spec_a += base * (1.0f - spec_a);
                specular = cscale(specular, spec_a);
            }
        }
        const Color3 r0 = cadd(c3p(sc.ambient), cmul(c3p(m), light));
        if (m[7] != 0.0f && depth < sc.max_reflect_depth) {
            if (depth < NT_DEV_MAX_REFLECT) {
                Level &Lv = levels[depth];
                Lv.spec = specular;
                Lv.spec_a = spec_a;
                Lv.r0 = r0;
                Lv.c = c3p(m);
                Lv.refl = m[7];
            } else {                        // beyond the level stack: folded into a running affine pair (see composite_color)
                const float k1 = 1.0f - spec_a;
                const Color3 alpha = cadd(specular, cscale(cscale(r0, 1.0f - m[7]), k1));
                const Color3 beta = cscale(cscale(c3p(m), m[7]), k1);
                deep_a = cadd(deep_a, cmul(deep_b, alpha));
                deep_b = cmul(deep_b, beta);
            }
            const float f = -2.0f * sine;
            for (int k = 0; k < n; ++k) dir[k] = dir[k] - nd[k] * f;
            var_set_ray(cx, no, dir);
            skip_item = hit.item;
            skip_lane = hit.lane;
            ++depth;
            continue;
        }
        result = cadd(specular, cscale(r0, 1.0f - spec_a));
        break;
    }
    if (depth > NT_DEV_MAX_REFLECT) {
        result = cadd(deep_a, cmul(deep_b, result));
        depth = NT_DEV_MAX_REFLECT;
    }
    while (depth > 0) {
        --depth;
        const Level &Lv = levels[depth];
        const Color3 r = cadd(cscale(cmul(Lv.c, result), Lv.refl), cscale(Lv.r0, 1.0f - Lv.refl));
        result = cadd(Lv.spec, cscale(r, 1.0f - Lv.spec_a));
    }
    return result;
}

// --------------------------------------------------------------------------------------
// Transparent materials, and the reference's o_hit.normal handling, at run-time n: composite_kernel_t (nt_composite.hpp)
// restated with the current ray in LDS.  The ray_color frames -- one per reflection level, each with its ray, the walk's
// normal ray and its surface list -- live in global scratch, [frame][word][lane slot], sized by the host for
// max_reflect_depth + 1 levels: no depth limit here, which is why scenes with transparency whose depth is beyond the
// compile-time-N kernel's frame stack are sent here as well, whatever their n.
// --------------------------------------------------------------------------------------
struct VarFrames {
    float *base;             // this lane's column
    long long stride;        // lane slots
    int fw;                  // words per frame
};
// frame words: o[n] d[n] hn_o[n] hn_d[n], then the scalars below, then (NT_TH_MAX + 1) surfaces of 3 words
enum { VF_DEPTH = 0, VF_SKIP_ITEM, VF_SKIP_LANE, VF_NSURF, VF_J, VF_R, VF_SPEC = VF_R + 3, VF_R0 = VF_SPEC + 3, VF_C = VF_R0 + 3,
       VF_SPEC_A = VF_C + 3, VF_REFL, VF_SURF, VF_WORDS = VF_SURF + 3 * (NT_TH_MAX + 1) };
__host__ __device__ __forceinline__ int var_frame_words(int n) { return 4 * n + VF_WORDS; }

// the frame stack of lane slot `slot` of the launch's scratch (filled in place: returned by value, the kernels' code changes)
__device__ __forceinline__ void var_frames(VarFrames &fr, const NtCompositeDev &sc, long long slot, int n) {
    fr.base = sc.tframes + slot;
    fr.stride = sc.checked_lanes;
    fr.fw = var_frame_words(n);
}

#define FRW(f, w) (fr.base[((long long)(f) * fr.fw + (w)) * fr.stride])
#define FRI(f, w) (reinterpret_cast<int *>(fr.base)[((long long)(f) * fr.fw + (w)) * fr.stride])

__device__ __forceinline__ Color3 fr_get3(const VarFrames &fr, int f, int w) { return c3(FRW(f, w), FRW(f, w + 1), FRW(f, w + 2)); }
__device__ __forceinline__ void fr_put3(const VarFrames &fr, int f, int w, Color3 c) { FRW(f, w) = c.r; FRW(f, w + 1) = c.g; FRW(f, w + 2) = c.b; }

// test_item (nt_composite.hpp) on the current ray
template <bool CLIP = false>
__device__ __forceinline__ float test_item_var(const VarCtx &cx, int item, float cutoff, int skip_item, int skip_lane, int &lane_out) {
    const NtCompositeDev &sc = cx.sc;
    const int kind = item & 3, idx = item >> 2;
    lane_out = -1;
    if (kind == 0) {
        const int sl = item == skip_item ? skip_lane : -1;
        float min_t = cutoff;
        int r = -1;
        for (int l = 0; l < NT_DEV_BATCH; ++l) {
            const float t = clip_keep_var<CLIP>(cx, simplex_var(sc.batch_recs + ((size_t)idx * NT_DEV_BATCH + l) * sc.rec_stride, cx.n, cx.L, cx.lane, false, 0.0f));
            if (l != sl && t != 0.0f && t < min_t) { min_t = t; r = l; }
        }
        lane_out = r;
        return r >= 0 ? min_t : 0.0f;
    }
    if (kind == 1) return clip_keep_var<CLIP>(cx, simplex_var(sc.tri_recs + (size_t)idx * sc.rec_stride, cx.n, cx.L, cx.lane, true, cutoff));
    return clip_keep_var<CLIP>(cx, solid_var(cx, idx, cutoff, false, nullptr, nullptr));
}

// the normal ray of a hit on the current ray (hit_normal in nt_composite.hpp)
__device__ __forceinline__ void hit_normal_var(const VarCtx &cx, const Hit &hit, float *no, float *nd) {
    const NtCompositeDev &sc = cx.sc;
    const int n = cx.n;
    const int kind = hit.item & 3, idx = hit.item >> 2;
    if (kind == 2) {
        solid_var(cx, idx, FLT_MAX, true, no, nd);
        return;
    }
    const float *rec = kind == 0 ? sc.batch_recs + ((size_t)idx * NT_DEV_BATCH + hit.lane) * sc.rec_stride
                                 : sc.tri_recs + (size_t)idx * sc.rec_stride;
    float denom = 0.0f, fsq = 0.0f;
    for (int k = 0; k < n; ++k) {
        const float fn = rec[1 + k];
        const float pd = fn * VD(k);
        denom = k == 0 ? pd : denom + pd;
        fsq = k == 0 ? fn * fn : fsq + fn * fn;
    }
    const float flen = sqrtf(fsq);
    for (int k = 0; k < n; ++k) {
        no[k] = VO(k) + hit.dist * VD(k);
        const float u = rec[1 + k] / flen;
        nd[k] = denom > 0.0f ? -u : u;
    }
}

// solid::intersects writing through to the caller's normal ray as the reference does (solid_intersects_marks /
// cube_local_marks in nt_composite.hpp; tracer.hpp:126-152, 251-276)
__device__ __noinline__ float solid_marks_var(const VarCtx &cx, int idx, float cutoff, float *no, float *nd) {
    const int n = cx.n;
    const float *orient = cx.sc.solid_recs + (size_t)idx * (2 * n * n + n);
    const float *inv = orient + n * n;
    const float *pos = inv + n * n;
    float lo[NT_DEV_MAX_DIM], ld[NT_DEV_MAX_DIM];
    for (int i = 0; i < n; ++i) {
        float so = 0.0f, sd = 0.0f;
        for (int k = 0; k < n; ++k) {
            const float m = inv[i * n + k];
            const float po = m * VO(k), pd = m * VD(k);
            so = k == 0 ? po : so + po;
            sd = k == 0 ? pd : sd + pd;
        }
        lo[i] = so - pos[i];
        ld[i] = sd;
    }
    float dist = 0.0f;
    if (cx.sc.solid_types[idx] == 1) {
        for (int i = 0; i < n; ++i) {
            const float di = ld[i];
            if (di == 0.0f) continue;
            const float s = di < 0.0f ? 1.0f : -1.0f;
            no[i] = s;
            const float t = (s - lo[i]) / di;
            if (!(t > 0.0f)) continue;
            bool ok = true;
            for (int j = 0; j < n; ++j) {
                if (j != i) {
                    const float p = ld[j] * t + lo[j];
                    no[j] = p;
                    if (fabsf(p) > (1.0f + NT_FUZZ)) { ok = false; break; }
                }
            }
            if (!ok) continue;
            if (t >= cutoff) return 0.0f;
            dist = t;
            for (int j = 0; j < n; ++j) nd[j] = j == i ? s : 0.0f;
            break;
        }
    } else {
        float a = 0.0f, b = 0.0f, c = 0.0f;
        for (int k = 0; k < n; ++k) {
            const float pa = ld[k] * ld[k], pb = ld[k] * lo[k], pc = lo[k] * lo[k];
            a = k == 0 ? pa : a + pa;
            b = k == 0 ? pb : b + pb;
            c = k == 0 ? pc : c + pc;
        }
        b = 2.0f * b;
        c = c - 1.0f;
        const float disc = b * b - 4.0f * a * c;
        if (disc < 0.0f) return 0.0f;
        const float t = (-b - sqrtf(disc)) / (2.0f * a);
        if (t <= 0.0f || t >= cutoff) return 0.0f;
        dist = t;
        for (int j = 0; j < n; ++j) { no[j] = lo[j] + ld[j] * t; nd[j] = no[j]; }
    }
    if (dist == 0.0f) return 0.0f;
    // (lo, ld are done with: they hold the local normal ray while it is turned back to world space)
    for (int i = 0; i < n; ++i) { lo[i] = no[i] + pos[i]; ld[i] = nd[i]; }
    for (int i = 0; i < n; ++i) {
        float so = 0.0f, sd = 0.0f;
        for (int k = 0; k < n; ++k) {
            const float m = orient[i * n + k];
            const float po = m * lo[k], pd = m * ld[k];
            so = k == 0 ? po : so + po;
            sd = k == 0 ? pd : sd + pd;
        }
        no[i] = so;
        nd[i] = sd;
    }
    return dist;
}

template <bool CLIP = false>
__device__ __forceinline__ float test_item_marks_var(const VarCtx &cx, int item, float cutoff, int skip_item, int skip_lane, int &lane_out,
                                                     float *no, float *nd) {
    if ((item & 3) == 2) {
        lane_out = -1;
        return solid_marks_var(cx, item >> 2, cutoff, no, nd);
    }
    const float t = test_item_var<CLIP>(cx, item, cutoff, skip_item, skip_lane, lane_out);
    if (t != 0.0f) {
        Hit h;
        h.dist = t;
        h.item = item;
        h.lane = lane_out;
        hit_normal_var(cx, h, no, nd);
    }
    return t;
}

// leaf_closest_t (nt_composite.hpp): kd_leaf<Store,true>::intersects with transparent hits (tracer.hpp:977-1086)
template <bool ALIAS, bool CLIP = false>
__device__ __noinline__ bool leaf_closest_var_t(const VarCtx &cx, int start, int count, int skip_item, int skip_lane, Hit &hit, TList &th,
                                                const Checked &ck, float *hn_o, float *hn_d, float *nn_o, float *nn_d) {
    const NtCompositeDev &sc = cx.sc;
    const int h_start = th.n;
    bool found = false;
    float dist_last = 0.0f;
    for (int i = 0; i < count; ++i) {
        const int item = sc.items[start + i];
        if ((item & 3) != 0 && item == skip_item) continue;
        if (checked_seen(ck, item)) continue;
        int l;
        float t;
        if constexpr (CLIP) static_cast<const VarCtxClip &>(cx).cwin[2] = 0.0f;       // the rejections of THIS item are counted below
        if (ALIAS) {
            if (!found) {
                t = test_item_marks_var<CLIP>(cx, item, hit.dist, skip_item, skip_lane, l, hn_o, hn_d);
            } else {
                t = test_item_marks_var<CLIP>(cx, item, hit.dist, skip_item, skip_lane, l, nn_o, nn_d);
                if (t != 0.0f && material_of(sc, item, l)[6] >= 1.0f) {
                    for (int k = 0; k < cx.n; ++k) { hn_o[k] = nn_o[k]; hn_d[k] = nn_d[k]; }
                }
            }
        } else {
            t = test_item_var<CLIP>(cx, item, hit.dist, skip_item, skip_lane, l);
        }
        if constexpr (CLIP) {
            // An item ALL of whose primitives were cut away -- the one of a triangle, the NT_DEV_BATCH of a batch -- is as if it
            // had not been tested: dist_last stays.  A batch that keeps a primitive has been tested, and a miss of what it keeps
            // is today's miss.
            const float rejected = static_cast<const VarCtxClip &>(cx).cwin[2];
            if (t == 0.0f && rejected >= ((item & 3) == 0 ? (float)NT_DEV_BATCH : 1.0f)) continue;
        }
        dist_last = t;
        if (t != 0.0f) {
            if (material_of(sc, item, l)[6] >= 1.0f) {
                hit.dist = t;
                hit.item = item;
                hit.lane = l;
                if (!found) {
                    found = true;
                    dist_last = 0.0f;
                }
            } else {
                tl_add(th, t, item, l);
            }
        }
    }
    if (found) tl_trim(th, dist_last, h_start);
    return found;
}

// trace_closest_t (nt_composite.hpp) for the current ray, on the same kd_descend / kd_resume_tagged
template <bool ALIAS, typename ROOT = RootWhole, bool CLIP = false>
__device__ __noinline__ bool trace_closest_var_t(const VarCtx &cx, float t_near, int skip_item, int skip_lane, Hit &hit, TList &th,
                                                 const Checked &ck, float *hn_o, float *hn_d, float *nn_o, float *nn_d, const ROOT root = ROOT()) {
    const NtCompositeDev &sc = cx.sc;
    const WaveLds &w = cx.w;
    const int lane = cx.lane;
    hit.dist = FLT_MAX;
    hit.item = -1;
    hit.lane = -1;
    th.n = 0;
    checked_reset(ck);
    if constexpr (CLIP) clip_window_var(cx);
    int node = sc.root, sp = 0, dirty = 0;
    float t_far = root.t_far();
    const int max_sp = sc.stack_depth;
    for (;;) {
        while (node >= 0) {
            const NtNode nd = sc.nodes[node];
            if (nd.axis < 0) {
                if (leaf_closest_var_t<ALIAS, CLIP>(cx, nd.left, nd.right, skip_item, skip_lane, hit, th, ck, hn_o, hn_d, nn_o, nn_d)) dirty = sp;
                node = -1;
                break;
            }
            const KdStep s = kd_descend(w, lane, nd, node, sp, max_sp, t_near, t_far, (unsigned)th.n << 24);
            if (s.crossed) t_near = s.t;
        }
        if (!kd_resume_tagged(sc, w, lane, node, sp, dirty, hit.dist, th, t_near, t_far, root.t_far())) break;
    }
    return hit.item >= 0;
}

// trace_occluded_t (nt_composite.hpp) for the current ray: transparent hits are collected, an opaque one blocks
template <typename ROOT = RootWhole, bool CLIP = false>
__device__ __noinline__ bool trace_occluded_var_t(const VarCtx &cx, float ldistance, int skip_item, int skip_lane, TList &sh, const ROOT root = ROOT()) {
    const NtCompositeDev &sc = cx.sc;
    const WaveLds &w = cx.w;
    const int lane = cx.lane;
    sh.n = 0;
    if constexpr (CLIP) clip_window_var(cx);
    int node = sc.root, sp = 0;
    float t_near = root.t_near(), t_far = root.t_far();
    const int max_sp = sc.stack_depth;
    for (;;) {
        while (node >= 0) {
            const NtNode nd = sc.nodes[node];
            if (nd.axis < 0) {
                for (int i = 0; i < nd.right; ++i) {
                    const int item = sc.items[nd.left + i];
                    if ((item & 3) != 0 && item == skip_item) continue;
                    int l;
                    const float t = test_item_var<CLIP>(cx, item, ldistance, skip_item, skip_lane, l);
                    if (t != 0.0f) {
                        if (material_of(sc, item, l)[6] >= 1.0f) return true;
                        tl_add(sh, t, item, l);
                    }
                }
                node = -1;
                break;
            }
            const KdStep s = kd_descend(w, lane, nd, node, sp, max_sp, t_near, t_far, 0u);
            if (s.crossed) {
                if (s.t < ldistance) { node = -1; break; }
                t_near = s.t;
            }
        }
        if (!kd_resume_occluded(sc, w, lane, node, sp, ldistance, t_near)) return false;
        t_far = kd_t_far_below(sc, w, lane, sp, root.t_far());
    }
}

// light_reaches (tracer.hpp:1750-1766); the shadow ray is the current ray
template <bool CLIP = false>
__device__ __forceinline__ bool light_reaches_var_t(const VarCtx &cx, float ldistance, int skip_item, int skip_lane, Color3 &filtered) {
    TList sh;
    if (trace_occluded_var_t<RootWhole, CLIP>(cx, ldistance, skip_item, skip_lane, sh)) return false;
    if (sh.n) {
        tl_sort_unique(sh);
        for (int i = sh.n - 1; i >= 0; --i) filtered = cscale(filtered, 1.0f - material_of(cx.sc, sh.e[i].item, sh.e[i].lane)[6]);
    }
    return true;
}

// composite_color_t (nt_composite.hpp): ray_color / base_color as a state machine over the frame stack.  On entry the
// primary ray is the current ray; `nframes` frames are there (max_reflect_depth + 1 when anything reflects).
template <bool ALIAS, bool CLIP = false>
__device__ __noinline__ Color3 composite_color_var_t(const VarCtx &cx, const VarFrames &fr, const Checked &ck, int nframes) {
    const NtCompositeDev &sc = cx.sc;
    const int n = cx.n;
    const int S = 4 * n;                  // first scalar word of a frame
    float a0[NT_DEV_MAX_DIM], a1[NT_DEV_MAX_DIM], a2[NT_DEV_MAX_DIM], a3[NT_DEV_MAX_DIM];
    for (int k = 0; k < n; ++k) { FRW(0, k) = VO(k); FRW(0, n + k) = VD(k); }
    FRI(0, S + VF_DEPTH) = 0;
    FRI(0, S + VF_SKIP_ITEM) = -1;
    FRI(0, S + VF_SKIP_LANE) = -1;
    int fp = 0;
    int state = 0;          // 0: trace the frame's ray, 1: shade its next surface, 2: a reflection has returned
    Color3 result = c3(0.0f, 0.0f, 0.0f);
    for (;;) {
        if (state == 0) {
            // ---- ray_color: intersect (tracer.hpp:1861-1868); the frame's ray becomes the current ray
            float *hn_o = a0, *hn_d = a1;
            for (int k = 0; k < n; ++k) {
                const float dk = FRW(fp, n + k);
                cx.L.dv[k * 64 + cx.lane] = dk;
                cx.L.ray[k * 64 + cx.lane] = make_float2(FRW(fp, k), dk != 0.0f ? 1.0f / dk : __int_as_float(0x7fc00000));
                hn_o[k] = 0.0f;
                hn_d[k] = 0.0f;
            }
            TList th;
            th.n = 0;
            Hit hit;
            hit.item = -1; hit.lane = -1; hit.dist = FLT_MAX;
            const float dist = aabb_distance_var(cx);
            if (dist >= 0.0f) {
                if constexpr (CLIP) {
                    if (fp == 0) {
                        // the primary ray under clip planes: the walk starts at max(aabb entry, t0) and ends at t1
                        float tn = dist;
                        RootWindow root;
                        if (clip_primary_var(cx, tn, root))
                            trace_closest_var_t<ALIAS, RootWindow, true>(cx, tn, FRI(fp, S + VF_SKIP_ITEM), FRI(fp, S + VF_SKIP_LANE), hit, th, ck, hn_o, hn_d,
                                                                         a2, a3, root);
                    } else {
                        trace_closest_var_t<ALIAS, RootWhole, true>(cx, dist, FRI(fp, S + VF_SKIP_ITEM), FRI(fp, S + VF_SKIP_LANE), hit, th, ck, hn_o, hn_d, a2, a3);
                    }
                } else {
                    trace_closest_var_t<ALIAS>(cx, dist, FRI(fp, S + VF_SKIP_ITEM), FRI(fp, S + VF_SKIP_LANE), hit, th, ck, hn_o, hn_d, a2, a3);
                }
            }
            if (ALIAS) {
                for (int k = 0; k < n; ++k) { FRW(fp, 2 * n + k) = hn_o[k]; FRW(fp, 3 * n + k) = hn_d[k]; }
            }
            tl_sort_unique(th);
            FRW(fp, S + VF_SURF) = hit.dist;
            FRI(fp, S + VF_SURF + 1) = hit.item;
            FRI(fp, S + VF_SURF + 2) = hit.lane;
            for (int i = 0; i < th.n; ++i) {          // farthest first (:1874)
                const THit e = th.e[th.n - 1 - i];
                FRW(fp, S + VF_SURF + 3 * (1 + i)) = e.dist;
                FRI(fp, S + VF_SURF + 3 * (1 + i) + 1) = e.item;
                FRI(fp, S + VF_SURF + 3 * (1 + i) + 2) = e.lane;
            }
            FRI(fp, S + VF_NSURF) = 1 + th.n;
            FRI(fp, S + VF_J) = 0;
            fr_put3(fr, fp, S + VF_R, c3(0.0f, 0.0f, 0.0f));
            state = 1;
            continue;
        }
        const int j = FRI(fp, S + VF_J);
        Color3 col;
        float opacity = 1.0f;
        if (state == 1) {
            if (j == FRI(fp, S + VF_NSURF)) {
                // ---- the frame is complete: hand its colour to the waiting base_color, or finish
                result = fr_get3(fr, fp, S + VF_R);
                if (fp == 0) break;
                --fp;
                state = 2;
                continue;
            }
            Hit hit;
            hit.dist = FRW(fp, S + VF_SURF + 3 * j);
            hit.item = FRI(fp, S + VF_SURF + 3 * j + 1);
            hit.lane = FRI(fp, S + VF_SURF + 3 * j + 2);
            float *dir = a0, *no = a1, *nd = a2, *lv = a3;
            for (int k = 0; k < n; ++k) dir[k] = FRW(fp, n + k);
            if (hit.item < 0) {            // miss: background (only surface 0 can be this)
                const float iv = dir[sc.bg_axis];
                fr_put3(fr, fp, S + VF_R, iv >= 0.0f ? cadd(cscale(c3p(sc.bg1), iv), cscale(c3p(sc.bg2), 1.0f - iv))
                                                     : cadd(cscale(c3p(sc.bg3), -iv), cscale(c3p(sc.bg2), 1.0f + iv)));
                FRI(fp, S + VF_J) = j + 1;
                continue;
            }
            // ---- base_color (tracer.hpp:1768-1854)
            if (ALIAS && j == 0) {
                // the opaque hit is shaded with o_hit.normal as the walk left it (tracer.hpp:1864)
                for (int k = 0; k < n; ++k) { no[k] = FRW(fp, 2 * n + k); nd[k] = FRW(fp, 3 * n + k); }
            } else {
                // (shadow rays and reflections have replaced the current ray since the frame was traced)
                for (int k = 0; k < n; ++k) {
                    cx.L.dv[k * 64 + cx.lane] = dir[k];
                    cx.L.ray[k * 64 + cx.lane].x = FRW(fp, k);
                }
                hit_normal_var(cx, hit, no, nd);
            }
            const float *m = material_of(sc, hit.item, hit.lane);
            opacity = m[6];
            Color3 light = c3(0.0f, 0.0f, 0.0f), specular = c3(0.0f, 0.0f, 0.0f);
            float spec_a = 0.0f;
            for (int li = 0; li < sc.n_point_lights; ++li) {
                const float *pos = sc.pl_pos + (size_t)li * n;
                const Color3 plc = c3p(sc.pl_color + 3 * li);
                for (int k = 0; k < n; ++k) lv[k] = no[k] - pos[k];
                const float ldist = sqrtf(dot_var(n, lv, lv));
                for (int k = 0; k < n; ++k) lv[k] = lv[k] / ldist;
                const float sine = dot_var(n, nd, lv);
                if (sine > 0.0f) {
                    const float strength = nt_falloff(ldist, n - 1);
                    if (sc.shadows) {
                        if (fmaxf(plc.r, fmaxf(plc.g, plc.b)) * strength * sine > NT_LIGHT_THRESHOLD) {
                            Color3 filtered = plc;
                            var_set_ray(cx, no, lv);
                            if (light_reaches_var_t<CLIP>(cx, ldist, hit.item, hit.lane, filtered)) {
                                filtered = cscale(filtered, strength);
                                light = cadd(light, cscale(filtered, sine));
                                if (m[8] != 0.0f) append_specular_var(n, specular, spec_a, m, filtered, dir, nd, lv);
                            }
                        }
                    } else {
                        light = cadd(light, cscale(cscale(plc, strength), sine));
                    }
                }
            }
            for (int li = 0; li < sc.n_global_lights; ++li) {
                const float *gd = sc.gl_dir + (size_t)li * n;
                const Color3 glc = c3p(sc.gl_color + 3 * li);
                const float sine = -dot_var(n, nd, gd);
                if (sine > 0.0f) {
                    if (sc.shadows) {
                        for (int k = 0; k < n; ++k) lv[k] = -gd[k];
                        Color3 filtered = glc;
                        var_set_ray(cx, no, lv);
                        if (light_reaches_var_t<CLIP>(cx, FLT_MAX, hit.item, hit.lane, filtered)) {
                            light = cadd(light, cscale(filtered, sine));
                            if (m[8] != 0.0f) append_specular_var(n, specular, spec_a, m, filtered, dir, nd, lv);
                        }
                    } else {
                        light = cadd(light, cscale(glc, sine));
                    }
                }
            }
            const float sine = -dot_var(n, dir, nd);
            if (sc.camera_light && sine > 0.0f) {
                light = cadd(light, c3(sine, sine, sine));
                if (m[8] != 0.0f) {
                    const float base = powf(sine, m[9]) * m[8];
                    specular = cadd(specular, cscale(cscale(c3p(m + 3), base), (1.0f - spec_a)));
                    spec_a += base * (1.0f - spec_a);
                    specular = cscale(specular, spec_a);
                }
            }
            const Color3 r0 = cadd(c3p(sc.ambient), cmul(c3p(m), light));
            const int depth = FRI(fp, S + VF_DEPTH);
            if (m[7] != 0.0f && depth < sc.max_reflect_depth && fp + 1 < nframes) {
                fr_put3(fr, fp, S + VF_SPEC, specular);
                FRW(fp, S + VF_SPEC_A) = spec_a;
                fr_put3(fr, fp, S + VF_R0, r0);
                fr_put3(fr, fp, S + VF_C, c3p(m));
                FRW(fp, S + VF_REFL) = m[7];
                const float f = -2.0f * sine;
                for (int k = 0; k < n; ++k) { FRW(fp + 1, n + k) = dir[k] - nd[k] * f; FRW(fp + 1, k) = no[k]; }
                FRI(fp + 1, S + VF_DEPTH) = depth + 1;
                FRI(fp + 1, S + VF_SKIP_ITEM) = hit.item;
                FRI(fp + 1, S + VF_SKIP_LANE) = hit.lane;
                ++fp;
                state = 0;
                continue;
            }
            col = cadd(specular, cscale(r0, 1.0f - spec_a));
        } else {
            // ---- state 2: the reflection of surface j returned `result` (tracer.hpp:1842-1853)
            const float refl = FRW(fp, S + VF_REFL);
            const Color3 r = cadd(cscale(cmul(fr_get3(fr, fp, S + VF_C), result), refl), cscale(fr_get3(fr, fp, S + VF_R0), 1.0f - refl));
            col = cadd(fr_get3(fr, fp, S + VF_SPEC), cscale(r, 1.0f - FRW(fp, S + VF_SPEC_A)));
            opacity = material_of(sc, FRI(fp, S + VF_SURF + 3 * j + 1), FRI(fp, S + VF_SURF + 3 * j + 2))[6];
            state = 1;
        }
        // ---- ray_color: the opaque hit is the base, transparent hits are blended over it (:1864, :1878)
        if (j == 0) fr_put3(fr, fp, S + VF_R, col);
        else fr_put3(fr, fp, S + VF_R, cadd(cscale(col, opacity), cscale(fr_get3(fr, fp, S + VF_R), 1.0f - opacity)));
        FRI(fp, S + VF_J) = j + 1;
    }
    return result;
}

#undef FRW
#undef FRI

// The blocks stride over the 8x8-pixel tiles of the launch (the scratch -- `checked` columns and frame stacks -- is sized by
// the grid, not by the image), one wave per block as in composite_kernel_var.
template <bool ALIAS>
__global__ __launch_bounds__(64) void composite_kernel_var_t(NtCamera cam, NtCompositeDev sc, NtTarget tg, int n, int tiles_x, int tiles_y,
                                                             int frames, NtClipPlanes cp) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    {
        // var_lds_carve's layout, written out: through the function this kernel alone compiles to other code
        char *p = reinterpret_cast<char *>(lds_raw);
        L.ray = reinterpret_cast<float2 *>(p);
        L.dv = reinterpret_cast<float *>(p + (size_t)64 * n * 8);
        L.ps = L.dv + (size_t)64 * n;
        L.stack = reinterpret_cast<int *>(L.ps + (size_t)64 * n);
        L.mbox = L.stack + (size_t)64 * sc.stack_depth;
    }
    WaveLds w;
    w.ray = L.ray;
    w.stack = L.stack;
    w.mbox = L.mbox;
    const long long slot = (long long)blockIdx.x * 64 + lane;
    Checked ck;
    ck.bits = sc.checked + slot;
    ck.stride = sc.checked_lanes;
    ck.words = sc.checked_words;
    ck.n_batches = sc.n_batches;
    ck.n_triangles = sc.n_triangles;
    VarFrames fr;
    var_frames(fr, sc, slot, n);
    float cwin[3];                            // (clip planes: the window of the lane's current ray)
    const VarCtxClip cxc = {{sc, L, w, n, lane}, cp.planes, cp.count, cwin};
    const VarCtx &cx = cxc;
    const long long total = (long long)tiles_x * tiles_y * frames;
    for (long long tile = (long long)blockIdx.x; tile < total; tile += gridDim.x) {
        if (nt_aborted(tg)) return;                       // (one wave a block)
        const int bz = (int)(tile / ((long long)tiles_x * tiles_y));
        const int rem = (int)(tile - (long long)bz * tiles_x * tiles_y);
        const int by = rem / tiles_x;
        const int bx = rem - by * tiles_x;
        const PixelRef pr = tg.colors_out ? locate_pixel_at<8, 8>(tg, bx, by, bz, 0, 0, lane)
                                          : locate_pixel_at<8, 8>(tg, bx, by, bz, lane & 7, lane >> 3, lane);
        if (!pr.valid) continue;
        const float *c = cam.buf ? cam.buf + (size_t)bz * 4 * n : nullptr;
        // ---- primary ray (tracer.hpp:60-76) becomes the current ray
        const float sx = tg.fovI * ((float)pr.x - tg.half_w);
        const float sy = tg.fovI * ((float)pr.y - tg.half_h);
        float sq = 0.0f;
        for (int k = 0; k < n; ++k) {
            const float rk = c ? c[n + k] : cam.inl[n + k];
            const float uk = c ? c[2 * n + k] : cam.inl[2 * n + k];
            const float fk = c ? c[3 * n + k] : cam.inl[3 * n + k];
            const float v = (fk + rk * sx) - uk * sy;
            L.dv[k * 64 + lane] = v;
            sq = k == 0 ? v * v : sq + v * v;
        }
        const float len = sqrtf(sq);
        for (int k = 0; k < n; ++k) {
            const float dk = L.dv[k * 64 + lane] / len;
            L.dv[k * 64 + lane] = dk;
            const float ok_ = c ? c[k] : cam.inl[k];
            L.ray[k * 64 + lane] = make_float2(ok_, dk != 0.0f ? 1.0f / dk : __int_as_float(0x7fc00000));
        }
        const Color3 col = cp.count ? composite_color_var_t<ALIAS, true>(cx, fr, ck, sc.tframe_count) : composite_color_var_t<ALIAS>(cx, fr, ck, sc.tframe_count);
        emit_pixel(tg, pr, col.r, col.g, col.b);
    }
}

__global__ __launch_bounds__(64) void composite_kernel_var(NtCamera cam, NtCompositeDev sc, NtTarget tg, int n, NtClipPlanes cp) {
    extern __shared__ float2 lds_raw[];
    if (nt_aborted(tg)) return;
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    const PixelRef pr = tg.colors_out ? locate_pixel<8, 8>(tg, 0, 0, lane) : locate_pixel<8, 8>(tg, lane & 7, lane >> 3, lane);
    if (!pr.valid) return;
    const float *c = cam.buf ? cam.buf + (size_t)blockIdx.z * 4 * n : nullptr;

    // ---- primary ray (tracer.hpp:60-76) becomes the current ray
    const float sx = tg.fovI * ((float)pr.x - tg.half_w);
    const float sy = tg.fovI * ((float)pr.y - tg.half_h);
    float sq = 0.0f;
    for (int k = 0; k < n; ++k) {
        const float rk = c ? c[n + k] : cam.inl[n + k];
        const float uk = c ? c[2 * n + k] : cam.inl[2 * n + k];
        const float fk = c ? c[3 * n + k] : cam.inl[3 * n + k];
        const float v = (fk + rk * sx) - uk * sy;
        L.dv[k * 64 + lane] = v;
        sq = k == 0 ? v * v : sq + v * v;
    }
    const float len = sqrtf(sq);
    for (int k = 0; k < n; ++k) {
        const float dk = L.dv[k * 64 + lane] / len;
        L.dv[k * 64 + lane] = dk;
        const float ok_ = c ? c[k] : cam.inl[k];
        L.ray[k * 64 + lane] = make_float2(ok_, dk != 0.0f ? 1.0f / dk : __int_as_float(0x7fc00000));
    }
    float cwin[3];                            // (clip planes: the window of the lane's current ray)
    const VarCtxClip cxc = {{sc, L, w, n, lane}, cp.planes, cp.count, cwin};
    const VarCtx &cx = cxc;
    const Color3 col = cp.count ? composite_color_var<true>(cx) : composite_color_var(cx);
    emit_pixel(tg, pr, col.r, col.g, col.b);
}

// --------------------------------------------------------------------------------------
// X-ray views at run-time n (the rule in full: ntracer_hip.h; nt_xray.hpp has the packet walk): the general
// route, for n = 11..64, trees deeper than the packet's stack, more items than its bitset holds and NTRACER_FORCE_VAR=1.  A
// per-lane walk over the lane's own [dist0, FLT_MAX] window with no hit, hence no cutoff and nothing to prune: every far side is
// resumed.  The exact per-lane `Checked` bitset of the transparent kernels keeps an item met in several leaves from counting
// twice.  The blocks stride over the 8x8-pixel tiles as composite_kernel_var_t's do: the scratch is sized by the grid.
// --------------------------------------------------------------------------------------
template <bool COUNTS>
__global__ __launch_bounds__(64) void xray_var(NtCompositeDev sc, NtTarget tg, NtXray xr, int n, int tiles_x, int tiles_y, int frames) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    const long long slot = (long long)blockIdx.x * 64 + lane;
    Checked ck;
    ck.bits = sc.checked + slot;
    ck.stride = sc.checked_lanes;
    ck.words = sc.checked_words;
    ck.n_batches = sc.n_batches;
    ck.n_triangles = sc.n_triangles;
    const VarCtx cx = {sc, L, w, n, lane};
    const int max_sp = sc.stack_depth;
    const long long total = (long long)tiles_x * tiles_y * frames;
    for (long long tile = (long long)blockIdx.x; tile < total; tile += gridDim.x) {
        if (nt_aborted(tg)) return;                       // (one wave a block)
        const int bz = (int)(tile / ((long long)tiles_x * tiles_y));
        const int rem = (int)(tile - (long long)bz * tiles_x * tiles_y);
        const int by = rem / tiles_x;
        const int bx = rem - by * tiles_x;
        const PixelRef pr = locate_pixel_at<8, 8>(tg, bx, by, bz, lane & 7, lane >> 3, lane);
        if (!pr.valid) continue;
        const float *c = xr.cams + (size_t)bz * 4 * n;
        // ---- primary ray (tracer.hpp:60-76) becomes the current ray
        const float sx = tg.fovI * ((float)pr.x - tg.half_w);
        const float sy = tg.fovI * ((float)pr.y - tg.half_h);
        float sq = 0.0f;
        for (int k = 0; k < n; ++k) {
            const float v = (c[3 * n + k] + c[n + k] * sx) - c[2 * n + k] * sy;
            L.dv[k * 64 + lane] = v;
            sq = k == 0 ? v * v : sq + v * v;
        }
        const float len = sqrtf(sq);
        for (int k = 0; k < n; ++k) {
            const float dk = L.dv[k * 64 + lane] / len;
            L.dv[k * 64 + lane] = dk;
            L.ray[k * 64 + lane] = make_float2(c[k], dk != 0.0f ? 1.0f / dk : __int_as_float(0x7fc00000));
        }
        int count = 0;
        float fr = 1.0f, fg = 1.0f, fb = 1.0f;
        float t_near = aabb_distance_var(cx);
        if (t_near >= 0.0f) {
            // the Solids, every one of them in front of the walk, as xray_packet has them: the rule knows no tree, and the trees of
            // the reference's builder leave Solids out of cells they reach.  The leaves' own are skipped below.
            for (int idx = 0; idx < sc.n_solids; ++idx) {
                int lane_out;
                const float t = test_item_var(cx, (idx << 2) | 2, FLT_MAX, -1, -1, lane_out);
                if (t == 0.0f) continue;
                ++count;
                if (!COUNTS) {
                    const float *tm = xr.trans + (size_t)sc.solid_mats[idx] * 3;
                    fr = fr * tm[0]; fg = fg * tm[1]; fb = fb * tm[2];
                }
            }
            checked_reset(ck);
            int node = sc.root, sp = 0;
            float t_far = FLT_MAX;
            for (;;) {
                while (node >= 0) {
                    const NtNode nd = sc.nodes[node];
                    if (nd.axis < 0) {
                        for (int i = 0; i < nd.right; ++i) {
                            const int item = sc.items[nd.left + i];
                            const int kind = item & 3, idx = item >> 2;
                            if (kind > 1 || checked_seen(ck, item)) continue;
                            if (kind == 0) {
                                const unsigned int lv = xr.live[idx];
                                for (int l = 0; l < NT_DEV_BATCH; ++l) {
                                    if (((lv >> l) & 1u) == 0u) continue;
                                    const float t = simplex_var(sc.batch_recs + ((size_t)idx * NT_DEV_BATCH + l) * sc.rec_stride, n, L, lane, false, 0.0f);
                                    if (t == 0.0f) continue;
                                    ++count;
                                    if (!COUNTS) {
                                        const float *tm = xr.trans + (size_t)sc.batch_mats[idx * NT_DEV_BATCH + l] * 3;
                                        fr = fr * tm[0]; fg = fg * tm[1]; fb = fb * tm[2];
                                    }
                                }
                                continue;
                            }
                            // (test_item_var: the scalar rule and the Solid's own test, each with the cutoff it is handed)
                            int lane_out;
                            const float t = test_item_var(cx, item, FLT_MAX, -1, -1, lane_out);
                            if (t == 0.0f) continue;
                            ++count;
                            if (!COUNTS) {
                                const float *tm = xr.trans + (size_t)(kind == 1 ? sc.tri_mats[idx] : sc.solid_mats[idx]) * 3;
                                fr = fr * tm[0]; fg = fg * tm[1]; fb = fb * tm[2];
                            }
                        }
                        node = -1;
                        break;
                    }
                    // kd_node_intersection::operator() (tracer.hpp:1179-1243) without a hit: trace_closest_var's branch step
                    const float2 oi = w.ray[nd.axis * 64 + lane];
                    const float oa = oi.x, inv = oi.y;
                    if (inv == inv) {
                        if (oa == nd.split) { node = inv > 0.0f ? nd.right : nd.left; continue; }
                        const float t = (nd.split - oa) * inv;
                        const bool gt = oa > nd.split;
                        const int n_near = gt ? nd.right : nd.left;
                        const int n_far = gt ? nd.left : nd.right;
                        if (t < 0.0f || t > t_far) { node = n_near; continue; }
                        if (t < t_near) { node = n_far; continue; }
                        if (n_near >= 0) {
                            if (sp < max_sp) { w.stack[sp * 64 + lane] = node; ++sp; }
                            t_far = t;
                            node = n_near;
                            continue;
                        }
                        node = n_far;
                        t_near = t;
                        continue;
                    }
                    node = oa >= nd.split ? nd.right : nd.left;
                }
                bool resumed = false;
                while (sp > 0) {
                    --sp;
                    const NtNode nd = sc.nodes[w.stack[sp * 64 + lane]];
                    bool gt;
                    const float t = branch_t(w, lane, nd, gt);
                    const int far = gt ? nd.left : nd.right;
                    if (far < 0) continue;
                    node = far;
                    t_near = t;
                    t_far = FLT_MAX;
                    if (sp > 0) {
                        const NtNode up = sc.nodes[w.stack[(sp - 1) * 64 + lane]];
                        bool g2;
                        t_far = branch_t(w, lane, up, g2);
                    }
                    resumed = true;
                    break;
                }
                if (!resumed) break;
            }
        }
        if (COUNTS) {
            xr.counts[((long long)bz * tg.height + pr.y) * tg.width + pr.x] = count;
            continue;
        }
        const float iv = L.dv[sc.bg_axis * 64 + lane];
        const Color3 bgc = iv >= 0.0f ? cadd(cscale(c3p(sc.bg1), iv), cscale(c3p(sc.bg2), 1.0f - iv))
                                      : cadd(cscale(c3p(sc.bg3), -iv), cscale(c3p(sc.bg2), 1.0f + iv));
        emit_pixel(tg, pr, bgc.r * fr, bgc.g * fg, bgc.b * fb);
    }
}

// --------------------------------------------------------------------------------------
// Hit layers at run-time n (the rule in full: ntracer_hip.h; nt_layers.hpp has the packet walk): xray_var's
// per-lane walk with its exact `checked` columns -- its control through kd_descend and kd_resume_closest with nothing ever
// "dirty", which resumes every far side as xray_var's own text does; where xray_var counts a crossing the lane also inserts its
// key into the sorted list of nt_layer_list.hpp -- always the 8-key list, of which the first ly.layers planes are stored.  One frame.
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void layers_var(NtCompositeDev sc, NtTarget tg, NtLayers ly, int n, int tiles_x, int tiles_y) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    const long long slot = (long long)blockIdx.x * 64 + lane;
    Checked ck;
    ck.bits = sc.checked + slot;
    ck.stride = sc.checked_lanes;
    ck.words = sc.checked_words;
    ck.n_batches = sc.n_batches;
    ck.n_triangles = sc.n_triangles;
    const VarCtx cx = {sc, L, w, n, lane};
    const int max_sp = sc.stack_depth;
    const long long total = (long long)tiles_x * tiles_y;
    const long long px = (long long)tg.width * tg.height;
    for (long long tile = (long long)blockIdx.x; tile < total; tile += gridDim.x) {
        if (nt_aborted(tg)) return;                       // (one wave a block)
        const int by = (int)(tile / tiles_x);
        const int bx = (int)(tile - (long long)by * tiles_x);
        const PixelRef pr = locate_pixel_at<8, 8>(tg, bx, by, 0, lane & 7, lane >> 3, lane);
        if (!pr.valid) continue;
        const float *c = ly.cams;
        // ---- primary ray (tracer.hpp:60-76) becomes the current ray
        const float sx = tg.fovI * ((float)pr.x - tg.half_w);
        const float sy = tg.fovI * ((float)pr.y - tg.half_h);
        float sq = 0.0f;
        for (int k = 0; k < n; ++k) {
            const float v = (c[3 * n + k] + c[n + k] * sx) - c[2 * n + k] * sy;
            L.dv[k * 64 + lane] = v;
            sq = k == 0 ? v * v : sq + v * v;
        }
        const float len = sqrtf(sq);
        for (int k = 0; k < n; ++k) {
            const float dk = L.dv[k * 64 + lane] / len;
            L.dv[k * 64 + lane] = dk;
            L.ray[k * 64 + lane] = make_float2(c[k], dk != 0.0f ? 1.0f / dk : __int_as_float(0x7fc00000));
        }
        int count = 0;
        LayerList<NT_DEV_LAYERS_MAX> ls;
        ls.clear();
        float t_near = aabb_distance_var(cx);
        if (t_near >= 0.0f) {
            // the Solids, every one of them in front of the walk, as xray_var has them; the leaves' own are skipped below
            for (int idx = 0; idx < sc.n_solids; ++idx) {
                int lane_out;
                float t = test_item_var(cx, (idx << 2) | 2, FLT_MAX, -1, -1, lane_out);
                if (t == 0.0f) continue;
                ++count;
                // (a sphere's distance once more in float64: layer_sphere_t says why)
                if (sc.solid_types[idx] != 1)
                    t = layer_sphere_t(sc.solid_recs + (size_t)idx * (2 * n * n + n), n, t, [&](int k) { return L.ray[k * 64 + lane].x; },
                                       [&](int k) { return L.dv[k * 64 + lane]; });
                ls.insert(layer_key(true, t, (idx << 2) | 2, -1));
            }
            checked_reset(ck);
            int node = sc.root, sp = 0;
            int dirty = 0;
            float t_far = FLT_MAX;
            const float none = FLT_MAX;
            for (;;) {
                while (node >= 0) {
                    const NtNode nd = sc.nodes[node];
                    if (nd.axis < 0) {
                        for (int i = 0; i < nd.right; ++i) {
                            const int item = sc.items[nd.left + i];
                            const int kind = item & 3, idx = item >> 2;
                            if (kind > 1 || checked_seen(ck, item)) continue;
                            if (kind == 0) {
                                const unsigned int lv = ly.live[idx];
                                for (int l = 0; l < NT_DEV_BATCH; ++l) {
                                    if (((lv >> l) & 1u) == 0u) continue;
                                    const float t = simplex_var(sc.batch_recs + ((size_t)idx * NT_DEV_BATCH + l) * sc.rec_stride, n, L, lane, false, 0.0f);
                                    if (t == 0.0f) continue;
                                    ++count;
                                    ls.insert(layer_key(true, t, item, l));
                                }
                                continue;
                            }
                            // (test_item_var: the scalar rule with the cutoff it is handed)
                            int lane_out;
                            const float t = test_item_var(cx, item, FLT_MAX, -1, -1, lane_out);
                            if (t == 0.0f) continue;
                            ++count;
                            ls.insert(layer_key(true, t, item, -1));
                        }
                        node = -1;
                        break;
                    }
                    const KdStep s = kd_descend(w, lane, nd, node, sp, max_sp, t_near, t_far, 0u);
                    if (s.crossed) t_near = s.t;
                }
                // (no hit, so nothing prunes: every far side is resumed)
                if (!kd_resume_closest(sc, w, lane, node, sp, dirty, none, t_near)) break;
                t_far = kd_t_far_below(sc, w, lane, sp, FLT_MAX);
            }
        }
        layers_store<NT_DEV_LAYERS_MAX>(ly.records, (long long)pr.y * tg.width + pr.x, px, ly.layers, ls, count);
    }
}

// --------------------------------------------------------------------------------------
// Ray queries at run-time n (n = 11..64, and every n under NTRACER_FORCE_VAR=1): the kernels of nt_query.hpp on the walks
// above.  One lane per ray and one wave a block, as the run-time-n render kernels have it -- their n-vectors in LDS make
// four waves' worth too much at the upper dimensions -- so lane l of block b takes ray 64 b + l, and the blocks stride on.
// --------------------------------------------------------------------------------------
__device__ __forceinline__ void query_store_normal_var(const NtQuery &q, long long r, int n, const float *no, const float *nd) {
    if (q.normal_origin) for (int k = 0; k < n; ++k) q.normal_origin[r * n + k] = no[k];
    if (q.normal_dir) for (int k = 0; k < n; ++k) q.normal_dir[r * n + k] = nd[k];
}

__global__ __launch_bounds__(64) void query_closest_var(NtCompositeDev sc, NtQuery q, int n) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    const VarCtx cx = {sc, L, w, n, lane};
    for (long long base = (long long)blockIdx.x * 64; base < q.count; base += (long long)gridDim.x * 64) {
        if (query_aborted(q)) return;
        const long long r = base + lane;
        if (r >= q.count) continue;
        var_set_ray(cx, q.origins + r * n, q.directions + r * n);
        const QueryRay p = query_ray(q, r);
        RootWindow root;
        root.tn = p.t_near;
        root.tf = p.t_far;
        Hit hit;
        trace_closest_var<RootWindow>(cx, p.t_near, p.skip_item, p.skip_lane, hit, root);
        query_store(q.hits, r, hit.dist, hit.item, hit.lane, 0);
        if (hit.item >= 0 && (q.normal_origin || q.normal_dir)) {
            float no[NT_DEV_MAX_DIM], nd[NT_DEV_MAX_DIM];
            hit_normal_var(cx, hit, no, nd);
            query_store_normal_var(q, r, n, no, nd);
        }
        if (q.transparent) {
            TList none;
            none.n = 0;
            query_store_list(q, r, none);
        }
    }
}

template <bool ALIAS>
__global__ __launch_bounds__(64) void query_closest_var_t(NtCompositeDev sc, NtQuery q, int n) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    const VarCtx cx = {sc, L, w, n, lane};
    Checked ck;
    ck.bits = sc.checked + ((long long)blockIdx.x * 64 + lane);
    ck.stride = sc.checked_lanes;
    ck.words = sc.checked_words;
    ck.n_batches = sc.n_batches;
    ck.n_triangles = sc.n_triangles;
    for (long long base = (long long)blockIdx.x * 64; base < q.count; base += (long long)gridDim.x * 64) {
        if (query_aborted(q)) return;
        const long long r = base + lane;
        if (r >= q.count) continue;
        var_set_ray(cx, q.origins + r * n, q.directions + r * n);
        const QueryRay p = query_ray(q, r);
        RootWindow root;
        root.tn = p.t_near;
        root.tf = p.t_far;
        Hit hit;
        TList th;
        float hn_o[NT_DEV_MAX_DIM], hn_d[NT_DEV_MAX_DIM], nn_o[NT_DEV_MAX_DIM], nn_d[NT_DEV_MAX_DIM];
        for (int k = 0; k < n; ++k) { hn_o[k] = 0.0f; hn_d[k] = 0.0f; }       // ray_intersection starts out zeroed
        trace_closest_var_t<ALIAS, RootWindow>(cx, p.t_near, p.skip_item, p.skip_lane, hit, th, ck, hn_o, hn_d, nn_o, nn_d, root);
        query_store(q.hits, r, hit.dist, hit.item, hit.lane, th.n);
        if (hit.item >= 0 && (q.normal_origin || q.normal_dir)) {
            if (!ALIAS) hit_normal_var(cx, hit, hn_o, hn_d);
            query_store_normal_var(q, r, n, hn_o, hn_d);
        }
        query_store_list(q, r, th);
    }
}

__global__ __launch_bounds__(64) void query_occluded_var(NtCompositeDev sc, NtQuery q, int n) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    const VarCtx cx = {sc, L, w, n, lane};
    for (long long base = (long long)blockIdx.x * 64; base < q.count; base += (long long)gridDim.x * 64) {
        if (query_aborted(q)) return;
        const long long r = base + lane;
        if (r >= q.count) continue;
        var_set_ray(cx, q.origins + r * n, q.directions + r * n);
        const QueryRay p = query_ray(q, r);
        RootWindow root;
        root.tn = p.t_near;
        root.tf = p.t_far;
        const bool blocked = trace_occluded_var<RootWindow>(cx, p.distance, p.skip_item, p.skip_lane, root);
        query_store(q.hits, r, blocked ? 1.0f : 0.0f, -1, -1, 0);
        if (q.transparent) {
            TList none;
            none.n = 0;
            query_store_list(q, r, none);
        }
    }
}

__global__ __launch_bounds__(64) void query_occluded_var_t(NtCompositeDev sc, NtQuery q, int n) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    const VarCtx cx = {sc, L, w, n, lane};
    for (long long base = (long long)blockIdx.x * 64; base < q.count; base += (long long)gridDim.x * 64) {
        if (query_aborted(q)) return;
        const long long r = base + lane;
        if (r >= q.count) continue;
        var_set_ray(cx, q.origins + r * n, q.directions + r * n);
        const QueryRay p = query_ray(q, r);
        RootWindow root;
        root.tn = p.t_near;
        root.tf = p.t_far;
        TList sh;
        const bool blocked = trace_occluded_var_t<RootWindow>(cx, p.distance, p.skip_item, p.skip_lane, sh, root);
        query_store(q.hits, r, blocked ? 1.0f : 0.0f, -1, -1, sh.n);
        query_store_list(q, r, sh);
    }
}

// --------------------------------------------------------------------------------------
// Primary-hit buffers at run-time n: the kernels of nt_hits.hpp on the walks above, one wave a block and an 8x8 tile a wave
// as composite_kernel_var has it, the blocks striding over [frame][tile row][tile column].
// --------------------------------------------------------------------------------------
// the pixel's primary ray (tracer.hpp:60-76) becomes the current ray: composite_kernel_var's operations, in its order
__device__ __forceinline__ void hits_set_ray_var(const VarCtx &cx, const NtTarget &tg, const NtHits &h, const HitsPixel &p) {
    const int n = cx.n, lane = cx.lane;
    const float *c = h.cams + (size_t)p.frame * 4 * n;
    const float sx = tg.fovI * ((float)p.x - tg.half_w);
    const float sy = tg.fovI * ((float)p.y - tg.half_h);
    float sq = 0.0f;
    for (int k = 0; k < n; ++k) {
        const float v = (c[3 * n + k] + c[n + k] * sx) - c[2 * n + k] * sy;
        cx.L.dv[k * 64 + lane] = v;
        sq = k == 0 ? v * v : sq + v * v;
    }
    const float len = sqrtf(sq);
    for (int k = 0; k < n; ++k) {
        const float dk = cx.L.dv[k * 64 + lane] / len;
        cx.L.dv[k * 64 + lane] = dk;
        cx.L.ray[k * 64 + lane] = make_float2(c[k], dk != 0.0f ? 1.0f / dk : __int_as_float(0x7fc00000));
    }
}

__device__ __forceinline__ void hits_store_normal_var(const NtHits &h, long long r, int n, const float *no, const float *nd) {
    if (h.normal_origin) for (int k = 0; k < n; ++k) h.normal_origin[r * n + k] = no[k];
    if (h.normal_dir) for (int k = 0; k < n; ++k) h.normal_dir[r * n + k] = nd[k];
}

__global__ __launch_bounds__(64) void hits_closest_var(NtCompositeDev sc, NtTarget tg, NtHits h, int n, int tiles_x, int tiles_y, NtClipPlanes cp) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    float cwin[3];                            // (clip planes: the window of the lane's current ray)
    const VarCtxClip cxc = {{sc, L, w, n, lane}, cp.planes, cp.count, cwin};
    const VarCtx &cx = cxc;
    const long long total = (long long)tiles_x * tiles_y * h.nframes;
    for (long long tile = (long long)blockIdx.x; tile < total; tile += gridDim.x) {
        if (nt_aborted(tg)) return;                       // (one wave a block)
        const HitsPixel p = hits_pixel<8, 8>(tg, h, tile, tiles_x, tiles_y, lane & 7, lane >> 3);
        if (!p.valid) continue;
        hits_set_ray_var(cx, tg, h, p);
        Hit hit;
        hit.dist = FLT_MAX; hit.item = -1; hit.lane = -1;
        const float dist0 = aabb_distance_var(cx);
        if (dist0 >= 0.0f) {
            if (cp.count) {
                float tn = dist0;
                RootWindow root;
                if (clip_primary_var(cx, tn, root)) trace_closest_var<RootWindow, true>(cx, tn, -1, -1, hit, root);
            } else {
                trace_closest_var(cx, dist0, -1, -1, hit);
            }
        }
        query_store(h.hits, p.rec, hit.dist, hit.item, hit.lane, 0);
        if (hit.item >= 0 && (h.normal_origin || h.normal_dir)) {
            float no[NT_DEV_MAX_DIM], nd[NT_DEV_MAX_DIM];
            hit_normal_var(cx, hit, no, nd);
            hits_store_normal_var(h, p.rec, n, no, nd);
        }
    }
}

template <bool ALIAS>
__global__ __launch_bounds__(64) void hits_closest_var_t(NtCompositeDev sc, NtTarget tg, NtHits h, int n, int tiles_x, int tiles_y, NtClipPlanes cp) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    float cwin[3];                            // (clip planes: the window of the lane's current ray)
    const VarCtxClip cxc = {{sc, L, w, n, lane}, cp.planes, cp.count, cwin};
    const VarCtx &cx = cxc;
    Checked ck;
    ck.bits = sc.checked + ((long long)blockIdx.x * 64 + lane);
    ck.stride = sc.checked_lanes;
    ck.words = sc.checked_words;
    ck.n_batches = sc.n_batches;
    ck.n_triangles = sc.n_triangles;
    const long long total = (long long)tiles_x * tiles_y * h.nframes;
    for (long long tile = (long long)blockIdx.x; tile < total; tile += gridDim.x) {
        if (nt_aborted(tg)) return;
        const HitsPixel p = hits_pixel<8, 8>(tg, h, tile, tiles_x, tiles_y, lane & 7, lane >> 3);
        if (!p.valid) continue;
        hits_set_ray_var(cx, tg, h, p);
        Hit hit;
        hit.dist = FLT_MAX; hit.item = -1; hit.lane = -1;
        TList th;
        th.n = 0;
        float hn_o[NT_DEV_MAX_DIM], hn_d[NT_DEV_MAX_DIM], nn_o[NT_DEV_MAX_DIM], nn_d[NT_DEV_MAX_DIM];
        for (int k = 0; k < n; ++k) { hn_o[k] = 0.0f; hn_d[k] = 0.0f; }       // ray_intersection starts out zeroed
        const float dist0 = aabb_distance_var(cx);
        if (dist0 >= 0.0f) {
            if (cp.count) {
                float tn = dist0;
                RootWindow root;
                if (clip_primary_var(cx, tn, root)) trace_closest_var_t<ALIAS, RootWindow, true>(cx, tn, -1, -1, hit, th, ck, hn_o, hn_d, nn_o, nn_d, root);
            } else {
                trace_closest_var_t<ALIAS>(cx, dist0, -1, -1, hit, th, ck, hn_o, hn_d, nn_o, nn_d);
            }
        }
        query_store(h.hits, p.rec, hit.dist, hit.item, hit.lane, th.n);
        if (hit.item >= 0 && (h.normal_origin || h.normal_dir)) {
            if (!ALIAS) hit_normal_var(cx, hit, hn_o, hn_d);
            hits_store_normal_var(h, p.rec, n, hn_o, hn_d);
        }
    }
}

// --------------------------------------------------------------------------------------
// The colours of the caller's rays at run-time n (n = 11..64 -- BoxScene: 25..64 -- and every n under NTRACER_FORCE_VAR=1): the
// kernels of nt_rays.hpp on composite_color_var / composite_color_var_t above.  One lane per ray and one wave a block, as the
// run-time-n render kernels have it, so lane l of block b takes ray 64 b + l, and the blocks stride on.
// --------------------------------------------------------------------------------------
// ray r becomes the current ray: the origin as given, the direction normalised as composite_kernel_var normalises its primary ray
__device__ __forceinline__ void rays_set_ray_var(const VarCtx &cx, const NtRayJob &job, long long r) {
    const int n = cx.n, lane = cx.lane;
    const float *pd = job.directions + r * n;
    const float *po = job.shared_origin ? job.origins : job.origins + r * n;
    float sq = 0.0f;
    for (int k = 0; k < n; ++k) {
        const float v = pd[k];
        cx.L.dv[k * 64 + lane] = v;
        sq = k == 0 ? v * v : sq + v * v;
    }
    const float len = sqrtf(sq);
    for (int k = 0; k < n; ++k) {
        const float dk = cx.L.dv[k * 64 + lane] / len;
        cx.L.dv[k * 64 + lane] = dk;
        cx.L.ray[k * 64 + lane] = make_float2(po[k], dk != 0.0f ? 1.0f / dk : __int_as_float(0x7fc00000));
    }
}

__global__ __launch_bounds__(64) void rays_color_var(NtCompositeDev sc, NtRayJob job, NtTarget tg, int n) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    const VarCtx cx = {sc, L, w, n, lane};
    for (long long base = (long long)blockIdx.x * 64; base < job.count; base += (long long)gridDim.x * 64) {
        if (nt_aborted(tg)) return;                       // (one wave a block)
        const long long r = base + lane;
        if (r >= job.count) continue;
        rays_set_ray_var(cx, job, r);
        const Color3 col = composite_color_var(cx);
        emit_pixel(tg, rays_pixel(tg, r), col.r, col.g, col.b);
    }
}

// ... with transparent materials or the reference's o_hit.normal handling: the `checked` column and the frame stack of the
// lane's slot, so the grid is what that scratch has columns for
template <bool ALIAS>
__global__ __launch_bounds__(64) void rays_color_var_t(NtCompositeDev sc, NtRayJob job, NtTarget tg, int n) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    const VarCtx cx = {sc, L, w, n, lane};
    const long long slot = (long long)blockIdx.x * 64 + lane;
    Checked ck;
    ck.bits = sc.checked + slot;
    ck.stride = sc.checked_lanes;
    ck.words = sc.checked_words;
    ck.n_batches = sc.n_batches;
    ck.n_triangles = sc.n_triangles;
    VarFrames fr;
    var_frames(fr, sc, slot, n);
    for (long long base = (long long)blockIdx.x * 64; base < job.count; base += (long long)gridDim.x * 64) {
        if (nt_aborted(tg)) return;
        const long long r = base + lane;
        if (r >= job.count) continue;
        rays_set_ray_var(cx, job, r);
        const Color3 col = composite_color_var_t<ALIAS>(cx, fr, ck, sc.tframe_count);
        emit_pixel(tg, rays_pixel(tg, r), col.r, col.g, col.b);
    }
}

// BoxScene at run-time n: box_kernel_var's evaluation -- the reference's arithmetic on the faces in a near-tie with the candidate
// reached last, see box_color -- for every ray, origin and direction as per-lane n-vectors in LDS, [k][lane]
__global__ __launch_bounds__(64) void rays_box_var(NtRayJob job, NtTarget tg, int n) {
    extern __shared__ float lds_vec[];    // [n][64] direction, [n][64] origin
    const int lane = (int)threadIdx.x;
    float *dir = lds_vec + lane;          // dir[j] at dir[j * 64]
    float *org = lds_vec + (size_t)n * 64 + lane;
    for (long long base = (long long)blockIdx.x * 64; base < job.count; base += (long long)gridDim.x * 64) {
        if (nt_aborted(tg)) return;
        const long long r = base + lane;
        if (r >= job.count) continue;
        const float *pd = job.directions + r * n;
        const float *po = job.shared_origin ? job.origins : job.origins + r * n;
        float sq = 0.0f;
        for (int j = 0; j < n; ++j) {
            const float v = pd[j];
            dir[j * 64] = v;
            org[j * 64] = po[j];
            sq = j == 0 ? v * v : sq + v * v;
        }
        const float len = sqrtf(sq);
        for (int j = 0; j < n; ++j) dir[j * 64] = dir[j * 64] / len;
        bool done = false;
        float shade = 0.0f;
        float aK = 0.0f, bK = 1.0f, oK = 0.0f;
        bool any = false;
        for (int i = 0; i < n; ++i) {
            const float di = dir[i * 64];
            const float oi = org[i * 64];
            const float num = (di < 0.0f ? 1.0f : -1.0f) - oi;
            const bool pre = (num > 0.0f && di > 0.0f) || (num < 0.0f && di < 0.0f);
            const float a = fabsf(num), bb = fabsf(di);
            if (pre && (!any || a * bK > aK * bb)) { aK = a; bK = bb; oK = oi; any = true; }
        }
        const float mu = 1e-4f * (1.0f + fabsf(oK));
        const float aKm = (aK - mu) * (1.0f - 1e-6f);
        for (int i = 0; i < n; ++i) {
            const float di = dir[i * 64];
            const float oi = org[i * 64];
            const float s = di < 0.0f ? 1.0f : -1.0f;
            const float num = s - oi;
            const bool pre = (num > 0.0f && di > 0.0f) || (num < 0.0f && di < 0.0f);
            const bool tie = pre && !done && !(fabsf(num) * bK < fabsf(di) * aKm);
            if (!tie) continue;
            const float dist = num / di;
            bool ok = dist > 0.0f;
            for (int j = 0; j < n; ++j) {
                if (j != i) {
                    const float p = dir[j * 64] * dist + org[j * 64];
                    ok = ok && !(fabsf(p) > (1.0f + NT_FUZZ));
                }
            }
            if (ok) {
                done = true;
                if (dist >= FLT_MAX) shade = -1.0f;
                else {
                    const float sine = di * s;
                    shade = sine <= 0.0f ? -sine : 0.0f;
                }
            }
        }
        float cr, cg, cb;
        if (done && shade >= 0.0f) {
            cr = shade * 1.0f;
            cg = shade * 0.5f;
            cb = shade * 0.5f;
        } else {
            box_background(dir[0], cr, cg, cb);
        }
        emit_pixel(tg, rays_pixel(tg, r), cr, cg, cb);
    }
}

// BoxScene hit buffers at run-time n (nt_boxhits.hpp has the compile-time-N kernel and the record): rays_box_var's layout and
// evaluation -- the direction as a per-lane n-vector in LDS, [k][lane] -- with the camera's rows behind it, staged once a block as
// box_kernel_var stages them, keeping the face and the distance instead of the shade.  One wave a block, a lane walks a column
// of NT_BOXROWS rows; frames in blockIdx.z.
__global__ __launch_bounds__(64) void box_hits_var(NtCamera cam, NtTarget tg, NtBoxFaces bf) {
    extern __shared__ float lds_vec[];    // [n][64] direction, then [4][n] camera rows (broadcast reads)
    if (nt_aborted(tg)) return;           // (every lane reads the same word: the whole block leaves, ahead of the barrier)
    const int lane = (int)threadIdx.x;
    const int n = cam.n;
    float *camrow = lds_vec + (size_t)n * 64;
    {
        const float *src = cam.buf ? cam.buf + (size_t)blockIdx.z * 4 * n : nullptr;
        for (int k = lane; k < 4 * n; k += 64) camrow[k] = src ? src[k] : cam.inl[k];
    }
    __syncthreads();
    const float *c = camrow;              // origin, right, up, forward
    float *dir = lds_vec + lane;          // dir[j] at dir[j * 64]
    float dots[4];
    if (cam.buf) {
        const float *dp = cam.dots + (size_t)blockIdx.z * 4;
        dots[0] = dp[0]; dots[1] = dp[1]; dots[2] = dp[2]; dots[3] = dp[3];
    } else {
        dots[0] = cam.odots[0]; dots[1] = cam.odots[1]; dots[2] = cam.odots[2]; dots[3] = cam.odots[3];
    }
    const int x = (int)blockIdx.x * 64 + lane;
    if (x >= tg.width) return;
    const float sx = tg.fovI * ((float)x - tg.half_w);
    int4 *out = reinterpret_cast<int4 *>(bf.recs) + (long long)blockIdx.z * bf.frame_stride + x;
    for (int rr = 0; rr < NT_BOXROWS; ++rr) {
        const int y = (int)blockIdx.y * NT_BOXROWS + rr;
        if (y >= tg.height) return;
        const float sy = tg.fovI * ((float)y - tg.half_h);
        float sq = 0.0f;
        for (int j = 0; j < n; ++j) {
            const float v = (c[3 * n + j] + c[n + j] * sx) - c[2 * n + j] * sy;
            dir[j * 64] = v;
            sq = j == 0 ? v * v : sq + v * v;
        }
        const bool maybe = box_may_hit(n, dots, sx, sy, sq);
        int face = -1, side = -1;
        float fdist = FLT_MAX;
        if (__builtin_amdgcn_ballot_w64(maybe) != 0ull) {
            const float len = sqrtf(sq);
            for (int j = 0; j < n; ++j) dir[j * 64] = dir[j * 64] / len;
            bool done = false;
            float aK = 0.0f, bK = 1.0f, oK = 0.0f;
            bool any = false;
            for (int i = 0; i < n; ++i) {
                const float di = dir[i * 64];
                const float oi = c[i];
                const float num = (di < 0.0f ? 1.0f : -1.0f) - oi;
                const bool pre = maybe && ((num > 0.0f && di > 0.0f) || (num < 0.0f && di < 0.0f));
                const float a = fabsf(num), bb = fabsf(di);
                if (pre && (!any || a * bK > aK * bb)) { aK = a; bK = bb; oK = oi; any = true; }
            }
            const float mu = 1e-4f * (1.0f + fabsf(oK));
            const float aKm = (aK - mu) * (1.0f - 1e-6f);
            for (int i = 0; i < n; ++i) {
                const float di = dir[i * 64];
                const float oi = c[i];
                const float num = (di < 0.0f ? 1.0f : -1.0f) - oi;
                const bool pre = maybe && ((num > 0.0f && di > 0.0f) || (num < 0.0f && di < 0.0f));
                const bool tie = pre && !done && !(fabsf(num) * bK < fabsf(di) * aKm);
                if (!tie) continue;
                const float dist = num / di;
                bool ok = dist > 0.0f;
                for (int j = 0; j < n; ++j) {
                    if (j != i) {
                        const float p = dir[j * 64] * dist + c[j];
                        ok = ok && !(fabsf(p) > (1.0f + NT_FUZZ));
                    }
                }
                if (ok) {
                    done = true;
                    // `if(dist >= cutoff) return 0` with cutoff = FLT_MAX (tracer.hpp:142): a miss
                    if (!(dist >= FLT_MAX)) { face = i; side = di < 0.0f ? 1 : 0; fdist = dist; }
                }
            }
        }
        out[(long long)y * tg.width] = make_int4(__float_as_int(fdist), face, side, 0);
    }
}

// Face lines at run-time n, behind box_hits_var: one lane a pixel reads its record and those of its four neighbours inside the
// image from `bf.recs` ([frame][height][width]), applies the rule (ntracer_hip.h; box_line_pair of nt_boxhits.hpp) and
// writes the mask byte -- or (DRAW) re-forms its own ray for the plain colour, |d_face| or the background from d_0, blends and
// emits.  A block: 64 x 4 pixels of frame blockIdx.z; the camera's rows staged in LDS as box_kernel_var stages them.
template <bool DRAW>
__global__ __launch_bounds__(256) void box_lines_var(NtCamera cam, NtTarget tg, NtBoxFaces bf) {
    extern __shared__ float lds_vec[];    // [4][n] camera rows (broadcast reads)
    if (nt_aborted(tg)) return;           // (the whole block leaves, ahead of the barrier)
    const int tid = (int)threadIdx.x;
    const int n = cam.n;
    if (DRAW) {
        const float *src = cam.buf ? cam.buf + (size_t)blockIdx.z * 4 * n : nullptr;
        for (int k = tid; k < 4 * n; k += 256) lds_vec[k] = src ? src[k] : cam.inl[k];
        __syncthreads();
    }
    const int x = (int)blockIdx.x * 64 + (tid & 63), y = (int)blockIdx.y * 4 + (tid >> 6);
    if (x >= tg.width || y >= tg.height) return;
    const int4 *fr = reinterpret_cast<const int4 *>(bf.recs) + (long long)blockIdx.z * bf.frame_stride;
    const long long at = (long long)y * tg.width + x;
    const int4 rec = fr[at];
    int m = 0;
    if (rec.y >= 0) {
        const float pd = __int_as_float(rec.x);
        for (int k = 0; k < 4; ++k) {
            const int qx = x + (k == 0 ? -1 : (k == 1 ? 1 : 0));
            const int qy = y + (k == 2 ? -1 : (k == 3 ? 1 : 0));
            if (qx < 0 || qy < 0 || qx >= tg.width || qy >= tg.height) continue;
            const int4 q = fr[(long long)qy * tg.width + qx];
            m |= box_line_pair(pd, 2 * rec.y + rec.z, __int_as_float(q.x), q.y < 0 ? -1 : 2 * q.y + q.z);
        }
        m &= bf.kinds;
    }
    if (!DRAW) {
        bf.mask[((long long)blockIdx.z * tg.height + y) * tg.width + x] = (uint8_t)m;
        return;
    }
    const float *c = lds_vec;             // origin, right, up, forward
    const float sx = tg.fovI * ((float)x - tg.half_w);
    const float sy = tg.fovI * ((float)y - tg.half_h);
    const int pick = rec.y >= 0 ? rec.y : 0;
    float sq = 0.0f, vp = 0.0f;
    for (int j = 0; j < n; ++j) {
        const float v = (c[3 * n + j] + c[n + j] * sx) - c[2 * n + j] * sy;
        sq = j == 0 ? v * v : sq + v * v;
        vp = j == pick ? v : vp;
    }
    const float xval = vp / sqrtf(sq);
    PixelRef pr;
    pr.x = x;
    pr.y = y;
    pr.offset = (long long)blockIdx.z * tg.frame_stride + (long long)y * tg.pitch + (long long)x * tg.bpp;
    pr.hit_index = 0;
    pr.valid = true;
    float r, g, b;
    if (rec.y >= 0) {
        const float shade = fabsf(xval);
        r = shade * 1.0f;
        g = shade * 0.5f;
        b = shade * 0.5f;
    } else {
        box_background(xval, r, g, b);
    }
    const float keep = 1.0f - bf.strength;
    float p[3] = {r, g, b};
    for (int k = 0; k < 3; ++k) {
        float v = p[k] > 0.0f ? p[k] : 0.0f;
        v = v < 1.0f ? v : 1.0f;
        p[k] = m != 0 ? (v * keep) + (bf.color[k] * bf.strength) : v;
    }
    emit_pixel(tg, pr, p[0], p[1], p[2]);
}

// Face shading at run-time n (nt_boxshade.hpp has the compile-time-N kernels and the rule's one copy), behind box_hits_var:
// box_lines_var's shape -- one lane a pixel reads its record from `bs.recs`, with LINES those of its four neighbours inside the
// image too -- re-forms its own ray exactly as box_hits_var formed it, d_k = v_k / |v|, for the shade, the background and the
// tint sum, and hands over to box_shade_emit.  A block: 64 x 4 pixels of frame blockIdx.z; the camera's rows and the face-colour
// table staged in LDS once a block.
static_assert(sizeof(NtCamera) + sizeof(NtTarget) + sizeof(NtBoxShade) <= 4096, "box_shaded_var's arguments fit the kernel argument segment");
template <bool LINES>
__global__ __launch_bounds__(256) void box_shaded_var(NtCamera cam, NtTarget tg, NtBoxShade bs) {
    extern __shared__ float lds_vec[];    // [4][n] camera rows (broadcast reads), then [2 n][3] the table
    if (nt_aborted(tg)) return;           // (the whole block leaves, ahead of the barrier)
    const int tid = (int)threadIdx.x;
    const int n = cam.n;
    {
        const float *src = cam.buf ? cam.buf + (size_t)blockIdx.z * 4 * n : nullptr;
        for (int k = tid; k < 4 * n; k += 256) lds_vec[k] = src ? src[k] : cam.inl[k];
    }
    float *tab = lds_vec + 4 * n;
    box_shade_stage(bs, n, tid, 256, tab);
    __syncthreads();
    const int x = (int)blockIdx.x * 64 + (tid & 63), y = (int)blockIdx.y * 4 + (tid >> 6);
    if (x >= tg.width || y >= tg.height) return;
    const int4 *fr = reinterpret_cast<const int4 *>(bs.recs) + (long long)blockIdx.z * bs.frame_stride;
    const int4 rec = fr[(long long)y * tg.width + x];
    const float pd = __int_as_float(rec.x);
    const int code = rec.y >= 0 ? 2 * rec.y + rec.z : -1;
    int m = 0;
    if (LINES && rec.y >= 0) {
        for (int k = 0; k < 4; ++k) {
            const int qx = x + (k == 0 ? -1 : (k == 1 ? 1 : 0));
            const int qy = y + (k == 2 ? -1 : (k == 3 ? 1 : 0));
            if (qx < 0 || qy < 0 || qx >= tg.width || qy >= tg.height) continue;
            const int4 q = fr[(long long)qy * tg.width + qx];
            m |= box_line_pair(pd, code, __int_as_float(q.x), q.y < 0 ? -1 : 2 * q.y + q.z);
        }
        m &= bs.kinds;
    }
    const float *c = lds_vec;             // origin, right, up, forward
    const float sx = tg.fovI * ((float)x - tg.half_w);
    const float sy = tg.fovI * ((float)y - tg.half_h);
    const int pick = rec.y >= 0 ? rec.y : 0;
    float sq = 0.0f, vp = 0.0f;
    for (int j = 0; j < n; ++j) {
        const float v = (c[3 * n + j] + c[n + j] * sx) - c[2 * n + j] * sy;
        sq = j == 0 ? v * v : sq + v * v;
        vp = j == pick ? v : vp;
    }
    const float len = sqrtf(sq);
    const float xval = vp / len;
    float s = 0.0f;
    if (rec.y >= 0 && bs.cue_on && bs.cue.tint)
        s = box_shade_tint_sum(bs, n, pd, [&](int k) { return ((c[3 * n + k] + c[n + k] * sx) - c[2 * n + k] * sy) / len; }, [&](int k) { return c[k]; });
    box_shade_emit(tg, bs, tab, box_shade_pixel(tg, x, y), code, pd, xval, s, m);
}

// --------------------------------------------------------------------------------------
// A render through a lens (nt_lens.hpp) on the ray-colour kernels above: every scene the packet walk does not take.  The table
// and the frame's camera are expanded into the unnormalised directions v[j] = (fwd[j] * sz + right[j] * sx) - up[j] * sy of a
// band of whole rows -- run-time n, one lane a pixel, the blocks striding -- which the rays_* kernels then take with the camera's
// origin shared; a masked pixel gets a zero direction there, whose colour is unspecified, and (0, 0, 0) from lens_mask_fill
// afterwards.  The ray entry points themselves pay nothing for it.
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lens_expand(const float *table, const float *cam, int n, long long first, long long count, float *out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const float *e = table + (first + i) * 3;
        const float sx = e[0], sy = e[1], sz = e[2];
        float *v = out + i * n;
        if (lens_masked(sx, sy, sz)) {
            for (int j = 0; j < n; ++j) v[j] = 0.0f;
        } else {
            for (int j = 0; j < n; ++j) v[j] = (cam[3 * n + j] * sz + cam[n + j] * sx) - cam[2 * n + j] * sy;
        }
    }
}

__global__ __launch_bounds__(256) void lens_mask_fill(const float *table, long long first, long long count, NtTarget tg) {
    if (nt_aborted(tg)) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const float *e = table + (first + i) * 3;
        if (lens_masked(e[0], e[1], e[2])) emit_pixel(tg, rays_pixel(tg, i), 0.0f, 0.0f, 0.0f);
    }
}

// --------------------------------------------------------------------------------------
// A render under the parallel projection (nt_parallel.hpp) on the ray-colour kernels above: every scene the packet walk does
// not take.  Pixels [first, first + count) of a view `width` wide -- a band of whole rows -- get their origin
// o'[j] = (origin[j] + right[j] * sx) - up[j] * sy into out[i][n] and the unnormalised forward row into out[count + i][n]:
// run-time n, one lane a pixel, the blocks striding.  The rays_* kernels then take one origin a ray.
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void parallel_expand(const float *cam, int n, int width, float k, float half_w, float half_h, long long first,
                                                       long long count, float *out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const long long p = first + i;
        const int y = (int)(p / width), x = (int)(p - (long long)y * width);
        const float sx = k * ((float)x - half_w);
        const float sy = k * ((float)y - half_h);
        float *o = out + i * n, *v = out + (count + i) * n;
        for (int j = 0; j < n; ++j) {
            o[j] = (cam[j] + cam[n + j] * sx) - cam[2 * n + j] * sy;
            v[j] = cam[3 * n + j];
        }
    }
}

// --------------------------------------------------------------------------------------
// Ambient occlusion (nt_ao.hpp) on the closest-hit query kernels above: every scene ao_kernel does not take.
// ao_expand writes the K rays of pixels [first, first + pixels) of the launch -- one lane a ray, ray k of pixel i at i * K + k,
// run-time n, the blocks striding -- from the pixel's record and normal rows: origin o' = no + nd * b, direction +-t_k, the window
// [0, radius] and the primary hit as the skip target, by ao_kernel's operations in ao_kernel's order (d is primary_dir's, formed
// on the fly: the same operands give the same bits twice).  A pixel without an opaque hit gets rays with an inverted window,
// which end in the first leaf they reach and whose answers nobody reads.  The query launch then answers all of them, and
// ao_reduce, one lane a pixel, counts item >= 0 && dist <= radius over each K records.
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ao_expand(NtTarget tg, NtAo ao, NtAoRays ar, int n) {
    const long long rays = ar.pixels * ao.count;
    const long long per_frame = (long long)tg.width * tg.height;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < rays; i += (long long)gridDim.x * 256) {
        const long long pl = i / ao.count;
        const int k = (int)(i - pl * ao.count);
        const long long pix = ar.first + pl;
        const int4 rec = reinterpret_cast<const int4 *>(ao.recs)[pix];
        const float *t = ao.dirs + (size_t)k * n;
        float *o = ar.origins + i * n, *v = ar.directions + i * n;
        ar.t_near[i] = 0.0f;
        if (rec.y < 0) {
            for (int j = 0; j < n; ++j) { o[j] = 0.0f; v[j] = t[j]; }
            ar.t_far[i] = -1.0f;
            ar.skip_item[i] = -1;
            ar.skip_lane[i] = -1;
            continue;
        }
        const int frame = (int)(pix / per_frame);
        const int rem = (int)(pix - (long long)frame * per_frame);
        const int y = rem / tg.width, x = rem - y * tg.width;
        const float *c = ao.cams + (size_t)frame * 4 * n;
        const float sx = tg.fovI * ((float)x - tg.half_w);
        const float sy = tg.fovI * ((float)y - tg.half_h);
        float sq = 0.0f;
        for (int j = 0; j < n; ++j) {
            const float u = (c[3 * n + j] + c[n + j] * sx) - c[2 * n + j] * sy;
            sq = j == 0 ? u * u : sq + u * u;
        }
        const float len = sqrtf(sq);
        const float *no = ao.normal_origin + pix * n, *nd = ao.normal_dir + pix * n;
        float dn = 0.0f, s = 0.0f;
        for (int j = 0; j < n; ++j) {
            const float dj = ((c[3 * n + j] + c[n + j] * sx) - c[2 * n + j] * sy) / len;
            dn = j == 0 ? dj * nd[j] : dn + dj * nd[j];
            s = j == 0 ? nd[j] * t[j] : s + nd[j] * t[j];
        }
        const float side = -dn;
        const float b = side < 0.0f ? -ao.bias : ao.bias;
        const bool flip = (s < 0.0f) != (side < 0.0f);
        for (int j = 0; j < n; ++j) {
            o[j] = no[j] + nd[j] * b;
            v[j] = flip ? -t[j] : t[j];
        }
        ar.t_far[i] = ao.radius;
        ar.skip_item[i] = rec.y;
        ar.skip_lane[i] = rec.z;
    }
}

__global__ __launch_bounds__(256) void ao_reduce(NtTarget tg, NtAo ao, NtAoRays ar) {
    if (nt_aborted(tg)) return;
    for (long long pl = (long long)blockIdx.x * 256 + threadIdx.x; pl < ar.pixels; pl += (long long)gridDim.x * 256) {
        const long long pix = ar.first + pl;
        int blocked = -1;
        if (reinterpret_cast<const int4 *>(ao.recs)[pix].y >= 0) {
            const int4 *r = reinterpret_cast<const int4 *>(ar.results) + pl * ao.count;
            blocked = 0;
            for (int k = 0; k < ao.count; ++k) {
                const int4 e = r[k];
                if (e.y >= 0 && __int_as_float(e.x) <= ao.radius) ++blocked;
            }
        }
        ao.blocked[pix] = blocked;
    }
}

// Drawing: pixel = P * (1 - strength * blocked / K) through emit_pixel, P the base frame (three big-endian floats a pixel, clamped
// to [0, 1] by the packer that wrote them), blocked = -1 counting as 0.  adaptive_flag's geometry: a block is 64 pixels of four
// rows, one wave a row, so the shared dword stores of 3- and 6-byte pixels find their aligned groups; the grid's z is the frame.
__global__ __launch_bounds__(256) void ao_apply(const uint32_t *base, const int *blocked, int count, float strength, NtTarget tg) {
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * 64 + (tid & 63);
    const int y = (int)blockIdx.y * 4 + (tid >> 6);
    if (y >= tg.height || x >= tg.width) return;
    const long long pix = ((long long)blockIdx.z * tg.height + y) * tg.width + x;
    const uint32_t *p = base + pix * 3;
    const int bl = blocked[pix];
    const float a = bl < 0 ? 0.0f : (float)bl / (float)count;
    const float f = 1.0f - strength * a;
    PixelRef pr;
    pr.valid = true;
    pr.hit_index = 0;
    pr.x = x;
    pr.y = y;
    pr.offset = (long long)blockIdx.z * tg.frame_stride + (long long)y * tg.pitch + (long long)x * tg.bpp;
    emit_pixel(tg, pr, __uint_as_float(bswap32(p[0])) * f, __uint_as_float(bswap32(p[1])) * f, __uint_as_float(bswap32(p[2])) * f);
}

// --------------------------------------------------------------------------------------
// Outlines (nt_outline.hpp) behind a primary-hit pass with normal rows: every scene the packet route does not
// take.  outline_mark, one lane a pixel at run-time n in ao_apply's geometry (64 pixels of four rows a block, the grid's z the
// frame: no division finds a pixel, and the abort word is read once a block), applies outline_pair to the
// pixel's record and those of its four neighbours within its own frame; the dot products read the two normal rows as stored.
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void outline_mark(NtTarget tg, NtOutline ol, int n) {
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * 64 + (tid & 63);
    const int y = (int)blockIdx.y * 4 + (tid >> 6);
    if (y >= tg.height || x >= tg.width) return;
    const long long pix = ((long long)blockIdx.z * tg.height + y) * tg.width + x;
    const int4 *recs = reinterpret_cast<const int4 *>(ol.recs);
    const int4 rec = recs[pix];
    int m = 0;
    if (rec.y >= 0) {
        const float *a = ol.normal_dir + pix * n;
        for (int k = 0; k < 4; ++k) {
            const int qx = x + (k == 0 ? -1 : (k == 1 ? 1 : 0));
            const int qy = y + (k == 2 ? -1 : (k == 3 ? 1 : 0));
            if (qx < 0 || qy < 0 || qx >= tg.width || qy >= tg.height) continue;
            const long long qi = pix + (long long)(qy - y) * tg.width + (qx - x);
            const float *b = ol.normal_dir + qi * n;
            m |= outline_pair(rec, recs[qi], ol.cc, ol.depth_gap, [&](float &c, float &la, float &lb) {
                c = a[0] * b[0];
                la = a[0] * a[0];
                lb = b[0] * b[0];
                for (int j = 1; j < n; ++j) {
                    c = c + a[j] * b[j];
                    la = la + a[j] * a[j];
                    lb = lb + b[j] * b[j];
                }
            });
        }
    }
    ol.mask[pix] = (uint8_t)m;
}

// Drawing: a pixel whose mask byte is set becomes (P * (1 - strength)) + (color * strength) through emit_pixel, every other pixel
// P, the base frame (three big-endian floats a pixel, clamped to [0, 1] by the packer that wrote them).  ao_apply's geometry.
__global__ __launch_bounds__(256) void outline_apply(const uint32_t *base, NtOutline ol, NtTarget tg) {
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * 64 + (tid & 63);
    const int y = (int)blockIdx.y * 4 + (tid >> 6);
    if (y >= tg.height || x >= tg.width) return;
    const long long pix = ((long long)blockIdx.z * tg.height + y) * tg.width + x;
    const uint32_t *p = base + pix * 3;
    float c[3] = {__uint_as_float(bswap32(p[0])), __uint_as_float(bswap32(p[1])), __uint_as_float(bswap32(p[2]))};
    if (ol.mask[pix] != 0) {
        const float keep = 1.0f - ol.strength;
        for (int k = 0; k < 3; ++k) c[k] = (c[k] * keep) + (ol.color[k] * ol.strength);
    }
    PixelRef pr;
    pr.valid = true;
    pr.hit_index = 0;
    pr.x = x;
    pr.y = y;
    pr.offset = (long long)blockIdx.z * tg.frame_stride + (long long)y * tg.pitch + (long long)x * tg.bpp;
    emit_pixel(tg, pr, c[0], c[1], c[2]);
}

// --------------------------------------------------------------------------------------
// Depth cues (nt_cue.hpp) behind a primary-hit pass: every scene the packet route does not take.  One lane a
// pixel at run-time n in ao_apply's geometry (64 pixels of four rows a block, the grid's z the frame); cue_pixel and cue_blend are
// nt_cue.hpp's.  The pixel's direction is primary_dir's, formed on the fly as ao_expand forms it: the same operands give the same
// bits twice.
// --------------------------------------------------------------------------------------
__device__ __forceinline__ void cue_pixel_var(const NtTarget &tg, const NtCue &cu, int n, int x, int y, long long pix, float &f, float &g) {
    const int4 rec = reinterpret_cast<const int4 *>(cu.recs)[pix];
    const float *c = cu.cams + (size_t)blockIdx.z * 4 * n;
    const float sx = tg.fovI * ((float)x - tg.half_w);
    const float sy = tg.fovI * ((float)y - tg.half_h);
    float len = 1.0f;
    if (rec.y >= 0 && cu.tint) {
        float sq = 0.0f;
        for (int j = 0; j < n; ++j) {
            const float u = (c[3 * n + j] + c[n + j] * sx) - c[2 * n + j] * sy;
            sq = j == 0 ? u * u : sq + u * u;
        }
        len = sqrtf(sq);
    }
    cue_pixel(cu, rec, n, [&](int k) { return ((c[3 * n + k] + c[n + k] * sx) - c[2 * n + k] * sy) / len; }, [&](int k) { return c[k]; }, f, g);
}

__global__ __launch_bounds__(256) void cue_factors(NtTarget tg, NtCue cu, int n) {
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * 64 + (tid & 63);
    const int y = (int)blockIdx.y * 4 + (tid >> 6);
    if (y >= tg.height || x >= tg.width) return;
    const long long pix = ((long long)blockIdx.z * tg.height + y) * tg.width + x;
    float f, g;
    cue_pixel_var(tg, cu, n, x, y, pix, f, g);
    reinterpret_cast<float2 *>(cu.factors)[pix] = make_float2(f, g);
}

// Drawing: the base frame's pixel P (three big-endian floats, clamped to [0, 1] by the packer that wrote them) through cue_blend
// and emit_pixel.
__global__ __launch_bounds__(256) void cue_apply(const uint32_t *base, NtCue cu, NtTarget tg, int n) {
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * 64 + (tid & 63);
    const int y = (int)blockIdx.y * 4 + (tid >> 6);
    if (y >= tg.height || x >= tg.width) return;
    const long long pix = ((long long)blockIdx.z * tg.height + y) * tg.width + x;
    float f, g;
    cue_pixel_var(tg, cu, n, x, y, pix, f, g);
    const uint32_t *p = base + pix * 3;
    float c[3] = {__uint_as_float(bswap32(p[0])), __uint_as_float(bswap32(p[1])), __uint_as_float(bswap32(p[2]))};
    cue_blend(cu, f, g, c);
    PixelRef pr;
    pr.valid = true;
    pr.hit_index = 0;
    pr.x = x;
    pr.y = y;
    pr.offset = (long long)blockIdx.z * tg.frame_stride + (long long)y * tg.pitch + (long long)x * tg.bpp;
    emit_pixel(tg, pr, c[0], c[1], c[2]);
}

// --------------------------------------------------------------------------------------
// Adaptive supersampling at run-time n (n = 11..64 -- BoxScene: 25..64 -- and every n under NTRACER_FORCE_VAR=1): the refine
// kernels of nt_adaptive.hpp on composite_color_var / composite_color_var_t and on rays_box_var's evaluation.  One lane a
// flagged pixel, one wave a block, the blocks striding over the list.
// --------------------------------------------------------------------------------------
// sample k = j * s + i of the pixel becomes the current ray: hits_set_ray_var's operations on the s W x s H view
__device__ __forceinline__ void refine_set_ray_var(const VarCtx &cx, const NtRefine &rf, const RefinePixel &p, int k) {
    const int n = cx.n, lane = cx.lane;
    const int j = k / rf.s, i = k - j * rf.s;
    const float *c = rf.cams + (size_t)p.frame * 4 * n;
    const float sx = rf.fovI * ((float)(rf.s * p.x + i) - rf.half_w);
    const float sy = rf.fovI * ((float)(rf.s * p.y + j) - rf.half_h);
    float sq = 0.0f;
    for (int q = 0; q < n; ++q) {
        const float v = (c[3 * n + q] + c[n + q] * sx) - c[2 * n + q] * sy;
        cx.L.dv[q * 64 + lane] = v;
        sq = q == 0 ? v * v : sq + v * v;
    }
    const float len = sqrtf(sq);
    for (int q = 0; q < n; ++q) {
        const float dk = cx.L.dv[q * 64 + lane] / len;
        cx.L.dv[q * 64 + lane] = dk;
        cx.L.ray[q * 64 + lane] = make_float2(c[q], dk != 0.0f ? 1.0f / dk : __int_as_float(0x7fc00000));
    }
}

__global__ __launch_bounds__(64) void refine_color_var(NtCompositeDev sc, NtRefine rf, NtTarget tg, int n) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    const VarCtx cx = {sc, L, w, n, lane};
    const long long count = (long long)*rf.count;
    const int ss = rf.s * rf.s;
    for (long long base = (long long)blockIdx.x * 64; base < count; base += (long long)gridDim.x * 64) {
        if (nt_aborted(tg)) return;
        if (base + lane >= count) continue;
        const RefinePixel p = refine_pixel(tg, rf, base + lane);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < ss; ++k) {
            refine_set_ray_var(cx, rf, p, k);
            const Color3 col = composite_color_var(cx);
            refine_add(acc, k, col.r, col.g, col.b);
        }
        refine_emit(tg, rf, p, acc);
    }
}

template <bool ALIAS>
__global__ __launch_bounds__(64) void refine_color_var_t(NtCompositeDev sc, NtRefine rf, NtTarget tg, int n) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    VarLds L;
    WaveLds w;
    var_lds_carve(reinterpret_cast<char *>(lds_raw), n, sc.stack_depth, L, w);
    const VarCtx cx = {sc, L, w, n, lane};
    const long long slot = (long long)blockIdx.x * 64 + lane;
    Checked ck;
    ck.bits = sc.checked + slot;
    ck.stride = sc.checked_lanes;
    ck.words = sc.checked_words;
    ck.n_batches = sc.n_batches;
    ck.n_triangles = sc.n_triangles;
    VarFrames fr;
    var_frames(fr, sc, slot, n);
    const long long count = (long long)*rf.count;
    const int ss = rf.s * rf.s;
    for (long long base = (long long)blockIdx.x * 64; base < count; base += (long long)gridDim.x * 64) {
        if (nt_aborted(tg)) return;
        if (base + lane >= count) continue;
        const RefinePixel p = refine_pixel(tg, rf, base + lane);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < ss; ++k) {
            refine_set_ray_var(cx, rf, p, k);
            const Color3 col = composite_color_var_t<ALIAS>(cx, fr, ck, sc.tframe_count);
            refine_add(acc, k, col.r, col.g, col.b);
        }
        refine_emit(tg, rf, p, acc);
    }
}

// BoxScene: rays_box_var's evaluation of the ray whose direction and origin lie in LDS as dir[j * 64], org[j * 64]
__device__ __forceinline__ void refine_box_color_var(const float *dir, const float *org, int n, float &cr, float &cg, float &cb) {
    bool done = false;
    float shade = 0.0f;
    float aK = 0.0f, bK = 1.0f, oK = 0.0f;
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const float di = dir[i * 64];
        const float oi = org[i * 64];
        const float num = (di < 0.0f ? 1.0f : -1.0f) - oi;
        const bool pre = (num > 0.0f && di > 0.0f) || (num < 0.0f && di < 0.0f);
        const float a = fabsf(num), bb = fabsf(di);
        if (pre && (!any || a * bK > aK * bb)) { aK = a; bK = bb; oK = oi; any = true; }
    }
    const float mu = 1e-4f * (1.0f + fabsf(oK));
    const float aKm = (aK - mu) * (1.0f - 1e-6f);
    for (int i = 0; i < n; ++i) {
        const float di = dir[i * 64];
        const float oi = org[i * 64];
        const float s = di < 0.0f ? 1.0f : -1.0f;
        const float num = s - oi;
        const bool pre = (num > 0.0f && di > 0.0f) || (num < 0.0f && di < 0.0f);
        const bool tie = pre && !done && !(fabsf(num) * bK < fabsf(di) * aKm);
        if (!tie) continue;
        const float dist = num / di;
        bool ok = dist > 0.0f;
        for (int j = 0; j < n; ++j) {
            if (j != i) {
                const float p = dir[j * 64] * dist + org[j * 64];
                ok = ok && !(fabsf(p) > (1.0f + NT_FUZZ));
            }
        }
        if (ok) {
            done = true;
            if (dist >= FLT_MAX) shade = -1.0f;
            else {
                const float sine = di * s;
                shade = sine <= 0.0f ? -sine : 0.0f;
            }
        }
    }
    if (done && shade >= 0.0f) {
        cr = shade * 1.0f;
        cg = shade * 0.5f;
        cb = shade * 0.5f;
    } else {
        box_background(dir[0], cr, cg, cb);
    }
}

__global__ __launch_bounds__(64) void refine_box_var(NtRefine rf, NtTarget tg, int n) {
    extern __shared__ float lds_vec[];    // [n][64] direction, [n][64] origin
    const int lane = (int)threadIdx.x;
    float *dir = lds_vec + lane;          // dir[j] at dir[j * 64]
    float *org = lds_vec + (size_t)n * 64 + lane;
    const long long count = (long long)*rf.count;
    const int ss = rf.s * rf.s;
    for (long long base = (long long)blockIdx.x * 64; base < count; base += (long long)gridDim.x * 64) {
        if (nt_aborted(tg)) return;
        if (base + lane >= count) continue;
        const RefinePixel p = refine_pixel(tg, rf, base + lane);
        const float *c = rf.cams + (size_t)p.frame * 4 * n;
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < ss; ++k) {
            const int sj = k / rf.s, si = k - sj * rf.s;
            const float sx = rf.fovI * ((float)(rf.s * p.x + si) - rf.half_w);
            const float sy = rf.fovI * ((float)(rf.s * p.y + sj) - rf.half_h);
            float sq = 0.0f;
            for (int j = 0; j < n; ++j) {
                const float v = (c[3 * n + j] + c[n + j] * sx) - c[2 * n + j] * sy;
                dir[j * 64] = v;
                org[j * 64] = c[j];
                sq = j == 0 ? v * v : sq + v * v;
            }
            const float len = sqrtf(sq);
            for (int j = 0; j < n; ++j) dir[j * 64] = dir[j * 64] / len;
            float cr, cg, cb;
            refine_box_color_var(dir, org, n, cr, cg, cb);
            refine_add(acc, k, cr, cg, cb);
        }
        refine_emit(tg, rf, p, acc);
    }
}

#undef VO
#undef VD

}  // namespace

// The camera table of a multi-frame launch, from pinned host memory (which the device reads in place) to device memory:
// a kernel on the launch stream instead of a copy-engine transfer the next kernel would have to wait for across queues.
namespace {
__global__ __launch_bounds__(256) void upload_kernel(const float *__restrict__ src, float *__restrict__ dst, int count) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i < count) dst[i] = src[i];
}

// --------------------------------------------------------------------------------------
// What the nt_launch_* below share.  The guards of a run-time-n launch, each with its message and its code in one place ...
// --------------------------------------------------------------------------------------
int var_dim_check(int n) {
    if (n >= 3 && n <= NT_DEV_MAX_DIM) return 0;
    snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "unsupported dimension %d", n);
    return -2;
}

// A walk kernel is about to be launched: the dimension check, the LDS the kernel carves (var_lds_bytes), refused beyond the
// 160 KiB of a CU, and beyond the 64 KiB a kernel gets unasked the attribute that admits it.  0 and `lds`; -2 (dimension) or
// -1 (too deep) and the launch error.
int var_walk_ready(int n, const NtCompositeDev &sc, const void *kernel, size_t &lds) {
    if (const int r = var_dim_check(n)) return r;
    lds = var_lds_bytes(sc.stack_depth, n);
    if (lds > 160 * 1024) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "scene too deep for the LDS budget (n %d, depth %d)", n, sc.stack_depth);
        return -1;
    }
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return 0;
}

// the kernels that shade through sc.tframes: the `checked` columns must be there, a block's worth at least
int var_frames_check(int n, const NtCompositeDev &sc) {
    if (n >= 3 && n <= NT_DEV_MAX_DIM && sc.checked && sc.checked_lanes >= 64) return 0;
    snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "run-time-n transparency kernel: bad launch (n %d)", n);
    return -2;
}

int no_checked_scratch() {
    snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: transparent scene without the checked-list scratch");
    return -1;
}

// ... the kernel of a <true> / <false> pair that sc.alias_normals picks ...
template <typename K>
const void *alias_kernel(const NtCompositeDev &sc, K *aliased, K *clean) {
    return reinterpret_cast<const void *>(sc.alias_normals ? aliased : clean);
}

// ... and the grids: as many one-wave blocks as the `checked` scratch has lane columns for, `want` at the most; the blocks of
// 256 lanes of a kernel that strides over `count` items (none: there is nothing to launch)
long long checked_blocks(const NtCompositeDev &sc, long long want = LLONG_MAX) {
    const long long have = sc.checked_lanes / 64;
    return want < have ? want : have;
}

long long stride_blocks(long long count) {
    const long long blocks = (count + 255) / 256;
    return blocks > NT_RAYS_MAX_BLOCKS ? NT_RAYS_MAX_BLOCKS : blocks;
}

// The routes that have compile-time-N kernels alone (a lens, the parallel projection, ambient occlusion, outlines): f is
// `[&](auto N) { return nt_X_fixed<N>(...); }`.  Any other n, and every n under force_var: "internal: <none> at run-time n" --
// the host sends those scenes another way.
template <typename F>
int launch_fixed_only(const NtLaunchInfo &li, const char *none, const char *what, F &&f) {
    int r = 0;
    if (!nt_dispatch_dim<3, NT_DEV_MAX_FIXED>(li.force_var ? 0 : li.n, r, f)) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: %s at run-time n (n %d)", none, li.n);
        return -1;
    }
    if (r) return r;
    return finish_launch(what);
}
}  // namespace

int nt_launch_upload(void *stream, const float *src_pinned, float *dst, int count) {
    hipLaunchKernelGGL(upload_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src_pinned, dst, count);
    return finish_launch("camera upload");
}

// the box filter of a supersampled render (nt_resolve.hpp)
int nt_launch_resolve(int s, void *stream, const void *samples, long long frame_stride_bytes, long long pitch_bytes, int nframes, const NtTarget &tg) {
    return launch_resolve_any(s, (hipStream_t)stream, samples, frame_stride_bytes, pitch_bytes, nframes, tg);
}

int nt_launch_box(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg) {
    int r;          // (launch_box_fixed returns 0 and nothing else)
    if (!nt_dispatch_dim<3, NT_DEV_MAX_FIXED_BOX>(li.force_var ? 0 : li.n, r, [&](auto N) { return nt_box_fixed<decltype(N)::value>(li, cam, tg); })) {
        // packed plain RGB of <= 10 bits in one aligned dword: the rows kernel (codes + lean loops), if its n-vectors fit LDS
        const size_t lds_rows = ((size_t)li.n * 256 + (size_t)4 * li.n + 4) * sizeof(float);
        if (!tg.colors_out && tg.plain_bits != 0u && tg.plain_bits <= 10u && tg.bpp == 4 && tg.aligned4 && lds_rows <= 160 * 1024 &&
            li.box_var_rows) {
            const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.row_count + 31) / 32), (unsigned)li.nframes);
            if (lds_rows > 64 * 1024)
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(box_rows_kernel_var), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rows);
            hipLaunchKernelGGL(box_rows_kernel_var, grid, dim3(256), lds_rows, (hipStream_t)li.stream, cam, tg);
        } else {
            dim3 grid;
            grid_for(tg, 64, 4, li.nframes, grid);
            const size_t lds = ((size_t)li.n * 256 + (size_t)4 * li.n) * sizeof(float);
            hipLaunchKernelGGL(box_kernel_var, grid, dim3(256), lds, (hipStream_t)li.stream, cam, tg);
        }
    }
    return finish_launch("box kernel launch");
}

// BoxScene hit buffers and face lines (nt_boxhits.hpp): the fixed-n launcher of the scene's dimension, or the run-time-n
// kernels above -- box_hits_var into bf.recs and, for the mask or the drawing, box_lines_var behind it.  Kept apart from
// nt_launch_box: this is no route of a plain render.
int nt_launch_box_faces(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg, const NtBoxFaces &bf) {
    int r = var_dim_check(li.n);
    if (r) return r;
    if (!nt_dispatch_dim<3, NT_DEV_MAX_FIXED_BOX>(li.force_var ? 0 : li.n, r, [&](auto N) { return nt_box_faces<decltype(N)::value>(li, cam, tg, bf); })) {
        if (!bf.recs || (bf.mode == NT_BOX_FACES_MASK && !bf.mask) ||
            (bf.mode == NT_BOX_FACES_DRAW && (tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1 || tg.colors_out))) {
            snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a face-line launch at run-time n without its records, or not for whole frames");
            return -1;
        }
        hipStream_t st = (hipStream_t)li.stream;
        const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + NT_BOXROWS - 1) / NT_BOXROWS), (unsigned)li.nframes);
        hipLaunchKernelGGL(box_hits_var, grid, dim3(64), ((size_t)li.n * 64 + (size_t)4 * li.n) * sizeof(float), st, cam, tg, bf);
        const dim3 lgrid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + 3) / 4), (unsigned)li.nframes);
        const size_t lds = (size_t)4 * li.n * sizeof(float);
        if (bf.mode == NT_BOX_FACES_DRAW) hipLaunchKernelGGL(box_lines_var<true>, lgrid, dim3(256), lds, st, cam, tg, bf);
        else if (bf.mode == NT_BOX_FACES_MASK) hipLaunchKernelGGL(box_lines_var<false>, lgrid, dim3(256), lds, st, cam, tg, bf);
    }
    if (r) return r;
    return finish_launch("box face kernel launch");
}

// BoxScene face shading (nt_boxshade.hpp): the fixed-n launcher of the scene's dimension, or at run-time n box_hits_var into
// bs.recs and box_shaded_var behind it.  Kept apart from nt_launch_box as nt_launch_box_faces is: no route of a plain render.
int nt_launch_box_shade(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg, const NtBoxShade &bs) {
    int r = var_dim_check(li.n);
    if (r) return r;
    if (!nt_dispatch_dim<3, NT_DEV_MAX_FIXED_BOX>(li.force_var ? 0 : li.n, r, [&](auto N) { return nt_box_shade<decltype(N)::value>(li, cam, tg, bs); })) {
        if (!bs.recs || bs.frame_stride < (long long)tg.width * tg.height || tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1 ||
            tg.colors_out) {
            snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a face-shading launch at run-time n without its records, or not for whole frames");
            return -1;
        }
        hipStream_t st = (hipStream_t)li.stream;
        NtBoxFaces bf{};
        bf.mode = NT_BOX_FACES_RECORDS;
        bf.recs = bs.recs;
        bf.frame_stride = bs.frame_stride;
        const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + NT_BOXROWS - 1) / NT_BOXROWS), (unsigned)li.nframes);
        hipLaunchKernelGGL(box_hits_var, grid, dim3(64), ((size_t)li.n * 64 + (size_t)4 * li.n) * sizeof(float), st, cam, tg, bf);
        const dim3 sgrid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + 3) / 4), (unsigned)li.nframes);
        const size_t lds = (size_t)10 * li.n * sizeof(float);
        if (bs.kinds) hipLaunchKernelGGL(box_shaded_var<true>, sgrid, dim3(256), lds, st, cam, tg, bs);
        else hipLaunchKernelGGL(box_shaded_var<false>, sgrid, dim3(256), lds, st, cam, tg, bs);
    }
    if (r) return r;
    return finish_launch("box shading kernel launch");
}

// words per ray_color frame of composite_kernel_var_t (the host sizes NtCompositeDev::tframes with it)
int nt_var_frame_words(int n) { return var_frame_words(n); }

namespace {
// The general route of a render or a primary-hit pass under clip planes: the run-time-n walks at every dimension, the planes
// their last argument.  Transparent materials need the `checked` columns, and a render of them its ray_color frames, as
// nt_launch_composite and nt_launch_hits want them.
int clip_var_launch(const NtLaunchInfo &li, const NtCamera &cam, const NtCompositeDev &sv, const NtTarget &tg, const NtClip &cl, bool draw) {
    const NtClipPlanes cp = {cl.planes, cl.count};
    int r;
    size_t lds;
    hipStream_t s = (hipStream_t)li.stream;
    if ((r = var_dim_check(li.n))) return r;
    if (!sv.all_opaque && !sv.checked) return no_checked_scratch();
    if (draw) {
        dim3 grid;
        grid_for(tg, 8, 8, li.nframes, grid);
        if (sv.checked) {
            if (!sv.tframes) return no_checked_scratch();
            if ((r = var_frames_check(li.n, sv))) return r;
            if ((r = var_walk_ready(li.n, sv, alias_kernel(sv, composite_kernel_var_t<true>, composite_kernel_var_t<false>), lds))) return r;
            const dim3 blocks((unsigned)checked_blocks(sv));
            if (sv.alias_normals)
                hipLaunchKernelGGL(composite_kernel_var_t<true>, blocks, dim3(64), lds, s, cam, sv, tg, li.n, (int)grid.x, (int)grid.y, (int)grid.z, cp);
            else
                hipLaunchKernelGGL(composite_kernel_var_t<false>, blocks, dim3(64), lds, s, cam, sv, tg, li.n, (int)grid.x, (int)grid.y, (int)grid.z, cp);
        } else {
            if ((r = var_walk_ready(li.n, sv, reinterpret_cast<const void *>(composite_kernel_var), lds))) return r;
            hipLaunchKernelGGL(composite_kernel_var, grid, dim3(64), lds, s, cam, sv, tg, li.n, cp);
        }
        return 0;
    }
    NtHits h;
    h.cams = cl.cams;
    h.nframes = li.nframes;
    h.frame_stride = cl.frame_stride;
    h.hits = cl.hits;
    h.normal_origin = cl.normal_origin;
    h.normal_dir = cl.normal_dir;
    const int tiles_x = (tg.width + 7) / 8, tiles_y = (tg.height + 7) / 8;
    const long long tiles = (long long)tiles_x * tiles_y * h.nframes;
    if (sv.checked) {
        if ((r = var_walk_ready(li.n, sv, alias_kernel(sv, hits_closest_var_t<true>, hits_closest_var_t<false>), lds))) return r;
        const dim3 tgrid((unsigned)checked_blocks(sv, tiles));
        if (sv.alias_normals) hipLaunchKernelGGL(hits_closest_var_t<true>, tgrid, dim3(64), lds, s, sv, tg, h, li.n, tiles_x, tiles_y, cp);
        else hipLaunchKernelGGL(hits_closest_var_t<false>, tgrid, dim3(64), lds, s, sv, tg, h, li.n, tiles_x, tiles_y, cp);
    } else {
        if ((r = var_walk_ready(li.n, sv, reinterpret_cast<const void *>(hits_closest_var), lds))) return r;
        const dim3 grid((unsigned)(tiles < (1 << 22) ? tiles : (1 << 22)));
        hipLaunchKernelGGL(hits_closest_var, grid, dim3(64), lds, s, sv, tg, h, li.n, tiles_x, tiles_y, cp);
    }
    return 0;
}
}  // namespace

// Clip planes (nt_clip.hpp): the packet route of the scene's dimension for what launch_composite_fixed would give the packet
// walk, the run-time-n kernels for every other scene.  Kept apart from nt_launch_composite and nt_launch_hits: with the
// setting off nothing here is reached.
int nt_launch_clip(const NtLaunchInfo &li, const NtCamera &cam, const NtCompositeDev &sc, const NtTarget &tg, const NtClip &cl, bool draw) {
    if (!cl.planes || cl.count < 1 || cl.count > NT_DEV_CLIP_MAX || !cl.cams || (!draw && !cl.hits)) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a clip launch without its planes, cameras or records");
        return -1;
    }
    int r = 0;
    const bool packet = sc.all_opaque && !sc.checked && sc.stack_depth <= 32 && li.kernel_choice == 0 && !li.force_var;
    if (!packet || !nt_dispatch_dim<3, NT_DEV_MAX_FIXED>(li.n, r, [&](auto N) { return nt_clip_packet<decltype(N)::value>(li, sc, tg, cl, draw); })) {
        r = clip_var_launch(li, cam, sc, tg, cl, draw);
    }
    if (r) return r;
    return finish_launch("clip kernel launch");
}

int nt_launch_composite(const NtLaunchInfo &li, const NtCamera &cam, const NtCompositeDev &sc, const NtTarget &tg) {
    int r;
    size_t lds;
    dim3 grid;
    if (sc.tframes) {
        // transparent materials / the reference's normal handling at run-time n (or beyond the fixed kernels' frame stack)
        if ((r = var_frames_check(li.n, sc))) return r;
        if ((r = var_walk_ready(li.n, sc, alias_kernel(sc, composite_kernel_var_t<true>, composite_kernel_var_t<false>), lds))) return r;
        grid_for(tg, 8, 8, li.nframes, grid);
        const dim3 blocks((unsigned)checked_blocks(sc));
        if (sc.alias_normals)
            hipLaunchKernelGGL(composite_kernel_var_t<true>, blocks, dim3(64), lds, (hipStream_t)li.stream, cam, sc, tg, li.n, (int)grid.x, (int)grid.y,
                               (int)grid.z, NtClipPlanes{nullptr, 0});
        else
            hipLaunchKernelGGL(composite_kernel_var_t<false>, blocks, dim3(64), lds, (hipStream_t)li.stream, cam, sc, tg, li.n, (int)grid.x, (int)grid.y,
                               (int)grid.z, NtClipPlanes{nullptr, 0});
        return finish_launch("composite kernel launch");
    }
    if (!nt_dispatch_dim<3, NT_DEV_MAX_FIXED>(li.force_var ? 0 : li.n, r, [&](auto N) { return nt_composite_fixed<decltype(N)::value>(li, cam, sc, tg); })) {
        if ((r = var_dim_check(li.n))) return r;
        if (!sc.all_opaque) {
            snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "the run-time-n kernel does not render transparent materials");
            return -2;
        }
        if ((r = var_walk_ready(li.n, sc, reinterpret_cast<const void *>(composite_kernel_var), lds))) return r;
        // run-time-n kernel: one wave per 8x8 tile (probe mode: 64 probes per block)
        grid_for(tg, 8, 8, li.nframes, grid);
        hipLaunchKernelGGL(composite_kernel_var, grid, dim3(64), lds, (hipStream_t)li.stream, cam, sc, tg, li.n, NtClipPlanes{nullptr, 0});
    }
    if (r) return r;
    return finish_launch("composite kernel launch");
}

// Ray queries (nt_query.hpp): the fixed-n launcher of the scene's dimension, or the run-time-n kernels above.  Kept apart from
// nt_launch_composite: these are no render routes.
int nt_launch_query(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtQuery &q) {
    int r;
    if (!nt_dispatch_dim<3, NT_DEV_MAX_FIXED>(li.force_var ? 0 : li.n, r, [&](auto N) { return nt_query_fixed<decltype(N)::value>(li, sc, q); })) {
        const void *kernel;
        if (q.occlusion) kernel = sc.all_opaque ? reinterpret_cast<const void *>(query_occluded_var) : reinterpret_cast<const void *>(query_occluded_var_t);
        else if (!sc.checked) kernel = reinterpret_cast<const void *>(query_closest_var);
        else kernel = alias_kernel(sc, query_closest_var_t<true>, query_closest_var_t<false>);
        size_t lds;
        if ((r = var_walk_ready(li.n, sc, kernel, lds))) return r;
        hipStream_t s = (hipStream_t)li.stream;
        const dim3 grid((unsigned)(((long long)q.count + 63) / 64));
        if (q.occlusion) {
            if (sc.all_opaque) hipLaunchKernelGGL(query_occluded_var, grid, dim3(64), lds, s, sc, q, li.n);
            else hipLaunchKernelGGL(query_occluded_var_t, grid, dim3(64), lds, s, sc, q, li.n);
        } else if (sc.checked) {
            // as many blocks as the `checked` scratch has lane columns for, striding over the rays
            const dim3 tgrid((unsigned)checked_blocks(sc));
            if (sc.alias_normals) hipLaunchKernelGGL(query_closest_var_t<true>, tgrid, dim3(64), lds, s, sc, q, li.n);
            else hipLaunchKernelGGL(query_closest_var_t<false>, tgrid, dim3(64), lds, s, sc, q, li.n);
        } else if (!sc.all_opaque) {
            return no_checked_scratch();
        } else {
            hipLaunchKernelGGL(query_closest_var, grid, dim3(64), lds, s, sc, q, li.n);
        }
    }
    if (r) return r;
    return finish_launch("query kernel launch");
}

// Primary-hit buffers (nt_hits.hpp): the fixed-n launcher of the scene's dimension, or the run-time-n kernels above.  Kept apart
// from nt_launch_composite and nt_launch_query: these are neither render routes nor query routes.
int nt_launch_hits(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtHits &h) {
    int r;
    if (!nt_dispatch_dim<3, NT_DEV_MAX_FIXED>(li.force_var ? 0 : li.n, r, [&](auto N) { return nt_hits_fixed<decltype(N)::value>(li, sc, tg, h); })) {
        const void *kernel;
        if (!sc.checked) kernel = reinterpret_cast<const void *>(hits_closest_var);
        else kernel = alias_kernel(sc, hits_closest_var_t<true>, hits_closest_var_t<false>);
        size_t lds;
        if ((r = var_walk_ready(li.n, sc, kernel, lds))) return r;
        hipStream_t s = (hipStream_t)li.stream;
        const int tiles_x = (tg.width + 7) / 8, tiles_y = (tg.height + 7) / 8;
        const long long tiles = (long long)tiles_x * tiles_y * h.nframes;
        if (sc.checked) {
            // as many blocks as the `checked` scratch has lane columns for, striding over the tiles
            const dim3 tgrid((unsigned)checked_blocks(sc, tiles));
            if (sc.alias_normals) hipLaunchKernelGGL(hits_closest_var_t<true>, tgrid, dim3(64), lds, s, sc, tg, h, li.n, tiles_x, tiles_y, NtClipPlanes{nullptr, 0});
            else hipLaunchKernelGGL(hits_closest_var_t<false>, tgrid, dim3(64), lds, s, sc, tg, h, li.n, tiles_x, tiles_y, NtClipPlanes{nullptr, 0});
        } else if (!sc.all_opaque) {
            return no_checked_scratch();
        } else {
            const dim3 grid((unsigned)(tiles < (1 << 22) ? tiles : (1 << 22)));
            hipLaunchKernelGGL(hits_closest_var, grid, dim3(64), lds, s, sc, tg, h, li.n, tiles_x, tiles_y, NtClipPlanes{nullptr, 0});
        }
    }
    if (r) return r;
    return finish_launch("primary-hit kernel launch");
}

// The colours of the caller's rays (nt_rays.hpp): the fixed-n launcher of the scene's dimension, or the run-time-n kernels above.
// Kept apart from nt_launch_box and nt_launch_composite: these are no render routes.  sc == nullptr: BoxScene.
int nt_launch_rays(const NtLaunchInfo &li, const NtCompositeDev *sc, const NtRayJob &job, const NtTarget &tg) {
    hipStream_t s = (hipStream_t)li.stream;
    int r = var_dim_check(li.n);
    if (r) return r;
    long long blocks = ((long long)job.count + 63) / 64;              // of the one-wave kernels
    size_t lds;
    if (!sc) {
        if (!nt_dispatch_dim<3, NT_DEV_MAX_FIXED_BOX>(li.force_var ? 0 : li.n, r, [&](auto N) { return nt_rays_box_fixed<decltype(N)::value>(li, job, tg); })) {
            if (blocks > NT_RAYS_MAX_BLOCKS) blocks = NT_RAYS_MAX_BLOCKS;
            lds = (size_t)2 * li.n * 64 * sizeof(float);
            hipLaunchKernelGGL(rays_box_var, dim3((unsigned)blocks), dim3(64), lds, s, job, tg, li.n);
        }
        if (r) return r;
        return finish_launch("ray-colour kernel launch");
    }
    if (sc->tframes) {
        // transparent materials / the reference's normal handling at run-time n (or beyond the fixed kernels' frame stack)
        if ((r = var_frames_check(li.n, *sc))) return r;
        if ((r = var_walk_ready(li.n, *sc, alias_kernel(*sc, rays_color_var_t<true>, rays_color_var_t<false>), lds))) return r;
        // as many blocks as the scratch has lane columns for, striding over the rays
        blocks = checked_blocks(*sc, blocks);
        if (sc->alias_normals) hipLaunchKernelGGL(rays_color_var_t<true>, dim3((unsigned)blocks), dim3(64), lds, s, *sc, job, tg, li.n);
        else hipLaunchKernelGGL(rays_color_var_t<false>, dim3((unsigned)blocks), dim3(64), lds, s, *sc, job, tg, li.n);
        return finish_launch("ray-colour kernel launch");
    }
    if (!nt_dispatch_dim<3, NT_DEV_MAX_FIXED>(li.force_var ? 0 : li.n, r, [&](auto N) { return nt_rays_fixed<decltype(N)::value>(li, *sc, job, tg); })) {
        if (!sc->all_opaque || sc->checked) {
            snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: the run-time-n kernel without frame scratch does not shade transparent materials");
            return -1;
        }
        if ((r = var_walk_ready(li.n, *sc, reinterpret_cast<const void *>(rays_color_var), lds))) return r;
        if (blocks > NT_RAYS_MAX_BLOCKS) blocks = NT_RAYS_MAX_BLOCKS;
        hipLaunchKernelGGL(rays_color_var, dim3((unsigned)blocks), dim3(64), lds, s, *sc, job, tg, li.n);
    }
    if (r) return r;
    return finish_launch("ray-colour kernel launch");
}

// Adaptive supersampling (nt_adaptive.hpp): the flag kernel, and the refine kernels chosen as nt_launch_rays chooses the rays_* ones
int nt_launch_adaptive_flag(void *stream, const NtAdaptive &ad, const NtTarget &tg) {
    launch_adaptive_flag((hipStream_t)stream, ad, tg);
    return finish_launch("adaptive flag kernel launch");
}

int nt_launch_refine(const NtLaunchInfo &li, const NtCompositeDev *sc, const NtRefine &rf, const NtTarget &tg) {
    hipStream_t s = (hipStream_t)li.stream;
    if (li.n < 3 || li.n > NT_DEV_MAX_DIM || rf.s < 2 || rf.s > 8) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "refine kernels: unsupported dimension %d or factor %d", li.n, rf.s);
        return -2;
    }
    long long blocks = refine_blocks(rf);
    int r = 0;
    size_t lds;
    if (!sc) {
        if (!nt_dispatch_dim<3, NT_DEV_MAX_FIXED_BOX>(li.force_var ? 0 : li.n, r, [&](auto N) { return nt_refine_box_fixed<decltype(N)::value>(li, rf, tg); })) {
            lds = (size_t)2 * li.n * 64 * sizeof(float);
            hipLaunchKernelGGL(refine_box_var, dim3((unsigned)blocks), dim3(64), lds, s, rf, tg, li.n);
        }
        if (r) return r;
        return finish_launch("refine kernel launch");
    }
    if (sc->tframes) {
        if ((r = var_frames_check(li.n, *sc))) return r;
        if ((r = var_walk_ready(li.n, *sc, alias_kernel(*sc, refine_color_var_t<true>, refine_color_var_t<false>), lds))) return r;
        blocks = checked_blocks(*sc, blocks);
        if (sc->alias_normals) hipLaunchKernelGGL(refine_color_var_t<true>, dim3((unsigned)blocks), dim3(64), lds, s, *sc, rf, tg, li.n);
        else hipLaunchKernelGGL(refine_color_var_t<false>, dim3((unsigned)blocks), dim3(64), lds, s, *sc, rf, tg, li.n);
        return finish_launch("refine kernel launch");
    }
    if (!nt_dispatch_dim<3, NT_DEV_MAX_FIXED>(li.force_var ? 0 : li.n, r, [&](auto N) { return nt_refine_fixed<decltype(N)::value>(li, *sc, rf, tg); })) {
        if (!sc->all_opaque || sc->checked) {
            snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: the run-time-n kernel without frame scratch does not shade transparent materials");
            return -1;
        }
        if ((r = var_walk_ready(li.n, *sc, reinterpret_cast<const void *>(refine_color_var), lds))) return r;
        hipLaunchKernelGGL(refine_color_var, dim3((unsigned)blocks), dim3(64), lds, s, *sc, rf, tg, li.n);
    }
    if (r) return r;
    return finish_launch("refine kernel launch");
}

// A render through a lens.  The packet route (nt_lens.hpp): the fixed-n launcher of the scene's dimension; there is no
// run-time-n packet walk, and the host sends those scenes through the ray route below.
int nt_launch_lens(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtLens &ln) {
    return launch_fixed_only(li, "no packet walk for a lens", "lens kernel launch",
                             [&](auto N) { return nt_lens_fixed<decltype(N)::value>(li, sc, tg, ln); });
}

// The ray route's two helpers around nt_launch_rays: pixels [first, first + count) of the table
int nt_launch_lens_expand(const NtLaunchInfo &li, const float *table, const float *cam, long long first, long long count, float *out) {
    const long long blocks = stride_blocks(count);
    if (blocks < 1) return 0;
    hipLaunchKernelGGL(lens_expand, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)li.stream, table, cam, li.n, first, count, out);
    return finish_launch("lens expansion kernel launch");
}

int nt_launch_lens_mask(const NtLaunchInfo &li, const float *table, long long first, long long count, const NtTarget &tg) {
    const long long blocks = stride_blocks(count);
    if (blocks < 1) return 0;
    hipLaunchKernelGGL(lens_mask_fill, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)li.stream, table, first, count, tg);
    return finish_launch("lens mask kernel launch");
}

// A render under the parallel projection.  The packet route (nt_parallel.hpp): the fixed-n launcher of the scene's dimension;
// there is no run-time-n packet walk, and the host sends those scenes through the ray route below.
int nt_launch_parallel(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtParallel &pl) {
    return launch_fixed_only(li, "no packet walk for the parallel projection", "parallel projection kernel launch",
                             [&](auto N) { return nt_parallel_fixed<decltype(N)::value>(li, sc, tg, pl); });
}

// The ray route's helper in front of nt_launch_rays: pixels [first, first + count) of the view
int nt_launch_parallel_expand(const NtLaunchInfo &li, const float *cam, int width, float k, float half_w, float half_h, long long first,
                              long long count, float *out) {
    const long long blocks = stride_blocks(count);
    if (blocks < 1) return 0;
    hipLaunchKernelGGL(parallel_expand, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)li.stream, cam, li.n, width, k, half_w, half_h, first, count, out);
    return finish_launch("parallel projection expansion kernel launch");
}

// Ambient occlusion.  The fast route (nt_ao.hpp): the fixed-n launcher of the scene's dimension; the host sends every other
// scene through the ray route below.
int nt_launch_ao(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtAo &ao) {
    return launch_fixed_only(li, "no ambient occlusion kernel", "ambient occlusion kernel launch",
                             [&](auto N) { return nt_ao_fixed<decltype(N)::value>(li, sc, tg, ao); });
}

// The ray route's two kernels around nt_launch_query: pixels [ar.first, ar.first + ar.pixels) of the launch
int nt_launch_ao_expand(const NtLaunchInfo &li, const NtTarget &tg, const NtAo &ao, const NtAoRays &ar) {
    const long long blocks = stride_blocks(ar.pixels * ao.count);
    if (blocks < 1) return 0;
    hipLaunchKernelGGL(ao_expand, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)li.stream, tg, ao, ar, li.n);
    return finish_launch("ambient occlusion expansion kernel launch");
}

int nt_launch_ao_reduce(const NtLaunchInfo &li, const NtTarget &tg, const NtAo &ao, const NtAoRays &ar) {
    const long long blocks = stride_blocks(ar.pixels);
    if (blocks < 1) return 0;
    hipLaunchKernelGGL(ao_reduce, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)li.stream, tg, ao, ar);
    return finish_launch("ambient occlusion count kernel launch");
}

int nt_launch_ao_apply(void *stream, const uint32_t *base, const int *blocked, int count, float strength, int nframes, const NtTarget &tg) {
    const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + 3) / 4), (unsigned)nframes);
    hipLaunchKernelGGL(ao_apply, grid, dim3(256), 0, (hipStream_t)stream, base, blocked, count, strength, tg);
    return finish_launch("ambient occlusion drawing kernel launch");
}

// Outlines.  The fast route (nt_outline.hpp): the fixed-n launcher of the scene's dimension -- the packet walk, then outline_shade
// (`draw`) or outline_mark_fixed; there is no run-time-n packet walk, and the host sends those scenes through the general route
// below.
static int nt_launch_outline_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtOutline &ol, bool draw) {
    return launch_fixed_only(li, "no packet walk for outlines", "outline kernel launch",
                             [&](auto N) { return nt_outline_fixed<decltype(N)::value>(li, sc, tg, ol, draw); });
}

int nt_launch_outline(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtOutline &ol) {
    return nt_launch_outline_fixed(li, sc, tg, ol, true);
}

int nt_launch_outline_mask(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtOutline &ol) {
    return nt_launch_outline_fixed(li, sc, tg, ol, false);
}

// The general route's two kernels behind nt_launch_hits: every pixel of the launch's frames
int nt_launch_outline_mark(const NtLaunchInfo &li, const NtTarget &tg, const NtOutline &ol) {
    const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + 3) / 4), (unsigned)ol.nframes);
    hipLaunchKernelGGL(outline_mark, grid, dim3(256), 0, (hipStream_t)li.stream, tg, ol, li.n);
    return finish_launch("outline mask kernel launch");
}

int nt_launch_outline_apply(void *stream, const uint32_t *base, const NtOutline &ol, const NtTarget &tg) {
    const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + 3) / 4), (unsigned)ol.nframes);
    hipLaunchKernelGGL(outline_apply, grid, dim3(256), 0, (hipStream_t)stream, base, ol, tg);
    return finish_launch("outline drawing kernel launch");
}

// Depth cues.  The fast route (nt_cue.hpp): the fixed-n launcher of the scene's dimension -- the packet walk, then cue_shade
// (`draw`) or cue_factors_fixed; there is no run-time-n packet walk, and the host sends those scenes through the general route
// below.
static int nt_launch_cue_packet(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtCue &cu, bool draw) {
    return launch_fixed_only(li, "no packet walk for depth cues", "depth cue kernel launch",
                             [&](auto N) { return nt_cue_packet<decltype(N)::value>(li, sc, tg, cu, draw); });
}

int nt_launch_cue(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtCue &cu) {
    return nt_launch_cue_packet(li, sc, tg, cu, true);
}

int nt_launch_cue_factors_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtCue &cu) {
    return nt_launch_cue_packet(li, sc, tg, cu, false);
}

// The general route's two kernels behind nt_launch_hits: every pixel of the launch's frames
int nt_launch_cue_factors(const NtLaunchInfo &li, const NtTarget &tg, const NtCue &cu) {
    const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + 3) / 4), (unsigned)cu.nframes);
    hipLaunchKernelGGL(cue_factors, grid, dim3(256), 0, (hipStream_t)li.stream, tg, cu, li.n);
    return finish_launch("depth cue factor kernel launch");
}

int nt_launch_cue_apply(const NtLaunchInfo &li, const uint32_t *base, const NtCue &cu, const NtTarget &tg) {
    const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + 3) / 4), (unsigned)cu.nframes);
    hipLaunchKernelGGL(cue_apply, grid, dim3(256), 0, (hipStream_t)li.stream, base, cu, tg, li.n);
    return finish_launch("depth cue drawing kernel launch");
}

namespace {
// the general route of an X-ray launch: xray_var, as many one-wave blocks as the `checked` scratch has lane columns for
int xray_var_launch(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtXray &xr) {
    int r;
    if ((r = var_dim_check(li.n))) return r;
    if (!sc.checked || sc.checked_lanes < 64 || !xr.cams || (sc.n_batches > 0 && !xr.live) || (!xr.counts && !xr.trans)) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: an X-ray launch without its scratch, cameras, masks or table");
        return -1;
    }
    size_t lds;
    const void *kernel = xr.counts ? reinterpret_cast<const void *>(xray_var<true>) : reinterpret_cast<const void *>(xray_var<false>);
    if ((r = var_walk_ready(li.n, sc, kernel, lds))) return r;
    const int tiles_x = (tg.width + 7) / 8, tiles_y = (tg.height + 7) / 8;
    const long long tiles = (long long)tiles_x * tiles_y * li.nframes;
    const dim3 grid((unsigned)checked_blocks(sc, tiles));
    if (xr.counts) hipLaunchKernelGGL(xray_var<true>, grid, dim3(64), lds, (hipStream_t)li.stream, sc, tg, xr, li.n, tiles_x, tiles_y, li.nframes);
    else hipLaunchKernelGGL(xray_var<false>, grid, dim3(64), lds, (hipStream_t)li.stream, sc, tg, xr, li.n, tiles_x, tiles_y, li.nframes);
    return 0;
}
}  // namespace

namespace {
// the general route of a hit-layer launch: layers_var, as many one-wave blocks as the `checked` scratch has lane columns for
int layers_var_launch(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtLayers &ly) {
    int r;
    if ((r = var_dim_check(li.n))) return r;
    if (!sc.checked || sc.checked_lanes < 64 || !ly.cams || (sc.n_batches > 0 && !ly.live) || !ly.records || ly.layers < 1 ||
        ly.layers > NT_DEV_LAYERS_MAX || li.nframes != 1) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a hit-layer launch without its scratch, cameras, masks or records");
        return -1;
    }
    size_t lds;
    if ((r = var_walk_ready(li.n, sc, reinterpret_cast<const void *>(layers_var), lds))) return r;
    const int tiles_x = (tg.width + 7) / 8, tiles_y = (tg.height + 7) / 8;
    const dim3 grid((unsigned)checked_blocks(sc, (long long)tiles_x * tiles_y));
    hipLaunchKernelGGL(layers_var, grid, dim3(64), lds, (hipStream_t)li.stream, sc, tg, ly, li.n, tiles_x, tiles_y);
    return 0;
}
}  // namespace

// Hit layers: the routes of nt_launch_xray, with layers_packet (nt_layers.hpp) and layers_var
int nt_launch_layers(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtLayers &ly) {
    int r = 0;
    if (!nt_xray_packet_route(li, sc) ||
        !nt_dispatch_dim<3, NT_DEV_MAX_FIXED>(li.n, r, [&](auto N) { return nt_layers_packet<decltype(N)::value>(li, sc, tg, ly); })) {
        r = layers_var_launch(li, sc, tg, ly);
    }
    if (r) return r;
    return finish_launch("hit-layer kernel launch");
}

// X-ray views.  The packet walk of the scene's dimension (nt_xray.hpp) where nt_xray_packet_route says so -- the item count is
// checked there, before the launch, against the bitset the walk can hold -- and xray_var for every other scene.  Kept apart from
// every launcher above: with the setting off and no count asked for, nothing here is reached.
int nt_launch_xray(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtXray &xr) {
    int r = 0;
    if (!nt_xray_packet_route(li, sc) ||
        !nt_dispatch_dim<3, NT_DEV_MAX_FIXED>(li.n, r, [&](auto N) { return nt_xray_packet<decltype(N)::value>(li, sc, tg, xr); })) {
        r = xray_var_launch(li, sc, tg, xr);
    }
    if (r) return r;
    return finish_launch("X-ray kernel launch");
}
