// nt_boxshade.hpp -- BoxScene face shading for compile-time N (nt_scene_set_box_shading): the frame shaded from
// the face record of every pixel (nt_boxhits.hpp) instead of the one plain colour -- a colour of its own for each of the 2n
// faces, the depth cues' fog and coordinate tint (the rule of nt_cue.hpp, word for word, on BoxScene's record) and, with the
// face-line setting on as well, the lines on top.  The rule in full: ntracer_hip.h, "BoxScene face shading".
// Two kernels.  box_shaded<N, false> has box_hits' block shape and keeps everything in registers: record, shade, emit.
// box_shaded<N, true> has box_lines' structure -- the records of a 64 x 32 tile and its one-pixel halo in LDS, one barrier -- and
// a lane keeps per row, besides what box_lines keeps, the tint sum s, formed in the record phase where d is live.
// The face-colour table is indexed by a lane's own face: from the kernel arguments it would go to scratch, so a block stages its
// 6 N floats in LDS once (at most 576 bytes here) and a hit pixel reads its three from there.
// Instantiated per N by nt_inst_boxshade.hip; the run-time-n kernel and the dispatcher (nt_launch_box_shade) are in nt_var.hip.
#pragma once
#include "nt_boxhits.hpp"

namespace {

// clamp01 of the factors, as the depth cues have it
__device__ __forceinline__ float box_shade_clamp01(float v) { return fmaxf(0.0f, fminf(1.0f, v)); }

// the tint sum of a pixel with a hit at `dist`: s = a_0 * x_0, then s = s + (a_k * x_k), x_k = (d_k * dist) + o_k; dir(k) and
// org(k) hand over component k (the one copy of the sum, for these kernels and box_shaded_var of nt_var.hip)
template <typename DIR, typename ORG>
__device__ __forceinline__ float box_shade_tint_sum(const NtBoxShade &bs, int n, float dist, DIR dir, ORG org) {
    float s = bs.cue.tint_axis[0] * ((dir(0) * dist) + org(0));
#pragma unroll
    for (int k = 1; k < n; ++k) s = s + (bs.cue.tint_axis[k] * ((dir(k) * dist) + org(k)));
    return s;
}

// box_line_record with the tint sum: s is formed only where the setting has a tint and a lane of the wave a hit, and read only
// for a hit under a tint
template <int N>
__device__ __forceinline__ void box_shade_record(const NtBoxShade &bs, const float (&org)[N], const float (&base)[N], const float (&up)[N],
                                                 const float (&dots)[4], float sx, float sy, float &dist, int &code, float &xval, float &s) {
    float dir[N];
#pragma unroll
    for (int j = 0; j < N; ++j) dir[j] = base[j] - up[j] * sy;
    float sq = dir[0] * dir[0];
#pragma unroll
    for (int j = 1; j < N; ++j) sq = sq + dir[j] * dir[j];
    const bool maybe = box_may_hit(N, dots, sx, sy, sq);
    int face = -1, side = -1;
    dist = FLT_MAX;
    s = 0.0f;
    if (__builtin_amdgcn_ballot_w64(maybe) != 0ull) {
        const float len = sqrtf(sq);
#pragma unroll
        for (int j = 0; j < N; ++j) dir[j] = dir[j] / len;
        box_face<N>(org, dir, maybe, face, side, dist);
        xval = dir[0];
#pragma unroll
        for (int j = 1; j < N; ++j) xval = face == j ? dir[j] : xval;
        if (bs.cue_on && bs.cue.tint && __builtin_amdgcn_ballot_w64(face >= 0) != 0ull)
            s = box_shade_tint_sum(bs, N, dist, [&](int k) { return dir[k]; }, [&](int k) { return org[k]; });
    } else {
        xval = dir[0] / sqrtf(sq);          // (the one component the background needs)
    }
    code = face >= 0 ? 2 * face + side : -1;
}

// The rule from the record on (ntracer_hip.h): B from the table or the background, P, the factors (f, g), Q, the lines' blend
// where the mask is set, and the pixel emitted.  `tab`: the table [2 n][3] as the kernels read it (LDS); xval: d_face on a hit and
// d_0 without one.  A wave without a marked pixel goes through the emitters of the plain kernels where the target allows and
// bs.gb_equal says that the setting leaves g == b: the table's entries, both tint colours and the fog colour (the background has
// it by itself, and the lines' colour touches marked pixels only).  Every other wave quantises its three components one by one.
__device__ __forceinline__ void box_shade_emit(const NtTarget &tg, const NtBoxShade &bs, const float *tab, const PixelRef &pr, int code, float dist,
                                               float xval, float s, int m) {
    const bool hit = code >= 0;
    const float *t = tab + 3 * (hit ? code : 0);
    const float t0 = t[0], t1 = t[1], t2 = t[2];
    float p[3];
    if (hit) {
        const float shade = fabsf(xval);      // sine = d_i * (-sign d_i) <= 0, shade = -sine (tracer.hpp:105-107)
        p[0] = shade * t0;
        p[1] = shade * t1;
        p[2] = shade * t2;
    } else {
        box_background(xval, p[0], p[1], p[2]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = p[k] > 0.0f ? p[k] : 0.0f;
        p[k] = v < 1.0f ? v : 1.0f;
    }
    if (bs.cue_on) {
        const NtCue &cu = bs.cue;
        float f = -1.0f, g = -1.0f;
        if (hit) {
            f = box_shade_clamp01((dist - cu.fog_near) * cu.inv_fog);
            if (cu.tint) g = box_shade_clamp01((s - cu.tint_lo) * cu.inv_tint);
        } else if (cu.fog_background) {
            f = 1.0f;
        }
        if (g >= 0.0f) {
            const float keep = 1.0f - g;
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = p[k] * ((cu.tint_color_lo[k] * keep) + (cu.tint_color_hi[k] * g));
        }
        if (f >= 0.0f) {
            const float w = f * cu.fog_strength;
            const float keep = 1.0f - w;
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = (p[k] * keep) + (cu.fog_color[k] * w);
        }
    }
    if (bs.gb_equal && __builtin_amdgcn_ballot_w64(m != 0) == 0ull) {
        if (tg.plain_f32[0] >= 0 && tg.bpp == 12 && tg.aligned4) { emit_f32x3(tg, pr.offset, p[0], p[1]); return; }
        if (plain_rgb(tg)) { emit_plain(tg, pr, plain_quantize(tg, p[0]), plain_quantize(tg, p[1])); return; }
    }
    if (m != 0) {
        const float keep = 1.0f - bs.line_strength;
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = (p[k] * keep) + (bs.line_color[k] * bs.line_strength);
    }
    if (plain_rgb(tg)) {
        // emit_plain's dword with a quantisation of its own for each component: in these layouts a channel's value is the
        // component itself, so the bits are emit_pixel's
        const uint32_t w = plain_quantize(tg, p[0]) * tg.plain_mul[0] + plain_quantize(tg, p[1]) * tg.plain_mul[1] + plain_quantize(tg, p[2]) * tg.plain_mul[2];
        *reinterpret_cast<uint32_t *>(tg.dest + pr.offset) = tg.reversed ? w : bswap32(w);
        return;
    }
    emit_pixel(tg, pr, p[0], p[1], p[2]);
}

// the block's copy of the table: 6 n floats from the kernel arguments into LDS (the caller's barrier makes them visible)
__device__ __forceinline__ void box_shade_stage(const NtBoxShade &bs, int n, int tid, int nthreads, float *tab) {
    const float *src = bs.colors;
    for (int k = tid; k < 6 * n; k += nthreads) tab[k] = src[k];
}

__device__ __forceinline__ PixelRef box_shade_pixel(const NtTarget &tg, int x, int y) {
    PixelRef pr;
    pr.x = x;
    pr.y = y;
    pr.offset = (long long)blockIdx.z * tg.frame_stride + (long long)y * tg.pitch + (long long)x * tg.bpp;
    pr.hit_index = 0;
    pr.valid = true;
    return pr;
}

// LINES false: box_hits' block shape (a lane walks a column of NT_BOXROWS rows, four waves a block, frames in blockIdx.z): the
// record in registers, shaded and emitted; box_may_hit in front, so a wave that sees nothing draws the background, or the full
// fog, without a face test and with one division a pixel instead of N -- not with none: the background's colour is a function
// of d_0 = dir[0] / |dir|, as in box_line_record.  The only LDS is the table.
// LINES true: box_lines<N, true>'s structure (64 x 32 tile, one-pixel halo, 17 952 bytes of records, one barrier -- the table's
// too); a lane keeps (dist, code, xval, s) per row and not d; halo pixels need neither xval nor s.
template <int N, bool LINES>
__global__ __launch_bounds__(256) void box_shaded(NtCameraFixed cam, NtTarget tg, NtBoxShade bs) {
    __shared__ float tab[6 * N];
    __shared__ int2 tile[LINES ? (NT_BOXLINES_TH + 2) * NT_BOXLINES_PITCH : 1];
    if (nt_aborted(tg)) return;               // (every lane reads the same word: the whole block leaves, ahead of the barrier)
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    box_shade_stage(bs, N, tid, 256, tab);
    float org[N], right[N], up[N], fwd[N];
    load_camera<N>(cam, org, right, up, fwd);
    float dots[4];
    if (cam.buf) {
        const float *dp = cam.dots + (size_t)blockIdx.z * 4;
        dots[0] = dp[0]; dots[1] = dp[1]; dots[2] = dp[2]; dots[3] = dp[3];
    } else {
        dots[0] = cam.odots[0]; dots[1] = cam.odots[1]; dots[2] = cam.odots[2]; dots[3] = cam.odots[3];
    }
    constexpr int R = NT_BOXROWS;
    const int x0 = (int)blockIdx.x * NT_BOXLINES_TW, y0 = (int)blockIdx.y * NT_BOXLINES_TH;
    const int x = x0 + lane;
    if (!LINES) {
        __syncthreads();                       // the table
        if (x >= tg.width) return;
        const float sx = tg.fovI * ((float)x - tg.half_w);
        float base[N];
#pragma unroll
        for (int j = 0; j < N; ++j) base[j] = fwd[j] + right[j] * sx;
        for (int rr = 0; rr < R; ++rr) {
            const int y = y0 + wv * R + rr;                 // the same for the whole wave
            if (y >= tg.height) return;
            float dist, xval, s;
            int code;
            box_shade_record<N>(bs, org, base, up, dots, sx, tg.fovI * ((float)y - tg.half_h), dist, code, xval, s);
            box_shade_emit(tg, bs, tab, box_shade_pixel(tg, x, y), code, dist, xval, s, 0);
        }
        return;
    }
    float pdist[R], pxval[R], ps[R];
    int pcode[R];
    {
        const float sx = tg.fovI * ((float)x - tg.half_w);
        float base[N];
#pragma unroll
        for (int j = 0; j < N; ++j) base[j] = fwd[j] + right[j] * sx;
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int ly = wv * R + rr;
            const int y = y0 + ly;                          // the same for the whole wave
            pdist[rr] = FLT_MAX;
            pcode[rr] = -2;
            pxval[rr] = 0.0f;
            ps[rr] = 0.0f;
            if (x < tg.width && y < tg.height)
                box_shade_record<N>(bs, org, base, up, dots, sx, tg.fovI * ((float)y - tg.half_h), pdist[rr], pcode[rr], pxval[rr], ps[rr]);
            tile[(ly + 1) * NT_BOXLINES_PITCH + lane + 1] = make_int2(__float_as_int(pdist[rr]), pcode[rr]);
        }
    }
    if (tid < 2 * NT_BOXLINES_TW + 2 * NT_BOXLINES_TH) {
        // the halo: the row above, the row below, the column to the left, the column to the right
        int hx, hy;
        if (tid < NT_BOXLINES_TW) { hx = tid; hy = -1; }
        else if (tid < 2 * NT_BOXLINES_TW) { hx = tid - NT_BOXLINES_TW; hy = NT_BOXLINES_TH; }
        else if (tid < 2 * NT_BOXLINES_TW + NT_BOXLINES_TH) { hx = -1; hy = tid - 2 * NT_BOXLINES_TW; }
        else { hx = NT_BOXLINES_TW; hy = tid - 2 * NT_BOXLINES_TW - NT_BOXLINES_TH; }
        const int gx = x0 + hx, gy = y0 + hy;
        float hdist = FLT_MAX, hxval;
        int hcode = -2;
        if (gx >= 0 && gy >= 0 && gx < tg.width && gy < tg.height) {
            const float sx = tg.fovI * ((float)gx - tg.half_w);
            float base[N];
#pragma unroll
            for (int j = 0; j < N; ++j) base[j] = fwd[j] + right[j] * sx;
            box_line_record<N, false>(org, base, up, dots, sx, tg.fovI * ((float)gy - tg.half_h), hdist, hcode, hxval);
        }
        tile[(hy + 1) * NT_BOXLINES_PITCH + hx + 1] = make_int2(__float_as_int(hdist), hcode);
    }
    __syncthreads();
    if (x >= tg.width) return;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int ly = wv * R + rr;
        const int y = y0 + ly;
        if (y >= tg.height) return;
        int m = 0;
        if (pcode[rr] >= 0) {
            const int at = (ly + 1) * NT_BOXLINES_PITCH + lane + 1;
            m = box_line_pair(pdist[rr], pcode[rr], tile[at - 1]) | box_line_pair(pdist[rr], pcode[rr], tile[at + 1]) |
                box_line_pair(pdist[rr], pcode[rr], tile[at - NT_BOXLINES_PITCH]) | box_line_pair(pdist[rr], pcode[rr], tile[at + NT_BOXLINES_PITCH]);
            m &= bs.kinds;
        }
        box_shade_emit(tg, bs, tab, box_shade_pixel(tg, x, y), pcode[rr], pdist[rr], pxval[rr], ps[rr], m);
    }
}

template <int N>
int launch_box_shade(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg, const NtBoxShade &bs) {
    if (tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1 || tg.colors_out) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a face-shading launch that is not for whole frames");
        return -1;
    }
    NtCameraFixed cf;
    cf.buf = cam.buf;
    cf.dots = cam.dots;
    for (int k = 0; k < 4; ++k) cf.odots[k] = cam.odots[k];
    cf.n = N;
    for (int k = 0; k < 4 * N; ++k) cf.inl[k] = cam.inl[k];
    hipStream_t st = (hipStream_t)li.stream;
    // (both shapes: 64 columns x 4 * NT_BOXROWS rows a block)
    const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + 4 * NT_BOXROWS - 1) / (4 * NT_BOXROWS)), (unsigned)li.nframes);
    if (bs.kinds) hipLaunchKernelGGL((box_shaded<N, true>), grid, dim3(256), 0, st, cf, tg, bs);
    else hipLaunchKernelGGL((box_shaded<N, false>), grid, dim3(256), 0, st, cf, tg, bs);
    return 0;
}

}  // namespace
