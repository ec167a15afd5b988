// nt_cue.hpp -- depth cues for compile-time N (nt_scene_set_depth_cue): a surface fades towards a fog colour with
// its distance from the eye and is tinted by where its visible point lies along a direction of n-space, from the primary-hit
// records of the render itself.
//
// A pixel's two factors (f, g) come from its own record, its own ray and the camera's origin (ntracer_hip.h has the rule in
// full; cue_pixel and cue_blend below are its one copy, for these kernels and the run-time-n ones of nt_var.hip): no neighbour
// is read and no normal rebuilt.  composite_packet<N, 32, false, SCAL, true> walks the view once into 16-byte records, as it
// does for nt_hits.hpp and nt_outline.hpp, and cue_shade, one lane a pixel, re-forms its ray, picks its record up, shades from
// it exactly as lens_shade does, clamps, applies the two factors and emits.  cue_factors_fixed is the same without the
// shading: the floats of nt_depth_cue_factors.  Opaque scenes on the packet walk only (what launch_composite_fixed would give
// it); every other scene goes through a primary-hit pass and the run-time-n kernels in nt_var.hip.  Instantiated per N by
// nt_inst_cue.hip.
#pragma once
#include "nt_hits.hpp"

namespace {

__device__ __forceinline__ float cue_clamp01(float v) { return fmaxf(0.0f, fminf(1.0f, v)); }

// (f, g) of a pixel whose record is `rec` = {dist, item, lane, n_transparent}; dir(k) and org(k) hand over component k of the
// pixel's unit direction and of the camera's origin, and are called only for a hit under a tint
template <typename DIR, typename ORG>
__device__ __forceinline__ void cue_pixel(const NtCue &cu, const int4 &rec, int n, DIR dir, ORG org, float &f, float &g) {
    f = -1.0f;
    g = -1.0f;
    if (rec.y >= 0) {
        const float t = __int_as_float(rec.x);
        f = cue_clamp01((t - cu.fog_near) * cu.inv_fog);
        if (cu.tint) {
            float s = cu.tint_axis[0] * ((dir(0) * t) + org(0));
#pragma unroll
            for (int k = 1; k < n; ++k) s = s + (cu.tint_axis[k] * ((dir(k) * t) + org(k)));
            g = cue_clamp01((s - cu.tint_lo) * cu.inv_tint);
        }
    } else if (cu.fog_background && rec.w == 0) {
        f = 1.0f;
    }
}

// Q of the rule from P = p, a pixel of the plain frame clamped to [0, 1]
__device__ __forceinline__ void cue_blend(const NtCue &cu, float f, float g, float (&p)[3]) {
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

// the factors of a pixel on its own ray (org, dir): n is the constant N, and the loop of cue_pixel unrolls over the registers
template <int N>
__device__ __forceinline__ void cue_pixel_fixed(const NtCue &cu, const int4 &rec, const float (&org)[N], const float (&dir)[N], float &f, float &g) {
    cue_pixel(cu, rec, N, [&](int k) { return dir[k]; }, [&](int k) { return org[k]; }, f, g);
}

// The shading pass behind the packet walk: lens_shade's geometry (a 256-thread block takes a 16x16 tile of frame blockIdx.z, its
// four independent waves an 8x8 tile each) and lens_shade's shading, with the rule in front of emit_pixel.
template <int N, bool FEAT, bool SCALP>
__global__ __launch_bounds__(256) NT_SHADE_OCC void cue_shade(NtCompositeDev sc, NtTarget tg, NtCue cu) {
    extern __shared__ float2 lds_raw[];
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const PixelRef pr = locate_pixel<16, 16>(tg, (wv & 1) * 8 + (lane & 7), (wv >> 1) * 8 + (lane >> 3), tid);
    if (!pr.valid) return;
    const float *cm = cu.cams + (size_t)blockIdx.z * 4 * N;
    float org[N], right[N], up[N], fwd[N], dir[N];
#pragma unroll
    for (int k = 0; k < N; ++k) { org[k] = cm[k]; right[k] = cm[N + k]; up[k] = cm[2 * N + k]; fwd[k] = cm[3 * N + k]; }
    primary_dir<N>(tg, right, up, fwd, pr.x, pr.y, dir);
    const int4 rec = reinterpret_cast<const int4 *>(cu.recs)[pr.hit_index];
    Hit hit;
    hit.dist = __int_as_float(rec.x);
    hit.item = rec.y;
    hit.lane = rec.z;
    float f, g;
    cue_pixel_fixed<N>(cu, rec, org, dir, f, g);
    Color3 c;
    if (FEAT) {
        const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), wv, sc.stack_depth, N);
        Stats st = {0, 0, 0, 0, 0, 0, 0, 0};
        c = composite_color<N, true, false, SCALP>(sc, w, lane, org, dir, st, &hit);
    } else {
        c = hit.item >= 0 ? surface_color_lean<N>(sc, hit, org, dir) : background_color<N>(sc, dir);
    }
    // P: the plain frame's pixel, clamped as the packer of a base frame clamps it (what the general route starts from)
    float p[3] = {c.r, c.g, c.b};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = p[k] > 0.0f ? p[k] : 0.0f;
        p[k] = v < 1.0f ? v : 1.0f;
    }
    cue_blend(cu, f, g, p);
    emit_pixel(tg, pr, p[0], p[1], p[2]);
}

// the factors alone: hits_normals' geometry, the blocks striding over [frame][tile row][tile column]
template <int N>
__global__ __launch_bounds__(256) void cue_factors_fixed(NtTarget tg, NtCue cu, int tiles_x, int tiles_y) {
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int px = (wv & 1) * 8 + (lane & 7), py = (wv >> 1) * 8 + (lane >> 3);
    NtHits h;
    h.cams = cu.cams;
    h.nframes = cu.nframes;
    h.frame_stride = (long long)tg.width * tg.height;
    const int4 *recs = reinterpret_cast<const int4 *>(cu.recs);
    const long long total = (long long)tiles_x * tiles_y * cu.nframes;
    for (long long tile = (long long)blockIdx.x; tile < total; tile += gridDim.x) {
        if (nt_aborted(tg)) return;
        const HitsPixel p = hits_pixel<16, 16>(tg, h, tile, tiles_x, tiles_y, px, py);
        if (!p.valid) continue;
        float org[N], dir[N];
        hits_ray<N>(tg, h, p, org, dir);
        float f, g;
        cue_pixel_fixed<N>(cu, recs[p.rec], org, dir, f, g);
        reinterpret_cast<float2 *>(cu.factors)[p.rec] = make_float2(f, g);
    }
}

// tg: the whole image of every frame (row_begin 0, row_count = height, no bands), or with `draw` false the view alone;
// li.hit_buf: li.hit_frames frames of width * height records.  Frames are chunked by what the hit and numerator scratch hold
// (packet_chunk); the walk is set up by packet_args and packet_chunk_head of nt_composite.hpp.
template <int N>
int launch_cue_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtCue &cu, bool draw) {
    if (!sc.all_opaque || sc.checked || sc.stack_depth > 32 || li.kernel_choice != 0 || !li.hit_buf || li.hit_frames < 1 || !cu.cams ||
        tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1 || (!draw && !cu.factors)) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a depth cue launch that is not for the packet walk");
        return -1;
    }
    const size_t lds = 4 * wave_lds_bytes(sc.stack_depth, N);
    const bool feat = scene_feat(sc);
    hipStream_t s = (hipStream_t)li.stream;
    PacketArgs pk = packet_args(li, sc, tg.width, tg.height);
    pk.hits_out = (float4 *)li.hit_buf;
    const int chunk = packet_chunk(li, li.nframes, true);
    const long long px = (long long)tg.width * tg.height;
    const NtTarget th = packet_record_view(tg, px);
    for (int f0 = 0; f0 < li.nframes; f0 += chunk) {
        const int cnt = packet_chunk_head<N>(li, sc, pk, cu.cams, f0, chunk, li.nframes);
        const dim3 pgrid = packet_grid(pk, cnt);
        if (sc.has_scalar_prims) hipLaunchKernelGGL((composite_packet<N, 32, false, true, true>), pgrid, dim3(256), (size_t)4 * pk.lds_per_wave, s, sc, th, pk);
        else hipLaunchKernelGGL((composite_packet<N, 32, false, false, true>), pgrid, dim3(256), (size_t)4 * pk.lds_per_wave, s, sc, th, pk);
        NtCue c2 = cu;
        c2.cams = pk.cams;
        c2.nframes = cnt;
        c2.recs = li.hit_buf;
        if (draw) {
            const NtTarget t2 = chunk_target(tg, f0);
            dim3 g2;
            grid_for(t2, 16, 16, cnt, g2);
            if (!feat) hipLaunchKernelGGL((cue_shade<N, false, false>), g2, dim3(256), 0, s, sc, t2, c2);
            else if (sc.has_scalar_prims) hipLaunchKernelGGL((cue_shade<N, true, true>), g2, dim3(256), lds, s, sc, t2, c2);
            else hipLaunchKernelGGL((cue_shade<N, true, false>), g2, dim3(256), lds, s, sc, t2, c2);
        } else {
            c2.factors = cu.factors + (long long)f0 * px * 2;
            const int tiles_x = (tg.width + 15) / 16, tiles_y = (tg.height + 15) / 16;
            const long long tiles = (long long)tiles_x * tiles_y * cnt;
            const dim3 grid((unsigned)strided_blocks(tiles));
            hipLaunchKernelGGL((cue_factors_fixed<N>), grid, dim3(256), 0, s, tg, c2, tiles_x, tiles_y);
        }
    }
    return 0;
}

}  // namespace
