// nt_outline.hpp -- outlines for compile-time N (nt_scene_set_outlines): a line along the silhouette, along every
// edge where two facets meet at an angle and along every jump in depth, from the primary-hit records of the render itself.
//
// The mask byte of a pixel p with an opaque hit is the OR of outline_pair(p, q) over its four neighbours q inside the image
// (ntracer_hip.h has the rule in full; outline_pair below is its one copy, for these kernels and the run-time-n ones of
// nt_var.hip).  The rule looks at the two records first -- a miss next door, the same simplex, the farther of the two -- and
// only a pair that passes needs the two normal rays, which is a few percent of the pixels.  So this route keeps no normal rows:
// composite_packet<N, 32, false, SCAL, true> walks the view once into 16-byte records, as it does for nt_hits.hpp, and
// outline_shade, one lane a pixel, reads its own record and its neighbours', rebuilds both normals with hit_normal on each
// pixel's own ray where the rule asks for them (the bits hits_normals would have stored), shades from its record exactly as
// lens_shade does, clamps, blends and emits.  outline_mark_fixed is the same without the shading: the bytes of nt_outline_mask.
// Opaque scenes on the packet walk only (what launch_composite_fixed would give it); every other scene goes through a
// primary-hit pass with normal rows and the run-time-n kernels in nt_var.hip.  Instantiated per N by nt_inst_outline.hip.
#pragma once
#include "nt_hits.hpp"

namespace {

// What neighbour q adds to the mask byte of p, a pixel with an opaque hit; the records are {dist, item, lane, -}.  `dots` hands
// over c = nd(p).nd(q), la = nd(p).nd(p), lb = nd(q).nd(q), each summed left to right, and is called for no other pair than
// those whose normals the rule reads.
template <typename DOTS>
__device__ __forceinline__ int outline_pair(const int4 &p, const int4 &q, float cc, float depth_gap, DOTS dots) {
    if (q.y < 0) return NT_DEV_OUTLINE_SILHOUETTE;
    if (q.y == p.y && q.z == p.z) return 0;
    const float dp = __int_as_float(p.x), dq = __int_as_float(q.x);
    if (dp > dq) return 0;
    float c, la, lb;
    dots(c, la, lb);
    int m = 0;
    if (c * c < cc * (la * lb)) m |= NT_DEV_OUTLINE_CREASE;
    if (depth_gap > 0.0f && (dq - dp) > depth_gap * dp) m |= NT_DEV_OUTLINE_DEPTH;
    return m;
}

// the mask byte of pixel (x, y) of frame `frame`, whose record is `rec` with rec.y >= 0, on its own ray (org, dir): the four
// neighbours' records from `recs` ([frame][height][width]) and, where the rule asks, both normals rebuilt
template <int N, bool SCALP>
__device__ __forceinline__ int outline_mask_fixed(const NtCompositeDev &sc, const NtTarget &tg, const int4 *recs, int frame, int x, int y,
                                                  const int4 &rec, const float (&org)[N], const float (&right)[N], const float (&up)[N],
                                                  const float (&fwd)[N], const float (&dir)[N], float cc, float depth_gap) {
    const int4 *fr = recs + (long long)frame * tg.height * tg.width;
    int m = 0;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int qx = x + (k == 0 ? -1 : (k == 1 ? 1 : 0));
        const int qy = y + (k == 2 ? -1 : (k == 3 ? 1 : 0));
        if (qx < 0 || qy < 0 || qx >= tg.width || qy >= tg.height) continue;
        const int4 q = fr[(long long)qy * tg.width + qx];
        m |= outline_pair(rec, q, cc, depth_gap, [&](float &c, float &la, float &lb) {
            Hit hp, hq;
            hp.dist = __int_as_float(rec.x); hp.item = rec.y; hp.lane = rec.z;
            hq.dist = __int_as_float(q.x); hq.item = q.y; hq.lane = q.z;
            float qd[N], no[N], na[N], nb[N];
            primary_dir<N>(tg, right, up, fwd, qx, qy, qd);
            hit_normal<N, SCALP>(sc, hp, org, dir, no, na);
            hit_normal<N, SCALP>(sc, hq, org, qd, no, nb);
            c = dotN<N>(na, nb);
            la = dotN<N>(na, na);
            lb = dotN<N>(nb, nb);
        });
    }
    return m;
}

// The shading pass behind the packet walk: lens_shade's geometry (a 256-thread block takes a 16x16 tile of frame blockIdx.z, its
// four independent waves an 8x8 tile each) and lens_shade's shading, with the blend in front of emit_pixel.
template <int N, bool FEAT, bool SCALP>
__global__ __launch_bounds__(256) NT_SHADE_OCC void outline_shade(NtCompositeDev sc, NtTarget tg, NtOutline ol) {
    extern __shared__ float2 lds_raw[];
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const PixelRef pr = locate_pixel<16, 16>(tg, (wv & 1) * 8 + (lane & 7), (wv >> 1) * 8 + (lane >> 3), tid);
    if (!pr.valid) return;
    const float *cm = ol.cams + (size_t)blockIdx.z * 4 * N;
    float org[N], right[N], up[N], fwd[N], dir[N];
#pragma unroll
    for (int k = 0; k < N; ++k) { org[k] = cm[k]; right[k] = cm[N + k]; up[k] = cm[2 * N + k]; fwd[k] = cm[3 * N + k]; }
    primary_dir<N>(tg, right, up, fwd, pr.x, pr.y, dir);
    const int4 *recs = reinterpret_cast<const int4 *>(ol.recs);
    const int4 rec = recs[pr.hit_index];
    Hit hit;
    hit.dist = __int_as_float(rec.x);
    hit.item = rec.y;
    hit.lane = rec.z;
    int m = 0;
    if (rec.y >= 0) m = outline_mask_fixed<N, SCALP>(sc, tg, recs, (int)blockIdx.z, pr.x, pr.y, rec, org, right, up, fwd, dir, ol.cc, ol.depth_gap);
    Color3 c;
    if (FEAT) {
        const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), wv, sc.stack_depth, N);
        Stats st = {0, 0, 0, 0, 0, 0, 0, 0};
        c = composite_color<N, true, false, SCALP>(sc, w, lane, org, dir, st, &hit);
    } else {
        c = hit.item >= 0 ? surface_color_lean<N>(sc, hit, org, dir) : background_color<N>(sc, dir);
    }
    // P: the plain frame's pixel, clamped as the packer of a base frame clamps it (marked or not: what the general route emits)
    const float keep = 1.0f - ol.strength;
    float p[3] = {c.r, c.g, c.b};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = p[k] > 0.0f ? p[k] : 0.0f;
        v = v < 1.0f ? v : 1.0f;
        p[k] = m != 0 ? (v * keep) + (ol.color[k] * ol.strength) : v;
    }
    c = c3(p[0], p[1], p[2]);
    emit_pixel(tg, pr, c.r, c.g, c.b);
}

// the mask bytes alone: hits_normals' geometry, the blocks striding over [frame][tile row][tile column]
template <int N, bool SCALP>
__global__ __launch_bounds__(256) void outline_mark_fixed(NtCompositeDev sc, NtTarget tg, NtOutline ol, int tiles_x, int tiles_y) {
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int px = (wv & 1) * 8 + (lane & 7), py = (wv >> 1) * 8 + (lane >> 3);
    NtHits h;
    h.cams = ol.cams;
    h.nframes = ol.nframes;
    h.frame_stride = (long long)tg.width * tg.height;
    const int4 *recs = reinterpret_cast<const int4 *>(ol.recs);
    const long long total = (long long)tiles_x * tiles_y * ol.nframes;
    for (long long tile = (long long)blockIdx.x; tile < total; tile += gridDim.x) {
        if (nt_aborted(tg)) return;
        const HitsPixel p = hits_pixel<16, 16>(tg, h, tile, tiles_x, tiles_y, px, py);
        if (!p.valid) continue;
        const int4 rec = recs[p.rec];
        int m = 0;
        if (rec.y >= 0) {
            const float *cm = ol.cams + (size_t)p.frame * 4 * N;
            float org[N], right[N], up[N], fwd[N], dir[N];
#pragma unroll
            for (int k = 0; k < N; ++k) { org[k] = cm[k]; right[k] = cm[N + k]; up[k] = cm[2 * N + k]; fwd[k] = cm[3 * N + k]; }
            primary_dir<N>(tg, right, up, fwd, p.x, p.y, dir);
            m = outline_mask_fixed<N, SCALP>(sc, tg, recs, p.frame, p.x, p.y, rec, org, right, up, fwd, dir, ol.cc, ol.depth_gap);
        }
        ol.mask[p.rec] = (uint8_t)m;
    }
}

// tg: the whole image of every frame (row_begin 0, row_count = height, no bands), or with `draw` false the view alone;
// li.hit_buf: li.hit_frames frames of width * height records.  Frames are chunked by what the hit and numerator scratch hold
// (packet_chunk); the walk is set up by packet_args and packet_chunk_head of nt_composite.hpp.
template <int N>
int launch_outline_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtOutline &ol, bool draw) {
    if (!sc.all_opaque || sc.checked || sc.stack_depth > 32 || li.kernel_choice != 0 || !li.hit_buf || li.hit_frames < 1 || !ol.cams ||
        tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1 || (!draw && !ol.mask)) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: an outline launch that is not for the packet walk");
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
        const int cnt = packet_chunk_head<N>(li, sc, pk, ol.cams, f0, chunk, li.nframes);
        const dim3 pgrid = packet_grid(pk, cnt);
        if (sc.has_scalar_prims) hipLaunchKernelGGL((composite_packet<N, 32, false, true, true>), pgrid, dim3(256), (size_t)4 * pk.lds_per_wave, s, sc, th, pk);
        else hipLaunchKernelGGL((composite_packet<N, 32, false, false, true>), pgrid, dim3(256), (size_t)4 * pk.lds_per_wave, s, sc, th, pk);
        NtOutline o2 = ol;
        o2.cams = pk.cams;
        o2.nframes = cnt;
        o2.recs = li.hit_buf;
        if (draw) {
            const NtTarget t2 = chunk_target(tg, f0);
            dim3 g2;
            grid_for(t2, 16, 16, cnt, g2);
            if (!feat) hipLaunchKernelGGL((outline_shade<N, false, false>), g2, dim3(256), 0, s, sc, t2, o2);
            else if (sc.has_scalar_prims) hipLaunchKernelGGL((outline_shade<N, true, true>), g2, dim3(256), lds, s, sc, t2, o2);
            else hipLaunchKernelGGL((outline_shade<N, true, false>), g2, dim3(256), lds, s, sc, t2, o2);
        } else {
            o2.mask = ol.mask + (long long)f0 * px;
            const int tiles_x = (tg.width + 15) / 16, tiles_y = (tg.height + 15) / 16;
            const long long tiles = (long long)tiles_x * tiles_y * cnt;
            const dim3 grid((unsigned)strided_blocks(tiles));
            if (sc.has_scalar_prims) hipLaunchKernelGGL((outline_mark_fixed<N, true>), grid, dim3(256), 0, s, sc, tg, o2, tiles_x, tiles_y);
            else hipLaunchKernelGGL((outline_mark_fixed<N, false>), grid, dim3(256), 0, s, sc, tg, o2, tiles_x, tiles_y);
        }
    }
    return 0;
}

}  // namespace
