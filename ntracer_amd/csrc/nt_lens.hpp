// nt_lens.hpp -- renders through a lens for compile-time N.  A lens is a table of [height][width][3] fp32 coefficients
// (sx, sy, sz), the size of the view; pixel (x, y)'s primary ray leaves the camera's origin along
//     v[j] = (fwd[j] * sz + right[j] * sx) - up[j] * sy,        d = v / |v|
// with d formed as primary_dir forms it (nt_pixel.hpp: |v|^2 summed left to right, sqrtf, one IEEE division a component;
// contraction off, as everywhere).  The pinhole of flat_origin_ray_source is sz = 1, sx = fovI * (x - half_w),
// sy = fovI * (y - half_h), and with sz = 1.0f lens_dir is primary_dir bit for bit.  Every projection that keeps the eye in one
// point is such a table (fisheye, equirectangular, cylindrical, a distorted pinhole); the table does not depend on the camera.
//   * An entry whose three coefficients are all zero, or that holds a NaN, is a masked pixel: no ray is cast and the pixel
//     gets colour (0, 0, 0) through the format.
//   * The table's size is the render's width x height; the scene's fov is ignored while a lens is set.
//   * Everything behind the ray source is a render's own: the scene-box test, the walk, the shading, the packing, and the
//     switches (strict_reference, NTRACER_CLEAN_NORMALS, NTRACER_FORCE_VAR, NTRACER_COMPOSITE_KERNEL).
//   * Whole images, one sample a pixel: no bands, no supersampling, no counters, no probes (refused by the host).
// Two routes.  This file is the packet route -- opaque scenes, stack depth <= 32, NTRACER_COMPOSITE_KERNEL unset: what
// launch_composite_fixed would give the packet walk.  The walk only needs the rays of a wave to share their origin, so
// composite_packet<N, 32, false, SCAL, HITS, LENS> walks the tile with directions from the table and leaves the 16-byte record
// of every pixel, as it does for nt_hits.hpp; lens_shade, one lane a pixel, re-forms d from the table, picks the record up and
// shades with the render kernels' own device functions -- surface_color_lean / background_color for scenes without lights,
// reflection and loose primitives, composite_color<N, true, ...>(..., &hit) otherwise -- into emit_pixel.  Every other scene
// (transparent materials, the reference's normals for Solids, run-time n, BoxScene) goes through the ray-colour kernels of
// nt_rays.hpp behind an expansion of the table into directions: nt_var.hip, next to the dispatchers.
#pragma once
#include "nt_composite.hpp"

namespace {

// The shading pass behind the LENS packet walk: a 256-thread block takes a 16x16 tile of frame blockIdx.z, its four
// independent waves an 8x8 tile each (the layout of composite_kernel, which emit_pixel's shared stores of 3- and 6-byte
// pixels count on).  FEAT / SCALP as composite_kernel has them; without FEAT no LDS is used.
template <int N, bool FEAT, bool SCALP>
__global__ __launch_bounds__(256) NT_SHADE_OCC void lens_shade(NtCompositeDev sc, NtTarget tg, NtLens ln) {
    extern __shared__ float2 lds_raw[];
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const PixelRef pr = locate_pixel<16, 16>(tg, (wv & 1) * 8 + (lane & 7), (wv >> 1) * 8 + (lane >> 3), tid);
    if (!pr.valid) return;
    const float *e = ln.table + ((long long)pr.y * tg.width + pr.x) * 3;
    const float sx = e[0], sy = e[1], sz = e[2];
    Color3 c = c3(0.0f, 0.0f, 0.0f);                       // a masked pixel
    if (!lens_masked(sx, sy, sz)) {
        const float *cm = ln.cams + (size_t)blockIdx.z * 4 * N;
        float org[N], right[N], up[N], fwd[N], dir[N];
#pragma unroll
        for (int k = 0; k < N; ++k) { org[k] = cm[k]; right[k] = cm[N + k]; up[k] = cm[2 * N + k]; fwd[k] = cm[3 * N + k]; }
        lens_dir<N>(right, up, fwd, sx, sy, sz, dir);
        const float4 h = reinterpret_cast<const float4 *>(ln.hits)[pr.hit_index];
        Hit hit;
        hit.dist = h.x;
        hit.item = __float_as_int(h.y);
        hit.lane = __float_as_int(h.z);
        if (FEAT) {
            const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), wv, sc.stack_depth, N);
            Stats st = {0, 0, 0, 0, 0, 0, 0, 0};
            c = composite_color<N, true, false, SCALP>(sc, w, lane, org, dir, st, &hit);
        } else {
            c = hit.item >= 0 ? surface_color_lean<N>(sc, hit, org, dir) : background_color<N>(sc, dir);
        }
    }
    emit_pixel(tg, pr, c.r, c.g, c.b);
}

// tg: the whole image of every frame (row_begin 0, row_count = height, no bands); li.hit_buf: li.hit_frames frames of
// width * height records.  Frames are chunked by what the hit and numerator scratch hold (packet_chunk), and the
// walk is set up by packet_args and packet_chunk_head of nt_composite.hpp.
template <int N>
int launch_lens_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtLens &ln) {
    if (!sc.all_opaque || sc.checked || sc.stack_depth > 32 || !li.hit_buf || li.hit_frames < 1 || !ln.cams || !ln.table ||
        tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a lens render that is not for the packet walk");
        return -1;
    }
    const size_t lds = 4 * wave_lds_bytes(sc.stack_depth, N);
    const bool feat = scene_feat(sc);
    hipStream_t s = (hipStream_t)li.stream;
    PacketArgs pk = packet_args(li, sc, tg.width, tg.height);
    pk.hits_out = (float4 *)li.hit_buf;
    pk.lens = ln.table;
    const int chunk = packet_chunk(li, li.nframes, true);
    const NtTarget th = packet_record_view(tg, (long long)tg.width * tg.height);
    for (int f0 = 0; f0 < li.nframes; f0 += chunk) {
        const int cnt = packet_chunk_head<N>(li, sc, pk, ln.cams, f0, chunk, li.nframes);
        const dim3 pgrid = packet_grid(pk, cnt);
        if (sc.has_scalar_prims) hipLaunchKernelGGL((composite_packet<N, 32, false, true, true, true>), pgrid, dim3(256), (size_t)4 * pk.lds_per_wave, s, sc, th, pk);
        else hipLaunchKernelGGL((composite_packet<N, 32, false, false, true, true>), pgrid, dim3(256), (size_t)4 * pk.lds_per_wave, s, sc, th, pk);
        const NtTarget t2 = chunk_target(tg, f0);
        NtLens l2 = ln;
        l2.cams = pk.cams;
        l2.hits = li.hit_buf;
        dim3 g2;
        grid_for(t2, 16, 16, cnt, g2);
        if (!feat) hipLaunchKernelGGL((lens_shade<N, false, false>), g2, dim3(256), 0, s, sc, t2, l2);
        else if (sc.has_scalar_prims) hipLaunchKernelGGL((lens_shade<N, true, true>), g2, dim3(256), lds, s, sc, t2, l2);
        else hipLaunchKernelGGL((lens_shade<N, true, false>), g2, dim3(256), lds, s, sc, t2, l2);
    }
    return 0;
}

}  // namespace
