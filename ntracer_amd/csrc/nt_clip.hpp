// nt_clip.hpp -- cutaway views for compile-time N (nt_scene_set_clip_planes): up to NT_DEV_CLIP_MAX planes
// a . x <= b whose keep-region every ray of a render honours -- primary, shadow and reflection rays alike -- so that the
// geometry cut away casts no shadow and shows in no mirror.  There are no caps: a cut shell is open and its inner side is seen.
//
// A convex keep-region meets a ray in one interval [t0, t1] (ntracer_hip.h has the rule in full; clip_window in
// nt_composite.hpp is its one copy for these kernels).  composite_packet<N, 32, false, SCAL, true, false, true> walks the view
// once into 16-byte records as it does for nt_hits.hpp -- the lane's window folded into active, t_near and t_far, and a
// candidate accepted only inside it -- and clip_shade, one lane a pixel, re-forms its ray, picks its record up and shades
// from it exactly as lens_shade does: surface_color_lean for unlit scenes, otherwise composite_color with ClipOn threaded
// through trace_closest / leaf_closest / trace_occluded / leaf_occludes.  A primary-hit pass under clip is that same walk, with
// hits_normals behind it when normal rows are asked for.  Opaque scenes on the packet walk only (what launch_composite_fixed
// would give it); every other scene goes through the run-time-n kernels in nt_var.hip.  Instantiated per N by nt_inst_clip.hip.
#pragma once
#include "nt_hits.hpp"

namespace {

// The shading pass behind the packet walk: lens_shade's geometry (a 256-thread block takes a 16x16 tile of frame blockIdx.z, its
// four independent waves an 8x8 tile each) and lens_shade's shading, every secondary ray under the planes.
template <int N, bool FEAT, bool SCALP>
__global__ __launch_bounds__(256) NT_SHADE_OCC void clip_shade(NtCompositeDev sc, NtTarget tg, NtClip cl) {
    extern __shared__ float2 lds_raw[];
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const PixelRef pr = locate_pixel<16, 16>(tg, (wv & 1) * 8 + (lane & 7), (wv >> 1) * 8 + (lane >> 3), tid);
    if (!pr.valid) return;
    const float *cm = cl.cams + (size_t)blockIdx.z * 4 * N;
    float org[N], right[N], up[N], fwd[N], dir[N];
#pragma unroll
    for (int k = 0; k < N; ++k) { org[k] = cm[k]; right[k] = cm[N + k]; up[k] = cm[2 * N + k]; fwd[k] = cm[3 * N + k]; }
    primary_dir<N>(tg, right, up, fwd, pr.x, pr.y, dir);
    const int4 rec = reinterpret_cast<const int4 *>(cl.hits)[pr.hit_index];
    Hit hit;
    hit.dist = __int_as_float(rec.x);
    hit.item = rec.y;
    hit.lane = rec.z;
    Color3 c;
    if (FEAT) {
        const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), wv, sc.stack_depth, N);
        Stats st = {0, 0, 0, 0, 0, 0, 0, 0};
        NtCompositeClip scc;                  // the scene with the planes behind it: what the ClipOn walks are handed
        static_cast<NtCompositeDev &>(scc) = sc;
        scc.clip = cl.planes;
        scc.clip_count = cl.count;
        c = composite_color<N, true, false, SCALP, ClipOn>(scc, w, lane, org, dir, st, &hit);
    } else {
        c = hit.item >= 0 ? surface_color_lean<N>(sc, hit, org, dir) : background_color<N>(sc, dir);
    }
    emit_pixel(tg, pr, c.r, c.g, c.b);
}

// draw: tg is the whole image of every frame (row_begin 0, row_count = height, no bands) and li.hit_buf holds li.hit_frames
// frames of width * height records; otherwise tg is the view alone and the records go to cl.hits, cl.frame_stride of them a
// frame, with the normal rows of the pixels that hit behind them.  Frames are chunked by what the hit and numerator scratch
// hold (packet_chunk); the walk is set up by packet_args and packet_chunk_head of nt_composite.hpp.
template <int N>
int launch_clip_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtClip &cl, bool draw) {
    if (!sc.all_opaque || sc.checked || sc.stack_depth > 32 || li.kernel_choice != 0 || !cl.cams || !cl.planes || cl.count < 1 ||
        cl.count > NT_DEV_CLIP_MAX || (draw && (!li.hit_buf || li.hit_frames < 1 || tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1)) ||
        (!draw && !cl.hits)) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a clip launch that is not for the packet walk");
        return -1;
    }
    const size_t lds = 4 * wave_lds_bytes(sc.stack_depth, N);
    const bool feat = scene_feat(sc);
    hipStream_t s = (hipStream_t)li.stream;
    PacketArgs pk = packet_args(li, sc, tg.width, tg.height);
    pk.clip = cl.planes;
    pk.clip_count = cl.count;
    const int chunk = packet_chunk(li, li.nframes, draw);
    const NtTarget th = packet_record_view(tg, draw ? (long long)tg.width * tg.height : cl.frame_stride);
    for (int f0 = 0; f0 < li.nframes; f0 += chunk) {
        const int cnt = packet_chunk_head<N>(li, sc, pk, cl.cams, f0, chunk, li.nframes);
        pk.hits_out = draw ? (float4 *)li.hit_buf : reinterpret_cast<float4 *>(cl.hits) + (long long)f0 * cl.frame_stride;
        const dim3 pgrid = packet_grid(pk, cnt);
        if (sc.has_scalar_prims) hipLaunchKernelGGL((composite_packet<N, 32, false, true, true, false, true>), pgrid, dim3(256), (size_t)4 * pk.lds_per_wave, s, sc, th, pk);
        else hipLaunchKernelGGL((composite_packet<N, 32, false, false, true, false, true>), pgrid, dim3(256), (size_t)4 * pk.lds_per_wave, s, sc, th, pk);
        if (!draw) continue;
        NtClip c2 = cl;
        c2.cams = pk.cams;
        c2.nframes = cnt;
        c2.hits = li.hit_buf;
        const NtTarget t2 = chunk_target(tg, f0);
        dim3 g2;
        grid_for(t2, 16, 16, cnt, g2);
        if (!feat) hipLaunchKernelGGL((clip_shade<N, false, false>), g2, dim3(256), 0, s, sc, t2, c2);
        else if (sc.has_scalar_prims) hipLaunchKernelGGL((clip_shade<N, true, true>), g2, dim3(256), lds, s, sc, t2, c2);
        else hipLaunchKernelGGL((clip_shade<N, true, false>), g2, dim3(256), lds, s, sc, t2, c2);
    }
    if (!draw && (cl.normal_origin || cl.normal_dir)) {
        // the normal rays of the records, as launch_hits_fixed adds them
        NtHits h;
        h.cams = cl.cams;
        h.nframes = li.nframes;
        h.frame_stride = cl.frame_stride;
        h.hits = cl.hits;
        h.normal_origin = cl.normal_origin;
        h.normal_dir = cl.normal_dir;
        const int tiles_x = (tg.width + 15) / 16, tiles_y = (tg.height + 15) / 16;
        const long long tiles = (long long)tiles_x * tiles_y * li.nframes;
        const dim3 grid((unsigned)strided_blocks(tiles));
        if (sc.has_scalar_prims) hipLaunchKernelGGL((hits_normals<N, true>), grid, dim3(256), 0, s, sc, tg, h, tiles_x, tiles_y);
        else hipLaunchKernelGGL((hits_normals<N, false>), grid, dim3(256), 0, s, sc, tg, h, tiles_x, tiles_y);
    }
    return 0;
}

}  // namespace
