// nt_rays.hpp -- the colours of the caller's own rays for compile-time N: ray_color(target, depth 0, no source) of the reference
// (src/tracer.hpp:1856-1883) behind composite_scene::calculate_color's scene-box test, and box_scene::calculate_color
// (:101-114), for `count` arbitrary rays read from device memory.  The shading is the render kernels' own (composite_color,
// composite_color_t, box_color) -- a batch of rays is a render whose ray source is an array: one lane per ray, four independent
// waves a block, lane l of block b takes ray 256 b + l and the blocks stride on where the grid is capped.  A wave's 64 rays are
// one contiguous run of 256 N bytes of `directions` (and of `origins`, unless one origin is shared: that one is a wave-uniform
// load), so the plain per-lane loads use every line they fetch.  The direction is normalised exactly as primary_dir does it.
// No packet walk and no stretch codes: the rays of a batch need not be coherent, and there are no stretches.
// Where a colour goes is the NtTarget's business (emit_pixel): rgb[ray] through colors_out, or pixel (ray % width, ray / width)
// of an image in any format.  Instantiated per N by nt_inst_rays.hip; the run-time-n kernels and the dispatcher
// (nt_launch_rays) are in nt_var.hip.
#pragma once
#include "nt_box.hpp"
#include "nt_composite.hpp"

namespace {

// ray r of the batch: the origin as given, the direction divided by its length (flat_origin_ray_source's own normalisation,
// tracer.hpp:71-75: |v|^2 summed left to right, sqrtf, one IEEE division per component)
template <int N>
__device__ __forceinline__ void rays_load(const NtRayJob &job, long long r, float (&o)[N], float (&d)[N]) {
    const float *pd = job.directions + r * N;
#pragma unroll
    for (int k = 0; k < N; ++k) d[k] = pd[k];
    if (job.shared_origin) {
#pragma unroll
        for (int k = 0; k < N; ++k) o[k] = job.origins[k];
    } else {
        const float *po = job.origins + r * N;
#pragma unroll
        for (int k = 0; k < N; ++k) o[k] = po[k];
    }
    float sq = d[0] * d[0];
#pragma unroll
    for (int k = 1; k < N; ++k) sq = sq + d[k] * d[k];
    const float len = sqrtf(sq);
#pragma unroll
    for (int k = 0; k < N; ++k) d[k] = d[k] / len;
}

// where ray r's colour goes: its row of colors_out, or its pixel of the image (whole image, no bands)
__device__ __forceinline__ PixelRef rays_pixel(const NtTarget &tg, long long r) {
    PixelRef pr;
    pr.valid = true;
    pr.hit_index = 0;
    if (tg.colors_out) {
        pr.x = 0;
        pr.y = 0;
        pr.offset = r;
    } else {
        pr.y = (int)(r / tg.width);
        pr.x = (int)(r - (long long)pr.y * tg.width);
        pr.offset = (long long)pr.y * tg.pitch + (long long)pr.x * tg.bpp;
    }
    return pr;
}

// Opaque scenes without Solids (or with them under NTRACER_CLEAN_NORMALS=1): composite_color with the 16-slot mailbox.
// FEAT: lights, shadows, reflection, loose triangles and solids, chosen as a render chooses it; SCALP: the leaves hold more
// than batches.
template <int N, bool FEAT, bool SCALP>
__global__ __launch_bounds__(256) void rays_color(NtCompositeDev sc, NtRayJob job, NtTarget tg) {
    extern __shared__ float2 lds_raw[];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), tid >> 6, sc.stack_depth, N);
    for (long long base = (long long)blockIdx.x * 256; base < job.count; base += (long long)gridDim.x * 256) {
        if (nt_aborted(tg)) return;                       // (the four waves of a block are independent: no barrier below)
        const long long r = base + tid;
        if (r >= job.count) continue;
        float o[N], d[N];
        rays_load<N>(job, r, o, d);
        Stats st = {0, 0, 0, 0, 0, 0, 0, 0};
        const Color3 c = composite_color<N, FEAT, false, SCALP>(sc, w, lane, o, d, st);
        emit_pixel(tg, rays_pixel(tg, r), c.r, c.g, c.b);
    }
}

// Scenes with transparent materials or Solids: composite_color_t on the exact `checked` list, a bitmap column per resident
// lane -- the grid is what that scratch has columns for.  ALIAS: o_hit.normal as the reference's walk leaves it.
template <int N, bool ALIAS>
__global__ __launch_bounds__(256) void rays_color_t(NtCompositeDev sc, NtRayJob job, NtTarget tg) {
    extern __shared__ float2 lds_raw[];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), tid >> 6, sc.stack_depth, N);
    Checked ck;
    ck.bits = sc.checked + ((long long)blockIdx.x * 256 + tid);
    ck.stride = sc.checked_lanes;
    ck.words = sc.checked_words;
    ck.n_batches = sc.n_batches;
    ck.n_triangles = sc.n_triangles;
    for (long long base = (long long)blockIdx.x * 256; base < job.count; base += (long long)gridDim.x * 256) {
        if (nt_aborted(tg)) return;
        const long long r = base + tid;
        if (r >= job.count) continue;
        float o[N], d[N];
        rays_load<N>(job, r, o, d);
        const Color3 c = composite_color_t<N, ALIAS>(sc, w, lane, o, d, ck);
        emit_pixel(tg, rays_pixel(tg, r), c.r, c.g, c.b);
    }
}

// BoxScene: box_color's complete reference-ordered evaluation for every ray (no circumsphere rejection in front: it works from
// the camera's dot products, and a miss costs the candidate search alone)
template <int N>
__global__ __launch_bounds__(256) void rays_box(NtRayJob job, NtTarget tg) {
    const int tid = (int)threadIdx.x;
    for (long long base = (long long)blockIdx.x * 256; base < job.count; base += (long long)gridDim.x * 256) {
        if (nt_aborted(tg)) return;
        const long long r = base + tid;
        if (r >= job.count) continue;
        float o[N], d[N];
        rays_load<N>(job, r, o, d);
        float cr, cg, cb;
        box_color<N>(o, d, true, cr, cg, cb);
        emit_pixel(tg, rays_pixel(tg, r), cr, cg, cb);
    }
}

template <int N>
int launch_rays_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtRayJob &job, const NtTarget &tg) {
    // per wave what the per-lane render kernels use: stack [depth + 1][64], ray table, mailbox
    size_t lds;
    if (const int r = lane_walk_lds(sc, N, 4, 160 * 1024, lds)) return r;
    hipStream_t s = (hipStream_t)li.stream;
    const long long blocks = ((long long)job.count + 255) / 256;
    if (sc.checked) {
        const dim3 tgrid((unsigned)checked_column_blocks(sc, 256, blocks));
        if (sc.alias_normals) hipLaunchKernelGGL((rays_color_t<N, true>), tgrid, dim3(256), lds, s, sc, job, tg);
        else hipLaunchKernelGGL((rays_color_t<N, false>), tgrid, dim3(256), lds, s, sc, job, tg);
        return 0;
    }
    if (!sc.all_opaque) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: transparent scene without the checked-list scratch");
        return -1;
    }
    const dim3 grid((unsigned)strided_blocks(blocks));
    const bool feat = scene_feat(sc);
    if (feat && !sc.has_scalar_prims) hipLaunchKernelGGL((rays_color<N, true, false>), grid, dim3(256), lds, s, sc, job, tg);
    else if (feat) hipLaunchKernelGGL((rays_color<N, true, true>), grid, dim3(256), lds, s, sc, job, tg);
    else hipLaunchKernelGGL((rays_color<N, false, false>), grid, dim3(256), lds, s, sc, job, tg);
    return 0;
}

template <int N>
int launch_rays_box_fixed(const NtLaunchInfo &li, const NtRayJob &job, const NtTarget &tg) {
    long long blocks = ((long long)job.count + 255) / 256;
    if (blocks > NT_RAYS_MAX_BLOCKS) blocks = NT_RAYS_MAX_BLOCKS;
    hipLaunchKernelGGL((rays_box<N>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)li.stream, job, tg);
    return 0;
}

}  // namespace
