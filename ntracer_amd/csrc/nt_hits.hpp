// nt_hits.hpp -- primary-hit buffers for compile-time N: what is under each pixel of a view.  For pixel (x, y) of every
// frame the record of composite_scene::ray_color at depth 0 up to the point where shading starts (tracer.hpp:1856-1868):
// d = primary_dir(x, y), t0 = aabb_distance(origin, d), and for t0 >= 0 kd_node_intersection on the root with t_near = t0,
// t_far = FLT_MAX and no source; one 16-byte record (nt_ray_hit) a pixel, optionally o_hit.normal of the pixels that hit.
// The walks are the render kernels' own and run as a render of the scene would run them:
//   composite_packet     opaque scenes, stack depth <= 32: the renders' packet walk (nt_composite.hpp) instantiated with HITS
//                        set -- one wave an 8x8 tile, 2x2 tiles a block, quads in the host's centre-first order, plane
//                        numerators from packet_numerators, the wave mailbox; nothing is shaded
//   hits_normals         the normal rays behind the packet walk, only when asked for: one lane a pixel rebuilds the ray, reads the
//                        record and calls hit_normal -- the packet kernel itself does not grow
//   hits_closest         opaque scenes on the per-lane walk (trace_closest): NTRACER_COMPOSITE_KERNEL != 0, or a deeper stack
//   hits_closest_t       transparent materials, and Solids with the reference's o_hit.normal handling (trace_closest_t on the
//                        exact `checked` list, a bitmap column per resident lane: the grid is what the scratch has columns for)
// The per-lane kernels are the query kernels of nt_query.hpp with the camera as the ray source: a 256-thread block takes a
// 16x16 tile, its four independent waves an 8x8 tile each -- a wave's rays stay neighbours -- and the blocks stride over
// [frame][tile row][tile column].  Instantiated per N by nt_inst_hits.hip; the run-time-n kernels and the dispatcher
// (nt_launch_hits) are in nt_var.hip.
#pragma once
#include "nt_query.hpp"

namespace {

struct HitsPixel {
    int x, y, frame;
    long long rec;      // index of the pixel's record, and of its normal rows
    bool valid;
};

// position (px, py) of tile `tile` of the launch, tiles of BW x BH pixels numbered [frame][tile row][tile column]
template <int BW, int BH>
__device__ __forceinline__ HitsPixel hits_pixel(const NtTarget &tg, const NtHits &h, long long tile, int tiles_x, int tiles_y, int px, int py) {
    HitsPixel p;
    p.frame = (int)(tile / ((long long)tiles_x * tiles_y));
    const int rem = (int)(tile - (long long)p.frame * tiles_x * tiles_y);
    const int by = rem / tiles_x;
    p.x = (rem - by * tiles_x) * BW + px;
    p.y = by * BH + py;
    p.valid = p.x < tg.width && p.y < tg.height;
    p.rec = (long long)p.frame * h.frame_stride + (long long)p.y * tg.width + p.x;
    return p;
}

// the pixel's ray: the frame's camera and flat_origin_ray_source::operator() (primary_dir), as every render kernel has it
template <int N>
__device__ __forceinline__ void hits_ray(const NtTarget &tg, const NtHits &h, const HitsPixel &p, float (&o)[N], float (&d)[N]) {
    const float *c = h.cams + (size_t)p.frame * 4 * N;
    float right[N], up[N], fwd[N];
#pragma unroll
    for (int k = 0; k < N; ++k) { o[k] = c[k]; right[k] = c[N + k]; up[k] = c[2 * N + k]; fwd[k] = c[3 * N + k]; }
    primary_dir<N>(tg, right, up, fwd, p.x, p.y, d);
}

template <int N>
__device__ __forceinline__ void hits_store_normal(const NtHits &h, long long r, const float (&no)[N], const float (&nd)[N]) {
    if (h.normal_origin) {
#pragma unroll
        for (int k = 0; k < N; ++k) h.normal_origin[r * N + k] = no[k];
    }
    if (h.normal_dir) {
#pragma unroll
        for (int k = 0; k < N; ++k) h.normal_dir[r * N + k] = nd[k];
    }
}

template <int N, bool SCALP>
__global__ __launch_bounds__(256) void hits_closest(NtCompositeDev sc, NtTarget tg, NtHits h, int tiles_x, int tiles_y) {
    extern __shared__ float2 lds_raw[];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), wv, sc.stack_depth, N);
    const int px = (wv & 1) * 8 + (lane & 7), py = (wv >> 1) * 8 + (lane >> 3);
    const long long total = (long long)tiles_x * tiles_y * h.nframes;
    for (long long tile = (long long)blockIdx.x; tile < total; tile += gridDim.x) {
        if (nt_aborted(tg)) return;                       // (the four waves of a block are independent: no barrier below)
        const HitsPixel p = hits_pixel<16, 16>(tg, h, tile, tiles_x, tiles_y, px, py);
        if (!p.valid) continue;
        float o[N], d[N];
        hits_ray<N>(tg, h, p, o, d);
        Hit hit;
        hit.dist = FLT_MAX; hit.item = -1; hit.lane = -1;
        const float dist0 = aabb_distance<N>(sc, o, d);
        if (dist0 >= 0.0f) {
            setup_ray_table<N>(w, lane, o, d);
            Stats st = {0, 0, 0, 0, 0, 0, 0, 0};
            trace_closest<N, SCALP, false, SCALP>(sc, w, lane, o, d, dist0, FLT_MAX, -1, -1, hit, st);
        }
        query_store(h.hits, p.rec, hit.dist, hit.item, hit.lane, 0);
        if (hit.item >= 0 && (h.normal_origin || h.normal_dir)) {
            float no[N], nd[N];
            hit_normal<N, SCALP>(sc, hit, o, d, no, nd);
            hits_store_normal<N>(h, p.rec, no, nd);
        }
    }
}

// ALIAS: o_hit.normal as the reference's walk leaves it
template <int N, bool ALIAS>
__global__ __launch_bounds__(256) void hits_closest_t(NtCompositeDev sc, NtTarget tg, NtHits h, int tiles_x, int tiles_y) {
    extern __shared__ float2 lds_raw[];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), wv, sc.stack_depth, N);
    Checked ck;
    ck.bits = sc.checked + ((long long)blockIdx.x * 256 + tid);
    ck.stride = sc.checked_lanes;
    ck.words = sc.checked_words;
    ck.n_batches = sc.n_batches;
    ck.n_triangles = sc.n_triangles;
    const int px = (wv & 1) * 8 + (lane & 7), py = (wv >> 1) * 8 + (lane >> 3);
    const long long total = (long long)tiles_x * tiles_y * h.nframes;
    for (long long tile = (long long)blockIdx.x; tile < total; tile += gridDim.x) {
        if (nt_aborted(tg)) return;
        const HitsPixel p = hits_pixel<16, 16>(tg, h, tile, tiles_x, tiles_y, px, py);
        if (!p.valid) continue;
        float o[N], d[N];
        hits_ray<N>(tg, h, p, o, d);
        Hit hit;
        hit.dist = FLT_MAX; hit.item = -1; hit.lane = -1;
        TList th;
        th.n = 0;
        float hn_o[N], hn_d[N];
#pragma unroll
        for (int k = 0; k < N; ++k) { hn_o[k] = 0.0f; hn_d[k] = 0.0f; }       // ray_intersection starts out zeroed
        const float dist0 = aabb_distance<N>(sc, o, d);
        if (dist0 >= 0.0f) {
            setup_ray_table<N>(w, lane, o, d);
            trace_closest_t<N, ALIAS>(sc, w, lane, o, d, dist0, -1, -1, hit, th, ck, hn_o, hn_d);
        }
        query_store(h.hits, p.rec, hit.dist, hit.item, hit.lane, th.n);
        if (hit.item >= 0 && (h.normal_origin || h.normal_dir)) {
            if (!ALIAS) hit_normal<N, true>(sc, hit, o, d, hn_o, hn_d);
            hits_store_normal<N>(h, p.rec, hn_o, hn_d);
        }
    }
}

// the normal rays of the records the packet walk wrote
template <int N, bool SCALP>
__global__ __launch_bounds__(256) void hits_normals(NtCompositeDev sc, NtTarget tg, NtHits h, int tiles_x, int tiles_y) {
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int px = (wv & 1) * 8 + (lane & 7), py = (wv >> 1) * 8 + (lane >> 3);
    const long long total = (long long)tiles_x * tiles_y * h.nframes;
    for (long long tile = (long long)blockIdx.x; tile < total; tile += gridDim.x) {
        if (nt_aborted(tg)) return;
        const HitsPixel p = hits_pixel<16, 16>(tg, h, tile, tiles_x, tiles_y, px, py);
        if (!p.valid) continue;
        const int4 rec = reinterpret_cast<const int4 *>(h.hits)[p.rec];
        if (rec.y < 0) continue;
        Hit hit;
        hit.dist = __int_as_float(rec.x);
        hit.item = rec.y;
        hit.lane = rec.z;
        float o[N], d[N], no[N], nd[N];
        hits_ray<N>(tg, h, p, o, d);
        hit_normal<N, SCALP>(sc, hit, o, d, no, nd);
        hits_store_normal<N>(h, p.rec, no, nd);
    }
}

template <int N>
int launch_hits_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtHits &h) {
    hipStream_t s = (hipStream_t)li.stream;
    const int tiles_x = (tg.width + 15) / 16, tiles_y = (tg.height + 15) / 16;
    const long long tiles = (long long)tiles_x * tiles_y * h.nframes;
    const dim3 grid((unsigned)strided_blocks(tiles));
    if (sc.all_opaque && !sc.checked && li.kernel_choice == 0 && sc.stack_depth <= 32) {
        // the packet walk (packet_args, packet_chunk and packet_chunk_head of nt_composite.hpp); frames per launch: what the
        // numerator scratch holds
        PacketArgs pk = packet_args(li, sc, tg.width, tg.height);
        const int chunk = packet_chunk(li, h.nframes, false);
        for (int f0 = 0; f0 < h.nframes; f0 += chunk) {
            const int cnt = packet_chunk_head<N>(li, sc, pk, h.cams, f0, chunk, h.nframes);
            pk.hits_out = reinterpret_cast<float4 *>(h.hits) + (long long)f0 * h.frame_stride;
            const dim3 pgrid = packet_grid(pk, cnt);
            if (sc.has_scalar_prims) hipLaunchKernelGGL((composite_packet<N, 32, false, true, true>), pgrid, dim3(256), (size_t)4 * pk.lds_per_wave, s, sc, tg, pk);
            else hipLaunchKernelGGL((composite_packet<N, 32, false, false, true>), pgrid, dim3(256), (size_t)4 * pk.lds_per_wave, s, sc, tg, pk);
        }
        if (h.normal_origin || h.normal_dir) {
            if (sc.has_scalar_prims) hipLaunchKernelGGL((hits_normals<N, true>), grid, dim3(256), 0, s, sc, tg, h, tiles_x, tiles_y);
            else hipLaunchKernelGGL((hits_normals<N, false>), grid, dim3(256), 0, s, sc, tg, h, tiles_x, tiles_y);
        }
        return 0;
    }
    // per wave what the per-lane render kernels use: stack [depth + 1][64], ray table, mailbox
    size_t lds;
    if (const int r = lane_walk_lds(sc, N, 4, 160 * 1024, lds)) return r;
    if (sc.checked) {
        const dim3 tgrid((unsigned)checked_column_blocks(sc, 256, tiles));
        if (sc.alias_normals) hipLaunchKernelGGL((hits_closest_t<N, true>), tgrid, dim3(256), lds, s, sc, tg, h, tiles_x, tiles_y);
        else hipLaunchKernelGGL((hits_closest_t<N, false>), tgrid, dim3(256), lds, s, sc, tg, h, tiles_x, tiles_y);
        return 0;
    }
    if (!sc.all_opaque) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: transparent scene without the checked-list scratch");
        return -1;
    }
    if (sc.has_scalar_prims) hipLaunchKernelGGL((hits_closest<N, true>), grid, dim3(256), lds, s, sc, tg, h, tiles_x, tiles_y);
    else hipLaunchKernelGGL((hits_closest<N, false>), grid, dim3(256), lds, s, sc, tg, h, tiles_x, tiles_y);
    return 0;
}

}  // namespace
