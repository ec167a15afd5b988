// nt_query.hpp -- batched ray queries for compile-time N: KDNode.intersects / KDNode.occludes of the reference
// (src/ntracer_body.hpp:1412-1496) for `count` arbitrary rays read from device memory.  The walks are the render kernels'
// own (nt_composite.hpp) -- a query is a render without a camera and without shading: one lane per ray, four independent waves
// a block, lane l of block b takes ray 256 b + l and the blocks stride on where the grid is capped.  A wave's 64 rays are one
// contiguous run of 256 N bytes of `origins` and of `directions`, so the plain per-lane loads use every line they fetch.
// What differs from a render's walk: there is no scene-box test in front (the reference's methods have none), the root call
// gets the caller's t_near / t_far (RootWindow), and the transparent hits are handed out as the walk left them, unsorted.
// Instantiated per N by nt_inst_query.hip; the run-time-n kernels and the dispatcher (nt_launch_query) are in nt_var.hip.
#pragma once
#include "nt_composite.hpp"

namespace {

__device__ __forceinline__ bool query_aborted(const NtQuery &q) {
    return q.abort_word != nullptr && __hip_atomic_load(q.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
}

// one ray's parameters other than the ray itself
struct QueryRay {
    float t_near, t_far, distance;
    int skip_item, skip_lane;
};
__device__ __forceinline__ QueryRay query_ray(const NtQuery &q, long long r) {
    QueryRay p;
    p.t_near = q.t_near ? q.t_near[r] : -FLT_MAX;
    p.t_far = q.t_far ? q.t_far[r] : FLT_MAX;
    p.distance = q.distance ? q.distance[r] : FLT_MAX;
    p.skip_item = q.skip_item ? q.skip_item[r] : -1;
    p.skip_lane = q.skip_lane ? q.skip_lane[r] : -1;
    return p;
}

// the 16-byte record of a ray (nt_ray_hit), one dwordx4 store
__device__ __forceinline__ void query_store(void *recs, long long at, float dist, int item, int lane, int n_transparent) {
    reinterpret_cast<int4 *>(recs)[at] = make_int4(__float_as_int(dist), item, lane, n_transparent);
}

// the first max_transparent entries of the list; the slots it does not reach say "none"
__device__ __forceinline__ void query_store_list(const NtQuery &q, long long r, const TList &th) {
    if (!q.transparent) return;
    for (int i = 0; i < q.max_transparent; ++i) {
        const long long at = r * q.max_transparent + i;
        if (i < th.n) query_store(q.transparent, at, th.e[i].dist, th.e[i].item, th.e[i].lane, 0);
        else query_store(q.transparent, at, FLT_MAX, -1, -1, 0);
    }
}

template <int N>
__device__ __forceinline__ void query_load_ray(const NtQuery &q, long long r, float (&o)[N], float (&d)[N]) {
    const float *po = q.origins + r * N, *pd = q.directions + r * N;
#pragma unroll
    for (int k = 0; k < N; ++k) { o[k] = po[k]; d[k] = pd[k]; }
}

template <int N>
__device__ __forceinline__ void query_store_normal(const NtQuery &q, long long r, const float (&no)[N], const float (&nd)[N]) {
    if (q.normal_origin) {
#pragma unroll
        for (int k = 0; k < N; ++k) q.normal_origin[r * N + k] = no[k];
    }
    if (q.normal_dir) {
#pragma unroll
        for (int k = 0; k < N; ++k) q.normal_dir[r * N + k] = nd[k];
    }
}

// Opaque scenes without Solids (or with them under NTRACER_CLEAN_NORMALS=1): trace_closest with the 16-slot mailbox, then the
// normal ray of what was hit.  There are no transparent hits to count.
template <int N, bool SCALP>
__global__ __launch_bounds__(256) void query_closest(NtCompositeDev sc, NtQuery q) {
    extern __shared__ float2 lds_raw[];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), tid >> 6, sc.stack_depth, N);
    for (long long base = (long long)blockIdx.x * 256; base < q.count; base += (long long)gridDim.x * 256) {
        if (query_aborted(q)) return;                     // (the four waves of a block are independent: no barrier below)
        const long long r = base + tid;
        if (r >= q.count) continue;
        float o[N], d[N];
        query_load_ray<N>(q, r, o, d);
        const QueryRay p = query_ray(q, r);
        setup_ray_table<N>(w, lane, o, d);
        Hit hit;
        Stats st = {0, 0, 0, 0, 0, 0, 0, 0};
        trace_closest<N, SCALP, false, SCALP>(sc, w, lane, o, d, p.t_near, p.t_far, p.skip_item, p.skip_lane, hit, st);
        query_store(q.hits, r, hit.dist, hit.item, hit.lane, 0);
        if (hit.item >= 0 && (q.normal_origin || q.normal_dir)) {
            float no[N], nd[N];
            hit_normal<N, SCALP>(sc, hit, o, d, no, nd);
            query_store_normal<N>(q, r, no, nd);
        }
        if (q.transparent) {
            TList none;
            none.n = 0;
            query_store_list(q, r, none);
        }
    }
}

// Scenes with transparent materials or Solids: trace_closest_t with the exact `checked` list, a bitmap column per resident
// lane -- the grid is what that scratch has columns for.  ALIAS: o_hit.normal as the reference's walk leaves it.
template <int N, bool ALIAS>
__global__ __launch_bounds__(256) void query_closest_t(NtCompositeDev sc, NtQuery q) {
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
    for (long long base = (long long)blockIdx.x * 256; base < q.count; base += (long long)gridDim.x * 256) {
        if (query_aborted(q)) return;
        const long long r = base + tid;
        if (r >= q.count) continue;
        float o[N], d[N];
        query_load_ray<N>(q, r, o, d);
        const QueryRay p = query_ray(q, r);
        setup_ray_table<N>(w, lane, o, d);
        Hit hit;
        TList th;
        float hn_o[N], hn_d[N];
#pragma unroll
        for (int k = 0; k < N; ++k) { hn_o[k] = 0.0f; hn_d[k] = 0.0f; }       // ray_intersection starts out zeroed
        RootWindow root;
        root.tn = p.t_near;
        root.tf = p.t_far;
        trace_closest_t<N, ALIAS, RootWindow>(sc, w, lane, o, d, p.t_near, p.skip_item, p.skip_lane, hit, th, ck, hn_o, hn_d, root);
        query_store(q.hits, r, hit.dist, hit.item, hit.lane, th.n);
        if (hit.item >= 0 && (q.normal_origin || q.normal_dir)) {
            if (!ALIAS) hit_normal<N, true>(sc, hit, o, d, hn_o, hn_d);
            query_store_normal<N>(q, r, hn_o, hn_d);
        }
        query_store_list(q, r, th);
    }
}

// KDNode.occludes on opaque scenes: dist = 1 when something opaque lies nearer than `distance`, else 0
template <int N, bool SCALP>
__global__ __launch_bounds__(256) void query_occluded(NtCompositeDev sc, NtQuery q) {
    extern __shared__ float2 lds_raw[];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), tid >> 6, sc.stack_depth, N);
    for (long long base = (long long)blockIdx.x * 256; base < q.count; base += (long long)gridDim.x * 256) {
        if (query_aborted(q)) return;
        const long long r = base + tid;
        if (r >= q.count) continue;
        RayArg<N> ray;
        query_load_ray<N>(q, r, ray.o, ray.d);
        const QueryRay p = query_ray(q, r);
        Stats st = {0, 0, 0, 0, 0, 0, 0, 0};
        RootWindow root;
        root.tn = p.t_near;
        root.tf = p.t_far;
        const bool blocked = trace_occluded<N, false, SCALP, RootWindow>(sc, w, lane, ray, p.distance, p.skip_item, p.skip_lane, st, root);
        query_store(q.hits, r, blocked ? 1.0f : 0.0f, -1, -1, 0);
        if (q.transparent) {
            TList none;
            none.n = 0;
            query_store_list(q, r, none);
        }
    }
}

// ... and with transparent materials: the transparent hits met on the way are collected (no `checked` list: the reference's
// occlusion walk keeps none, so a surface listed in two cells is collected twice)
template <int N>
__global__ __launch_bounds__(256) void query_occluded_t(NtCompositeDev sc, NtQuery q) {
    extern __shared__ float2 lds_raw[];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), tid >> 6, sc.stack_depth, N);
    for (long long base = (long long)blockIdx.x * 256; base < q.count; base += (long long)gridDim.x * 256) {
        if (query_aborted(q)) return;
        const long long r = base + tid;
        if (r >= q.count) continue;
        float o[N], d[N];
        query_load_ray<N>(q, r, o, d);
        const QueryRay p = query_ray(q, r);
        TList sh;
        RootWindow root;
        root.tn = p.t_near;
        root.tf = p.t_far;
        const bool blocked = trace_occluded_t<N, RootWindow>(sc, w, lane, o, d, p.distance, p.skip_item, p.skip_lane, sh, root);
        query_store(q.hits, r, blocked ? 1.0f : 0.0f, -1, -1, sh.n);
        query_store_list(q, r, sh);
    }
}

template <int N>
int launch_query_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtQuery &q) {
    // per wave what the per-lane render kernels use: stack [depth + 1][64], ray table, mailbox
    size_t lds;
    if (const int r = lane_walk_lds(sc, N, 4, 160 * 1024, lds)) return r;
    hipStream_t s = (hipStream_t)li.stream;
    const dim3 grid((unsigned)(((long long)q.count + 255) / 256));
    if (q.occlusion) {
        if (!sc.all_opaque) hipLaunchKernelGGL((query_occluded_t<N>), grid, dim3(256), lds, s, sc, q);
        else if (sc.has_scalar_prims) hipLaunchKernelGGL((query_occluded<N, true>), grid, dim3(256), lds, s, sc, q);
        else hipLaunchKernelGGL((query_occluded<N, false>), grid, dim3(256), lds, s, sc, q);
        return 0;
    }
    if (sc.checked) {
        // as many blocks as the `checked` scratch has lane columns for, striding over the rays
        const dim3 tgrid((unsigned)(sc.checked_lanes / 256));
        if (sc.alias_normals) hipLaunchKernelGGL((query_closest_t<N, true>), tgrid, dim3(256), lds, s, sc, q);
        else hipLaunchKernelGGL((query_closest_t<N, false>), tgrid, dim3(256), lds, s, sc, q);
        return 0;
    }
    if (!sc.all_opaque) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: transparent scene without the checked-list scratch");
        return -1;
    }
    if (sc.has_scalar_prims) hipLaunchKernelGGL((query_closest<N, true>), grid, dim3(256), lds, s, sc, q);
    else hipLaunchKernelGGL((query_closest<N, false>), grid, dim3(256), lds, s, sc, q);
    return 0;
}

}  // namespace
