// nt_ao.hpp -- ambient occlusion for compile-time N (nt_scene_set_ambient_occlusion): how many of K short rays
// from the primary hit of a pixel are blocked within `radius`.
//
// A primary-hit pass with normals (nt_hits.hpp) has left, for every pixel, the 16-byte record and the normal ray (no, nd) in
// scratch.  ao_kernel is one lane a pixel, a wave an 8x8 tile -- neighbouring lanes start in neighbouring leaves --, four
// independent waves a block, the blocks striding over [frame][tile row][tile column] as hits_closest's do.  A lane reads its
// record and normal rows once, rebuilds the primary direction d from the frame's camera (primary_dir: the bits the hit pass
// used), and forms in registers
//     side = -dot(d, nd),  b = side < 0 ? -bias : bias,  o'[j] = no[j] + nd[j] * b.
// Sample k of the table (rows used as given) is turned into the hemisphere of the side the ray came from,
//     s = dot(nd, t_k),  v = ((s < 0) != (side < 0)) ? -t_k : t_k,
// and walked by the render's own trace_closest with t_near = 0, t_far = radius and the primary hit as the skip target: exactly
// the closest-hit query of nt_query.hpp on that ray, so blocked <=> item >= 0 && dist <= radius.  k is wave-uniform: t_k comes
// through the scalar cache (the table is read in the constant address space at a uniform index), not from per-lane loads.  The
// K walks run one after the other, the count stays in a register, and one dword a pixel goes out: -1 without an opaque hit.
// A wave none of whose lanes has a hit leaves at once.  t_far = radius already keeps a walk out of every cell that starts beyond
// the radius; there is no earlier stop than trace_closest's own.
// Instantiated per N by nt_inst_ao.hip; the ray route's kernels, ao_apply and the dispatcher (nt_launch_ao) are in nt_var.hip.
#pragma once
#include "nt_hits.hpp"

namespace {

typedef const float __attribute__((address_space(4))) *ao_table_ptr;

template <int N, bool SCALP>
__global__ __launch_bounds__(256) void ao_kernel(NtCompositeDev sc, NtTarget tg, NtAo ao, int tiles_x, int tiles_y) {
    extern __shared__ float2 lds_raw[];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), wv, sc.stack_depth, N);
    const int px = (wv & 1) * 8 + (lane & 7), py = (wv >> 1) * 8 + (lane >> 3);
    NtHits h;
    h.cams = ao.cams;
    h.nframes = ao.nframes;
    h.frame_stride = (long long)tg.width * tg.height;
    const ao_table_ptr table = (ao_table_ptr)ao.dirs;
    const long long total = (long long)tiles_x * tiles_y * ao.nframes;
    for (long long tile = (long long)blockIdx.x; tile < total; tile += gridDim.x) {
        if (nt_aborted(tg)) return;                       // (the four waves of a block are independent: no barrier below)
        const HitsPixel p = hits_pixel<16, 16>(tg, h, tile, tiles_x, tiles_y, px, py);
        int4 rec = make_int4(0, -1, -1, 0);
        if (p.valid) rec = reinterpret_cast<const int4 *>(ao.recs)[p.rec];
        const bool has = p.valid && rec.y >= 0;
        if (__builtin_amdgcn_ballot_w64(has) == 0ull) {
            if (p.valid) ao.blocked[p.rec] = -1;
            continue;
        }
        float oo[N], nd[N];
        float side = 0.0f;
#pragma unroll
        for (int j = 0; j < N; ++j) { oo[j] = 0.0f; nd[j] = 0.0f; }
        if (has) {
            float co[N], d[N], no[N];
            hits_ray<N>(tg, h, p, co, d);
#pragma unroll
            for (int j = 0; j < N; ++j) { no[j] = ao.normal_origin[p.rec * N + j]; nd[j] = ao.normal_dir[p.rec * N + j]; }
            side = -dotN<N>(d, nd);
            const float b = side < 0.0f ? -ao.bias : ao.bias;
#pragma unroll
            for (int j = 0; j < N; ++j) oo[j] = no[j] + nd[j] * b;
        }
        int blocked = 0;
        for (int k = 0; k < ao.count; ++k) {
            float t[N];
#pragma unroll
            for (int j = 0; j < N; ++j) t[j] = table[k * N + j];          // uniform: scalar loads
            if (has) {
                const float s = dotN<N>(nd, t);
                const bool flip = (s < 0.0f) != (side < 0.0f);
                float v[N];
#pragma unroll
                for (int j = 0; j < N; ++j) v[j] = flip ? -t[j] : t[j];
                setup_ray_table<N>(w, lane, oo, v);
                Hit hit;
                Stats st = {0, 0, 0, 0, 0, 0, 0, 0};
                trace_closest<N, false, false, SCALP>(sc, w, lane, oo, v, 0.0f, ao.radius, rec.y, rec.z, hit, st);
                if (hit.item >= 0 && hit.dist <= ao.radius) ++blocked;
            }
        }
        if (p.valid) ao.blocked[p.rec] = has ? blocked : -1;
    }
}

template <int N>
int launch_ao_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtAo &ao) {
    // per wave what the query kernels use (launch_query_fixed): stack [depth + 1][64], ray table, mailbox
    size_t lds;
    if (const int r = lane_walk_lds(sc, N, 4, 160 * 1024, lds)) return r;
    if (!sc.all_opaque || sc.checked) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: the ambient occlusion kernel is for opaque scenes on the mailbox walk");
        return -1;
    }
    const int tiles_x = (tg.width + 15) / 16, tiles_y = (tg.height + 15) / 16;
    const long long tiles = (long long)tiles_x * tiles_y * ao.nframes;
    const dim3 grid((unsigned)strided_blocks(tiles));
    hipStream_t s = (hipStream_t)li.stream;
    if (sc.has_scalar_prims) hipLaunchKernelGGL((ao_kernel<N, true>), grid, dim3(256), lds, s, sc, tg, ao, tiles_x, tiles_y);
    else hipLaunchKernelGGL((ao_kernel<N, false>), grid, dim3(256), lds, s, sc, tg, ao, tiles_x, tiles_y);
    return 0;
}

}  // namespace
