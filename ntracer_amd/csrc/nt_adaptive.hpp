// nt_adaptive.hpp -- adaptive supersampling (nt_scene_set_adaptive_supersampling): of a W x H frame only the
// pixels that show contrast in the plain single-sample frame get the s x s samples of 4.3.
//
// Stage 1 is an ordinary render of the job in the plain fp32 x 3 format (12-byte pixels of big-endian floats, each component
// already clamped to [0, 1] by the packer) into scratch: the base frame P.  Stage 2, adaptive_flag, is one lane a pixel: it
// reads its own colour and its neighbours' from P and forms the contrast, the largest |P[x,y][c] - P[x',y'][c]| over the three
// components and the four neighbours inside the image.  contrast > t flags the pixel; an unflagged pixel goes into the caller's
// image at once, through emit_pixel; a flagged one is appended to a list of frame * H * W + y * W + x: one ballot and one
// atomicAdd a wave on a device counter, so a wave's flagged pixels lie side by side in the list, in lane order.  Stage 3,
// refine_*, are the rays_* kernels of nt_rays.hpp with another ray source and another sink: one lane a flagged pixel, which
// forms the ray of sample (i, j) -- pixel (s x + i, s y + j) of the s W x s H view, from the frame's camera rows in device memory,
// by primary_dir's operations -- shades it with the device function a ray_colors call of the scene would use, clamps, adds in
// row-major order and divides by (float)(s * s): the value resolve_kernel<S> forms from the same samples, operation for
// operation.  One wave a block (the list is short, and its length is not known to the host: many small blocks spread it over the
// chip); the blocks stride over the list, whose length they read from device memory.
// Instantiated per N by nt_inst_adaptive.hip; adaptive_flag, the run-time-n kernels and the dispatcher (nt_launch_refine) are in
// nt_var.hip.
#pragma once
#include "nt_rays.hpp"

namespace {

// the clamp of a sample, as emit_pixel clamps a plain fp32 component (simd::clamp, SSE NaN rule)
__device__ __forceinline__ float refine_clamp(float v) {
    v = v > 0.0f ? v : 0.0f;
    return v < 1.0f ? v : 1.0f;
}

// The counter starts at zero: a one-lane kernel in stream order, not hipMemsetAsync.  A precaution, not a diagnosis (DESIGN.md
// 4.9): an earlier form with hipMemsetAsync rendered every direct call correctly and faulted when a captured two-chunk table
// call was replayed; this form replays correctly.  Whether the replay ordered or ran the memset node wrongly was not isolated.
__global__ __launch_bounds__(64) void adaptive_reset(int *count) {
    if (threadIdx.x == 0) *count = 0;
}

// Stage 2.  A block is 64 pixels of four rows (one wave a row), the grid's z the frame.  MASK: the byte mask is written too.
template <bool MASK>
__global__ __launch_bounds__(256) void adaptive_flag(NtAdaptive ad, NtTarget tg) {
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int x = (int)blockIdx.x * 64 + lane;
    const int y = (int)blockIdx.y * 4 + (tid >> 6);
    if (y >= tg.height) return;                              // (the same for the whole wave)
    const bool inside = x < tg.width;
    const long long pix = ((long long)blockIdx.z * tg.height + y) * tg.width + x;
    bool flagged = false;
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (inside) {
        const uint32_t *p = ad.base + pix * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = __uint_as_float(bswap32(p[k]));
        const long long step[4] = {-3, 3, -3 * (long long)tg.width, 3 * (long long)tg.width};
        const bool there[4] = {x > 0, x + 1 < tg.width, y > 0, y + 1 < tg.height};
        float contrast = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (there[q]) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float d = fabsf(c[k] - __uint_as_float(bswap32(p[step[q] + k])));
                    contrast = d > contrast ? d : contrast;
                }
            }
        }
        flagged = contrast > ad.threshold;
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(flagged);
    if (m != 0ull) {
        // the wave's flagged pixels, side by side and in lane order (lane 0 is always here: rows leave as a whole)
        int first = 0;
        if (lane == 0) first = atomicAdd(ad.count, __popcll(m));
        first = __builtin_amdgcn_readfirstlane(first);
        // (the list has room for every pixel of the launch, and a pixel is appended once)
        if (flagged) ad.list[first + __popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)pix;
    }
    if (MASK && inside) ad.mask[pix] = flagged ? 1 : 0;
    if (ad.draw && inside && !flagged) {
        PixelRef pr;
        pr.valid = true;
        pr.hit_index = 0;
        pr.x = x;
        pr.y = y;
        pr.offset = (long long)blockIdx.z * tg.frame_stride + (long long)y * tg.pitch + (long long)x * tg.bpp;
        emit_pixel(tg, pr, c[0], c[1], c[2]);
    }
}

inline void launch_adaptive_flag(hipStream_t stream, const NtAdaptive &ad, const NtTarget &tg) {
    const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + 3) / 4), (unsigned)ad.nframes);
    hipLaunchKernelGGL(adaptive_reset, dim3(1), dim3(64), 0, stream, ad.count);
    if (ad.mask) hipLaunchKernelGGL(adaptive_flag<true>, grid, dim3(256), 0, stream, ad, tg);
    else hipLaunchKernelGGL(adaptive_flag<false>, grid, dim3(256), 0, stream, ad, tg);
}

struct RefinePixel {
    int x, y, frame;
};

// entry `i` of the list
__device__ __forceinline__ RefinePixel refine_pixel(const NtTarget &tg, const NtRefine &rf, long long i) {
    const uint32_t idx = rf.list[i];
    const uint32_t per_frame = (uint32_t)tg.width * (uint32_t)tg.height;
    RefinePixel p;
    p.frame = (int)(idx / per_frame);
    const uint32_t rem = idx - (uint32_t)p.frame * per_frame;
    p.y = (int)(rem / (uint32_t)tg.width);
    p.x = (int)(rem - (uint32_t)p.y * (uint32_t)tg.width);
    return p;
}

// where the pixel goes: the whole image, no bands
__device__ __forceinline__ PixelRef refine_dest(const NtTarget &tg, const RefinePixel &p) {
    PixelRef pr;
    pr.valid = true;
    pr.hit_index = 0;
    pr.x = p.x;
    pr.y = p.y;
    pr.offset = (long long)p.frame * tg.frame_stride + (long long)p.y * tg.pitch + (long long)p.x * tg.bpp;
    return pr;
}

// the ray of sample k = j * s + i of the pixel: the frame's camera (read again for every sample -- the rows are in cache, and
// 4 N registers stay free while the sample is shaded) and primary_dir's arithmetic on the s W x s H view
template <int N>
__device__ __forceinline__ void refine_ray(const NtRefine &rf, const RefinePixel &p, int k, float (&o)[N], float (&d)[N]) {
    const int j = k / rf.s, i = k - j * rf.s;
    const float *c = rf.cams + (size_t)p.frame * 4 * N;
    float right[N], up[N], fwd[N];
#pragma unroll
    for (int q = 0; q < N; ++q) { o[q] = c[q]; right[q] = c[N + q]; up[q] = c[2 * N + q]; fwd[q] = c[3 * N + q]; }
    const float sx = rf.fovI * ((float)(rf.s * p.x + i) - rf.half_w);
    const float sy = rf.fovI * ((float)(rf.s * p.y + j) - rf.half_h);
    lens_dir<N>(right, up, fwd, sx, sy, 1.0f, d);          // (with sz = 1 this is primary_dir bit for bit)
}

// a sample joins the sum: the first one starts it, as resolve_kernel has it
__device__ __forceinline__ void refine_add(float (&acc)[3], int k, float r, float g, float b) {
    r = refine_clamp(r);
    g = refine_clamp(g);
    b = refine_clamp(b);
    acc[0] = k == 0 ? r : acc[0] + r;
    acc[1] = k == 0 ? g : acc[1] + g;
    acc[2] = k == 0 ? b : acc[2] + b;
}

__device__ __forceinline__ void refine_emit(const NtTarget &tg, const NtRefine &rf, const RefinePixel &p, const float (&acc)[3]) {
    const float count = (float)(rf.s * rf.s);
    emit_pixel(tg, refine_dest(tg, p), acc[0] / count, acc[1] / count, acc[2] / count);
}

// rays_color's scenes
template <int N, bool FEAT, bool SCALP>
__global__ __launch_bounds__(64) void refine_color(NtCompositeDev sc, NtRefine rf, NtTarget tg) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), 0, sc.stack_depth, N);
    const long long count = (long long)*rf.count;
    const int ss = rf.s * rf.s;
    for (long long base = (long long)blockIdx.x * 64; base < count; base += (long long)gridDim.x * 64) {
        if (nt_aborted(tg)) return;
        if (base + lane >= count) continue;
        const RefinePixel p = refine_pixel(tg, rf, base + lane);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < ss; ++k) {
            float o[N], d[N];
            refine_ray<N>(rf, p, k, o, d);
            Stats st = {0, 0, 0, 0, 0, 0, 0, 0};
            const Color3 c = composite_color<N, FEAT, false, SCALP>(sc, w, lane, o, d, st);
            refine_add(acc, k, c.r, c.g, c.b);
        }
        refine_emit(tg, rf, p, acc);
    }
}

// rays_color_t's scenes: a `checked` column per resident lane, so the grid is what that scratch has columns for
template <int N, bool ALIAS>
__global__ __launch_bounds__(64) void refine_color_t(NtCompositeDev sc, NtRefine rf, NtTarget tg) {
    extern __shared__ float2 lds_raw[];
    const int lane = (int)threadIdx.x;
    const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), 0, sc.stack_depth, N);
    Checked ck;
    ck.bits = sc.checked + ((long long)blockIdx.x * 64 + lane);
    ck.stride = sc.checked_lanes;
    ck.words = sc.checked_words;
    ck.n_batches = sc.n_batches;
    ck.n_triangles = sc.n_triangles;
    const long long count = (long long)*rf.count;
    const int ss = rf.s * rf.s;
    for (long long base = (long long)blockIdx.x * 64; base < count; base += (long long)gridDim.x * 64) {
        if (nt_aborted(tg)) return;
        if (base + lane >= count) continue;
        const RefinePixel p = refine_pixel(tg, rf, base + lane);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < ss; ++k) {
            float o[N], d[N];
            refine_ray<N>(rf, p, k, o, d);
            const Color3 c = composite_color_t<N, ALIAS>(sc, w, lane, o, d, ck);
            refine_add(acc, k, c.r, c.g, c.b);
        }
        refine_emit(tg, rf, p, acc);
    }
}

// BoxScene: box_color's complete reference-ordered evaluation of every sample
template <int N>
__global__ __launch_bounds__(64) void refine_box(NtRefine rf, NtTarget tg) {
    const int lane = (int)threadIdx.x;
    const long long count = (long long)*rf.count;
    const int ss = rf.s * rf.s;
    for (long long base = (long long)blockIdx.x * 64; base < count; base += (long long)gridDim.x * 64) {
        if (nt_aborted(tg)) return;
        if (base + lane >= count) continue;
        const RefinePixel p = refine_pixel(tg, rf, base + lane);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < ss; ++k) {
            float o[N], d[N];
            refine_ray<N>(rf, p, k, o, d);
            float cr, cg, cb;
            box_color<N>(o, d, true, cr, cg, cb);
            refine_add(acc, k, cr, cg, cb);
        }
        refine_emit(tg, rf, p, acc);
    }
}

// the grid of a refine launch: a wave for every 64 pixels that could be flagged, capped as the rays_* kernels cap theirs
inline long long refine_blocks(const NtRefine &rf) {
    const long long blocks = strided_blocks((rf.max_count + 63) / 64);
    return blocks < 1 ? 1 : blocks;
}

template <int N>
int launch_refine_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtRefine &rf, const NtTarget &tg) {
    // one wave's share of what launch_rays_fixed asks for: stack [depth + 1][64], ray table, mailbox.  A block is one wave, so
    // this is the block's whole allocation, held to the 64 KiB a launch gets without asking for more: at N = 10 that is a stack
    // of 220 levels, beyond what the base frame's own kernels take (their four-wave blocks stop at 124)
    size_t lds;
    if (const int r = lane_walk_lds(sc, N, 1, 64 * 1024, lds)) return r;
    hipStream_t s = (hipStream_t)li.stream;
    const long long blocks = refine_blocks(rf);
    if (sc.checked) {
        const dim3 tgrid((unsigned)checked_column_blocks(sc, 64, blocks));
        if (sc.alias_normals) hipLaunchKernelGGL((refine_color_t<N, true>), tgrid, dim3(64), lds, s, sc, rf, tg);
        else hipLaunchKernelGGL((refine_color_t<N, false>), tgrid, dim3(64), lds, s, sc, rf, tg);
        return 0;
    }
    if (!sc.all_opaque) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: transparent scene without the checked-list scratch");
        return -1;
    }
    const dim3 grid((unsigned)blocks);
    const bool feat = scene_feat(sc);
    if (feat && !sc.has_scalar_prims) hipLaunchKernelGGL((refine_color<N, true, false>), grid, dim3(64), lds, s, sc, rf, tg);
    else if (feat) hipLaunchKernelGGL((refine_color<N, true, true>), grid, dim3(64), lds, s, sc, rf, tg);
    else hipLaunchKernelGGL((refine_color<N, false, false>), grid, dim3(64), lds, s, sc, rf, tg);
    return 0;
}

template <int N>
int launch_refine_box_fixed(const NtLaunchInfo &li, const NtRefine &rf, const NtTarget &tg) {
    hipLaunchKernelGGL((refine_box<N>), dim3((unsigned)refine_blocks(rf)), dim3(64), 0, (hipStream_t)li.stream, rf, tg);
    return 0;
}

}  // namespace
