// nt_stack.hpp -- view stacks (nt_scene_set_view_stack): one picture from K cameras that differ from the frame's
// camera by a small offset -- depth of field, slabs along a hidden axis, anaglyph stereo.  ntracer_hip.h has the rule in full.
//
//   stack_cameras   [F] cameras -> [F][K] sample cameras and their dot products, by the rule: every product and sum rounded on
//                   its own (the build's -ffp-contract=off), so the bits are nt_view_stack_cameras' on the host.
//   stack_resolve   the frames route, every scene: the K plain fp32 x 3 frames of a pixel, which the ordinary render wrote into
//                   scratch for the sample cameras, summed in the order of k -- acc + (w * c) -- and packed.  One lane a pixel,
//                   three dwords a sample.  A chunk of consecutive k hands its sums on through an fp32 accumulator frame.
//   box_stack<N>    BoxScene's fused route, N = 3..24: the per-pixel kernel's geometry (64 columns x 4 rows a block, the grid's z
//                   the frame); the origins, forward rows and dot products of the K samples staged once a block in LDS, right
//                   and up wave-uniform; a lane loops over k -- primary_dir's operations without the normalisation, stack_box_color
//                   (box_pixel's general path without the emitting), clamp, accumulate -- and emits once.  No sample crosses device memory.
//
// Instantiated by nt_inst_stack.hip: once per N for box_stack, once without a dimension for the other two.
#pragma once
#include "nt_box.hpp"

namespace {

// the packer's clamp of a plain fp32 frame (emit_pixel, plain_f32): what a sample's component is before it is weighted
__device__ __forceinline__ float stack_clamp01(float v) {
    v = v > 0.0f ? v : 0.0f;
    return v < 1.0f ? v : 1.0f;
}

// One block a sample camera (frame f, sample k), one lane a component j < n.
__global__ __launch_bounds__(64) void stack_cameras(int n, int count, const float *cams, const float *axes, const float *offsets, float r,
                                                    float *out_cams, float *out_dots) {
    const int f = (int)blockIdx.x / count, k = (int)blockIdx.x - f * count;
    const int j = (int)threadIdx.x;
    const float *c = cams + (size_t)f * 4 * n;
    const float *a = axes + (size_t)f * n * n;
    const float *e = offsets + (size_t)k * n;
    float *o = out_cams + (size_t)blockIdx.x * 4 * n;
    if (j < n) {
        float s = e[0] * a[j];
        for (int i = 1; i < n; ++i) s = s + (e[i] * a[(size_t)i * n + j]);
        o[j] = c[j] + s;
        o[n + j] = c[n + j];
        o[2 * n + j] = c[2 * n + j];
        o[3 * n + j] = c[3 * n + j] - (s * r);
    }
    __syncthreads();
    // |o|^2, o.right, o.up, o.forward of the sample camera, as the host's camera_dots sums them: in double, left to right
    if (j < 4) {
        double q = 0.0;
        for (int i = 0; i < n; ++i) q += (double)o[i] * (double)o[j * n + i];
        out_dots[(size_t)blockIdx.x * 4 + j] = (float)q;
    }
}

__global__ __launch_bounds__(256) void stack_resolve(NtTarget tg, NtStack sk, NtStackChunk ch) {
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * 64 + (tid & 63);
    const int y = (int)blockIdx.y * 4 + (tid >> 6);
    if (y >= tg.height || x >= tg.width) return;
    const long long px = (long long)tg.width * tg.height;
    const long long pix = (long long)y * tg.width + x;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (ch.acc_in) {
        const float *a = ch.acc_in + pix * 3;
        acc[0] = a[0]; acc[1] = a[1]; acc[2] = a[2];
    }
    const uint32_t *p = ch.samples + ((long long)blockIdx.z * ch.kc * px + pix) * 3;
    for (int kk = 0; kk < ch.kc; ++kk, p += px * 3) {
        const float *w = sk.weights + 3 * (ch.k0 + kk);
        // (the packer that wrote the sample has clamped it)
        const float c0 = __uint_as_float(bswap32(p[0])), c1 = __uint_as_float(bswap32(p[1])), c2 = __uint_as_float(bswap32(p[2]));
        acc[0] = acc[0] + (w[0] * c0);
        acc[1] = acc[1] + (w[1] * c1);
        acc[2] = acc[2] + (w[2] * c2);
    }
    if (ch.acc_out) {
        float *a = ch.acc_out + pix * 3;
        a[0] = acc[0]; a[1] = acc[1]; a[2] = acc[2];
        return;
    }
    PixelRef pr;
    pr.valid = true;
    pr.hit_index = 0;
    pr.x = x;
    pr.y = y;
    pr.offset = (long long)blockIdx.z * tg.frame_stride + (long long)y * tg.pitch + (long long)x * tg.bpp;
    emit_pixel(tg, pr, acc[0], acc[1], acc[2]);
}

// The colour of one BoxScene ray from its UNNORMALISED direction v (|v|^2 = sq), its camera's dot products and the pixel's sx, sy:
// what box_pixel<N, false> (nt_box.hpp) computes on its general path -- every format, no stretch codes, no sets -- without the
// emitting: the circumsphere rejection, the sort into miss, hit at K and unclear (box_classify), the reference's arithmetic for
// the unclear lanes on the faces still in question (box_resolve) -- one IEEE division a ray, of the component the colour is made
// of -- and box_color's full evaluation for a wave with a lane that has no usable entry time.  box_pixel writes its pixel where
// this returns the colour, which is why it is not called here; the two sites must stay in step: a change to box_pixel's sorting
// between `maybe` and the final `x / sqrtf(sq)` belongs here too (tests/test_view_stack_gpu.py holds both to the oracle).
template <int N>
__device__ __forceinline__ void stack_box_color(const float (&org)[N], float (&dir)[N], float sq, const float *dots, float sx, float sy,
                                                float &r, float &g, float &b) {
    float margin = fabsf(org[0]);
#pragma unroll
    for (int j = 1; j < N; ++j) margin = fmaxf(margin, fabsf(org[j]));
    margin = NT_BOX_MARGIN * (1.0f + margin);
    const bool maybe = box_may_hit(N, dots, sx, sy, sq);
    bool hit = false, unclear = false;
    float x = dir[0];
    float near[N], tn = 0.0f, vK = 0.0f;
    if (__builtin_amdgcn_ballot_w64(maybe) != 0ull) box_classify<N>(org, dir, margin, maybe, hit, unclear, x, near, tn, vK);
    const bool hard = unclear && !(tn > 1e-3f && tn < 1e30f);
    if (__builtin_amdgcn_ballot_w64(unclear) != 0ull && __builtin_amdgcn_ballot_w64(hard) == 0ull) {
        box_resolve<N>(org, dir, sqrt_wave(sq), margin, near, tn, vK, unclear, hit, x);
        unclear = false;
    }
    if (__builtin_amdgcn_ballot_w64(unclear) == 0ull) {
        const float in = x / sqrtf(sq);
        if (hit) {
            const float shade = fabsf(in);
            r = shade * 1.0f;
            g = shade * 0.5f;
            b = shade * 0.5f;
        } else {
            box_background(in, r, g, b);
        }
    } else {
        const float len = sqrtf(sq);
#pragma unroll
        for (int j = 0; j < N; ++j) dir[j] = dir[j] / len;
        box_color<N>(org, dir, maybe, r, g, b);
    }
}

// LDS of box_stack: a sample's origin, forward row and four dot products
template <int N>
constexpr int box_stack_pitch() { return 2 * N + 4; }

template <int N>
__global__ __launch_bounds__(256) void box_stack(NtTarget tg, NtStack sk) {
    extern __shared__ float stack_lds[];
    if (nt_aborted(tg)) return;
    constexpr int P = box_stack_pitch<N>();
    const int tid = (int)threadIdx.x;
    const int K = sk.count;
    const float *cm = sk.cams + (size_t)blockIdx.z * K * 4 * N;
    const float *dt = sk.dots + (size_t)blockIdx.z * K * 4;
    for (int i = tid; i < K * N; i += 256) {
        const int k = i / N, j = i - k * N;
        stack_lds[k * P + j] = cm[(size_t)k * 4 * N + j];
        stack_lds[k * P + N + j] = cm[(size_t)k * 4 * N + 3 * N + j];
    }
    for (int i = tid; i < K * 4; i += 256) stack_lds[(i >> 2) * P + 2 * N + (i & 3)] = dt[i];
    // right and up are the frame's own for every sample
    float right[N], up[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { right[j] = cm[N + j]; up[j] = cm[2 * N + j]; }
    __syncthreads();
    const PixelRef pr = locate_pixel<64, 4>(tg, tid & 63, tid >> 6, tid);
    if (!pr.valid) return;
    // flat_origin_ray_source::operator() (tracer.hpp:71-75), as primary_dir has it
    const float sx = tg.fovI * ((float)pr.x - tg.half_w);
    const float sy = tg.fovI * ((float)pr.y - tg.half_h);
    float side[N];
#pragma unroll
    for (int j = 0; j < N; ++j) side[j] = right[j] * sx;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < K; ++k) {
        const float *s = stack_lds + k * P;
        float org[N], dir[N];
#pragma unroll
        for (int j = 0; j < N; ++j) { org[j] = s[j]; dir[j] = (s[N + j] + side[j]) - up[j] * sy; }
        float sq = dir[0] * dir[0];
#pragma unroll
        for (int j = 1; j < N; ++j) sq = sq + dir[j] * dir[j];
        float r, g, b;
        stack_box_color<N>(org, dir, sq, s + 2 * N, sx, sy, r, g, b);
        const float *w = sk.weights + 3 * k;
        acc[0] = acc[0] + (w[0] * stack_clamp01(r));
        acc[1] = acc[1] + (w[1] * stack_clamp01(g));
        acc[2] = acc[2] + (w[2] * stack_clamp01(b));
    }
    emit_pixel(tg, pr, acc[0], acc[1], acc[2]);
}

template <int N>
int launch_box_stack(const NtLaunchInfo &li, const NtTarget &tg, const NtStack &sk) {
    if (tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1 || tg.colors_out || !sk.cams || !sk.dots || sk.count < 1 ||
        sk.count > NT_DEV_STACK_MAX) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a view stack launch that is not for whole frames, or without its cameras");
        return -1;
    }
    dim3 grid;
    grid_for(tg, 64, 4, li.nframes, grid);
    const size_t lds = (size_t)sk.count * box_stack_pitch<N>() * sizeof(float);
    hipLaunchKernelGGL(box_stack<N>, grid, dim3(256), lds, (hipStream_t)li.stream, tg, sk);
    return 0;
}

}  // namespace
