// nt_resolve.hpp -- the second stage of a supersampled render (nt_scene_set_supersampling): the box filter
// that turns the s x s samples of a pixel into the pixel.
//
// The first stage is an ordinary render of the s*W x s*H frame in the plain fp32 x 3 format (12-byte pixels of big-endian
// floats, each component already clamped to [0, 1] by the packer) into a scratch buffer.  This kernel reads those samples,
// sums the s*s of a pixel in fp32 in row-major order (plain adds: -ffp-contract=off), divides by (float)(s*s) and hands the
// colour to emit_pixel -- the code every render kernel ends in, so every container, `reversed`, any pitch and an unaligned
// `dest` behave exactly as they do for a single-sample frame.
//
// A wave owns 64 consecutive pixels of an output row (one block = one wave).  Its share of one sample row is one contiguous
// run of 64 * s * 12 bytes, which it loads with lane-contiguous dwords (16 bytes a lane where the rows are 16-byte aligned)
// and turns round in LDS, so that each lane then finds the 3 * s floats of its own pixel side by side; a lane's LDS stride
// is made odd, which keeps those reads free of bank conflicts.  Streaming: 12 * s * s bytes in, bpp bytes out a pixel.
#pragma once
#include "nt_pixel.hpp"

namespace {

struct NtResolveSrc {
    const uint32_t *samples;  // first sample row of the launch's first frame
    long long frame_stride;   // dwords between the frames of the launch
    long long pitch;          // dwords a sample row (3 * s * width)
    int vec4;                 // every sample row starts on a 16-byte boundary
};

template <int S>
__global__ __launch_bounds__(64) void resolve_kernel(NtResolveSrc src, NtTarget tg) {
    constexpr int PX = 3 * S;                            // dwords a pixel in one sample row
    constexpr int STRIDE = PX | 1;                       // ... and its stride in LDS: odd
    constexpr int G = S <= 4 ? S : (S == 5 ? 3 : 2);     // sample rows in flight (3 * S * G registers of loads a lane)
    constexpr int RUN = 64 * PX;                         // dwords of the wave in one sample row
    constexpr int NV = (RUN / 4 + 63) / 64;              // 16-byte loads a lane and sample row
    __shared__ uint32_t lds[G * 64 * STRIDE];
    if (nt_aborted(tg)) return;
    const int lane = (int)threadIdx.x;
    const int row = (int)blockIdx.y;                     // relative to row_begin
    const int orow = tg.row_begin + row;
    const int y = nt_image_row(tg, orow);
    if (row >= tg.row_count || y >= tg.height) return;   // (the same for the whole block)
    const int x0 = (int)blockIdx.x * 64;
    const int x = x0 + lane;
    const int inside = tg.width - x0 < 64 ? PX * (tg.width - x0) : RUN;    // dwords of the run that lie in the image
    const uint32_t *base = src.samples + (long long)blockIdx.z * src.frame_stride + (long long)row * S * src.pitch + (long long)x0 * PX;
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j0 = 0; j0 < S; j0 += G) {
        if (src.vec4) {
            uint4 v[G][NV];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (j0 + g < S) {
                    const uint4 *p = reinterpret_cast<const uint4 *>(base + (long long)(j0 + g) * src.pitch);
#pragma unroll
                    for (int k = 0; k < NV; ++k) {
                        const int q = k * 64 + lane;
                        v[g][k] = 4 * q < inside ? p[q] : make_uint4(0u, 0u, 0u, 0u);     // (`inside` is a multiple of 4 here)
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (j0 + g < S) {
#pragma unroll
                    for (int k = 0; k < NV; ++k) {
                        const int e = 4 * (k * 64 + lane);
                        if (e < RUN) {
                            const uint32_t w[4] = {v[g][k].x, v[g][k].y, v[g][k].z, v[g][k].w};
#pragma unroll
                            for (int t = 0; t < 4; ++t) lds[g * 64 * STRIDE + (e + t) + (e + t) / PX * (STRIDE - PX)] = w[t];
                        }
                    }
                }
            }
        } else {
            uint32_t v[G][PX];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (j0 + g < S) {
                    const uint32_t *p = base + (long long)(j0 + g) * src.pitch;
#pragma unroll
                    for (int k = 0; k < PX; ++k) {
                        const int e = k * 64 + lane;
                        v[g][k] = e < inside ? p[e] : 0u;
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (j0 + g < S) {
#pragma unroll
                    for (int k = 0; k < PX; ++k) {
                        const int e = k * 64 + lane;
                        lds[g * 64 * STRIDE + e + e / PX * (STRIDE - PX)] = v[g][k];
                    }
                }
            }
        }
        __syncthreads();
        // the pixel's samples, one after the other: j outer, i inner, starting from sample (0, 0)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (j0 + g < S) {
#pragma unroll
                for (int i = 0; i < S; ++i) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float f = __uint_as_float(bswap32(lds[g * 64 * STRIDE + lane * STRIDE + 3 * i + c]));
                        acc[c] = (j0 + g == 0 && i == 0) ? f : acc[c] + f;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (x >= tg.width) return;
    const float count = (float)(S * S);
    PixelRef pr;
    pr.x = x;
    pr.y = y;
    pr.offset = (long long)blockIdx.z * tg.frame_stride + (long long)(tg.compact ? orow : y) * tg.pitch + (long long)x * tg.bpp;
    pr.hit_index = 0;
    pr.valid = true;
    emit_pixel(tg, pr, acc[0] / count, acc[1] / count, acc[2] / count);
}

template <int S>
void launch_resolve(hipStream_t stream, const NtResolveSrc &src, int nframes, const NtTarget &tg) {
    const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)tg.row_count, (unsigned)nframes);
    hipLaunchKernelGGL(resolve_kernel<S>, grid, dim3(64), 0, stream, src, tg);
}

// `samples`: the s * row_count sample rows of each of the launch's frames (12-byte pixels, `pitch_bytes` = 12 * s * width a
// row, `frame_stride_bytes` between frames); tg: where the pixels of owned rows [row_begin, row_begin + row_count) go
int launch_resolve_any(int s, hipStream_t stream, const void *samples, long long frame_stride_bytes, long long pitch_bytes, int nframes,
                       const NtTarget &tg) {
    NtResolveSrc src;
    src.samples = (const uint32_t *)samples;
    src.frame_stride = frame_stride_bytes / 4;
    src.pitch = pitch_bytes / 4;
    src.vec4 = ((uintptr_t)samples % 16 == 0 && frame_stride_bytes % 16 == 0 && pitch_bytes % 16 == 0) ? 1 : 0;
    switch (s) {
        case 2: launch_resolve<2>(stream, src, nframes, tg); break;
        case 3: launch_resolve<3>(stream, src, nframes, tg); break;
        case 4: launch_resolve<4>(stream, src, nframes, tg); break;
        case 5: launch_resolve<5>(stream, src, nframes, tg); break;
        case 6: launch_resolve<6>(stream, src, nframes, tg); break;
        case 7: launch_resolve<7>(stream, src, nframes, tg); break;
        case 8: launch_resolve<8>(stream, src, nframes, tg); break;
        default:
            snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "resolve kernel: no such supersampling factor (%d)", s);
            return -2;
    }
    return finish_launch("resolve kernel launch");
}

}  // namespace
