// nt_boxhits.hpp -- BoxScene hit buffers for compile-time N: which face of the cube a pixel sees, and how far away it is.  For
// pixel (x, y) of every frame the record of hypercube_intersects (tracer.hpp:115-152) taken one step further than the colour
// needs it: the face (axis i, side s) whose entry test passes first in the reference's ascending order, and its dist -- one
// 16-byte record (nt_ray_hit: dist, item = i, lane = 1 for the face at +1 and 0 for the face at -1, n_transparent = 0) a pixel,
// FLT_MAX, -1, -1, 0 where the ray sees nothing.  The rule in full: ntracer_hip.h, "BoxScene hit buffers".
// Face lines (nt_scene_set_box_lines): a pixel with a hit is marked where a neighbour sees nothing (silhouette) or another face
// that is not nearer (an edge of the cube); box_lines computes the records of a tile and its one-pixel halo into LDS, marks from
// them and draws in the same kernel, so no record crosses HBM.
// Instantiated per N by nt_inst_boxhits.hip; the run-time-n kernels and the dispatcher (nt_launch_box_faces) are in nt_var.hip.
#pragma once
#include "nt_box.hpp"

namespace {

// box_color<N>'s candidate search and near-tie loop (see there for why only the near-ties of the candidate reached last can pass
// the reference's test), keeping the face and the distance instead of the shade.  face = -1: no face passes, or the one that
// does lies at dist >= FLT_MAX (tracer.hpp:142 with the default cutoff); side and dist are then left as they came in.
template <int N>
__device__ __forceinline__ void box_face(const float (&o)[N], const float (&dir)[N], bool maybe, int &face, int &side, float &dist_out) {
    bool done = false;     // a face passed the slab test (hit, or dist >= cutoff)
    float num[N];
    bool pre[N];
    // candidates: dist > 0 needs a non-zero numerator with the sign of d_i; track the last-reached one
    float aK = 0.0f, bK = 1.0f, oK = 0.0f;
    bool any = false;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float di = dir[i];
        const float s = di < 0.0f ? 1.0f : -1.0f;
        num[i] = s - o[i];
        pre[i] = maybe && ((num[i] > 0.0f && di > 0.0f) || (num[i] < 0.0f && di < 0.0f));
        const float a = fabsf(num[i]), bb = fabsf(di);
        // a/bb > aK/bK  <=>  a*bK > aK*bb   (all positive)
        if (pre[i] && (!any || a * bK > aK * bb)) { aK = a; bK = bb; oK = o[i]; any = true; }
    }
    const float mu = 1e-4f * (1.0f + fabsf(oK));
    const float aKm = (aK - mu) * (1.0f - 1e-6f);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        // near-tie with the last-reached face (always true for that face itself); NaN-safe: !(x < y)
        const bool tie = pre[i] && !done && !(fabsf(num[i]) * bK < fabsf(dir[i]) * aKm);
        if (__builtin_amdgcn_ballot_w64(tie) != 0ull) {
            const float di = dir[i];
            const float dist = num[i] / di;
            bool ok = tie && dist > 0.0f;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                if (j != i) {
                    const float p = dir[j] * dist + o[j];
                    ok = ok && !(fabsf(p) > (1.0f + NT_FUZZ));
                }
            }
            if (ok) {
                done = true;
                if (!(dist >= FLT_MAX)) {
                    face = i;
                    side = di < 0.0f ? 1 : 0;       // s = +1: the face at +1
                    dist_out = dist;
                }
            }
        }
    }
}

// The records of whole frames.  box_kernel's block shape: a lane walks a column of NT_BOXROWS rows, a wave covers 64 consecutive
// pixels of a row (one 1 KiB run of dwordx4 stores), four waves a block; frames in blockIdx.z.  box_may_hit in front: a wave none
// of whose rays can reach the cube writes its "no hit" records without a division.
template <int N>
__global__ __launch_bounds__(256) void box_hits(NtCameraFixed cam, NtTarget tg, NtBoxFaces bf) {
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    float org[N], right[N], up[N], fwd[N], dir[N];
    load_camera<N>(cam, org, right, up, fwd);
    float dots[4];
    if (cam.buf) {
        const float *dp = cam.dots + (size_t)blockIdx.z * 4;
        dots[0] = dp[0]; dots[1] = dp[1]; dots[2] = dp[2]; dots[3] = dp[3];
    } else {
        dots[0] = cam.odots[0]; dots[1] = cam.odots[1]; dots[2] = cam.odots[2]; dots[3] = cam.odots[3];
    }
    constexpr int R = NT_BOXROWS;
    const int row0 = ((int)blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(tid >> 6)) * R;
    const int x = (int)blockIdx.x * 64 + (tid & 63);
    if (x >= tg.width) return;
    const float sx = tg.fovI * ((float)x - tg.half_w);
    float base[N];
#pragma unroll
    for (int j = 0; j < N; ++j) base[j] = fwd[j] + right[j] * sx;
    int4 *out = reinterpret_cast<int4 *>(bf.recs) + (long long)blockIdx.z * bf.frame_stride + x;
    for (int rr = 0; rr < R; ++rr) {
        const int y = row0 + rr;                        // the same for the whole wave
        if (y >= tg.height) return;
        // flat_origin_ray_source::operator() (tracer.hpp:71-75), as the plain kernels form it
        const float sy = tg.fovI * ((float)y - tg.half_h);
#pragma unroll
        for (int j = 0; j < N; ++j) dir[j] = base[j] - up[j] * sy;
        float sq = dir[0] * dir[0];
#pragma unroll
        for (int j = 1; j < N; ++j) sq = sq + dir[j] * dir[j];
        const bool maybe = box_may_hit(N, dots, sx, sy, sq);
        int face = -1, side = -1;
        float dist = FLT_MAX;
        if (__builtin_amdgcn_ballot_w64(maybe) != 0ull) {
            const float len = sqrtf(sq);
#pragma unroll
            for (int j = 0; j < N; ++j) dir[j] = dir[j] / len;
            box_face<N>(org, dir, maybe, face, side, dist);
        }
        out[(long long)y * tg.width] = make_int4(__float_as_int(dist), face, side, 0);
    }
}

// ---- face lines -------------------------------------------------------------------------------------------------------
// The tile of a block: 64 x 32 pixels, box_kernel's block shape again (four waves, a lane walks a column of NT_BOXROWS rows, a
// wave covers 64 consecutive pixels of a row).  Its records with a one-pixel halo, 8 bytes each -- (dist, code), code =
// 2 * axis + side, -1: the ray sees nothing, -2: no pixel there (outside the image: "no neighbour", not "no hit") -- are
// 66 x 34 x 8 = 17 952 bytes of LDS; the 192 halo pixels (the corners are never read) are one more pixel for three of the four
// waves, 9.4 % of the face tests done twice.
#define NT_BOXLINES_TW 64
#define NT_BOXLINES_TH (4 * NT_BOXROWS)
#define NT_BOXLINES_PITCH (NT_BOXLINES_TW + 2)

// the record of the pixel at (sx, sy) from base = forward + right * sx; xval (WANT_X): the component of d the plain colour is made
// of, d_face on a hit and d_0 without one
template <int N, bool WANT_X>
__device__ __forceinline__ void box_line_record(const float (&org)[N], const float (&base)[N], const float (&up)[N], const float (&dots)[4],
                                                float sx, float sy, float &dist, int &code, float &xval) {
    float dir[N];
#pragma unroll
    for (int j = 0; j < N; ++j) dir[j] = base[j] - up[j] * sy;
    float sq = dir[0] * dir[0];
#pragma unroll
    for (int j = 1; j < N; ++j) sq = sq + dir[j] * dir[j];
    const bool maybe = box_may_hit(N, dots, sx, sy, sq);
    int face = -1, side = -1;
    dist = FLT_MAX;
    if (__builtin_amdgcn_ballot_w64(maybe) != 0ull) {
        const float len = sqrtf(sq);
#pragma unroll
        for (int j = 0; j < N; ++j) dir[j] = dir[j] / len;
        box_face<N>(org, dir, maybe, face, side, dist);
        xval = dir[0];
#pragma unroll
        for (int j = 1; j < N; ++j) xval = face == j ? dir[j] : xval;
    } else if (WANT_X) {
        xval = dir[0] / sqrtf(sq);          // (the one component the background needs)
    }
    code = face >= 0 ? 2 * face + side : -1;
}

// what neighbour q = (dist, code) adds to the mask byte of p, a pixel with a hit: outline_pair's rule with the crease test always
// true -- two different faces of a cube are perpendicular or opposite
// (the one copy of the rule, for box_lines and for box_lines_var of nt_var.hip)
__device__ __forceinline__ int box_line_pair(float pdist, int pcode, float qdist, int qcode) {
    if (qcode == -2) return 0;                                   // no pixel there
    if (qcode < 0) return NT_DEV_OUTLINE_SILHOUETTE;
    if (qcode == pcode) return 0;
    if (pdist > qdist) return 0;                                 // the nearer pixel carries the line (both on an exact tie)
    return NT_DEV_OUTLINE_CREASE;
}
__device__ __forceinline__ int box_line_pair(float pdist, int pcode, const int2 &q) { return box_line_pair(pdist, pcode, __int_as_float(q.x), q.y); }

// the plain colour of a pixel from xval, clamped, blended with the lines' colour where the mask is set (ntracer_hip.h), and emitted:
// a wave without a marked pixel through the emitters of the plain kernels where the target allows (BoxScene colours have g == b)
__device__ __forceinline__ void box_line_emit(const NtTarget &tg, const NtBoxFaces &bf, const PixelRef &pr, bool hit, float xval, int m) {
    float r, g, b;
    if (hit) {
        const float shade = fabsf(xval);      // sine = d_i * (-sign d_i) <= 0, shade = -sine (tracer.hpp:105-107)
        r = shade * 1.0f;
        g = shade * 0.5f;
        b = shade * 0.5f;
    } else {
        box_background(xval, r, g, b);
    }
    if (__builtin_amdgcn_ballot_w64(m != 0) == 0ull) {
        if (tg.plain_f32[0] >= 0 && tg.bpp == 12 && tg.aligned4) { emit_f32x3(tg, pr.offset, r, g); return; }
        if (plain_rgb(tg)) { emit_plain(tg, pr, plain_quantize(tg, r), plain_quantize(tg, g)); return; }
    }
    const float keep = 1.0f - bf.strength;
    float p[3] = {r, g, b};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = p[k] > 0.0f ? p[k] : 0.0f;
        v = v < 1.0f ? v : 1.0f;
        p[k] = m != 0 ? (v * keep) + (bf.color[k] * bf.strength) : v;
    }
    emit_pixel(tg, pr, p[0], p[1], p[2]);
}

// DRAW: the frame with the lines drawn into tg (the whole image of frame blockIdx.z, no bands); else the mask bytes into bf.mask
template <int N, bool DRAW>
__global__ __launch_bounds__(256) void box_lines(NtCameraFixed cam, NtTarget tg, NtBoxFaces bf) {
    __shared__ int2 tile[(NT_BOXLINES_TH + 2) * NT_BOXLINES_PITCH];
    if (nt_aborted(tg)) return;               // (every lane reads the same word: the whole block leaves, ahead of the barrier)
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    float org[N], right[N], up[N], fwd[N];
    load_camera<N>(cam, org, right, up, fwd);
    float dots[4];
    if (cam.buf) {
        const float *dp = cam.dots + (size_t)blockIdx.z * 4;
        dots[0] = dp[0]; dots[1] = dp[1]; dots[2] = dp[2]; dots[3] = dp[3];
    } else {
        dots[0] = cam.odots[0]; dots[1] = cam.odots[1]; dots[2] = cam.odots[2]; dots[3] = cam.odots[3];
    }
    constexpr int R = NT_BOXROWS;
    const int x0 = (int)blockIdx.x * NT_BOXLINES_TW, y0 = (int)blockIdx.y * NT_BOXLINES_TH;
    const int x = x0 + lane;
    float pdist[R], pxval[R];
    int pcode[R];
    {
        const float sx = tg.fovI * ((float)x - tg.half_w);
        float base[N];
#pragma unroll
        for (int j = 0; j < N; ++j) base[j] = fwd[j] + right[j] * sx;
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int ly = wv * R + rr;
            const int y = y0 + ly;                          // the same for the whole wave
            pdist[rr] = FLT_MAX;
            pcode[rr] = -2;
            pxval[rr] = 0.0f;
            if (x < tg.width && y < tg.height)
                box_line_record<N, DRAW>(org, base, up, dots, sx, tg.fovI * ((float)y - tg.half_h), pdist[rr], pcode[rr], pxval[rr]);
            tile[(ly + 1) * NT_BOXLINES_PITCH + lane + 1] = make_int2(__float_as_int(pdist[rr]), pcode[rr]);
        }
    }
    if (tid < 2 * NT_BOXLINES_TW + 2 * NT_BOXLINES_TH) {
        // the halo: the row above, the row below, the column to the left, the column to the right
        int hx, hy;
        if (tid < NT_BOXLINES_TW) { hx = tid; hy = -1; }
        else if (tid < 2 * NT_BOXLINES_TW) { hx = tid - NT_BOXLINES_TW; hy = NT_BOXLINES_TH; }
        else if (tid < 2 * NT_BOXLINES_TW + NT_BOXLINES_TH) { hx = -1; hy = tid - 2 * NT_BOXLINES_TW; }
        else { hx = NT_BOXLINES_TW; hy = tid - 2 * NT_BOXLINES_TW - NT_BOXLINES_TH; }
        const int gx = x0 + hx, gy = y0 + hy;
        float hdist = FLT_MAX, hxval;
        int hcode = -2;
        if (gx >= 0 && gy >= 0 && gx < tg.width && gy < tg.height) {
            const float sx = tg.fovI * ((float)gx - tg.half_w);
            float base[N];
#pragma unroll
            for (int j = 0; j < N; ++j) base[j] = fwd[j] + right[j] * sx;
            box_line_record<N, false>(org, base, up, dots, sx, tg.fovI * ((float)gy - tg.half_h), hdist, hcode, hxval);
        }
        tile[(hy + 1) * NT_BOXLINES_PITCH + hx + 1] = make_int2(__float_as_int(hdist), hcode);
    }
    __syncthreads();
    if (x >= tg.width) return;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int ly = wv * R + rr;
        const int y = y0 + ly;
        if (y >= tg.height) return;
        int m = 0;
        if (pcode[rr] >= 0) {
            const int at = (ly + 1) * NT_BOXLINES_PITCH + lane + 1;
            m = box_line_pair(pdist[rr], pcode[rr], tile[at - 1]) | box_line_pair(pdist[rr], pcode[rr], tile[at + 1]) |
                box_line_pair(pdist[rr], pcode[rr], tile[at - NT_BOXLINES_PITCH]) | box_line_pair(pdist[rr], pcode[rr], tile[at + NT_BOXLINES_PITCH]);
            m &= bf.kinds;
        }
        if (DRAW) {
            PixelRef pr;
            pr.x = x;
            pr.y = y;
            pr.offset = (long long)blockIdx.z * tg.frame_stride + (long long)y * tg.pitch + (long long)x * tg.bpp;
            pr.hit_index = 0;
            pr.valid = true;
            box_line_emit(tg, bf, pr, pcode[rr] >= 0, pxval[rr], m);
        } else {
            bf.mask[((long long)blockIdx.z * tg.height + y) * tg.width + x] = (uint8_t)m;
        }
    }
}

template <int N>
int launch_box_faces(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg, const NtBoxFaces &bf) {
    NtCameraFixed cf;
    cf.buf = cam.buf;
    cf.dots = cam.dots;
    for (int k = 0; k < 4; ++k) cf.odots[k] = cam.odots[k];
    cf.n = N;
    for (int k = 0; k < 4 * N; ++k) cf.inl[k] = cam.inl[k];
    hipStream_t st = (hipStream_t)li.stream;
    // (both shapes: 64 columns x 4 * NT_BOXROWS rows a block)
    const dim3 grid((unsigned)((tg.width + 63) / 64), (unsigned)((tg.height + 4 * NT_BOXROWS - 1) / (4 * NT_BOXROWS)), (unsigned)li.nframes);
    if (bf.mode == NT_BOX_FACES_RECORDS) {
        hipLaunchKernelGGL(box_hits<N>, grid, dim3(256), 0, st, cf, tg, bf);
        return 0;
    }
    if (bf.mode == NT_BOX_FACES_DRAW && (tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1 || tg.colors_out)) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a face-line launch that is not for whole frames");
        return -1;
    }
    if (bf.mode == NT_BOX_FACES_DRAW) hipLaunchKernelGGL((box_lines<N, true>), grid, dim3(256), 0, st, cf, tg, bf);
    else hipLaunchKernelGGL((box_lines<N, false>), grid, dim3(256), 0, st, cf, tg, bf);
    return 0;
}

}  // namespace
