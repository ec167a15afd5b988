// nt_parallel.hpp -- renders under the parallel (orthographic) projection for compile-time N.  With half_width > 0 set on a
// scene, pixel (x, y) of a width x height render casts
//     k = half_width / half_w,   sx = k * ((float)x - half_w),   sy = k * ((float)y - half_h)
//     o'[j] = (origin[j] + right[j] * sx) - up[j] * sy,          v = forward,   d = v / |v|
// with d formed as primary_dir forms it (nt_pixel.hpp: |v|^2 summed left to right, sqrtf, one IEEE division a component;
// contraction off, as everywhere); k comes from the host in fp32, in tg.fovI's place.  The image spans 2 * half_width scene
// units across, with square pixels; the scene's fov is ignored.  Everything behind the ray source is a render's own: the
// scene-box test, the walk, the shading, the packing, and the switches.  Whole images, one sample a pixel: no bands, no
// supersampling, no counters, no probes (refused by the host).
// Two routes, as under a lens (nt_lens.hpp).  This file is the packet route -- opaque scenes, stack depth <= 32,
// NTRACER_COMPOSITE_KERNEL unset: parallel_packet walks the tile and leaves the 16-byte record of every pixel; parallel_shade,
// one lane a pixel, re-forms (o', d), picks the record up and shades with the render kernels' own device functions into
// emit_pixel.  Every other scene goes through the ray-colour kernels of nt_rays.hpp behind parallel_expand (nt_var.hip).
#pragma once
#include "nt_composite.hpp"

namespace {

// The packet walk for rays that share their DIRECTION instead of their origin: composite_packet's walk (nt_composite.hpp; its
// mailbox, frame stack and leaf loop are used as they are there) with the branch step turned round.  What the walk needs is a
// wave-uniform control flow -- which node comes next, which leaf items are tested -- and a shared direction gives that as a
// shared origin does: the order in which a ray meets the two children of a branch is decided by the sign of dir[axis], the same
// in all 64 lanes.
//     first = dir[axis] < 0 ? right : left          (left when dir[axis] == 0),       second = the other child.
// Per lane the reference's rules (tracer.hpp:1189-1240) decide, with the lane's own oa = o'[axis], between its near child
// (oa > split ? right : left), its far child, or both; then near / far are put as first / second:
//   * dir[axis] != 0, oa != split: t = (split - oa) * inv.  Mathematically t > 0 exactly when the ray moves towards the split,
//     that is when the lane's near child is `first`.  In floats: split - oa is not zero (gradual underflow) and has the sign of
//     the real difference; |d[axis]| <= 1, since |v|^2 is a left-to-right sum of non-negative terms whose term v[axis]^2 it
//     cannot fall below, and sqrtf(fl(x * x)) == |x| -- so |inv| >= 1, and the product's magnitude is at least |split - oa|: it
//     cannot round to +-0.  Hence t < 0 exactly when the lane is on the far side of the split moving away from it (near ==
//     second; the reference says "near": SECOND ONLY, interval untouched), and t > 0 otherwise (near == first): t > t_far is
//     FIRST ONLY, t < t_near is the reference's "far" = SECOND ONLY, else BOTH -- first with t_far = t, then second with
//     t_near = t unless the first subtree brought a hit with dist <= t.  That is composite_packet's frame, with near = first.
//   * dir[axis] != 0, oa == split: the reference takes direction > 0 ? right : left, which is `second` either way.
//   * dir[axis] == 0: first = left, and the lane takes oa >= split ? right (second) : left (first).
// The null-child rules (:1214, :1234-1237) are composite_packet's, per lane.  On a resume et / ef are recomputed from the
// level's (split, axis) with the lane's own o'.  Per lane the hit is that of the per-lane walk, and so are the leaves it visits
// and their t_near, with composite_packet's one looseness: a `both` lane at a branch without a second child pushes no frame, so
// a later resume restores t_far from the level below -- larger than the reference's, never smaller -- and the lane may then
// enter a second child the reference would have skipped (more tests, the same closest hit).  d and invd are the same in every
// lane (same operands, same operations): the branch decisions on them are taken on readfirstlane'd values.  The plane
// numerators -(N.o' + d) are per lane here, so the leaf computes them itself (the branch composite_packet takes without a
// packet_numerators table); N.d is what is uniform now.
// Always the hit-writing form: records out through pa.hits_out, th.frame_stride bytes between frames.
template <int N, int DEPTH, bool SCAL>
__global__ __launch_bounds__(256, (N <= 4 && !SCAL) ? NT_PACKET_WAVES4 : (N <= 7 ? 5 : 4)) void parallel_packet(NtCompositeDev sc, NtTarget tg, PacketArgs pa) {
    extern __shared__ float2 lds_raw[];
    if (nt_aborted(tg)) return;                           // (four independent waves: no barrier in this kernel)
    const int lane = (int)threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long long slot = (long long)blockIdx.x;
    int rank, frame;
    if (pa.frame_major) { frame = (int)(slot / pa.quads); rank = (int)(slot - (long long)frame * pa.quads); }
    else { rank = (int)(slot / pa.nframes); frame = (int)(slot - (long long)rank * pa.nframes); }
    int *wm = reinterpret_cast<int *>(reinterpret_cast<char *>(lds_raw) + (size_t)wv * pa.lds_per_wave);   // [NT_WM][4] wave mailbox
    int *ustack = wm + NT_WM * 4;                 // [DEPTH][8]: second node, second-lane mask lo, hi, split, axis

    // ---- this wave's tile (whole images: owned row == image row)
    const int quad = pa.order ? pa.order[rank] : rank;
    const int qy = quad / pa.quads_x, qx = quad - qy * pa.quads_x;
    const int tx = qx * 2 + (wv & 1), ty = qy * 2 + (wv >> 1);
    if (tx >= pa.tiles_x || ty >= pa.tiles_y) return;
    const int x = tx * 8 + (lane & 7);
    const int y = ty * 8 + (lane >> 3);
    const bool valid = x < tg.width && y < tg.height;

    float o[N], d[N], invd[N];
    {
        const float *c = pa.cams + (size_t)frame * 4 * N;
        float org[N], right[N], up[N], fwd[N];
#pragma unroll
        for (int k = 0; k < N; ++k) { org[k] = c[k]; right[k] = c[N + k]; up[k] = c[2 * N + k]; fwd[k] = c[3 * N + k]; }
        parallel_origin<N>(tg, org, right, up, x, y, o);
        parallel_dir<N>(fwd, d);
        // invdir = 1/direction (tracer.hpp:1174); NaN marks direction == 0 (see setup_ray_table)
#pragma unroll
        for (int k = 0; k < N; ++k) invd[k] = d[k] != 0.0f ? 1.0f / d[k] : __int_as_float(0x7fc00000);
    }
    Hit hit;
    hit.dist = FLT_MAX; hit.item = -1; hit.lane = -1;
    const float dist0 = aabb_distance<N>(sc, o, d);
    bool active = valid && dist0 >= 0.0f;
    float t_near = dist0, t_far = FLT_MAX;
    int dirty = 0;
    unsigned int bothbits = 0u;   // bit k: this lane entered BOTH sides of the branch pushed at stack level k
    wm_reset(wm, lane);

    int node = sc.root;      // wave-uniform
    int sp = 0;              // wave-uniform
    for (;;) {
        while (node >= 0) {
            if (sc.prune) active = active && !nt_beyond_hit(hit.dist, t_near);
            if (__builtin_amdgcn_ballot_w64(active) == 0ull) { node = -1; break; }
            const NtNode nd = sc.nodes[node];                // uniform address -> scalar load
            if (nd.axis < 0) {
                // ---- leaf: kd_leaf<Store,true>::intersects (tracer.hpp:977-1086), batches only; composite_packet's loop
                // with the numerators formed here
                bool improved = false;
                int item = __builtin_amdgcn_readfirstlane(sc.items[nd.left]);
                bool doit = wm_claim(wm, lane, item, active);
                for (int i = 0; i < nd.right; ++i) {
                    const int cur = item;
                    const bool cur_doit = doit;
                    const bool more = i + 1 < nd.right;
                    if (more) item = __builtin_amdgcn_readfirstlane(sc.items[nd.left + i + 1]);
                    if (__builtin_amdgcn_ballot_w64(cur_doit) == 0ull) {
                        doit = false;
                        if (more) doit = wm_claim(wm, lane, item, active);
                        continue;
                    }
                    if (SCAL && (cur & 3) != 0) {
                        // an unbatched triangle or a solid: the per-lane tests of leaf_closest
                        doit = false;
                        if (more) doit = wm_claim(wm, lane, item, active);
                        if (cur_doit) {
                            float t;
                            if ((cur & 3) == 1) {
                                SimplexRec<N> sr;
                                sr.load(sc.tri_recs + (size_t)(cur >> 2) * sc.rec_stride);
                                t = simplex_scalar_form<N>(sr, o, d, hit.dist);
                            } else {
                                float no_[N], nd_[N];
                                t = solid_intersects<N>(sc, cur >> 2, o, d, hit.dist, false, no_, nd_);
                            }
                            if (t != 0.0f) { hit.dist = t; hit.item = cur; hit.lane = -1; improved = true; }
                        }
                        continue;
                    }
                    const float *base = sc.batch_recs + (size_t)(cur >> 2) * NT_DEV_BATCH * sc.rec_stride;
                    float tl[NT_DEV_BATCH];
                    bool ok1[NT_DEV_BATCH];
#pragma unroll
                    for (int l = 0; l < NT_DEV_BATCH; ++l) {
                        const float *rec = base + (size_t)l * sc.rec_stride;
                        float denom = rec[1] * d[0];
#pragma unroll
                        for (int k = 1; k < N; ++k) denom = denom + rec[1 + k] * d[k];
                        float no = rec[1] * o[0];
#pragma unroll
                        for (int k = 1; k < N; ++k) no = no + rec[1 + k] * o[k];
                        tl[l] = -(no + rec[0]) / denom;
                        ok1[l] = denom != 0.0f && tl[l] >= 0.0f;
                    }
                    doit = false;
                    if (more) doit = wm_claim(wm, lane, item, active);
                    float min_t = hit.dist;
                    int r = -1;
#pragma unroll
                    for (int l = 0; l < NT_DEV_BATCH; ++l) {
                        // stage 2 only if some lane can still accept this simplex (same accept rule as below)
                        const float t = tl[l];
                        if (__builtin_amdgcn_ballot_w64(cur_doit && ok1[l] && t != 0.0f && t < min_t) == 0ull) continue;
                        const float *rec = base + (size_t)l * sc.rec_stride;
                        float pside[N];
#pragma unroll
                        for (int k = 0; k < N; ++k) pside[k] = rec[1 + N + k] - (o[k] + t * d[k]);
                        bool ok = ok1[l];
                        float tot = 0.0f;
#pragma unroll
                        for (int e = 0; e < N - 1; ++e) {
                            const float *en = rec + 1 + 2 * N + e * N;
                            float area = en[0] * pside[0];
#pragma unroll
                            for (int k = 1; k < N; ++k) area = area + en[k] * pside[k];
                            ok = ok && area >= -NT_FUZZ;
                            tot += area;
                        }
                        ok = ok && tot <= (1.0f + NT_FUZZ);
                        if (ok && t != 0.0f && t < min_t) { min_t = t; r = l; }
                    }
                    if (cur_doit && r >= 0) { hit.dist = min_t; hit.item = cur; hit.lane = r; improved = true; }
                }
                if (improved) dirty = sp;
                node = -1;
                break;
            }
            // ---- branch: kd_node_intersection::operator() (tracer.hpp:1189-1240), see the head comment
            const int axis = __builtin_amdgcn_readfirstlane(nd.axis);      // uniform
            float oa = o[0];                                   // per lane
#pragma unroll
            for (int k = 1; k < N; ++k) oa = axis == k ? o[k] : oa;
            const float inv = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pick_uniform<N>(invd, axis))));   // uniform
            const bool rev = inv < 0.0f;                       // (false for the NaN of dir[axis] == 0)
            const int n_first = rev ? nd.right : nd.left;
            const int n_second = rev ? nd.left : nd.right;
            bool go_first = false, go_second = false, both = false;
            float t = 0.0f;
            if (active) {
                if (inv == inv) {
                    if (oa == nd.split) {
                        go_second = true;
                    } else {
                        t = (nd.split - oa) * inv;
                        if (t < 0.0f) go_second = true;        // the lane's near child is `second`
                        else if (t > t_far) go_first = true;
                        else if (t < t_near) go_second = true;
                        else both = true;
                    }
                } else {
                    // direction[axis] == 0: node = origin >= split ? right : left, and first == left
                    if (oa >= nd.split) go_second = true; else go_first = true;
                }
            }
            // a `both` lane with no first child continues in second with t_near = t (tracer.hpp:1234-1237);
            // with no second child it returns after first (:1214)
            const bool first_lane = (go_first || both) && n_first >= 0;
            const bool second_after = (go_second || both) && n_second >= 0 && n_first >= 0;      // second AFTER a first subtree
            const unsigned long long m_first = __builtin_amdgcn_ballot_w64(first_lane);
            const unsigned long long m_second = __builtin_amdgcn_ballot_w64(second_after);
            if (m_first != 0ull) {
                if (m_second != 0ull && sp < DEPTH) {
                    if (lane == 0) {
                        ustack[sp * 8 + 0] = n_second;
                        ustack[sp * 8 + 1] = (int)(unsigned int)(m_second & 0xffffffffull);
                        ustack[sp * 8 + 2] = (int)(unsigned int)(m_second >> 32);
                        ustack[sp * 8 + 3] = __float_as_int(nd.split);
                        ustack[sp * 8 + 4] = axis;
                    }
                    bothbits = both ? (bothbits | (1u << sp)) : (bothbits & ~(1u << sp));
                    ++sp;
                }
                if (both && first_lane) t_far = t;
                active = first_lane;
                node = n_first;
            } else {
                // no lane enters first: lanes bound for second go there now
                const bool goes = (go_second || both) && n_second >= 0;
                if (both && goes) t_near = t;
                active = goes;
                node = __builtin_amdgcn_ballot_w64(goes) != 0ull ? n_second : -1;
            }
        }
        // ---- the frame returned: resume the innermost pending second side
        if (sp == 0) break;
        --sp;
        const int far = __builtin_amdgcn_readfirstlane(ustack[sp * 8 + 0]);
        if (tg.abort_word != nullptr && (far & NT_ABORT_POLL_MASK) == 0 && nt_aborted(tg)) return;
        const unsigned long long m = ((unsigned long long)(unsigned int)__builtin_amdgcn_readfirstlane(ustack[sp * 8 + 2]) << 32) |
                                     (unsigned int)__builtin_amdgcn_readfirstlane(ustack[sp * 8 + 1]);
        const bool was_both = ((bothbits >> sp) & 1u) != 0u;
        const bool near_hit = sp < dirty;
        if (dirty > sp) dirty = sp;
        bool join = ((m >> lane) & 1ull) != 0ull;
        if (__builtin_amdgcn_ballot_w64(join && was_both) != 0ull) {
            // the split distance of the branch being resumed, recomputed from its (split, axis) and the lane's o': same
            // operands, same operations as at the push, hence the same float
            const float psplit = __int_as_float(__builtin_amdgcn_readfirstlane(ustack[sp * 8 + 3]));
            const int paxis = __builtin_amdgcn_readfirstlane(ustack[sp * 8 + 4]);
            float poa = o[0];
#pragma unroll
            for (int k = 1; k < N; ++k) poa = paxis == k ? o[k] : poa;
            const float et = (psplit - poa) * pick_uniform<N>(invd, paxis);
            // t_far of the frame being resumed = the split distance of the innermost pending branch below that this
            // lane entered on both sides (its first subtree is where we are); none: the root's t_far
            const unsigned int below = bothbits & ((1u << sp) - 1u);
            float ef = FLT_MAX;
            if (below != 0u) {
                const int ks = 31 - __clz((int)below);
                const float s2 = __int_as_float(ustack[ks * 8 + 3]);
                const int a2 = ustack[ks * 8 + 4];
                ef = (s2 - pick_lane<N>(o, a2)) * pick_lane<N>(invd, a2);
            }
            if (join && was_both) {                        // a `both` lane: (hit && o_hit.dist <= t) -> return
                if (near_hit && hit.dist <= et) join = false;
                else { t_near = et; t_far = ef; }
            }
        }
        active = join;
        node = far;
    }
    // a pixel whose ray misses the scene box, or hits nothing in it: FLT_MAX, -1, -1
    if (valid) *reinterpret_cast<float4 *>(reinterpret_cast<char *>(pa.hits_out) + (long long)frame * tg.frame_stride +
                                          ((long long)y * tg.width + x) * 16) =
        make_float4(hit.dist, __int_as_float(hit.item), __int_as_float(hit.lane), 0.0f);
}

// The shading pass behind parallel_packet: lens_shade's layout (a 256-thread block takes a 16x16 tile of frame blockIdx.z, its
// four independent waves an 8x8 tile each); FEAT / SCALP as composite_kernel has them; without FEAT no LDS is used.
template <int N, bool FEAT, bool SCALP>
__global__ __launch_bounds__(256) NT_SHADE_OCC void parallel_shade(NtCompositeDev sc, NtTarget tg, NtParallel pl) {
    extern __shared__ float2 lds_raw[];
    if (nt_aborted(tg)) return;
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const PixelRef pr = locate_pixel<16, 16>(tg, (wv & 1) * 8 + (lane & 7), (wv >> 1) * 8 + (lane >> 3), tid);
    if (!pr.valid) return;
    const float *cm = pl.cams + (size_t)blockIdx.z * 4 * N;
    float cam_o[N], right[N], up[N], fwd[N], org[N], dir[N];
#pragma unroll
    for (int k = 0; k < N; ++k) { cam_o[k] = cm[k]; right[k] = cm[N + k]; up[k] = cm[2 * N + k]; fwd[k] = cm[3 * N + k]; }
    parallel_origin<N>(tg, cam_o, right, up, pr.x, pr.y, org);
    parallel_dir<N>(fwd, dir);
    const float4 h = reinterpret_cast<const float4 *>(pl.hits)[pr.hit_index];
    Hit hit;
    hit.dist = h.x;
    hit.item = __float_as_int(h.y);
    hit.lane = __float_as_int(h.z);
    Color3 c;
    if (FEAT) {
        const WaveLds w = wave_lds(reinterpret_cast<char *>(lds_raw), wv, sc.stack_depth, N);
        Stats st = {0, 0, 0, 0, 0, 0, 0, 0};
        c = composite_color<N, true, false, SCALP>(sc, w, lane, org, dir, st, &hit);
    } else {
        c = hit.item >= 0 ? surface_color_lean<N>(sc, hit, org, dir) : background_color<N>(sc, dir);
    }
    emit_pixel(tg, pr, c.r, c.g, c.b);
}

// tg: the whole image of every frame (row_begin 0, row_count = height, no bands), tg.fovI = half_width / half_w; li.hit_buf:
// li.hit_frames frames of width * height records.  Frames are chunked by what the hit scratch holds.
template <int N>
int launch_parallel_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtParallel &pl) {
    if (!sc.all_opaque || sc.checked || sc.stack_depth > 32 || !li.hit_buf || li.hit_frames < 1 || !pl.cams ||
        tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a parallel render that is not for the packet walk");
        return -1;
    }
    const size_t lds = 4 * wave_lds_bytes(sc.stack_depth, N);
    const bool feat = scene_feat(sc);
    hipStream_t s = (hipStream_t)li.stream;
    PacketArgs pk = packet_args(li, sc, tg.width, tg.height);
    pk.hits_out = (float4 *)li.hit_buf;
    // (this walk reads no numerators: the hit scratch alone decides the chunk, and packet_frames is the whole chunk head)
    const int chunk = li.hit_frames < li.nframes ? li.hit_frames : li.nframes;
    const NtTarget th = packet_record_view(tg, (long long)tg.width * tg.height);
    for (int f0 = 0; f0 < li.nframes; f0 += chunk) {
        const int cnt = packet_frames<N>(pk, pl.cams, f0, chunk, li.nframes);
        const dim3 pgrid = packet_grid(pk, cnt);
        if (sc.has_scalar_prims) hipLaunchKernelGGL((parallel_packet<N, 32, true>), pgrid, dim3(256), (size_t)4 * pk.lds_per_wave, s, sc, th, pk);
        else hipLaunchKernelGGL((parallel_packet<N, 32, false>), pgrid, dim3(256), (size_t)4 * pk.lds_per_wave, s, sc, th, pk);
        const NtTarget t2 = chunk_target(tg, f0);
        NtParallel p2 = pl;
        p2.cams = pk.cams;
        p2.hits = li.hit_buf;
        dim3 g2;
        grid_for(t2, 16, 16, cnt, g2);
        if (!feat) hipLaunchKernelGGL((parallel_shade<N, false, false>), g2, dim3(256), 0, s, sc, t2, p2);
        else if (sc.has_scalar_prims) hipLaunchKernelGGL((parallel_shade<N, true, true>), g2, dim3(256), lds, s, sc, t2, p2);
        else hipLaunchKernelGGL((parallel_shade<N, true, false>), g2, dim3(256), lds, s, sc, t2, p2);
    }
    return 0;
}

}  // namespace
