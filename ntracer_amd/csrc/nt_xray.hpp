// nt_xray.hpp -- X-ray views for compile-time N (nt_scene_set_xray, nt_crossing_counts): every primitive the
// primary ray of a pixel crosses, counted, and the background behind them times the product of their materials' transmittances
// (ntracer_hip.h has the rule in full).
//
// xray_packet is composite_packet's wave-uniform walk -- shared origin, the uniform frame stack `ustack`, `bothbits`, scalar loads
// of nodes, items and records, packet_numerators when the launch has them -- without a hit: no cutoff, no pruning, a lane stays
// active over its whole [dist0, FLT_MAX] window, and the wave visits every leaf some lane's ray pierces.  What a nearest-hit walk
// may forget a count may not: wm_claim's direct-mapped mailbox evicts, and a repeated test would count twice.  So the wave keeps
// an exact "seen" bit for every item of the scene in LDS -- batches, triangles and Solids concatenated the way `checked_words`
// counts them -- cleared once a tile (a wave walks one tile a launch).  The FIRST time the wave meets an item every valid lane
// with dist0 >= 0 tests it, whether or not that lane's own interval reaches this leaf; the item is skipped ever after.  The test
// does not depend on the leaf, so the result is the rule's tree-independent set: the tree only culls.  Solids are the exception:
// all of them are tested in front of the walk (see there), and their bits of the set stay clear.
// Instantiated per N by nt_inst_xray.hip; the run-time-n route, xray_var, is in nt_var.hip.
#pragma once
#include "nt_composite.hpp"

namespace {

// the bytes a wave of xray_packet carves: the uniform frame stack [DEPTH = 32][8] and the seen bitset, whole 16-byte rows of it
__host__ __device__ __forceinline__ size_t xray_lds_per_wave(long long items) {
    return (size_t)32 * 32 + (size_t)((items + 127) / 128) * 16;
}

// first meeting of `id` by this wave?  Uniform address, uniform answer; lane 0 records it with an ordinary LDS store, which the
// wave's later reads of the word follow in program order.
__device__ __forceinline__ bool xray_first(uint32_t *seen, int lane, int id) {
    uint32_t *p = seen + (id >> 5);
    const uint32_t v = (uint32_t)__builtin_amdgcn_readfirstlane((int)*p);
    const uint32_t m = 1u << (id & 31);
    if ((v & m) != 0u) return false;
    if (lane == 0) *p = v | m;
    return true;
}

// SCAL: the scene has unbatched triangles or Solids.  COUNTS: the int32 count of every pixel out through xr.counts
// ([frame][height][width]); nothing is drawn and tg.dest is never touched.
template <int N, int DEPTH, bool SCAL, bool COUNTS>
__global__ __launch_bounds__(256, 4) void xray_packet(NtCompositeDev sc, NtTarget tg, PacketArgs pa, NtXray xr, int seen_words) {
    extern __shared__ float2 lds_raw[];
    if (nt_aborted(tg)) return;                           // (four independent waves: no barrier in this kernel)
    const int lane = (int)threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long long slot = (long long)blockIdx.x;
    int rank, frame;
    if (pa.frame_major) { frame = (int)(slot / pa.quads); rank = (int)(slot - (long long)frame * pa.quads); }
    else { rank = (int)(slot / pa.nframes); frame = (int)(slot - (long long)rank * pa.nframes); }
    int *ustack = reinterpret_cast<int *>(reinterpret_cast<char *>(lds_raw) + (size_t)wv * pa.lds_per_wave);     // [DEPTH][8]
    uint32_t *seen = reinterpret_cast<uint32_t *>(ustack + DEPTH * 8);                                            // [seen_words]

    // ---- this wave's tile
    const float *numer = pa.numer ? pa.numer + (size_t)frame * pa.n_batches * NT_DEV_BATCH : nullptr;     // uniform
    const int quad = pa.order ? pa.order[rank] : rank;
    const int qy = quad / pa.quads_x, qx = quad - qy * pa.quads_x;
    const int tx = qx * 2 + (wv & 1), ty = qy * 2 + (wv >> 1);
    if (tx >= pa.tiles_x || ty >= pa.tiles_y) return;
    const int x = tx * 8 + (lane & 7);
    const int row = ty * 8 + (lane >> 3);
    bool valid = x < tg.width && row < tg.row_count;
    const int orow = tg.row_begin + row;
    const int y = nt_image_row(tg, orow);
    valid = valid && y < tg.height;

    float o[N], d[N], invd[N];
    {
        const float *c = pa.cams + (size_t)frame * 4 * N;
        float right[N], up[N], fwd[N];
#pragma unroll
        for (int k = 0; k < N; ++k) { o[k] = c[k]; right[k] = c[N + k]; up[k] = c[2 * N + k]; fwd[k] = c[3 * N + k]; }
        primary_dir<N>(tg, right, up, fwd, x, y, d);
#pragma unroll
        for (int k = 0; k < N; ++k) invd[k] = d[k] != 0.0f ? 1.0f / d[k] : __int_as_float(0x7fc00000);
    }
    const float dist0 = aabb_distance<N>(sc, o, d);
    const bool alive = valid && dist0 >= 0.0f;            // the lanes that test an item when the wave first meets it
    bool active = alive;
    float t_near = dist0, t_far = FLT_MAX;
    unsigned int bothbits = 0u;   // bit k: this lane entered BOTH sides of the branch pushed at stack level k
    for (int wd = lane; wd < seen_words; wd += 64) seen[wd] = 0u;
    int count = 0;
    float fr = 1.0f, fg = 1.0f, fb = 1.0f;
    const int tri_base = sc.n_batches;

    // ---- the Solids, every one of them in front of the walk: the trees of the reference's builder leave Solids out of cells they
    // reach (scene_dev, nt_api.cpp: its goldens show it), and the rule knows no tree.  They are few; the leaves' own are skipped.
    if (SCAL) {
        for (int idx = 0; idx < sc.n_solids; ++idx) {
            float t = 0.0f;
            int lane_out;
            if (alive) t = test_item<N>(sc, (idx << 2) | 2, o, d, FLT_MAX, -1, -1, lane_out);
            if (t != 0.0f) {
                ++count;
                if (!COUNTS) {
                    const float *tm = xr.trans + (size_t)sc.solid_mats[idx] * 3;
                    fr = fr * tm[0]; fg = fg * tm[1]; fb = fb * tm[2];
                }
            }
        }
    }

    int node = sc.root;      // wave-uniform
    int sp = 0;              // wave-uniform
    for (;;) {
        while (node >= 0) {
            if (__builtin_amdgcn_ballot_w64(active) == 0ull) { node = -1; break; }
            const NtNode nd = sc.nodes[node];                // uniform address -> scalar load
            if (nd.axis < 0) {
                // ---- leaf: every item the wave has not met yet, tested by every live lane
                for (int i = 0; i < nd.right; ++i) {
                    const int cur = __builtin_amdgcn_readfirstlane(sc.items[nd.left + i]);
                    const int kind = cur & 3, idx = cur >> 2;
                    if (kind > 1) continue;                  // (a Solid: counted in front of the walk)
                    if (!xray_first(seen, lane, kind == 0 ? idx : tri_base + idx)) continue;
                    if (SCAL && kind != 0) {
                        // an unbatched triangle: the per-lane test, on a record every lane reads from the same address
                        // (test_item: the scalar rule with the cutoff it is handed)
                        float t = 0.0f;
                        int lane_out;
                        if (alive) t = test_item<N>(sc, cur, o, d, FLT_MAX, -1, -1, lane_out);
                        const int mat = sc.tri_mats[idx];
                        if (t != 0.0f) {
                            ++count;
                            if (!COUNTS) {
                                const float *tm = xr.trans + (size_t)mat * 3;
                                fr = fr * tm[0]; fg = fg * tm[1]; fb = fb * tm[2];
                            }
                        }
                        continue;
                    }
                    if (!SCAL && kind != 0) continue;        // (a scene without such items has none in its leaves)
                    const float *base = sc.batch_recs + (size_t)idx * NT_DEV_BATCH * sc.rec_stride;
                    const unsigned int lv = xr.live[idx];    // uniform
                    // stage 1 for the 4 simplices at once, as composite_packet has it
                    float tl[NT_DEV_BATCH];
                    bool ok1[NT_DEV_BATCH];
#pragma unroll
                    for (int l = 0; l < NT_DEV_BATCH; ++l) {
                        const float *rec = base + (size_t)l * sc.rec_stride;
                        float denom = rec[1] * d[0];
#pragma unroll
                        for (int k = 1; k < N; ++k) denom = denom + rec[1 + k] * d[k];
                        float num;
                        if (numer) {
                            num = numer[(size_t)idx * NT_DEV_BATCH + l];
                        } else {
                            float no = rec[1] * o[0];
#pragma unroll
                            for (int k = 1; k < N; ++k) no = no + rec[1 + k] * o[k];
                            num = -(no + rec[0]);
                        }
                        tl[l] = num / denom;
                        ok1[l] = alive && ((lv >> l) & 1u) != 0u && denom != 0.0f && tl[l] >= 0.0f && tl[l] != 0.0f;
                    }
#pragma unroll
                    for (int l = 0; l < NT_DEV_BATCH; ++l) {
                        // stage 2 only where stage 1 leaves somebody
                        if (__builtin_amdgcn_ballot_w64(ok1[l]) == 0ull) continue;
                        const float t = tl[l];
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
                        if (ok) ++count;
                        if (!COUNTS) {
                            const float *tm = xr.trans + (size_t)sc.batch_mats[idx * NT_DEV_BATCH + l] * 3;     // uniform
                            const float a = tm[0], b = tm[1], c = tm[2];
                            fr = ok ? fr * a : fr; fg = ok ? fg * b : fg; fb = ok ? fb * c : fb;
                        }
                    }
                }
                node = -1;
                break;
            }
            // ---- branch: composite_packet's, with nothing to stop a lane but its interval
            const int axis = __builtin_amdgcn_readfirstlane(nd.axis);      // uniform
            float oa = o[0];                                   // the same in every lane (shared origin)
#pragma unroll
            for (int k = 1; k < N; ++k) oa = axis == k ? o[k] : oa;
            const float inv = pick_uniform<N>(invd, axis);
            const bool gt = __builtin_amdgcn_readfirstlane((int)(oa > nd.split)) != 0;
            const int n_near = gt ? nd.right : nd.left;
            const int n_far = gt ? nd.left : nd.right;
            bool go_near = false, go_far = false, both = false;
            float t = 0.0f;
            if (active) {
                if (inv == inv) {
                    if (oa == nd.split) {
                        if (inv > 0.0f) go_far = true; else go_near = true;
                    } else {
                        t = (nd.split - oa) * inv;
                        if (t < 0.0f || t > t_far) go_near = true;
                        else if (t < t_near) go_far = true;
                        else both = true;
                    }
                } else {
                    const bool to_right = oa >= nd.split;
                    if (to_right == gt) go_near = true; else go_far = true;       // near == right iff gt
                }
            }
            const bool near_lane = (go_near || both) && n_near >= 0;
            const bool far_after = (go_far || both) && n_far >= 0 && n_near >= 0;      // far AFTER a near subtree
            const unsigned long long m_near = __builtin_amdgcn_ballot_w64(near_lane);
            const unsigned long long m_far = __builtin_amdgcn_ballot_w64(far_after);
            if (m_near != 0ull) {
                if (m_far != 0ull && sp < DEPTH) {
                    if (lane == 0) {
                        ustack[sp * 8 + 0] = n_far;
                        ustack[sp * 8 + 1] = (int)(unsigned int)(m_far & 0xffffffffull);
                        ustack[sp * 8 + 2] = (int)(unsigned int)(m_far >> 32);
                        ustack[sp * 8 + 3] = __float_as_int(nd.split);
                        ustack[sp * 8 + 4] = axis;
                    }
                    bothbits = both ? (bothbits | (1u << sp)) : (bothbits & ~(1u << sp));
                    ++sp;
                }
                if (both && near_lane) t_far = t;
                active = near_lane;
                node = n_near;
            } else {
                const bool goes = (go_far || both) && n_far >= 0;
                if (both && goes) t_near = t;
                active = goes;
                node = __builtin_amdgcn_ballot_w64(goes) != 0ull ? n_far : -1;
            }
        }
        // ---- the frame returned: resume the innermost pending far side
        if (sp == 0) break;
        --sp;
        const int far = __builtin_amdgcn_readfirstlane(ustack[sp * 8 + 0]);
        if (tg.abort_word != nullptr && (far & NT_ABORT_POLL_MASK) == 0 && nt_aborted(tg)) return;
        const unsigned long long m = ((unsigned long long)(unsigned int)__builtin_amdgcn_readfirstlane(ustack[sp * 8 + 2]) << 32) |
                                     (unsigned int)__builtin_amdgcn_readfirstlane(ustack[sp * 8 + 1]);
        const bool was_both = ((bothbits >> sp) & 1u) != 0u;
        const bool join = ((m >> lane) & 1ull) != 0ull;
        if (__builtin_amdgcn_ballot_w64(join && was_both) != 0ull) {
            // the interval of the far side, recomputed from the level's (split, axis) as composite_packet recomputes it
            const float psplit = __int_as_float(__builtin_amdgcn_readfirstlane(ustack[sp * 8 + 3]));
            const int paxis = __builtin_amdgcn_readfirstlane(ustack[sp * 8 + 4]);
            float poa = o[0];
#pragma unroll
            for (int k = 1; k < N; ++k) poa = paxis == k ? o[k] : poa;
            const float et = (psplit - poa) * pick_uniform<N>(invd, paxis);
            const unsigned int below = bothbits & ((1u << sp) - 1u);
            float ef = FLT_MAX;
            if (below != 0u) {
                const int ks = 31 - __clz((int)below);
                const float s2 = __int_as_float(ustack[ks * 8 + 3]);
                const int a2 = ustack[ks * 8 + 4];
                ef = (s2 - pick_lane<N>(o, a2)) * pick_lane<N>(invd, a2);
            }
            if (join && was_both) { t_near = et; t_far = ef; }
        }
        active = join;
        node = far;
    }

    if (!valid) return;
    if (COUNTS) {
        xr.counts[((long long)frame * tg.height + y) * tg.width + x] = count;
        return;
    }
    const Color3 bgc = background_color<N>(sc, d);
    PixelRef pr;
    pr.x = x;
    pr.y = y;
    pr.offset = (long long)frame * tg.frame_stride + (long long)(tg.compact ? orow : y) * tg.pitch + (long long)x * tg.bpp;
    pr.hit_index = 0;
    pr.valid = true;
    emit_pixel(tg, pr, bgc.r * fr, bgc.g * fg, bgc.b * fb);
}

// tg: the whole image of every frame (row_begin 0, row_count = height, no bands), or with xr.counts the view alone.  Frames are
// chunked by what the numerator scratch holds (packet_chunk); the walk is set up by packet_args and packet_chunk_head of nt_composite.hpp.
template <int N>
int launch_xray_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtXray &xr) {
    const long long items = (long long)sc.n_batches + sc.n_triangles + sc.n_solids;
    // (never a bitset the launch cannot hold)
    if (!nt_xray_packet_route(li, sc) || items > NT_DEV_XRAY_PACKET_ITEMS || !xr.cams || (sc.n_batches > 0 && !xr.live) ||
        (!xr.counts && !xr.trans) || tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: an X-ray launch that is not for the packet walk");
        return -1;
    }
    hipStream_t s = (hipStream_t)li.stream;
    PacketArgs pk = packet_args(li, sc, tg.width, tg.height);
    pk.lds_per_wave = (int)xray_lds_per_wave(items);
    const int seen_words = (int)((items + 127) / 128) * 4;
    const size_t lds = (size_t)4 * pk.lds_per_wave;          // at most 4 * (1 + 8) KiB: under the 64 KiB a kernel gets unasked
    const bool scal = sc.has_scalar_prims || sc.n_solids > 0;      // (a Solid counts even where no leaf holds it)
    const int chunk = packet_chunk(li, li.nframes, false);
    const long long px = (long long)tg.width * tg.height;
    for (int f0 = 0; f0 < li.nframes; f0 += chunk) {
        const int cnt = packet_chunk_head<N>(li, sc, pk, xr.cams, f0, chunk, li.nframes);
        const NtTarget t2 = xr.counts ? tg : chunk_target(tg, f0);
        NtXray x2 = xr;
        if (xr.counts) x2.counts = xr.counts + (long long)f0 * px;
        const dim3 pgrid = packet_grid(pk, cnt);
        if (xr.counts) {
            if (scal) hipLaunchKernelGGL((xray_packet<N, 32, true, true>), pgrid, dim3(256), lds, s, sc, t2, pk, x2, seen_words);
            else hipLaunchKernelGGL((xray_packet<N, 32, false, true>), pgrid, dim3(256), lds, s, sc, t2, pk, x2, seen_words);
        } else {
            if (scal) hipLaunchKernelGGL((xray_packet<N, 32, true, false>), pgrid, dim3(256), lds, s, sc, t2, pk, x2, seen_words);
            else hipLaunchKernelGGL((xray_packet<N, 32, false, false>), pgrid, dim3(256), lds, s, sc, t2, pk, x2, seen_words);
        }
    }
    return 0;
}

}  // namespace
