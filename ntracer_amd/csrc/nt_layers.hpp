// nt_layers.hpp -- hit layers for compile-time N (nt_hit_layers): the K nearest crossings of every pixel's
// primary ray, in the order of (t, item, lane), with the pixel's full crossing count (ntracer_hip.h has the rule in full).
//
// layers_packet is xray_packet's walk (nt_xray.hpp) -- the 8 x 8 tile a wave, four independent waves a block, `ustack` and the
// exact "seen" bitset in dynamic LDS, the Solids in front of the walk, the live mask, packet_numerators when the launch has
// them, the abort poll -- written a second time: where xray_packet does ++count, each lane also inserts (t, id) into its own
// sorted list of KCAP keys.  The walk is a copy and not a shared template on purpose (DESIGN.md 4.18 says why): nt_xray.hpp stays
// as it is, and whoever changes the walk there changes it here.
// Instantiated per N by nt_inst_layers.hip; the run-time-n route, layers_var, is in nt_var.hip.
#pragma once
#include "nt_xray.hpp"
#include "nt_layer_list.hpp"

namespace {

// layer_sphere_t on the ray of a lane of the packet walk: out of line as solid_intersects is, with the ray where that call keeps it
template <int N>
__device__ __noinline__ float layer_sphere_fixed(const float *__restrict__ rec, const float (&o)[N], const float (&d)[N], float t32) {
    return layer_sphere_t(rec, N, t32, [&](int k) { return o[k]; }, [&](int k) { return d[k]; });
}

// SCAL: the scene has unbatched triangles or Solids.  KCAP: the list's length, the smallest of 2, 4, 8 that holds ly.layers.
// Four waves a SIMD as xray_packet: no instantiation spills its list under the 128 VGPRs of that bound (DESIGN.md 4.18 has the table).
template <int N, int DEPTH, bool SCAL, int KCAP>
__global__ __launch_bounds__(256, 4) void layers_packet(NtCompositeDev sc, NtTarget tg, PacketArgs pa, NtLayers ly, int seen_words) {
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
    LayerList<KCAP> ls;
    ls.clear();
    const int tri_base = sc.n_batches;

    // ---- the Solids, every one of them in front of the walk, as xray_packet has them
    if (SCAL) {
        for (int idx = 0; idx < sc.n_solids; ++idx) {
            float t = 0.0f;
            int lane_out;
            if (alive) t = test_item<N>(sc, (idx << 2) | 2, o, d, FLT_MAX, -1, -1, lane_out);
            const bool ok = t != 0.0f;
            if (ok) ++count;
            // (a sphere's distance once more in float64: layer_sphere_t says why)
            if (sc.solid_types[idx] != 1 && ok) t = layer_sphere_fixed<N>(sc.solid_recs + (size_t)idx * (2 * N * N + N), o, d, t);
            if (__builtin_amdgcn_ballot_w64(ok) != 0ull) ls.insert(layer_key(ok, t, (idx << 2) | 2, -1));
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
                    if (kind > 1) continue;                  // (a Solid: listed in front of the walk)
                    if (!xray_first(seen, lane, kind == 0 ? idx : tri_base + idx)) continue;
                    if (SCAL && kind != 0) {
                        // an unbatched triangle: the per-lane test, on a record every lane reads from the same address
                        float t = 0.0f;
                        int lane_out;
                        if (alive) t = test_item<N>(sc, cur, o, d, FLT_MAX, -1, -1, lane_out);
                        const bool ok = t != 0.0f;
                        if (ok) ++count;
                        if (__builtin_amdgcn_ballot_w64(ok) != 0ull) ls.insert(layer_key(ok, t, cur, -1));
                        continue;
                    }
                    if (!SCAL && kind != 0) continue;        // (a scene without such items has none in its leaves)
                    const float *base = sc.batch_recs + (size_t)idx * NT_DEV_BATCH * sc.rec_stride;
                    const unsigned int lv = ly.live[idx];    // uniform
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
                        // the insertion only where some lane of the wave accepted
                        if (__builtin_amdgcn_ballot_w64(ok) != 0ull) ls.insert(layer_key(ok, t, cur, l));
                    }
                }
                node = -1;
                break;
            }
            // ---- branch: xray_packet's, with nothing to stop a lane but its interval
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
    const long long px = (long long)tg.width * tg.height;
    layers_store<KCAP>(ly.records, (long long)y * tg.width + x, px, ly.layers, ls, count);
}

template <int N, bool SCAL, int KCAP>
void launch_layers_kernel(dim3 grid, size_t lds, hipStream_t s, const NtCompositeDev &sc, const NtTarget &tg, const PacketArgs &pk, const NtLayers &ly,
                          int seen_words) {
    hipLaunchKernelGGL((layers_packet<N, 32, SCAL, KCAP>), grid, dim3(256), lds, s, sc, tg, pk, ly, seen_words);
}

// tg: the view (row_begin 0, row_count = height, no bands); one frame.  The walk is set up by packet_args and packet_chunk_head of
// nt_composite.hpp, as launch_xray_fixed sets it up.
template <int N>
int launch_layers_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtLayers &ly) {
    const long long items = (long long)sc.n_batches + sc.n_triangles + sc.n_solids;
    // (never a bitset the launch cannot hold, never a key that does not hold the item)
    if (!nt_xray_packet_route(li, sc) || items > NT_DEV_XRAY_PACKET_ITEMS || !ly.cams || (sc.n_batches > 0 && !ly.live) || !ly.records ||
        ly.layers < 1 || ly.layers > NT_DEV_LAYERS_MAX || li.nframes != 1 || tg.row_begin != 0 || tg.row_count != tg.height || tg.band_world > 1) {
        snprintf(nt_launch_error_buf(), NT_LAUNCH_ERROR_LEN, "internal: a hit-layer launch that is not for the packet walk");
        return -1;
    }
    hipStream_t s = (hipStream_t)li.stream;
    PacketArgs pk = packet_args(li, sc, tg.width, tg.height);
    pk.lds_per_wave = (int)xray_lds_per_wave(items);
    const int seen_words = (int)((items + 127) / 128) * 4;
    const size_t lds = (size_t)4 * pk.lds_per_wave;          // at most 4 * (1 + 8) KiB: under the 64 KiB a kernel gets unasked
    const bool scal = sc.has_scalar_prims || sc.n_solids > 0;      // (a Solid counts even where no leaf holds it)
    const int cnt = packet_chunk_head<N>(li, sc, pk, ly.cams, 0, 1, 1);
    const dim3 pgrid = packet_grid(pk, cnt);
    const int kcap = ly.layers <= 2 ? 2 : ly.layers <= 4 ? 4 : 8;
    if (scal) {
        if (kcap == 2) launch_layers_kernel<N, true, 2>(pgrid, lds, s, sc, tg, pk, ly, seen_words);
        else if (kcap == 4) launch_layers_kernel<N, true, 4>(pgrid, lds, s, sc, tg, pk, ly, seen_words);
        else launch_layers_kernel<N, true, 8>(pgrid, lds, s, sc, tg, pk, ly, seen_words);
    } else {
        if (kcap == 2) launch_layers_kernel<N, false, 2>(pgrid, lds, s, sc, tg, pk, ly, seen_words);
        else if (kcap == 4) launch_layers_kernel<N, false, 4>(pgrid, lds, s, sc, tg, pk, ly, seen_words);
        else launch_layers_kernel<N, false, 8>(pgrid, lds, s, sc, tg, pk, ly, seen_words);
    }
    return 0;
}

}  // namespace
