// nt_api.cpp -- host side of libntracer_hip.so: the C ABI declared in include/ntracer_hip.h.
//
// Mirrors, for the ray-cast path only, what the reference does in C++ above its scenes:
//   ImageFormat/Channel validation      src/render.cpp:120-164, 187-209, 249-288
//   renderer frame loop and protocol    src/render.cpp:853-923 (busy / lock / abort)
//   box_scene / composite_scene state   src/tracer.hpp:83-123, 1710-1748
// The per-pixel work itself is in nt_box.hpp / nt_composite.hpp / nt_var.hip.  There is NO CPU fallback: without a HIP
// device every render entry point fails with NT_E_DEVICE.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ntracer_hip.h"
#include "nt_device.hpp"
#include "nt_box_span.hpp"

namespace {

thread_local std::string g_error;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(e_ == hipErrorOutOfMemory ? NT_E_NOMEM : NT_E_DEVICE, \
                                          "%s failed: %s", #expr, hipGetErrorString(e_));       \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap && p) return 0;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = std::max<size_t>(bytes, 256);
        HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct ChanTable {
    std::vector<NtChanDev> host;
    NtChanDev *dev = nullptr;
};

// NtTarget::rowtab: what the BoxScene tile kernel needs to know about a row, per owned row of one (view, band split, pitch) --
// or, with interleaved rows (NtTarget::row_il), per slot of one launch geometry
struct RowTable {
    int height = 0, pitch = 0, rank = 0, world = 1, rows = 0, compact = 0;
    int il = 0, il_rows = 0, il_count = 0;   // interleave stride (waves per column strip), rows a wave, rows of the launch
    uint32_t half_h = 0, fovI = 0;       // float bits
    void *dev = nullptr;
};

// everything a scene keeps on one HIP device
struct DeviceState {
    int device = -1;
    hipStream_t stream = nullptr;        // used by the host-buffer entry points
    // The per-device scratch of a scene (camera table, BoxScene's redo bitmap, hit records ...) is shared by its launches, which
    // are ordered by their stream.  A call that arrives on another stream than the one before first waits (on the host) for
    // that stream to drain: see use_stream
    hipStream_t last_stream = nullptr;
    bool have_last_stream = false;
    // nt_render's abort: a dword in device memory (NtTarget::abort_word: read past the caches by every block that starts, a
    // microsecond from HBM -- from mapped host memory the same read made a 120-cell frame four times as long) that the host
    // raises, by a 4-byte copy on a stream of its own, when the caller's flag goes up; and the event the host waits on
    DevBuf abort_word;
    int *abort_one = nullptr;            // pinned source of that copy: the value 1
    hipStream_t side_stream = nullptr;
    hipEvent_t frame_done = nullptr;
    bool scene_uploaded = false;
    DevBuf nodes, items, batch_recs, batch_mats, tri_recs, tri_mats, solid_recs, solid_types, solid_mats, materials, aabb;
    DevBuf lights;                       // pl_pos | pl_color | gl_dir | gl_color
    unsigned long long lights_version = 0;
    DevBuf framebuffer, cams, probes, stats, counter;
    DevBuf hits;                         // primary-hit records between the two passes of a lit render
    DevBuf stats_frame;                  // where the statistics launch of a "faithful" scene draws (discarded)
    DevBuf samples;                      // supersampling: the fp32 x 3 samples between the render and the resolve kernel; adaptive
                                         // supersampling: the base frame, the list of flagged pixels and the host forms' mask;
                                         // ambient occlusion: the hit records, both normal rows, the base frame and the counts
                                         // of a chunk of frames, and on the ray route the ray arrays and answers of a chunk of rows;
                                         // outlines: the hit records of a chunk of frames and, off the packet walk, their normal
                                         // rows, base frame and mask bytes; depth cues: the hit records of a chunk of frames and,
                                         // off the packet walk, their base frame, and the host form's factors
    DevBuf refine_count;                 // adaptive supersampling: the length of that list
    DevBuf ao_dirs;                      // ambient occlusion: the table of directions
    unsigned long long ao_version = 0;
    DevBuf clip;                         // clip planes: [count][n + 1] floats, a plane's normal and then its offset
    unsigned long long clip_version = 0;
    DevBuf live;                         // X-ray views: the live masks, a byte a batch
    DevBuf xr_table;                     // ... and the transmittances [n_materials][3]
    unsigned long long xr_version = 0;
    DevBuf stack_offsets;                // view stack: the table of offsets
    unsigned long long stack_version = 0;
    DevBuf stack_in;                     // ... the scene's own camera for stack_cameras: its four rows, then all its axes
    DevBuf stack_cams;                   // ... the sample cameras of a launch's frames and their dot products (NtStack)
    DevBuf numer;                        // packet kernel: -(N.o + d) per (frame, simplex)
    DevBuf cull;                         // BoxScene: row culling bits
    bool cull_clean = false;             // `cull` is all zero (what the fused BoxScene path needs and leaves behind)
    DevBuf checked;                      // reference-faithful normals: the exact `checked` bitmap, one column per resident lane
    DevBuf ties;                         // BoxScene: tie sets of the marked stretches (fused path)
    DevBuf tframes;                      // run-time-n transparency kernel: the ray_color frame stacks, one column per resident lane
    DevBuf lens_dirs;                    // renders through a lens on the ray route: the directions of a band of rows; under the
                                         // parallel projection the band's origins and directions
    // camera tables travel through pinned host memory (a pageable source makes hipMemcpyAsync wait for the copy on the
    // host, which stalls the launch pipeline of back-to-back calls): a ring of slots, each guarded by an event
    struct Stage { void *host = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool in_flight = false; };
    Stage stage[8];
    unsigned stage_next = 0;
    struct TileOrder { int tx = 0, ty = 0; DevBuf buf; };
    std::vector<std::unique_ptr<TileOrder>> tile_orders;   // packet kernel: tiles sorted centre-out, per tile grid
    int cu_count = 0;
    std::vector<std::unique_ptr<ChanTable>> chan_tables;
    std::vector<std::unique_ptr<RowTable>> row_tables;
};

struct Format {                          // validated image_format (render.cpp:167-172)
    int width = 0, height = 0, pitch = 0, bpp = 0, reversed = 0;
    int pack_mode = NT_PACK_GENERIC;
    // "plain RGB" layouts (every live channel is exactly one of r, g, b, same bit size, one 32-bit word): the three
    // multipliers place a quantised component into all the fields that carry it; 0 bits = not such a layout
    uint32_t plain_bits = 0, plain_maxval = 0, plain_mul[3] = {0, 0, 0};
    // three fp32 channels, each exactly one of r, g, b (12-byte pixels): component of float k, or -1 if not this layout
    int plain_f32[3] = {-1, -1, -1};
    std::vector<NtChanDev> chans;        // live channels only (all-zero channels contribute no bits)
};

}  // namespace

// A lens (ntracer_hip.h): the coefficient table, and its copy on every device that has rendered through it.  Shared by the
// handles (nt_lens) and the scenes it is set on; the last owner frees the device copies.
struct NtLensData {
    int width = 0, height = 0;
    long long masked = 0;                // entries that cast no ray
    std::vector<float> coeffs;           // [height][width][3]
    std::mutex mu;
    std::map<int, void *> dev;           // device -> the table there
    ~NtLensData() {
        for (auto &kv : dev) {
            if (hipSetDevice(kv.first) != hipSuccess) continue;
            (void)hipDeviceSynchronize();          // launches that read the table may still be queued
            (void)hipFree(kv.second);
        }
    }
};

struct nt_lens {
    std::shared_ptr<NtLensData> d;
};

struct nt_scene {
    bool composite = false;
    int n = 0;
    std::mutex mu;
    int locked = 0;
    bool busy = false;
    float fov = 0.8f;                    // tracer.hpp:91,1731
    int supersampling = 1;               // s x s samples a pixel (nt_scene_set_supersampling; the reference has none)
    int ss_scratch_mb = 1024;            // ... and the cap of their scratch buffer, MiB per device (nt_scene_set_supersampling_scratch_mb)
    bool adaptive = false;               // with supersampling > 1: only pixels whose contrast exceeds adaptive_t get the s x s samples
    float adaptive_t = 0.0f;             // (nt_scene_set_adaptive_supersampling)
    std::vector<float> origin, axes;     // camera<Store>: origin[n], t_orientation[n][n] (camera.hpp:7-15)
    std::shared_ptr<NtLensData> lens;    // not null: the renders' ray source (nt_scene_set_lens); fov is then ignored
    float parallel = 0.0f;               // > 0: the parallel projection's half_width (nt_scene_set_parallel); excludes a lens
    int ao_count = 0;                    // > 0: ambient occlusion with that many samples a pixel (nt_scene_set_ambient_occlusion)
    std::vector<float> ao_dirs;          // ... their directions [ao_count][n], used as given
    float ao_radius = 0.0f, ao_bias = 0.0f, ao_strength = 0.0f;
    unsigned long long ao_version = 1;   // counts the changes of ao_dirs
    bool outlines = false;               // silhouette, crease and depth lines on the renders (nt_scene_set_outlines)
    float ol_crease_cos = 0.0f, ol_depth_gap = 0.0f, ol_color[3] = {0, 0, 0}, ol_strength = 0.0f;
    bool cue = false, cue_tint = false;  // distance fog and a coordinate tint on the renders (nt_scene_set_depth_cue)
    nt_depth_cue cue_set{};              // ... as the caller gave it, the tint's fields zero without a tint,
    std::vector<float> cue_axis;         // ... the tint axis [n], empty without a tint,
    float cue_inv_fog = 0.0f, cue_inv_tint = 0.0f;   // ... and the two reciprocals of the rule, formed once
    int clip_count = 0;                  // clip planes that every ray of a render honours (nt_scene_set_clip_planes), 0: off
    std::vector<float> clip_planes;      // ... [clip_count][n + 1]: a plane's normal and then its offset, as the kernels read them
    unsigned long long clip_version = 1; // counts the changes of clip_planes
    int box_lines = 0;                   // BoxScene: != 0, the kinds of face lines on the renders (nt_scene_set_box_lines)
    float bl_color[3] = {0, 0, 0}, bl_strength = 0.0f;
    bool box_shading = false;            // BoxScene: face colours, fog and a tint on the renders (nt_scene_set_box_shading)
    bool bs_colors = false, bs_cue = false, bs_tint = false;   // ... which of its three parts the caller gave,
    std::vector<float> bs_table;         // ... the face colours [n][2][3], empty without a table of the caller's own,
    nt_depth_cue bs_set{};               // ... the cue as the caller gave it, the tint's fields zero without a tint,
    std::vector<float> bs_axis;          // ... the tint axis [n], empty without a tint,
    float bs_inv_fog = 0.0f, bs_inv_tint = 0.0f;     // ... and the two reciprocals of the rule, formed once
    int stack_count = 0;                 // > 0: a view stack of that many sample cameras on the renders (nt_scene_set_view_stack)
    std::vector<float> stack_offsets;    // ... their offsets [stack_count][n] in the camera's own frame,
    std::vector<float> stack_weights;    // ... their weights [stack_count][3],
    float stack_focus = 0.0f, stack_r = 0.0f;        // ... the focus (0: none) and r = 1.0f / focus, formed once (0 without a focus)
    unsigned long long stack_version = 1;            // counts the changes of stack_offsets
    int stack_route = NT_STACK_ROUTE_AUTO;           // NT_STACK_ROUTE_FRAMES: BoxScene's stacks through the frames route too (nt_scene_set_view_stack_route)
    bool xray = false;                   // the renders draw the X-ray colour instead of the shaded one (nt_scene_set_xray)
    float xr_absorbance = 0.0f, xr_tint = 0.0f;
    std::vector<float> xr_table;         // ... the transmittances T [n_materials][3], formed by the setter
    unsigned long long xr_version = 1;   // counts the changes of xr_table
    std::vector<uint8_t> live_masks;     // the X-ray rule's live mask of every batch, formed when the scene is made

    // composite_scene (tracer.hpp:1713-1740)
    int root = -1;
    int depth = 0;
    std::vector<NtNode> nodes;
    std::vector<int32_t> items;
    int rec_len = 0, rec_stride = 0;
    std::vector<float> batch_recs, tri_recs, solid_recs, materials, aabb;
    std::vector<int32_t> batch_mats, tri_mats, solid_types, solid_mats;
    int n_batches = 0, n_triangles = 0, n_solids = 0, n_materials = 0;
    bool all_opaque = true, any_reflective = false, has_scalar = false;
    int shadows = 0, camera_light = 1, max_reflect_depth = 4, bg_axis = 1;
    float ambient[3] = {0, 0, 0}, bg1[3] = {1, 1, 1}, bg2[3] = {0, 0, 0}, bg3[3] = {0, 1, 1};
    std::vector<float> pl_pos, pl_color, gl_dir, gl_color;
    unsigned long long lights_version = 1;

    std::map<int, std::unique_ptr<DeviceState>> devs;
    nt_stats last_stats{};
    bool have_stats = false;
    int stats_device = -1;
};

namespace {

// ---------------------------------------------------------------------------------------------
// formats: Channel.__new__ (render.cpp:120-164), im_set_channels (:192-209), ImageFormat.__new__
// (:249-288), im_check_buffer_size (:187-190)
// ---------------------------------------------------------------------------------------------
int parse_format(const nt_image_format *f, Format &out) {
    if (!f) return fail(NT_E_INVALID, "format is NULL");
    if (f->nchannels < 0 || (f->nchannels > 0 && !f->channels)) return fail(NT_E_INVALID, "invalid channel list");
    long bits = 0;
    out.chans.clear();
    for (int i = 0; i < f->nchannels; ++i) {
        const nt_channel &c = f->channels[i];
        if (c.tfloat) {
            if (c.bit_size != 32) return fail(NT_E_INVALID, "if \"tfloat\" is true, \"bit_size\" can only be 32");
        } else {
            if (c.bit_size > NT_MAX_BITSIZE) return fail(NT_E_INVALID, "\"bit_size\" cannot be greater than %d (unless \"tfloat\" is true)", NT_MAX_BITSIZE);
            if (c.bit_size < 1) return fail(NT_E_INVALID, "\"bit_size\" cannot be less than 1");
        }
        NtChanDev d;
        d.f_r = c.f_r; d.f_g = c.f_g; d.f_b = c.f_b; d.f_c = c.f_c;
        d.bits = c.bit_size;
        d.tfloat = c.tfloat ? 1u : 0u;
        d.offset = (uint32_t)bits;
        d.maxval = c.tfloat ? 0u : (0xffffffffu >> (32 - c.bit_size));
        bits += c.bit_size;
        // clamp((0*g + 0*b) + (0*r + 0)) is 0 for every colour (NaN included): such a channel (the X of
        // RGBX8, padding) writes no bits, so it is dropped from the device table
        const bool dead = c.f_r == 0.0f && c.f_g == 0.0f && c.f_b == 0.0f && c.f_c == 0.0f;
        if (!dead) out.chans.push_back(d);
    }
    if (bits > NT_MAX_PIXELSIZE * 8) return fail(NT_E_INVALID, "Too many bytes per pixel. The maximum is %d.", NT_MAX_PIXELSIZE);
    out.bpp = (int)((bits + 7) / 8);
    out.pack_mode = NT_PACK_GENERIC;
    if (out.chans.size() <= 4 && bits <= 32) out.pack_mode = NT_PACK_WORD32;
    else if (out.chans.size() <= 4 && bits <= 64) out.pack_mode = NT_PACK_WORD64;
    if (out.chans.size() == 3 && bits == 96) {
        int comp[3] = {-1, -1, -1};
        bool ok = true;
        for (int k = 0; k < 3 && ok; ++k) {
            const NtChanDev &d = out.chans[k];
            const float f[3] = {d.f_r, d.f_g, d.f_b};
            int ones = 0, zeros = 0;
            for (int c = 0; c < 3; ++c) {
                if (f[c] == 1.0f) { comp[k] = c; ++ones; }
                else if (f[c] == 0.0f && !std::signbit(f[c])) ++zeros;
            }
            ok = ones == 1 && zeros == 2 && d.f_c == 0.0f && !std::signbit(d.f_c) && d.tfloat && d.offset == (uint32_t)(32 * k);
        }
        if (ok) for (int k = 0; k < 3; ++k) out.plain_f32[k] = comp[k];
    }
    if (out.pack_mode == NT_PACK_WORD32 && !out.chans.empty()) {
        bool plain = true;
        uint32_t mul[3] = {0, 0, 0};
        for (const NtChanDev &d : out.chans) {
            const float f[3] = {d.f_r, d.f_g, d.f_b};
            int comp = -1, ones = 0, zeros = 0;
            for (int k = 0; k < 3; ++k) {
                if (f[k] == 1.0f) { comp = k; ++ones; }
                else if (f[k] == 0.0f && !std::signbit(f[k])) ++zeros;
            }
            if (ones != 1 || zeros != 2 || d.f_c != 0.0f || std::signbit(d.f_c) || d.tfloat || d.bits != out.chans[0].bits) { plain = false; break; }
            mul[comp] |= 1u << (32u - d.offset - d.bits);
        }
        if (plain) {
            out.plain_bits = out.chans[0].bits;
            out.plain_maxval = out.chans[0].maxval;
            for (int k = 0; k < 3; ++k) out.plain_mul[k] = mul[k];
        }
    }
    if (f->width < 1 || f->height < 1) return fail(NT_E_INVALID, "width and height must be at least 1");
    if (f->pitch < 0) return fail(NT_E_INVALID, "pitch cannot be negative");
    out.width = f->width;
    out.height = f->height;
    out.reversed = f->reversed ? 1 : 0;
    if (f->pitch) {
        if (f->pitch < f->width * out.bpp) return fail(NT_E_INVALID, "\"pitch\" must be at least \"width\" times the size of one pixel in bytes");
        out.pitch = f->pitch;
    } else {
        out.pitch = f->width * out.bpp;
    }
    return NT_OK;
}

struct Bands {
    int rank = 0, world = 1, rows = NT_RENDER_CHUNK_SIZE, compact = 0;
    int owned_rows = 0;
};

int parse_bands(const nt_render_opts *o, int height, Bands &b) {
    if (o) {
        b.world = o->band_world > 1 ? o->band_world : 1;
        b.rank = b.world > 1 ? o->band_rank : 0;
        b.rows = o->band_rows > 0 ? o->band_rows : NT_RENDER_CHUNK_SIZE;
        b.compact = o->compact ? 1 : 0;
        if (b.rank < 0 || b.rank >= b.world) return fail(NT_E_INVALID, "band_rank %d out of range for band_world %d", o->band_rank, b.world);
    }
    if (b.world == 1) {
        b.owned_rows = height;
    } else {
        // rows of bands rank, rank+world, ... clipped to the image
        int owned = 0;
        const int nbands = (height + b.rows - 1) / b.rows;
        for (int band = b.rank; band < nbands; band += b.world) owned += std::min(b.rows, height - band * b.rows);
        b.owned_rows = owned;
    }
    return NT_OK;
}

size_t required_len(const Format &f, const Bands &b) {
    return (size_t)f.pitch * (size_t)(b.compact ? b.owned_rows : f.height);
}

// ---------------------------------------------------------------------------------------------
// devices
// ---------------------------------------------------------------------------------------------
int pick_device(const nt_render_opts *o, int explicit_dev, int &dev) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count < 1)
        return fail(NT_E_DEVICE, "no HIP device available (%s): the ray-cast path has no CPU fallback", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    dev = explicit_dev;
    if (o && o->device >= 0) dev = o->device;
    if (dev < 0) {
        HIP_TRY(hipGetDevice(&dev));
    }
    if (dev >= count) return fail(NT_E_INVALID, "device %d does not exist (%d devices)", dev, count);
    HIP_TRY(hipSetDevice(dev));
    return NT_OK;
}

int device_state(nt_scene *s, int dev, DeviceState *&out) {
    auto it = s->devs.find(dev);
    if (it == s->devs.end()) {
        auto ds = std::make_unique<DeviceState>();
        ds->device = dev;
        HIP_TRY(hipDeviceGetAttribute(&ds->cu_count, hipDeviceAttributeMultiprocessorCount, dev));
        it = s->devs.emplace(dev, std::move(ds)).first;
    }
    out = it->second.get();
    return NT_OK;
}

// The stream of the entry points that take none (nt_render, nt_colors_at), made when one of them first needs it: a scene that
// is only ever drawn through the device entry points -- on the caller's streams -- creates no stream of its own.  (The device
// has a handful of hardware queues and the runtime deals its streams out over them; streams nobody uses still take their turn,
// and two of the caller's streams that end up on one queue no longer overlap: a process that had made a dozen scenes lost the
// overlap of alternating calls, 48 -> 88 us a step.)
int own_stream(DeviceState *ds) {
    if (!ds->stream) HIP_TRY(hipStreamCreateWithFlags(&ds->stream, hipStreamNonBlocking));
    return NT_OK;
}

// launches of one scene on one device are ordered by their stream; when the stream changes, the old one is drained first
int use_stream(DeviceState *ds, hipStream_t st) {
    if (ds->have_last_stream && ds->last_stream != st) HIP_TRY(hipStreamSynchronize(ds->last_stream));
    ds->last_stream = st;
    ds->have_last_stream = true;
    return NT_OK;
}

// a pinned slot of at least `bytes`, free to be overwritten (its previous copy has left the host)
int stage_slot(DeviceState *ds, size_t bytes, DeviceState::Stage *&out) {
    DeviceState::Stage &st = ds->stage[ds->stage_next++ % 8];
    if (st.in_flight) {
        HIP_TRY(hipEventSynchronize(st.done));
        st.in_flight = false;
    }
    if (st.cap < bytes) {
        if (st.host) { (void)hipHostFree(st.host); st.host = nullptr; st.cap = 0; }
        const size_t want = std::max<size_t>(bytes, 4096);
        HIP_TRY(hipHostMalloc(&st.host, want, hipHostMallocDefault));
        st.cap = want;
    }
    if (!st.done) HIP_TRY(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    out = &st;
    return NT_OK;
}

template <typename T>
int upload(DevBuf &b, const std::vector<T> &v) {
    if (int r = b.ensure(std::max<size_t>(v.size() * sizeof(T), 16))) return r;
    if (!v.empty()) HIP_TRY(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return NT_OK;
}

int upload_scene(nt_scene *s, DeviceState *ds) {
    if (s->stack_count > 0 && ds->stack_version != s->stack_version) {
        // (a fresh allocation, as for the lights below)
        DevBuf fresh;
        if (int r = upload(fresh, s->stack_offsets)) return r;
        if (ds->stack_offsets.p) { (void)hipDeviceSynchronize(); ds->stack_offsets.release(); }
        ds->stack_offsets = fresh;
        ds->stack_version = s->stack_version;
    }
    if (!s->composite) return NT_OK;
    if (!ds->scene_uploaded) {
        if (int r = upload(ds->nodes, s->nodes)) return r;
        if (int r = upload(ds->items, s->items)) return r;
        if (int r = upload(ds->batch_recs, s->batch_recs)) return r;
        if (int r = upload(ds->batch_mats, s->batch_mats)) return r;
        if (int r = upload(ds->tri_recs, s->tri_recs)) return r;
        if (int r = upload(ds->tri_mats, s->tri_mats)) return r;
        if (int r = upload(ds->solid_recs, s->solid_recs)) return r;
        if (int r = upload(ds->solid_types, s->solid_types)) return r;
        if (int r = upload(ds->solid_mats, s->solid_mats)) return r;
        if (int r = upload(ds->materials, s->materials)) return r;
        if (int r = upload(ds->aabb, s->aabb)) return r;
        if (int r = upload(ds->live, s->live_masks)) return r;
        ds->scene_uploaded = true;
    }
    if (s->xray && ds->xr_version != s->xr_version) {
        // (a fresh allocation, as for the lights below)
        DevBuf fresh;
        if (int r = upload(fresh, s->xr_table)) return r;
        if (ds->xr_table.p) { (void)hipDeviceSynchronize(); ds->xr_table.release(); }
        ds->xr_table = fresh;
        ds->xr_version = s->xr_version;
    }
    if (ds->lights_version != s->lights_version) {
        std::vector<float> all;
        all.insert(all.end(), s->pl_pos.begin(), s->pl_pos.end());
        all.insert(all.end(), s->pl_color.begin(), s->pl_color.end());
        all.insert(all.end(), s->gl_dir.begin(), s->gl_dir.end());
        all.insert(all.end(), s->gl_color.begin(), s->gl_color.end());
        // a fresh allocation: launches already enqueued keep reading the old one
        DevBuf fresh;
        if (int r = upload(fresh, all)) return r;
        // the previous buffer may still be in use by enqueued work: free it only after the device drains
        if (ds->lights.p) { (void)hipDeviceSynchronize(); ds->lights.release(); }
        ds->lights = fresh;
        ds->lights_version = s->lights_version;
    }
    if (s->ao_count > 0 && ds->ao_version != s->ao_version) {
        // (a fresh allocation, as for the lights)
        DevBuf fresh;
        if (int r = upload(fresh, s->ao_dirs)) return r;
        if (ds->ao_dirs.p) { (void)hipDeviceSynchronize(); ds->ao_dirs.release(); }
        ds->ao_dirs = fresh;
        ds->ao_version = s->ao_version;
    }
    if (s->clip_count > 0 && ds->clip_version != s->clip_version) {
        // (a fresh allocation, as for the lights)
        DevBuf fresh;
        if (int r = upload(fresh, s->clip_planes)) return r;
        if (ds->clip.p) { (void)hipDeviceSynchronize(); ds->clip.release(); }
        ds->clip = fresh;
        ds->clip_version = s->clip_version;
    }
    return NT_OK;
}

// The first device calls of every entry point: the device -- of the options, else `explicit_dev`, else the current one --, the
// scene's state on it (ds->device says which it is) and the scene in its memory.  `table_device` >= 0: the call's camera table
// lives there, and any other device is refused before it is touched; `table_user` is what the message says the device is for.
int scene_on_device(nt_scene *s, const nt_render_opts *opts, int explicit_dev, DeviceState *&ds, int table_device = -1,
                    const char *table_user = nullptr) {
    int dev;
    if (int r = pick_device(opts, explicit_dev, dev)) return r;
    if (table_device >= 0 && dev != table_device)
        return fail(NT_E_INVALID, "the camera table lives on device %d, the %s is for device %d", table_device, table_user, dev);
    if (int r = device_state(s, dev, ds)) return r;
    return upload_scene(s, ds);
}

// ... and of the host forms, which bring no stream: the scene's own
int use_own_stream(DeviceState *ds) {
    if (int r = own_stream(ds)) return r;
    return use_stream(ds, ds->stream);
}

// The device forms outside the renders take three fields of their options.  `reader` is the subject and verb of the refusal, and
// `whose` its pronoun.
int only_device_strict_abort(const nt_render_opts *opts, const char *reader, const char *whose = "its") {
    if (opts && (opts->band_rank || opts->band_world || opts->band_rows || opts->compact || opts->collect_stats || opts->overlapped))
        return fail(NT_E_INVALID, "%s device, strict_reference and abort_device of %s options: every other field must be 0", reader, whose);
    return NT_OK;
}

int chan_table(DeviceState *ds, const Format &f, const NtChanDev *&dev_ptr) {
    for (auto &t : ds->chan_tables) {
        if (t->host.size() == f.chans.size() &&
            (f.chans.empty() || std::memcmp(t->host.data(), f.chans.data(), f.chans.size() * sizeof(NtChanDev)) == 0)) {
            dev_ptr = t->dev;
            return NT_OK;
        }
    }
    auto t = std::make_unique<ChanTable>();
    t->host = f.chans;
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, std::max<size_t>(f.chans.size() * sizeof(NtChanDev), 16)));
    t->dev = (NtChanDev *)p;
    if (!f.chans.empty()) HIP_TRY(hipMemcpy(p, f.chans.data(), f.chans.size() * sizeof(NtChanDev), hipMemcpyHostToDevice));
    dev_ptr = t->dev;
    ds->chan_tables.push_back(std::move(t));
    return NT_OK;
}

// The row table of a launch geometry (cached: a render loop keeps its view, band split and pitch).  Entry i belongs to owned
// row i: sy exactly as the ray source computes it (tracer.hpp:72-74: fovI * (y - half_h), two fp32 operations), whether
// the row exists, and where it starts in a frame; 64 entries of padding, as a wave reads its sixteen rows unclamped.
// Interleaved rows (tg.row_il = W > 0, il_rows = rows a wave): entry w * il_rows + rr belongs to row w + W * rr of the launch.
int row_table(DeviceState *ds, const NtTarget &tg, int il_rows, const void *&dev_ptr) {
    uint32_t hh, fi;
    std::memcpy(&hh, &tg.half_h, 4);
    std::memcpy(&fi, &tg.fovI, 4);
    const int world = std::max(tg.band_world, 1);
    const int il = tg.row_il;
    for (auto &t : ds->row_tables) {
        if (t->height == tg.height && t->pitch == tg.pitch && t->rank == tg.band_rank && t->world == world && t->rows == tg.band_rows &&
            t->compact == tg.compact && t->half_h == hh && t->fovI == fi && t->il == il &&
            (il == 0 || (t->il_rows == il_rows && t->il_count == tg.row_count))) {
            dev_ptr = t->dev;
            return NT_OK;
        }
    }
    struct Entry { float sy; uint32_t valid; long long off; };
    static_assert(sizeof(Entry) == 16, "16-byte row entries");
    std::vector<Entry> host;
    const int rows = std::max(tg.band_rows, 1);
    auto entry_of = [&](int orow, Entry &e) {            // false: no such band
        const int band = orow / rows;
        const int y = world > 1 ? (band * world + tg.band_rank) * rows + (orow - band * rows) : orow;
        if ((world > 1 ? (band * world + tg.band_rank) * rows : orow) >= tg.height) return false;
        e.sy = tg.fovI * ((float)y - tg.half_h);
        e.valid = y < tg.height ? 1u : 0u;
        e.off = (long long)(tg.compact ? orow : y) * tg.pitch;
        return true;
    };
    if (il > 0) {
        for (int w = 0; w < il; ++w)
            for (int rr = 0; rr < il_rows; ++rr) {
                Entry e{0.0f, 0u, 0};
                const int row = w + il * rr;
                if (row >= tg.row_count || !entry_of(tg.row_begin + row, e)) e = Entry{0.0f, 0u, 0};
                host.push_back(e);
            }
    } else {
        for (int orow = 0;; ++orow) {
            Entry e;
            if (!entry_of(orow, e)) break;
            host.push_back(e);
        }
    }
    for (int k = 0; k < 64; ++k) host.push_back(Entry{0.0f, 0u, 0});
    if (ds->row_tables.size() >= 8) {                       // a handful of geometries at a time
        (void)hipDeviceSynchronize();                       // (nothing in flight may still read the one that goes)
        if (ds->row_tables.front()->dev) (void)hipFree(ds->row_tables.front()->dev);
        ds->row_tables.erase(ds->row_tables.begin());
    }
    auto t = std::make_unique<RowTable>();
    t->height = tg.height; t->pitch = tg.pitch; t->rank = tg.band_rank; t->world = world; t->rows = tg.band_rows; t->compact = tg.compact;
    t->half_h = hh; t->fovI = fi;
    t->il = il; t->il_rows = il_rows; t->il_count = tg.row_count;
    HIP_TRY(hipMalloc(&t->dev, host.size() * sizeof(Entry)));
    HIP_TRY(hipMemcpy(t->dev, host.data(), host.size() * sizeof(Entry), hipMemcpyHostToDevice));
    dev_ptr = t->dev;
    ds->row_tables.push_back(std::move(t));
    return NT_OK;
}

// |o|^2, o.right, o.up, o.forward (see NtCamera)
void camera_dots(int n, const float *origin, const float *axes, float out[4]) {
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < n; ++k) {
        q[0] += (double)origin[k] * origin[k];
        for (int r = 0; r < 3; ++r) q[1 + r] += (double)origin[k] * axes[(size_t)r * n + k];
    }
    for (int r = 0; r < 4; ++r) out[r] = (float)q[r];
}

// camera rows the ray source needs: origin, right, up, forward (camera.hpp:40-45)
void pack_camera(int n, const float *origin, const float *axes, float *out) {
    std::memcpy(out, origin, sizeof(float) * n);
    std::memcpy(out + n, axes, sizeof(float) * n);            // right  = t_orientation[0]
    std::memcpy(out + 2 * n, axes + n, sizeof(float) * n);    // up     = t_orientation[1]
    std::memcpy(out + 3 * n, axes + 2 * n, sizeof(float) * n);// forward= t_orientation[2]
}

// a camera table (NtCamera::buf): the rows of all `nframes` cameras, then their dot products, (4 n + 4) * nframes floats
void pack_cameras(int n, int nframes, const float *origins, const float *axes, float *out) {
    for (int f = 0; f < nframes; ++f) {
        pack_camera(n, origins + (size_t)f * n, axes + (size_t)f * n * n, out + (size_t)f * 4 * n);
        camera_dots(n, origins + (size_t)f * n, axes + (size_t)f * n * n, out + (size_t)nframes * 4 * n + (size_t)f * 4);
    }
}

void fill_view(NtTarget &tg, const nt_scene *s, int w, int h) {
    // flat_origin_ray_source::set_params (tracer.hpp:65-69)
    tg.width = w;
    tg.height = h;
    tg.half_w = float(w) / float(2);
    tg.half_h = float(h) / float(2);
    tg.fovI = std::tan(s->fov / 2) / tg.half_w;
}

void fill_composite(const nt_scene *s, const DeviceState *ds, NtCompositeDev &c, bool stats) {
    std::memset(&c, 0, sizeof(c));
    c.nodes = (const NtNode *)ds->nodes.p;
    c.items = (const int *)ds->items.p;
    c.batch_recs = (const float *)ds->batch_recs.p;
    c.batch_mats = (const int *)ds->batch_mats.p;
    c.tri_recs = (const float *)ds->tri_recs.p;
    c.tri_mats = (const int *)ds->tri_mats.p;
    c.solid_recs = (const float *)ds->solid_recs.p;
    c.solid_types = (const int *)ds->solid_types.p;
    c.solid_mats = (const int *)ds->solid_mats.p;
    c.materials = (const float *)ds->materials.p;
    c.aabb = (const float *)ds->aabb.p;
    c.rec_stride = s->rec_stride;
    c.root = s->root;
    c.stack_depth = std::max(s->depth + 1, 2);
    c.shadows = s->shadows;
    c.camera_light = s->camera_light;
    c.max_reflect_depth = s->max_reflect_depth;
    c.bg_axis = s->bg_axis;
    for (int k = 0; k < 3; ++k) { c.ambient[k] = s->ambient[k]; c.bg1[k] = s->bg1[k]; c.bg2[k] = s->bg2[k]; c.bg3[k] = s->bg3[k]; }
    const float *lp = (const float *)ds->lights.p;
    c.n_point_lights = (int)(s->pl_color.size() / 3);
    c.n_global_lights = (int)(s->gl_color.size() / 3);
    c.pl_pos = lp;
    c.pl_color = lp + s->pl_pos.size();
    c.gl_dir = c.pl_color + s->pl_color.size();
    c.gl_color = c.gl_dir + s->gl_dir.size();
    c.all_opaque = s->all_opaque;
    c.any_reflective = s->any_reflective;
    c.has_scalar_prims = s->has_scalar;
    c.n_batches = s->n_batches;
    c.n_solids = s->n_solids;
    c.n_triangles = s->n_triangles;
    c.stats = stats ? (unsigned long long *)ds->stats.p : nullptr;
    c.checked = nullptr;
    c.alias_normals = 0;
    c.checked_words = 0;
    c.checked_lanes = 0;
    c.tframes = nullptr;
    c.tframe_count = 0;
}

int check_renderable(const nt_scene *s) {
    if (s->composite) {
        if (s->nodes.size() >= (1u << 24)) return fail(NT_E_UNSUPPORTED, "k-d trees with 2^24 or more nodes are not supported");
    }
    return NT_OK;
}

// the renderer protocol of obj_BlockingRenderer_render (render.cpp:878-904): refuse re-entry, lock the scene
struct RenderGuard {
    nt_scene *s;
    bool held = false;
    explicit RenderGuard(nt_scene *sc) : s(sc) {}
    int acquire() {
        std::lock_guard<std::mutex> g(s->mu);
        if (s->busy) return fail(NT_E_BUSY, "the renderer is already running");
        s->busy = true;
        ++s->locked;
        held = true;
        return NT_OK;
    }
    ~RenderGuard() {
        if (held) {
            std::lock_guard<std::mutex> g(s->mu);
            s->busy = false;
            --s->locked;
        }
    }
};

struct FrameJob {
    const Format *fmt;
    Bands bands;
    void *dest_dev;
    size_t frame_stride;
    int nframes;
    const float *cam_buf;     // device [nframes][4][n] or nullptr
    const float *cam_dots = nullptr;   // with cam_buf: device [nframes][4], the cameras' dot products (camera_dots)
    const float *cam_span = nullptr;   // with cam_buf, from a camera table only: device [nframes][2], the cameras' spans (NtCamera::span)
    const float *cam_axes = nullptr;   // with cam_buf, while a view stack is set: device [nframes][n][n], all the axes of the cameras
    hipStream_t stream;
    bool stats;
    bool strict = false;      // nt_render_opts.strict_reference
    const int *abort_word = nullptr;   // NtTarget::abort_word
    int overlapped = 0;                // nt_render_opts::overlapped
    bool counters_pass = false;        // (enqueue's own) the statistics launch of a scene whose pixels come from the faithful kernels
    bool samples_pass = false;         // (enqueue's own) the first stage of a supersampled render: the s*W x s*H samples
    int row_begin, row_count; // owned-row range
    // probe mode
    float *colors_out = nullptr;
    const int *xs = nullptr, *ys = nullptr;
    int probe_count = 0;
    int view_w = 0, view_h = 0;
    int layers = 1;                    // (nt_hit_layers alone) the planes of records a pixel gets
};

// The NTRACER_* render switches, read once per enqueue and never cached: a process may change its
// environment between calls.  Unset, a switch takes the default below; set, its value goes through atoi (empty: 0).
struct RenderSwitches {
    bool strict_reference, clean_normals, force_var, numerators, two_pass, tile_order, box_cull, box_interleave, box_var_rows;
    int composite_kernel, frame_major, chunk_frames;
};

int atoi_or(const char *e, int unset) { return e ? atoi(e) : unset; }

RenderSwitches read_switches() {
    RenderSwitches sw;
    sw.strict_reference = atoi_or(getenv("NTRACER_STRICT_REFERENCE"), 0) != 0;  // 1: the reference's exact k-d walk (nt_render_opts::strict_reference)
    sw.clean_normals = atoi_or(getenv("NTRACER_CLEAN_NORMALS"), 0) != 0;        // 1: a hit keeps the normal of what was hit (changes pixels: DESIGN.md 2)
    sw.force_var = atoi_or(getenv("NTRACER_FORCE_VAR"), 0) != 0;                // 1: the run-time-n kernels at every dimension, for tests to compare them
    sw.composite_kernel = atoi_or(getenv("NTRACER_COMPOSITE_KERNEL"), 0);       // NtLaunchInfo::kernel_choice: 1 persistent, 2 plain per-lane kernel
    sw.numerators = atoi_or(getenv("NTRACER_NUMERATORS"), 1) != 0;              // 0: no per-frame plane numerators for the packet kernel
    sw.two_pass = atoi_or(getenv("NTRACER_TWO_PASS"), 1) != 0;                  // 0: lit scenes in one packet kernel
    sw.tile_order = atoi_or(getenv("NTRACER_TILE_ORDER"), 1) != 0;              // 0: the packet kernel's quads in row-major order
    sw.frame_major = atoi_or(getenv("NTRACER_FRAME_MAJOR"), 1);                 // 0: the frames of a multi-frame packet launch interleaved
    sw.chunk_frames = atoi_or(getenv("NTRACER_CHUNK_FRAMES"), INT_MAX);         // (tests) at most max(k, 1) frames per packet launch; unset: no cap
    sw.box_cull = atoi_or(getenv("NTRACER_BOX_CULL"), 1) != 0;                  // 0: no stretch codes, every BoxScene format through the general kernel
    sw.box_interleave = atoi_or(getenv("NTRACER_BOX_INTERLEAVE"), 1) != 0;      // 0: a tile-kernel wave renders consecutive rows
    sw.box_var_rows = atoi_or(getenv("NTRACER_BOX_VAR_ROWS"), 1) != 0;          // 0: BoxScene at run-time n through the per-pixel kernel for every format
    return sw;
}

// Which kernels a composite scene goes to.  The launchers (nt_var.hip, nt_composite.hpp, nt_hits.hpp ...) decide the same way from
// what the host hands them, and the host allocates the scratch the chosen kernel reads -- the `checked` columns, the frame
// stacks -- so the rule is written here once and every enqueue takes its answers from it; what a site adds (no `checked` list
// for an occlusion query or a counters pass) it adds on top.
struct CompositeRoute {
    // Scenes with transparent materials or Solids are rendered with the reference's own handling of o_hit.normal (its
    // first leaf loop lets every primitive test write to the current hit's normal ray, tracer.hpp:1001,1020 -- see
    // composite_kernel_t<N, true>), which needs the reference's exact `checked` list: a bitmap column per resident
    // lane.  NTRACER_CLEAN_NORMALS=1 selects the intended semantics instead (a hit keeps the normal of what was hit).
    // (transparent materials need the exact list in either mode: the reference trims its transparent hits with the
    // distance of the LAST test, so a repeated test is not harmless there)
    bool faithful;
    bool var;            // the run-time-n kernels
    int frame_stack;     // ray_color frames a lane of a faithful walk keeps
    // The compile-time-N kernel keeps NT_TFRAMES ray_color frames in registers/scratch; above NT_MAX_FIXED_DIM, and
    // for reflection deeper than that among transparent things, the run-time-n kernel with its frames in global
    // scratch takes over (one wave per block there).
    bool var_t;
    // what launch_composite_fixed gives the packet walk, for a composite scene (the walk has a stack of 32 nodes)
    bool packet_walk;
};

CompositeRoute composite_route(const nt_scene *s, const RenderSwitches &sw) {
    CompositeRoute r;
    r.faithful = !s->all_opaque || (s->n_solids > 0 && !sw.clean_normals);
    r.var = s->n > NT_MAX_FIXED_DIM || sw.force_var;
    r.frame_stack = s->any_reflective ? s->max_reflect_depth + 1 : 1;
    r.var_t = r.var || r.frame_stack > 6;
    r.packet_walk = !r.faithful && !r.var && sw.composite_kernel == 0 && std::max(s->depth + 1, 2) <= 32;
    return r;
}

// the scene as the kernels of a launch see it
void scene_dev(const nt_scene *s, const DeviceState *ds, const RenderSwitches &sw, bool strict, bool stats, NtCompositeDev &c) {
    fill_composite(s, ds, c, stats);
    // closest-hit walks drop subtrees beyond the current hit unless the caller (or NTRACER_STRICT_REFERENCE=1)
    // asks for the reference's exact walk; the pixels are the same (nt_beyond_hit in nt_composite.hpp)
    // ... and never for scenes with Solids: trees from the reference's own builder leave solids out of some cells
    // they reach (its goldens show it), i.e. they break the invariant the shortcut relies on
    c.prune = (strict || sw.strict_reference || s->n_solids > 0) ? 0 : 1;
    if (c.root < 0) c.root = -1;
}

// what every launcher is told; the buffers of a route (counter, cameras, numerators, hit records, tile order, cull bits) are its
// enqueue's to add
NtLaunchInfo launch_info(const nt_scene *s, const DeviceState *ds, const RenderSwitches &sw, int nframes, hipStream_t stream) {
    NtLaunchInfo li{};
    li.n = s->n;
    li.nframes = nframes;
    li.stream = stream;
    li.cu_count = ds->cu_count;
    li.kernel_choice = sw.composite_kernel;
    li.frame_major = sw.frame_major;
    li.force_var = sw.force_var;
    li.box_var_rows = sw.box_var_rows;
    return li;
}

// a launcher's non-zero status: -2 is a launch the kernels refuse, anything else the device's own error
int launch_failed(int r) { return fail(r == -2 ? NT_E_UNSUPPORTED : NT_E_DEVICE, "%s", nt_launch_error()); }

// the cameras of a launch in device memory: the caller's table, or the scene's own camera, copied there in stream order
int device_camera(const nt_scene *s, DeviceState *ds, const float *cam_buf, hipStream_t stream, const float *&cams) {
    cams = cam_buf;
    if (cams) return NT_OK;
    float packed[4 * NT_DEV_MAX_DIM];
    pack_camera(s->n, s->origin.data(), s->axes.data(), packed);
    if (int e = ds->cams.ensure(sizeof(float) * 4 * s->n)) return e;
    HIP_TRY(hipMemcpyAsync(ds->cams.p, packed, sizeof(float) * 4 * s->n, hipMemcpyHostToDevice, stream));
    cams = (const float *)ds->cams.p;
    return NT_OK;
}

// the plain fp32 x 3 format, 12-byte pixels without padding: what a stage draws in when another kernel reads its pixels
int plain_f32_format(int w, int h, Format &out) {
    static const nt_channel plain[3] = {{1.0f, 0.0f, 0.0f, 0.0f, 32, 1, {0, 0}}, {0.0f, 1.0f, 0.0f, 0.0f, 32, 1, {0, 0}}, {0.0f, 0.0f, 1.0f, 0.0f, 32, 1, {0, 0}}};
    const nt_image_format desc = {(int32_t)w, (int32_t)h, 0, 3, plain, 0};
    return parse_format(&desc, out);
}

// the target of the kernels that draw nothing: the whole pinhole view of w x h, and the abort word
void view_target(const nt_scene *s, int w, int h, const int *abort_word, NtTarget &tg) {
    std::memset(&tg, 0, sizeof(tg));
    fill_view(tg, s, w, h);
    tg.band_world = 1;
    tg.band_rows = NT_RENDER_CHUNK_SIZE;
    tg.row_count = h;
    tg.abort_word = abort_word;
}

// The sub-job of a render that works on a base frame (adaptive supersampling, ambient occlusion): frames [f0, f0 + nf) of `job`,
// whole and without bands, in the plain format `bf` into scratch at `dest`, `frame_bytes` apart -- every route of a plain render
// comes with it.  No counters: such a render has refused them.
FrameJob base_frame_job(const nt_scene *s, const FrameJob &job, const Format &bf, int f0, int nf, void *dest, size_t frame_bytes) {
    FrameJob bj = job;
    bj.samples_pass = true;
    bj.fmt = &bf;
    bj.bands = Bands();
    bj.bands.owned_rows = bf.height;
    bj.row_begin = 0;
    bj.row_count = bf.height;
    bj.nframes = nf;
    bj.frame_stride = frame_bytes;
    bj.dest_dev = dest;
    bj.stats = false;
    if (job.cam_buf) {
        bj.cam_buf = job.cam_buf + (size_t)f0 * 4 * s->n;
        bj.cam_dots = job.cam_dots + (size_t)f0 * 4;
        if (job.cam_span) bj.cam_span = job.cam_span + (size_t)f0 * 2;
    }
    return bj;
}

// The scratch of the walks that keep the reference's exact `checked` list (renders and ray queries alike): a column of `words`
// dwords per resident lane, so the GRID is what the scratch has columns for and the blocks stride over the work.  `blocks` comes
// in as what the work could use and is halved, down to `min_blocks`, until the columns fit `cap_bytes` -- together with the
// ray_color frames a lane (`frame_stack` > 0: CompositeRoute::var_t), which get their columns in DeviceState::tframes here as
// well.  DevBuf::ensure only grows: after a call with the same shape nothing is allocated.
int checked_scratch(const nt_scene *s, DeviceState *ds, const RenderSwitches &sw, NtCompositeDev &c, long long lanes_per_block, long long &blocks,
                    long long min_blocks, int frame_stack, long long cap_bytes) {
    const long long words = ((long long)s->n_batches + s->n_triangles + s->n_solids + 31) / 32;
    const long long fwords = (long long)nt_var_frame_words(s->n) * frame_stack;
    while (blocks > min_blocks && blocks * lanes_per_block * (words + fwords) * 4 > cap_bytes) blocks /= 2;
    if (int e = ds->checked.ensure((size_t)(blocks * lanes_per_block * words * 4))) return e;
    c.checked = (uint32_t *)ds->checked.p;
    c.checked_words = (int)words;
    c.checked_lanes = (int)(blocks * lanes_per_block);
    c.alias_normals = sw.clean_normals ? 0 : 1;
    if (frame_stack > 0) {
        if (int e = ds->tframes.ensure((size_t)(blocks * lanes_per_block * fwords * 4))) return e;
        c.tframes = (float *)ds->tframes.p;
        c.tframe_count = frame_stack;
    }
    return NT_OK;
}

// the packet walk's plane numerators: as many frames as fit in 256 MB, at least one
int numerator_scratch(const nt_scene *s, DeviceState *ds, const RenderSwitches &sw, int nframes, NtLaunchInfo &li) {
    if (s->n_batches <= 0 || !sw.numerators) return NT_OK;
    const size_t per_frame = (size_t)s->n_batches * NT_BATCH_SIZE * sizeof(float);
    const size_t frames = std::max<size_t>(1, std::min<size_t>((size_t)nframes, ((size_t)256 << 20) / per_frame));
    if (int e = ds->numer.ensure(frames * per_frame)) return e;
    li.numer_buf = (float *)ds->numer.p;
    li.numer_frames = std::max(1, std::min((int)frames, sw.chunk_frames));
    return NT_OK;
}

// the primary hits between the two passes of a packet-walk render, `per_frame` bytes of records a frame: as many frames as fit in
// 512 MB, at least one
int hit_record_scratch(DeviceState *ds, const RenderSwitches &sw, size_t per_frame, int nframes, NtLaunchInfo &li) {
    const size_t frames = std::max<size_t>(1, std::min<size_t>((size_t)nframes, ((size_t)512 << 20) / std::max<size_t>(per_frame, 1)));
    if (int e = ds->hits.ensure(frames * per_frame)) return e;
    li.hit_buf = ds->hits.p;
    li.hit_frames = std::max(1, std::min((int)frames, sw.chunk_frames));
    return NT_OK;
}

// Dispatch order of the packet walk's quads (2x2 tiles of 8x8 pixels) for an image of `width` x `rows`: the waves that walk the
// middle of the scene run longest, so the quad rows nearest the centre go first; row-major within a row keeps neighbouring
// blocks on neighbouring rays.  A table per geometry, kept on the device.
int tile_order_for(DeviceState *ds, int width, int rows, const int *&dev_ptr) {
    const int tx = ((width + 7) / 8 + 1) / 2, ty = ((rows + 7) / 8 + 1) / 2;
    DeviceState::TileOrder *to = nullptr;
    for (auto &e : ds->tile_orders)
        if (e->tx == tx && e->ty == ty) to = e.get();
    if (!to) {
        std::vector<int> order((size_t)tx * ty);
        for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
        auto key = [&](int t) {
            const long long dy = 2 * (t / tx) - (ty - 1);
            return dy < 0 ? -dy : dy;
        };
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key(a) < key(b); });
        if (ds->tile_orders.size() >= 16) {
            // tables may still be read by launches queued on other streams
            HIP_TRY(hipDeviceSynchronize());
            for (auto &e : ds->tile_orders) e->buf.release();
            ds->tile_orders.clear();
        }
        std::unique_ptr<DeviceState::TileOrder> e(new DeviceState::TileOrder);
        if (int err = e->buf.ensure(order.size() * sizeof(int))) return err;
        HIP_TRY(hipMemcpy(e->buf.p, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
        e->tx = tx;
        e->ty = ty;
        to = e.get();
        ds->tile_orders.push_back(std::move(e));
    }
    dev_ptr = (const int *)to->buf.p;
    return NT_OK;
}

// enqueue's CompositeScene half: the device scene, the `checked` and frame scratch of the faithful kernels, and the packet
// kernel's counter, cameras, numerators, hit scratch and tile order
int plan_composite(const nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw, const NtTarget &tg,
                   const NtCamera &cam, NtLaunchInfo &li, NtCompositeDev &c) {
    scene_dev(s, ds, sw, job.strict, job.stats, c);
    const CompositeRoute rt = composite_route(s, sw);
    // (the statistics launch of a scene with Solids is the counting kernel, which keeps no `checked` list: see enqueue)
    const bool faithful = !job.counters_pass && rt.faithful;
    if (faithful) {
        const long long lpb = rt.var_t ? 64 : 256;        // lanes per block
        const long long tw = rt.var_t ? 8 : 16;           // tile edge
        long long tiles = job.colors_out ? (job.probe_count + lpb - 1) / lpb
                                         : (long long)((tg.width + tw - 1) / tw) * ((tg.row_count + tw - 1) / tw) * job.nframes;
        long long blocks = std::min<long long>(std::max<long long>(tiles, 1), rt.var_t ? 8192 : 4096);
        if (int e = checked_scratch(s, ds, sw, c, lpb, blocks, 64, rt.var_t ? rt.frame_stack : 0, (long long)512 << 20)) return e;
    }
    // image renders of opaque scenes made of batches go through the packet kernel (primary rays share the
    // camera origin): it needs the camera table in device memory (and, for the persistent variant, a counter)
    // (what is not faithful has opaque materials alone, a counters pass too: enqueue refuses it to any other scene)
    const bool packetable = !faithful;
    if (packetable && !job.stats && !job.colors_out && s->n <= NT_MAX_FIXED_DIM && li.kernel_choice != 2) {
        // persistent kernel: a zeroed work counter and the camera table in device memory (stream ordered)
        if (int e = ds->counter.ensure(8)) return e;
        HIP_TRY(hipMemsetAsync(ds->counter.p, 0, 8, job.stream));
        li.persist_counter = ds->counter.p;
        if (job.cam_buf) {
            li.persist_cams = job.cam_buf;
        } else {
            if (int e = ds->cams.ensure(sizeof(float) * 4 * s->n)) return e;
            HIP_TRY(hipMemcpyAsync(ds->cams.p, cam.inl, sizeof(float) * 4 * s->n, hipMemcpyHostToDevice, job.stream));
            li.persist_cams = (const float *)ds->cams.p;
        }
    }
    if (!li.persist_cams || tg.colors_out) return NT_OK;
    // ... and its numerators, the hit records of a two-pass render, and the order of its quads
    if (int e = numerator_scratch(s, ds, sw, job.nframes, li)) return e;
    const bool lit = !s->pl_color.empty() || !s->gl_color.empty() || c.any_reflective || c.has_scalar_prims;
    if (lit && sw.two_pass) {
        if (int e = hit_record_scratch(ds, sw, (size_t)16 * tg.width * tg.row_count, job.nframes, li)) return e;
    }
    if (sw.tile_order) {
        if (int e = tile_order_for(ds, tg.width, tg.row_count, li.tile_order)) return e;
    }
    return NT_OK;
}

// enqueue's BoxScene half: the cull buffer, whether the fused tile kernel takes the launch, its block shape and row table
int plan_box(const nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw, NtTarget &tg, NtLaunchInfo &li) {
    if (tg.colors_out || !sw.box_cull) return NT_OK;
    // one bit per 64-pixel stretch of a row: can any of its rays reach the cube? (box_cull_kernel)
    const size_t words = (size_t)(((tg.width + 63) / 64 + 31) / 32);
    // stretch codes (4 words per redo word) and 16 rows of padding (box_kernel reads a wave's rows without clamping); the
    // fused route's redo bitmap, one word per redo word, fits in the codes' place
    const size_t need = ((size_t)4 * job.nframes * tg.row_count + 64) * words * sizeof(uint32_t);
    if (need > ds->cull.cap || !ds->cull.p) ds->cull_clean = false;
    if (int e = ds->cull.ensure(need)) return e;
    // The fused kernels keep their redo bitmap at the start of this buffer and leave it zeroed; after anything else
    // has written there (a fresh allocation, box_cull_kernel's stretch codes) it is zeroed here, in stream order.
    // (the formats launch_box_fixed sends there: plain RGB of <= 10 bits in one aligned dword, or three plain fp32 channels)
    const bool fused = s->n <= NT_MAX_FIXED_BOX_DIM && tg.aligned4 &&
                       ((tg.plain_bits != 0u && tg.plain_bits <= 10u && tg.bpp == 4) || (tg.plain_f32[0] >= 0 && tg.bpp == 12));
    if (fused && !ds->cull_clean) {
        HIP_TRY(hipMemsetAsync(ds->cull.p, 0, ds->cull.cap, job.stream));
        ds->cull_clean = true;
    } else if (!fused) {
        ds->cull_clean = false;
    }
    li.cull_clean = fused ? 1 : 0;
    li.cull_buf = (uint32_t *)ds->cull.p;
    if (fused) {
        // interleaved rows (the default for launches that start at their first owned row; NTRACER_BOX_INTERLEAVE=0: A/B):
        // the waves of a column strip deal the rows out among themselves, so that the rows that need ray-by-ray work --
        // which come in runs of dozens -- are spread over all of them instead of making a few waves ten times as long as
        // the rest
        const NtBoxTileGeom geom = nt_box_tile_geom(tg.width, tg.row_count, job.nframes, job.overlapped);
        li.tile_rows = geom.rows;
        li.tile_waves = geom.waves;
        const int tile_rows = geom.rows * geom.waves;
        tg.row_il = (tg.row_begin == 0 && sw.box_interleave) ? (tg.row_count + tile_rows - 1) / tile_rows * geom.waves : 0;
        if (int e = row_table(ds, tg, geom.rows, tg.rowtab)) return e;
    }
    return NT_OK;
}

// where the pixels of a job go: the view, the format's packing constants, the band split and the owned-row range
int fill_target(const nt_scene *s, DeviceState *ds, const FrameJob &job, NtTarget &tg) {
    std::memset(&tg, 0, sizeof(tg));
    if (job.colors_out) {
        fill_view(tg, s, job.view_w, job.view_h);
        tg.colors_out = job.colors_out;
        tg.probe_xs = job.xs;
        tg.probe_ys = job.ys;
        tg.probe_count = job.probe_count;
        tg.band_world = 1;
        tg.band_rows = NT_RENDER_CHUNK_SIZE;
    } else {
        const Format &f = *job.fmt;
        fill_view(tg, s, f.width, f.height);
        tg.dest = (uint8_t *)job.dest_dev;
        tg.frame_stride = (long long)job.frame_stride;
        const NtChanDev *chans = nullptr;
        if (int r = chan_table(ds, f, chans)) return r;
        tg.chans = chans;
        tg.nchannels = (int)f.chans.size();
        tg.pack_mode = f.pack_mode;
        tg.plain_bits = f.plain_bits;
        tg.plain_maxval = f.plain_maxval;
        for (int k = 0; k < 3; ++k) tg.plain_mul[k] = f.plain_mul[k];
        tg.plain_sel = 0;
        if (f.plain_bits == 8 && ((f.plain_mul[0] | f.plain_mul[1] | f.plain_mul[2]) & ~0x01010101u) == 0) {
            // byte b of the MSB-first pixel word holds the component whose multiplier has bit 8b set; memory byte k is
            // byte 3-k of that word (or byte k when the pixel's bytes are reversed)
            uint32_t sel = 0;
            for (int k = 0; k < 4; ++k) {
                const int b = f.reversed ? k : 3 - k;
                uint32_t pick = 0x0c;                                            // constant 0
                if ((f.plain_mul[0] >> (8 * b)) & 1u) pick = 4;                  // byte 0 of src0: R
                else if (((f.plain_mul[1] | f.plain_mul[2]) >> (8 * b)) & 1u) pick = 0;     // byte 0 of src1: G = B
                sel |= pick << (8 * k);
            }
            tg.plain_sel = sel;
        }
        for (int k = 0; k < 3; ++k) tg.plain_f32[k] = f.plain_f32[k];
        tg.bpp = f.bpp;
        tg.reversed = f.reversed;
        tg.pitch = f.pitch;
        tg.band_rank = job.bands.rank;
        tg.band_world = job.bands.world;
        tg.band_rows = job.bands.rows;
        tg.compact = job.bands.compact;
        tg.row_begin = job.row_begin;
        tg.row_count = job.row_count;
        tg.aligned4 = ((uintptr_t)job.dest_dev % 4 == 0) && (f.pitch % 4 == 0) && (job.frame_stride % 4 == 0);
        tg.abort_word = job.abort_word;
    }
    return NT_OK;
}

int enqueue(nt_scene *s, DeviceState *ds, const FrameJob &job_in);

// A supersampled render (nt_scene_set_supersampling), in two stages per chunk: the job once more at s*W x s*H
// in the plain fp32 x 3 format -- the caller's owned rows [r, r + c) are sample rows [s*r, s*(r + c)) of a split into bands
// of s*band_rows rows, same rank and world -- into the scratch buffer, then resolve_kernel into the caller's `dest`, where
// the single-sample kernels would have written.  The scratch is capped (nt_scene_set_supersampling_scratch_mb): the job is cut into chunks
// of whole frames and, when one frame's samples are too many, into chunks of rows, each rendered and resolved before the
// next on the same stream.  Everything else (strict_reference, overlapped, the abort word, the counters) passes through.
int enqueue_supersampled(nt_scene *s, DeviceState *ds, const FrameJob &job) {
    const int ss = s->supersampling;
    const Format &f = *job.fmt;
    if (job.row_count <= 0 || f.bpp == 0) return NT_OK;         // nothing to draw
    const long long cap = (long long)s->ss_scratch_mb << 20;
    const long long hi_w = (long long)ss * f.width, hi_h = (long long)ss * f.height;
    const long long hi_pitch = 12 * hi_w;                        // bytes a sample row
    const long long row_bytes = hi_pitch * ss;                   // the samples of one output row
    if (hi_pitch > INT_MAX || hi_h > INT_MAX)
        return fail(NT_E_UNSUPPORTED, "supersampling %d of a %d x %d image: the %lld x %lld samples are beyond the 2^31 - 1 bytes a sample row "
                    "and the 2^31 - 1 sample rows the kernels address", ss, f.width, f.height, hi_w, hi_h);
    if (row_bytes > cap)
        return fail(NT_E_UNSUPPORTED, "supersampling %d of a %d pixel wide image: the samples of one row (%lld bytes) do not fit the scratch "
                    "buffer of %lld MiB (nt_scene_set_supersampling_scratch_mb)", ss, f.width, row_bytes, cap >> 20);
    Format hf;
    if (int r = plain_f32_format((int)hi_w, (int)hi_h, hf)) return r;
    // (16384 rows at most: the grids of the two stages count rows in their y)
    const long long rows_fit = std::min<long long>(cap / row_bytes, 16384);
    const int chunk_rows = (int)std::min<long long>(rows_fit, job.row_count);
    const int chunk_frames = chunk_rows < job.row_count ? 1 : (int)std::max<long long>(1, std::min<long long>(job.nframes, cap / (row_bytes * chunk_rows)));
    if (int e = ds->samples.ensure((size_t)chunk_frames * chunk_rows * row_bytes)) return e;
    NtTarget tg;
    if (int r = fill_target(s, ds, job, tg)) return r;
    for (int f0 = 0; f0 < job.nframes; f0 += chunk_frames) {
        const int nf = std::min(chunk_frames, job.nframes - f0);
        for (int r0 = 0; r0 < job.row_count; r0 += chunk_rows) {
            const int rc = std::min(chunk_rows, job.row_count - r0);
            FrameJob hj = job;
            hj.samples_pass = true;
            hj.fmt = &hf;
            hj.bands.rows = ss * job.bands.rows;
            hj.bands.compact = 1;
            hj.bands.owned_rows = ss * job.bands.owned_rows;
            hj.row_begin = ss * (job.row_begin + r0);
            hj.row_count = ss * rc;
            hj.nframes = nf;
            hj.frame_stride = (size_t)(rc * row_bytes);
            // (compact: owned sample row o of a frame lies at o * pitch, and the chunk's first one at the start of the scratch)
            hj.dest_dev = (char *)ds->samples.p - (long long)hj.row_begin * hi_pitch;
            if (job.cam_buf) {
                hj.cam_buf = job.cam_buf + (size_t)f0 * 4 * s->n;
                hj.cam_dots = job.cam_dots + (size_t)f0 * 4;
                if (job.cam_span) hj.cam_span = job.cam_span + (size_t)f0 * 2;
            }
            if (int e = enqueue(s, ds, hj)) return e;
            NtTarget rt = tg;
            rt.dest = tg.dest + (long long)f0 * tg.frame_stride;
            rt.row_begin = job.row_begin + r0;
            rt.row_count = rc;
            if (int r = nt_launch_resolve(ss, job.stream, ds->samples.p, (long long)hj.frame_stride, hi_pitch, nf, rt)) return launch_failed(r);
        }
    }
    return NT_OK;
}

// ---------------------------------------------------------------------------------------------
// the whole-view settings -- clip planes, depth cues, outlines, ambient occlusion, BoxScene's face lines --
// and what their passes and the adaptive one share
// ---------------------------------------------------------------------------------------------
int hits_enqueue(nt_scene *s, DeviceState *ds, int width, int height, const nt_hit_buffers *out, long long frame_stride, const float *cam_buf,
                 int nframes, bool strict, const int *abort_word, hipStream_t stream);

// A setting whose render comes from a pass over the records of the whole pinhole view, one sample a pixel, no kernel of which
// keeps counters.  The table is in the order of precedence: a scene with two of them on is refused by the one nearer the top,
// in `while_on`'s words of the other, not drawn with one of them missing.  Face lines are BoxScene's: they neither refuse the
// composite settings nor are refused by them (no `while_on`), and neither is face shading, which draws the lines itself when both
// are on.  The next setting is one more row, and one more line of enqueue.
struct ViewSetting {
    bool (*on)(const nt_scene *s);
    const char *subject;                 // of every message: "<subject> not available ..."
    const char *band_suffix;             // what the row-band message adds
    const char *while_on;                // how the rows above name this setting when they refuse it
    int (*extra)(const nt_scene *s);     // a term of its own, after all the others, or nullptr
};
enum { VS_XRAY, VS_STACK, VS_CLIP, VS_CUE, VS_OUTLINES, VS_AO, VS_BOX_LINES, VS_BOX_SHADING, VS_COUNT };
const ViewSetting kViewSettings[VS_COUNT] = {
    // (CompositeScene's alone, so BoxScene's two settings never meet it; a view stack is refused through its `while_on`)
    {[](const nt_scene *s) { return s->xray; }, "X-ray is", "", "X-ray is on", nullptr},
    {[](const nt_scene *s) { return s->stack_count > 0; }, "a view stack is", "", "a view stack is set",
     // BoxScene's two settings have no `while_on`: they are refused here
     [](const nt_scene *s) {
         if (!s->composite && s->box_lines) return fail(NT_E_UNSUPPORTED, "a view stack is not available while face lines are set");
         if (!s->composite && s->box_shading) return fail(NT_E_UNSUPPORTED, "a view stack is not available while face shading is set");
         return (int)NT_OK;
     }},
    {[](const nt_scene *s) { return s->clip_count > 0; }, "clip planes are", "", "clip planes are set",
     // a Solid cut open needs a cap or an inner wall, which nothing defines: refused, not approximated
     [](const nt_scene *s) {
         return s->n_solids > 0 ? fail(NT_E_UNSUPPORTED, "clip planes are not available for a scene with Solids (a Solid cut open has no cap)") : (int)NT_OK;
     }},
    {[](const nt_scene *s) { return s->cue; }, "depth cues are", "", "depth cues are on", nullptr},
    {[](const nt_scene *s) { return s->outlines; }, "outlines are", ": a pixel's mask needs its neighbours", "outlines are on", nullptr},
    {[](const nt_scene *s) { return s->ao_count > 0; }, "ambient occlusion is", "", "ambient occlusion is on", nullptr},
    {[](const nt_scene *s) { return s->box_lines && !s->composite; }, "face lines are", ": a pixel's mask needs its neighbours", nullptr, nullptr},
    {[](const nt_scene *s) { return s->box_shading && !s->composite; }, "face shading is", "", nullptr, nullptr},
};

// What a render with the setting of `row` on refuses, checked by the entry points before a device is touched (render_checks) and
// by the setting's enqueue again, for every way in.  The entry points hand over whole images: without bands their owned rows are
// all of them, so the row-range answer cannot be reached through the ABI; it guards the enqueues against callers within this
// file that split a job into rows.
int whole_view_check(const nt_scene *s, const ViewSetting &row, const Bands &b, bool stats, int row_begin, int row_count, int height) {
    if (!row.on(s)) return NT_OK;
    const char *w = row.subject;
    if (s->supersampling > 1) return fail(NT_E_UNSUPPORTED, "%s not available with a supersampling factor above 1 (%d)", w, s->supersampling);
    if (b.world > 1) return fail(NT_E_UNSUPPORTED, "%s not available with row bands (band_world %d)%s", w, b.world, row.band_suffix);
    if (row_begin != 0 || row_count != height) return fail(NT_E_UNSUPPORTED, "%s not available for a row range", w);
    if (stats) return fail(NT_E_UNSUPPORTED, "%s not available with collect_stats", w);
    if (s->lens) return fail(NT_E_UNSUPPORTED, "%s not available while a lens is set", w);
    if (s->parallel > 0.0f) return fail(NT_E_UNSUPPORTED, "%s not available while the parallel projection is set", w);
    // the settings further down the table, from the last to the first
    for (const ViewSetting *below = kViewSettings + VS_COUNT - 1; below > &row; --below)
        if (below->while_on && below->on(s)) return fail(NT_E_UNSUPPORTED, "%s not available while %s", w, below->while_on);
    return row.extra ? row.extra(s) : (int)NT_OK;
}

// What such a pass starts from.  With job.fmt it is a render; without, the setting's buffer alone, of one view of job.view_w x
// job.view_h.
struct ViewPass {
    bool draw;
    bool nothing;                        // a render into a format without bytes: nothing to draw
    int W, H;
    long long px, px_limit;              // the view's pixels, and how many the kernels address
    NtTarget tg;                         // the caller's image (fill_target), or the whole view (view_target)
    Format bf;                           // plain fp32 x 3 of W x H: the base frame that a stage draws into scratch
};

// `row`: the setting whose check the job must pass (nullptr: none).  `noun` is the pass as its refusals name it.
int begin_view_pass(const nt_scene *s, DeviceState *ds, const FrameJob &job, const ViewSetting *row, const char *noun, ViewPass &vp,
                    long long px_limit = INT_MAX, const char *beyond = "beyond 2^31 - 1 pixels") {
    vp.draw = job.fmt != nullptr;
    vp.W = vp.draw ? job.fmt->width : job.view_w;
    vp.H = vp.draw ? job.fmt->height : job.view_h;
    if (row) {
        if (int r = whole_view_check(s, *row, job.bands, job.stats, vp.draw ? job.row_begin : 0, vp.draw ? job.row_count : vp.H, vp.H)) return r;
    }
    vp.nothing = vp.draw && job.fmt->bpp == 0;
    if (vp.nothing) return NT_OK;
    vp.px = (long long)vp.W * vp.H;
    vp.px_limit = px_limit;
    if (vp.px > px_limit) return fail(NT_E_UNSUPPORTED, "%s of a %d x %d image: %s", noun, vp.W, vp.H, beyond);
    if (vp.draw) {
        if (int r = fill_target(s, ds, job, vp.tg)) return r;
    } else {
        view_target(s, vp.W, vp.H, job.abort_word, vp.tg);
    }
    return plain_f32_format(vp.W, vp.H, vp.bf);
}

// The whole frames of a chunk of the pass, whose scratch of `per_frame` bytes a frame sits under `cap`, the supersampling cap: as
// many as fit, as the kernels' pixel indices reach and as `limit` allows, at least one.  `parts`: what one frame holds, where the
// refusal lists it.
int plan_scratch_frames(const ViewPass &vp, int nframes, const char *noun, const char *parts, long long per_frame, long long cap,
                        long long limit, long long &chunk_frames) {
    if (per_frame > cap)
        return fail(NT_E_UNSUPPORTED, "%s of a %d x %d image: %s (%lld bytes) %s not fit the scratch buffer of %lld MiB (nt_scene_set_supersampling_scratch_mb)",
                    noun, vp.W, vp.H, parts ? parts : "the scratch of one frame", per_frame, parts ? "do" : "does", cap >> 20);
    chunk_frames = std::max<long long>(1, std::min<long long>(std::min<long long>(nframes, cap / per_frame), std::min<long long>(vp.px_limit / vp.px, limit)));
    return NT_OK;
}

// the scratch of a pass (DeviceState::samples), handed out front to back
struct Scratch {
    char *at = nullptr;
    int open(DeviceState *ds, size_t bytes) {
        if (int e = ds->samples.ensure(bytes)) return e;
        at = (char *)ds->samples.p;
        return NT_OK;
    }
    template <typename T>
    T *take(size_t bytes) {
        T *p = (T *)at;
        at += bytes;
        return p;
    }
};

// frames [f0, f0 + nf) of the job: what their launchers are told, their target -- of a render, the caller's frames from f0 on --
// and their cameras in the caller's table (nullptr: the scene's own)
struct ViewChunk {
    int f0, nf;
    NtLaunchInfo li;
    NtTarget ft;
    const float *cams;
};

ViewChunk view_chunk(const nt_scene *s, const DeviceState *ds, const FrameJob &job, const RenderSwitches &sw, const ViewPass &vp, int f0,
                     long long chunk_frames) {
    ViewChunk ch;
    ch.f0 = f0;
    ch.nf = (int)std::min<long long>(chunk_frames, job.nframes - f0);
    ch.li = launch_info(s, ds, sw, ch.nf, job.stream);
    ch.ft = vp.tg;
    if (vp.draw) ch.ft.dest = vp.tg.dest + (long long)f0 * vp.tg.frame_stride;
    ch.cams = job.cam_buf ? job.cam_buf + (size_t)f0 * 4 * s->n : nullptr;
    return ch;
}

// the packet walk's plane numerators and quad order, as hits_enqueue hands them over, and with `recs` the records' place
int packet_records(const nt_scene *s, DeviceState *ds, const RenderSwitches &sw, int W, int H, int nf, void *recs, NtLaunchInfo &li) {
    if (int e = numerator_scratch(s, ds, sw, nf, li)) return e;
    if (sw.tile_order) {
        if (int e = tile_order_for(ds, W, H, li.tile_order)) return e;
    }
    if (recs) {
        li.hit_buf = recs;
        li.hit_frames = nf;
    }
    return NT_OK;
}

// off the packet walk: the chunk's plain fp32 x 3 base frame into `base` (a render only), then its primary-hit pass into `hb`, both
// in scratch -- every route of a plain render and of hits_enqueue comes with them
int base_and_hits(nt_scene *s, DeviceState *ds, const FrameJob &job, const ViewPass &vp, const ViewChunk &ch, void *base, const nt_hit_buffers &hb) {
    if (vp.draw) {
        if (int e = enqueue(s, ds, base_frame_job(s, job, vp.bf, ch.f0, ch.nf, base, (size_t)vp.px * 12))) return e;
    }
    return hits_enqueue(s, ds, vp.W, vp.H, &hb, vp.px, ch.cams, ch.nf, job.strict, job.abort_word, job.stream);
}

// ---------------------------------------------------------------------------------------------
// adaptive supersampling (nt_scene_set_adaptive_supersampling; kernels in nt_adaptive.hpp and nt_var.hip)
// ---------------------------------------------------------------------------------------------
int rays_scene(const nt_scene *s, DeviceState *ds, const RenderSwitches &sw, bool strict, long long count, long long lpb_fixed, long long max_fixed,
               NtCompositeDev &c);

// What an adaptive render refuses, checked by the entry points before a device is touched (and by enqueue_adaptive again, for
// every way in): the contrast of a pixel needs its neighbours, which another rank's band holds, and the refine kernels keep no
// counters
int adaptive_refusals(const Bands &b, bool stats) {
    if (b.world > 1) return fail(NT_E_UNSUPPORTED, "row bands (band_world %d) are not available with adaptive supersampling: a pixel's contrast needs its neighbours", b.world);
    if (stats) return fail(NT_E_UNSUPPORTED, "collect_stats is not available with adaptive supersampling");
    return NT_OK;
}

int adaptive_check(const nt_scene *s, const Bands &b, bool stats) {
    if (!s->adaptive || s->supersampling <= 1) return NT_OK;
    return adaptive_refusals(b, stats);
}

// An adaptive render, in three stages per chunk of whole frames (nt_adaptive.hpp): the job once more in the plain fp32 x 3 format
// into scratch -- every route of a plain render comes with it --, adaptive_flag, which draws the unflagged pixels and lists the
// others, and the refine kernels over that list.  `mask_dev` (nt_adaptive_mask*): the [nframes][H][W] flag bytes go there, and
// with job.fmt == nullptr nothing is drawn: the view is then job.view_w x job.view_h and stage 3 is left out.  The scratch -- 12 + 4
// bytes a pixel a frame, and one more for `mask_scratch`, the host form's mask -- sits under the supersampling cap.  Enqueue only.
int enqueue_adaptive(nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw, uint8_t *mask_dev, bool mask_scratch,
                     uint8_t **mask_out) {
    const char *noun = "adaptive supersampling";
    const int ss = s->supersampling;
    if (int r = adaptive_refusals(job.bands, job.stats)) return r;
    if (job.fmt && (job.row_begin != 0 || job.row_count != job.fmt->height)) return fail(NT_E_UNSUPPORTED, "a row range is not available with adaptive supersampling");
    ViewPass vp;
    if (int r = begin_view_pass(s, ds, job, nullptr, noun, vp, INT_MAX / 4, "more pixels than the list of flagged pixels addresses")) return r;
    if (vp.nothing) return NT_OK;
    const bool draw = vp.draw;
    const int W = vp.W, H = vp.H;
    const long long px = vp.px;
    const long long per_frame = px * (mask_scratch ? 17 : 16);
    long long chunk_frames;
    if (int r = plan_scratch_frames(vp, job.nframes, noun, "the base frame and the list of one frame", per_frame, (long long)s->ss_scratch_mb << 20,
                                    LLONG_MAX, chunk_frames)) return r;
    if (draw && ((long long)ss * W > INT_MAX / 12 || (long long)ss * H > INT_MAX))
        return fail(NT_E_UNSUPPORTED, "supersampling %d of a %d x %d image: beyond the views the kernels address", ss, W, H);
    Scratch at;
    if (int e = at.open(ds, (size_t)chunk_frames * per_frame)) return e;
    if (int e = ds->refine_count.ensure(64)) return e;
    const size_t fpx = (size_t)chunk_frames * px;
    char *scratch = at.take<char>(fpx * 12);
    uint32_t *list = at.take<uint32_t>(fpx * 4);
    if (mask_scratch) mask_dev = at.take<uint8_t>(fpx);
    if (mask_out) *mask_out = mask_dev;
    for (int f0 = 0; f0 < job.nframes; f0 += (int)chunk_frames) {
        const ViewChunk ch = view_chunk(s, ds, job, sw, vp, f0, chunk_frames);
        const int nf = ch.nf;
        const FrameJob bj = base_frame_job(s, job, vp.bf, f0, nf, scratch, (size_t)px * 12);
        if (int e = enqueue(s, ds, bj)) return e;
        NtAdaptive ad{};
        ad.base = (const uint32_t *)scratch;
        ad.nframes = nf;
        ad.threshold = s->adaptive_t;
        ad.list = list;
        ad.count = (int *)ds->refine_count.p;
        ad.mask = mask_dev ? mask_dev + (size_t)f0 * px : nullptr;
        ad.draw = draw ? 1 : 0;
        NtTarget ft = ch.ft;
        if (int r = nt_launch_adaptive_flag(job.stream, ad, ft)) return launch_failed(r);
        if (!draw || ss <= 1) continue;
        NtRefine rf{};
        rf.list = list;
        rf.count = ad.count;
        rf.max_count = (long long)nf * px;
        // the chunk's cameras; the scene's own goes to device memory here, after the base frame, whose packet walk puts the same
        // rows there
        if (int e = device_camera(s, ds, bj.cam_buf, job.stream, rf.cams)) return e;
        rf.s = ss;
        NtTarget hv;
        fill_view(hv, s, ss * W, ss * H);                               // (the view of 4.3's first stage)
        rf.half_w = hv.half_w;
        rf.half_h = hv.half_h;
        rf.fovI = hv.fovI;
        // consecutive lanes hold the list's pixels, not the aligned groups of one row that emit_pixel's shared dword stores of
        // 3- and 6-byte pixels count on: those formats go out pixel by pixel (as rays_image_target has it)
        if (ft.bpp == 3 || ft.bpp == 6) ft.aligned4 = 0;
        NtCompositeDev c;
        if (s->composite) {
            if (int e = rays_scene(s, ds, sw, job.strict, rf.max_count, 64, 4096, c)) return e;
        }
        if (int r = nt_launch_refine(ch.li, s->composite ? &c : nullptr, rf, ft)) return launch_failed(r);
    }
    return NT_OK;
}

// ---------------------------------------------------------------------------------------------
// ambient occlusion (nt_scene_set_ambient_occlusion; kernels in nt_ao.hpp and nt_var.hip)
// ---------------------------------------------------------------------------------------------
int query_enqueue(nt_scene *s, DeviceState *ds, NtQuery &q, bool strict, hipStream_t stream);

// The blocked counts of every pixel of the job's frames and, with job.fmt, the render that uses them, per chunk of whole frames:
// the plain fp32 x 3 base frame into scratch (a render only), a primary-hit pass with normals into scratch (hits_enqueue: every
// route of it), the counts -- ao_kernel for the opaque scenes the fixed-n kernels draw, else ao_expand, the closest-hit query
// launch and ao_reduce over chunks of whole pixel rows --, and ao_apply into the caller's image.  Without job.fmt the view is
// job.view_w x job.view_h, one frame, and the counts go to `blocked_dev`, or with that nullptr stay in scratch: *blocked_out.
// The scratch -- per pixel and frame 16 bytes of record, 8 n of normal rows, 12 of base frame and 4 of count; on the ray route
// 8 n + 32 bytes a ray of a chunk behind them -- sits under the supersampling cap.  Enqueue only.
int enqueue_ao(nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw, int *blocked_dev, int **blocked_out) {
    const char *noun = "ambient occlusion";
    ViewPass vp;
    if (int r = begin_view_pass(s, ds, job, &kViewSettings[VS_AO], noun, vp)) return r;
    if (vp.nothing) return NT_OK;
    const bool draw = vp.draw;
    const int W = vp.W, H = vp.H, n = s->n, K = s->ao_count;
    const long long px = vp.px;
    const long long cap = (long long)s->ss_scratch_mb << 20;
    const long long per_frame = px * (16 + 8 * n + 12 + 4);
    long long chunk_frames;
    if (int r = plan_scratch_frames(vp, job.nframes, noun, "the base frame, the hit records, the normal rows and the counts of one frame", per_frame, cap,
                                    LLONG_MAX, chunk_frames)) return r;
    // the opaque scenes the fixed-n kernels draw have a counting kernel of their own; every other scene takes the ray route
    const CompositeRoute rt = composite_route(s, sw);
    const bool fast = !rt.faithful && !rt.var;
    // the ray route: the rays of whole pixel rows behind the frames, 16-byte aligned
    const long long row_bytes = (long long)W * K * (8 * n + 32);
    long long chunk_rows = 0;
    if (!fast) {
        chunk_frames = std::min(chunk_frames, (cap - 16 - row_bytes) / per_frame);
        if (chunk_frames < 1)
            return fail(NT_E_UNSUPPORTED, "ambient occlusion of a %d x %d image with %d samples: one frame (%lld bytes) and the rays of one pixel row "
                        "(%lld bytes) do not fit the scratch buffer of %lld MiB (nt_scene_set_supersampling_scratch_mb)", W, H, K, per_frame, row_bytes, cap >> 20);
        chunk_rows = std::min<long long>(std::min<long long>((cap - 16 - chunk_frames * per_frame) / row_bytes, chunk_frames * H), INT_MAX / ((long long)W * K));
        if (chunk_rows < 1) return fail(NT_E_UNSUPPORTED, "ambient occlusion of a %d pixel wide image with %d samples: beyond 2^31 - 1 rays a pixel row", W, K);
    }
    Scratch at;
    if (int e = at.open(ds, (size_t)(chunk_frames * per_frame + (fast ? 0 : 16 + chunk_rows * row_bytes)))) return e;
    const size_t fpx = (size_t)chunk_frames * px;
    void *recs = at.take<void>(fpx * 16);
    float *no = at.take<float>(fpx * n * 4);
    float *nd = at.take<float>(fpx * n * 4);
    char *base = at.take<char>(fpx * 12);
    int *counts = at.take<int>(fpx * 4);
    char *rays = (char *)(((uintptr_t)at.at + 15) & ~(uintptr_t)15);
    if (!draw && blocked_dev) counts = blocked_dev;
    if (blocked_out) *blocked_out = counts;
    const NtTarget &tg = vp.tg;
    for (int f0 = 0; f0 < job.nframes; f0 += (int)chunk_frames) {
        const ViewChunk ch = view_chunk(s, ds, job, sw, vp, f0, chunk_frames);
        const int nf = ch.nf;
        nt_hit_buffers hb{};
        hb.hits = (nt_ray_hit *)recs;
        hb.normal_origin = no;
        hb.normal_dir = nd;
        if (int e = base_and_hits(s, ds, job, vp, ch, base, hb)) return e;
        NtAo ao{};
        ao.cams = ch.cams ? ch.cams : (const float *)ds->cams.p;        // (hits_enqueue has put the scene's own camera there)
        ao.nframes = nf;
        ao.recs = recs;
        ao.normal_origin = no;
        ao.normal_dir = nd;
        ao.dirs = (const float *)ds->ao_dirs.p;
        ao.count = K;
        ao.radius = s->ao_radius;
        ao.bias = s->ao_bias;
        ao.blocked = counts;
        const NtLaunchInfo &li = ch.li;
        if (fast) {
            NtCompositeDev c;
            scene_dev(s, ds, sw, job.strict, false, c);
            if (int r = nt_launch_ao(li, c, tg, ao)) return launch_failed(r);
        } else {
            const long long rows = (long long)nf * H;
            for (long long r0 = 0; r0 < rows; r0 += chunk_rows) {
                NtAoRays ar{};
                ar.first = r0 * W;
                ar.pixels = std::min(chunk_rows, rows - r0) * W;
                const size_t nr = (size_t)ar.pixels * K;
                char *q0 = rays;
                ar.results = q0; q0 += nr * 16;
                ar.origins = (float *)q0; q0 += nr * n * 4;
                ar.directions = (float *)q0; q0 += nr * n * 4;
                ar.t_near = (float *)q0; q0 += nr * 4;
                ar.t_far = (float *)q0; q0 += nr * 4;
                ar.skip_item = (int *)q0; q0 += nr * 4;
                ar.skip_lane = (int *)q0;
                if (int r = nt_launch_ao_expand(li, tg, ao, ar)) return launch_failed(r);
                NtQuery q{};
                q.count = (int)nr;
                q.origins = ar.origins;
                q.directions = ar.directions;
                q.t_near = ar.t_near;
                q.t_far = ar.t_far;
                q.skip_item = ar.skip_item;
                q.skip_lane = ar.skip_lane;
                q.hits = (void *)ar.results;
                q.abort_word = job.abort_word;
                if (int e = query_enqueue(s, ds, q, job.strict, job.stream)) return e;
                if (int r = nt_launch_ao_reduce(li, tg, ao, ar)) return launch_failed(r);
            }
        }
        if (draw) {
            if (int r = nt_launch_ao_apply(job.stream, (const uint32_t *)base, counts, K, s->ao_strength, nf, ch.ft)) return launch_failed(r);
        }
    }
    return NT_OK;
}

// ---------------------------------------------------------------------------------------------
// outlines (nt_scene_set_outlines; kernels in nt_outline.hpp and nt_var.hip)
// ---------------------------------------------------------------------------------------------

static_assert(NT_OUTLINE_SILHOUETTE == NT_DEV_OUTLINE_SILHOUETTE && NT_OUTLINE_CREASE == NT_DEV_OUTLINE_CREASE &&
              NT_OUTLINE_DEPTH == NT_DEV_OUTLINE_DEPTH, "the mask bits of the ABI are the kernels'");

// The mask bytes of every pixel of the job's frames and, with job.fmt, the render that draws them, per chunk of whole frames.
// Opaque scenes that launch_composite_fixed would give the packet walk take one walk into hit records and outline_shade -- or
// outline_mark_fixed for the mask alone -- (nt_launch_outline*); every other scene the plain fp32 x 3 base frame into scratch (a
// render only), a primary-hit pass with normal_dir into scratch (hits_enqueue: every route of it), outline_mark and
// outline_apply into the caller's image.  Without job.fmt the view is job.view_w x job.view_h, one frame, and the bytes go to
// `mask_dev`, or with `mask_scratch` stay in scratch: *mask_out.  The scratch -- per pixel and frame 16 bytes of record on the
// packet route, 29 + 4 n elsewhere: record, normal row, base frame, mask byte (17 + 4 n for the mask alone, which has no base
// frame) -- sits under the supersampling cap.  Enqueue only.
int enqueue_outlines(nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw, uint8_t *mask_dev, bool mask_scratch,
                     uint8_t **mask_out) {
    const char *noun = "outlines";
    ViewPass vp;
    if (int r = begin_view_pass(s, ds, job, &kViewSettings[VS_OUTLINES], noun, vp)) return r;
    if (vp.nothing) return NT_OK;
    const bool draw = vp.draw;
    const int n = s->n;
    const long long px = vp.px;
    const bool fast = composite_route(s, sw).packet_walk;
    const long long per_frame = fast ? px * (16 + (mask_scratch ? 1 : 0)) : px * (16 + 4 * n + (draw ? 12 : 0) + 1);
    long long chunk_frames;
    if (int r = plan_scratch_frames(vp, job.nframes, noun, nullptr, per_frame, (long long)s->ss_scratch_mb << 20, std::max(sw.chunk_frames, 1),
                                    chunk_frames)) return r;
    Scratch at;
    if (int e = at.open(ds, (size_t)(chunk_frames * per_frame))) return e;
    const size_t fpx = (size_t)chunk_frames * px;
    void *recs = at.take<void>(fpx * 16);
    float *nd = fast ? nullptr : at.take<float>(fpx * n * 4);
    char *base = !fast && draw ? at.take<char>(fpx * 12) : nullptr;
    if (!fast || mask_scratch) mask_dev = mask_dev ? mask_dev : at.take<uint8_t>(fpx);
    if (mask_out) *mask_out = mask_dev;
    NtOutline ol{};
    ol.cc = s->ol_crease_cos * s->ol_crease_cos;
    ol.depth_gap = s->ol_depth_gap;
    for (int k = 0; k < 3; ++k) ol.color[k] = s->ol_color[k];
    ol.strength = s->ol_strength;
    ol.recs = recs;
    ol.normal_dir = nd;
    ol.mask = mask_dev;
    const float *all_cams = nullptr;
    NtCompositeDev c;
    if (fast) {
        if (int e = device_camera(s, ds, job.cam_buf, job.stream, all_cams)) return e;
        scene_dev(s, ds, sw, job.strict, false, c);
    }
    for (int f0 = 0; f0 < job.nframes; f0 += (int)chunk_frames) {
        ViewChunk ch = view_chunk(s, ds, job, sw, vp, f0, chunk_frames);
        ol.nframes = ch.nf;
        if (fast) {
            if (int e = packet_records(s, ds, sw, vp.W, vp.H, ch.nf, recs, ch.li)) return e;
            ol.cams = all_cams + (size_t)f0 * 4 * n;
            if (int r = draw ? nt_launch_outline(ch.li, c, ch.ft, ol) : nt_launch_outline_mask(ch.li, c, ch.ft, ol)) return launch_failed(r);
            continue;
        }
        nt_hit_buffers hb{};
        hb.hits = (nt_ray_hit *)recs;
        hb.normal_dir = nd;
        if (int e = base_and_hits(s, ds, job, vp, ch, base, hb)) return e;
        if (int r = nt_launch_outline_mark(ch.li, ch.ft, ol)) return launch_failed(r);
        if (draw) {
            if (int r = nt_launch_outline_apply(job.stream, (const uint32_t *)base, ol, ch.ft)) return launch_failed(r);
        }
    }
    return NT_OK;
}

// ---------------------------------------------------------------------------------------------
// BoxScene face lines (nt_scene_set_box_lines; kernels in nt_boxhits.hpp and nt_var.hip)
// ---------------------------------------------------------------------------------------------

// the camera of frames [f0, ...) of a job as the BoxScene kernels take it
void box_camera(const nt_scene *s, const float *cam_buf, const float *cam_dots, int f0, NtCamera &cam) {
    cam.buf = cam_buf ? cam_buf + (size_t)f0 * 4 * s->n : nullptr;
    cam.dots = cam_buf ? cam_dots + (size_t)f0 * 4 : nullptr;
    cam.n = s->n;
    if (!cam_buf) pack_camera(s->n, s->origin.data(), s->axes.data(), cam.inl);
    camera_dots(s->n, s->origin.data(), s->axes.data(), cam.odots);
}

// The mask bytes of every pixel of the job's frames or, with job.fmt, the render that draws the lines.  Up to NT_MAX_FIXED_BOX_DIM
// dimensions one kernel does either, its records in LDS, and needs no scratch (but the mask bytes of a host form: `mask_scratch`,
// *mask_out).  At run-time n (and under NTRACER_FORCE_VAR=1) box_hits_var writes 16 bytes a pixel and frame into scratch under
// the supersampling cap and box_lines_var reads them: per chunk of whole frames.  Without job.fmt the view is job.view_w x
// job.view_h, one frame.  Enqueue only.
int enqueue_box_lines(nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw, uint8_t *mask_dev, bool mask_scratch,
                      uint8_t **mask_out) {
    const char *noun = "face lines";
    // (the mask is one sample a pixel of the whole view whatever the supersampling factor says, as nt_box_hits is: the check is the
    // render's alone)
    ViewPass vp;
    if (int r = begin_view_pass(s, ds, job, job.fmt ? &kViewSettings[VS_BOX_LINES] : nullptr, noun, vp)) return r;
    if (vp.nothing) return NT_OK;
    const bool draw = vp.draw;
    const long long px = vp.px;
    const bool var = s->n > NT_MAX_FIXED_BOX_DIM || sw.force_var;
    const long long per_frame = px * ((var ? 16 : 0) + (mask_scratch ? 1 : 0));
    long long chunk_frames = job.nframes;                               // (the fixed-n kernel's frames need no scratch: one chunk)
    void *recs = nullptr;
    if (per_frame > 0) {
        long long fit;
        if (int r = plan_scratch_frames(vp, job.nframes, noun, nullptr, per_frame, (long long)s->ss_scratch_mb << 20, std::max(sw.chunk_frames, 1),
                                        fit)) return r;
        if (var) chunk_frames = fit;
        Scratch at;
        if (int e = at.open(ds, (size_t)(chunk_frames * per_frame))) return e;
        if (var) recs = at.take<void>((size_t)chunk_frames * px * 16);
        if (mask_scratch) mask_dev = at.take<uint8_t>((size_t)chunk_frames * px);
    }
    if (mask_out) *mask_out = mask_dev;
    NtBoxFaces bf{};
    bf.mode = draw ? NT_BOX_FACES_DRAW : NT_BOX_FACES_MASK;
    bf.recs = recs;
    bf.frame_stride = px;
    bf.mask = mask_dev;
    bf.kinds = s->box_lines;
    for (int k = 0; k < 3; ++k) bf.color[k] = s->bl_color[k];
    bf.strength = s->bl_strength;
    for (int f0 = 0; f0 < job.nframes; f0 += (int)chunk_frames) {
        const ViewChunk ch = view_chunk(s, ds, job, sw, vp, f0, chunk_frames);
        NtCamera cam;
        box_camera(s, job.cam_buf, job.cam_dots, f0, cam);
        if (int r = nt_launch_box_faces(ch.li, cam, ch.ft, bf)) return launch_failed(r);
    }
    return NT_OK;
}

// ---------------------------------------------------------------------------------------------
// BoxScene face shading (nt_scene_set_box_shading; kernels in nt_boxshade.hpp and nt_var.hip)
// ---------------------------------------------------------------------------------------------

// The render shaded from the face records, with the face lines on top when that setting is on too.  Up to NT_MAX_FIXED_BOX_DIM
// dimensions one kernel forms the records and draws from them -- in registers, or with lines in LDS -- and needs no scratch.  At
// run-time n (and under NTRACER_FORCE_VAR=1) box_hits_var writes 16 bytes a pixel and frame into scratch under the supersampling
// cap and box_shaded_var reads them: per chunk of whole frames.  Enqueue only.
int enqueue_box_shading(nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw) {
    const char *noun = "face shading";
    // (with face lines on as well their row, nearer the top, answers first: for every way in, as for the entry points)
    if (int r = whole_view_check(s, kViewSettings[VS_BOX_LINES], job.bands, job.stats, job.row_begin, job.row_count, job.fmt->height)) return r;
    ViewPass vp;
    if (int r = begin_view_pass(s, ds, job, &kViewSettings[VS_BOX_SHADING], noun, vp)) return r;
    if (vp.nothing) return NT_OK;
    const int n = s->n;
    const long long px = vp.px;
    const bool var = n > NT_MAX_FIXED_BOX_DIM || sw.force_var;
    long long chunk_frames = job.nframes;                               // (the fixed-n kernels' frames need no scratch: one chunk)
    void *recs = nullptr;
    if (var) {
        if (int r = plan_scratch_frames(vp, job.nframes, noun, nullptr, px * 16, (long long)s->ss_scratch_mb << 20, std::max(sw.chunk_frames, 1),
                                        chunk_frames)) return r;
        Scratch at;
        if (int e = at.open(ds, (size_t)(chunk_frames * px * 16))) return e;
        recs = at.take<void>((size_t)chunk_frames * px * 16);
    }
    NtBoxShade bs{};
    bool gb = true;
    for (int k = 0; k < 2 * n; ++k) {
        float *t = bs.colors + 3 * k;
        t[0] = s->bs_colors ? s->bs_table[3 * k] : 1.0f;
        t[1] = s->bs_colors ? s->bs_table[3 * k + 1] : 0.5f;
        t[2] = s->bs_colors ? s->bs_table[3 * k + 2] : 0.5f;
        gb = gb && t[1] == t[2];
    }
    NtCue &cu = bs.cue;
    bs.cue_on = s->bs_cue ? 1 : 0;
    if (s->bs_cue) {
        cu.fog_near = s->bs_set.fog_near;
        cu.inv_fog = s->bs_inv_fog;
        cu.fog_strength = s->bs_set.fog_strength;
        cu.fog_background = s->bs_set.fog_background != 0;
        cu.tint = s->bs_tint ? 1 : 0;
        cu.tint_lo = s->bs_set.tint_lo;
        cu.inv_tint = s->bs_inv_tint;
        for (int k = 0; k < 3; ++k) {
            cu.fog_color[k] = s->bs_set.fog_color[k];
            cu.tint_color_lo[k] = s->bs_set.tint_color_lo[k];
            cu.tint_color_hi[k] = s->bs_set.tint_color_hi[k];
        }
        for (int k = 0; k < n && s->bs_tint; ++k) cu.tint_axis[k] = s->bs_axis[k];
        gb = gb && cu.fog_color[1] == cu.fog_color[2];
        if (s->bs_tint) gb = gb && cu.tint_color_lo[1] == cu.tint_color_lo[2] && cu.tint_color_hi[1] == cu.tint_color_hi[2];
    }
    bs.gb_equal = gb ? 1 : 0;
    bs.kinds = s->box_lines;
    for (int k = 0; k < 3; ++k) bs.line_color[k] = s->bl_color[k];
    bs.line_strength = s->bl_strength;
    bs.recs = recs;
    bs.frame_stride = px;
    for (int f0 = 0; f0 < job.nframes; f0 += (int)chunk_frames) {
        const ViewChunk ch = view_chunk(s, ds, job, sw, vp, f0, chunk_frames);
        NtCamera cam;
        box_camera(s, job.cam_buf, job.cam_dots, f0, cam);
        if (int r = nt_launch_box_shade(ch.li, cam, ch.ft, bs)) return launch_failed(r);
    }
    return NT_OK;
}

// ---------------------------------------------------------------------------------------------
// depth cues (nt_scene_set_depth_cue; kernels in nt_cue.hpp and nt_var.hip)
// ---------------------------------------------------------------------------------------------

// The factors (f, g) of every pixel of the job's frames or, with job.fmt, the render they shape, per chunk of whole frames.
// Opaque scenes that launch_composite_fixed would give the packet walk take one walk into hit records and cue_shade -- or
// cue_factors_fixed for the factors alone -- (nt_launch_cue*); every other scene the plain fp32 x 3 base frame into scratch (a
// render only), a primary-hit pass without normal rows into scratch (hits_enqueue: every route of it) and cue_apply into the
// caller's image, or cue_factors.  Without job.fmt the view is job.view_w x job.view_h, one frame, and the floats go to
// `factors_dev`, or with `factors_scratch` stay in scratch: *factors_out.  The scratch -- per pixel and frame 16 bytes of record,
// 12 of base frame off the packet walk, 8 of factors for the host form -- sits under the supersampling cap.  Enqueue only.
int enqueue_cue(nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw, float *factors_dev, bool factors_scratch,
                float **factors_out) {
    const char *noun = "depth cue";
    ViewPass vp;
    if (int r = begin_view_pass(s, ds, job, &kViewSettings[VS_CUE], noun, vp)) return r;
    if (vp.nothing) return NT_OK;
    const bool draw = vp.draw;
    const int n = s->n;
    const long long px = vp.px;
    const bool fast = composite_route(s, sw).packet_walk;
    const long long per_frame = px * (16 + (!fast && draw ? 12 : 0) + (factors_scratch ? 8 : 0));
    long long chunk_frames;
    if (int r = plan_scratch_frames(vp, job.nframes, noun, nullptr, per_frame, (long long)s->ss_scratch_mb << 20, std::max(sw.chunk_frames, 1),
                                    chunk_frames)) return r;
    Scratch at;
    if (int e = at.open(ds, (size_t)(chunk_frames * per_frame))) return e;
    const size_t fpx = (size_t)chunk_frames * px;
    void *recs = at.take<void>(fpx * 16);
    char *base = !fast && draw ? at.take<char>(fpx * 12) : nullptr;
    if (factors_scratch) factors_dev = at.take<float>(fpx * 8);
    if (factors_out) *factors_out = factors_dev;
    NtCue cu{};
    cu.recs = recs;
    cu.fog_near = s->cue_set.fog_near;
    cu.inv_fog = s->cue_inv_fog;
    cu.fog_strength = s->cue_set.fog_strength;
    cu.fog_background = s->cue_set.fog_background != 0;
    cu.tint = s->cue_tint ? 1 : 0;
    cu.tint_lo = s->cue_set.tint_lo;
    cu.inv_tint = s->cue_inv_tint;
    for (int k = 0; k < 3; ++k) {
        cu.fog_color[k] = s->cue_set.fog_color[k];
        cu.tint_color_lo[k] = s->cue_set.tint_color_lo[k];
        cu.tint_color_hi[k] = s->cue_set.tint_color_hi[k];
    }
    for (int k = 0; k < n && s->cue_tint; ++k) cu.tint_axis[k] = s->cue_axis[k];
    cu.factors = factors_dev;
    const float *all_cams = nullptr;
    NtCompositeDev c;
    if (fast) {
        if (int e = device_camera(s, ds, job.cam_buf, job.stream, all_cams)) return e;
        scene_dev(s, ds, sw, job.strict, false, c);
    }
    for (int f0 = 0; f0 < job.nframes; f0 += (int)chunk_frames) {
        ViewChunk ch = view_chunk(s, ds, job, sw, vp, f0, chunk_frames);
        cu.nframes = ch.nf;
        if (fast) {
            if (int e = packet_records(s, ds, sw, vp.W, vp.H, ch.nf, recs, ch.li)) return e;
            cu.cams = all_cams + (size_t)f0 * 4 * n;
            if (int r = draw ? nt_launch_cue(ch.li, c, ch.ft, cu) : nt_launch_cue_factors_fixed(ch.li, c, ch.ft, cu)) return launch_failed(r);
            continue;
        }
        nt_hit_buffers hb{};
        hb.hits = (nt_ray_hit *)recs;
        if (int e = base_and_hits(s, ds, job, vp, ch, base, hb)) return e;
        cu.cams = ch.cams ? ch.cams : (const float *)ds->cams.p;        // (hits_enqueue has put the scene's own camera there)
        if (int r = draw ? nt_launch_cue_apply(ch.li, (const uint32_t *)base, cu, ch.ft) : nt_launch_cue_factors(ch.li, ch.ft, cu)) return launch_failed(r);
    }
    return NT_OK;
}

// ---------------------------------------------------------------------------------------------
// clip planes (nt_scene_set_clip_planes; kernels in nt_clip.hpp and nt_var.hip)
// ---------------------------------------------------------------------------------------------

// what the entry points that do not honour the setting say while it is on
int clip_refuses(const nt_scene *s, const char *what) {
    if (s && s->composite && s->clip_count > 0) return fail(NT_E_UNSUPPORTED, "clip planes are set: %s is not available under them", what);
    return NT_OK;
}

// The frames of a render under the planes.  Opaque scenes that launch_composite_fixed would give the packet walk take one
// clipped walk into hit records and clip_shade; every other scene the run-time-n kernels with the planes in the scene they
// see, whatever its dimension -- with the `checked` columns and ray_color frames of the faithful walks.  Enqueue only.
int enqueue_clip(nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw) {
    const int W = job.fmt->width, H = job.fmt->height;
    if (int r = whole_view_check(s, kViewSettings[VS_CLIP], job.bands, job.stats, job.row_begin, job.row_count, H)) return r;
    if (job.fmt->bpp == 0) return NT_OK;                                // nothing to draw
    NtTarget tg;
    if (int r = fill_target(s, ds, job, tg)) return r;
    NtCompositeDev c;
    scene_dev(s, ds, sw, job.strict, false, c);
    const CompositeRoute rt = composite_route(s, sw);
    NtLaunchInfo li = launch_info(s, ds, sw, job.nframes, job.stream);
    NtCamera cam;
    cam.n = s->n;
    cam.dots = job.cam_dots;
    pack_camera(s->n, s->origin.data(), s->axes.data(), cam.inl);
    camera_dots(s->n, s->origin.data(), s->axes.data(), cam.odots);
    if (int e = device_camera(s, ds, job.cam_buf, job.stream, cam.buf)) return e;
    NtClip cl{};
    cl.planes = (const float *)ds->clip.p;
    cl.count = s->clip_count;
    cl.cams = cam.buf;
    cl.nframes = job.nframes;
    if (rt.packet_walk) {
        // the packet walk's plane numerators, record scratch and quad order, as plan_composite hands them over
        if (int e = packet_records(s, ds, sw, W, H, job.nframes, nullptr, li)) return e;
        if (int e = hit_record_scratch(ds, sw, (size_t)16 * W * H, job.nframes, li)) return e;
    } else if (rt.faithful) {
        const long long tiles = (long long)((W + 7) / 8) * ((H + 7) / 8) * job.nframes;
        long long blocks = std::min<long long>(std::max<long long>(tiles, 1), 8192);
        if (int e = checked_scratch(s, ds, sw, c, 64, blocks, 64, rt.frame_stack, (long long)512 << 20)) return e;
    }
    if (int r = nt_launch_clip(li, cam, c, tg, cl, true)) return launch_failed(r);
    return NT_OK;
}

// ---------------------------------------------------------------------------------------------
// renders through a lens (nt_scene_set_lens; kernels in nt_lens.hpp and nt_var.hip)
// ---------------------------------------------------------------------------------------------

// What a lens render refuses, checked by the entry points before a device is touched (and by enqueue_lens again, for every
// way in): the lens is of the image's size, and nothing is asked that the lens routes do not do yet
int lens_check(const nt_scene *s, int width, int height, const Bands &b, bool stats, bool probes) {
    if (!s->lens) return NT_OK;
    if (probes) return fail(NT_E_UNSUPPORTED, "nt_colors_at / nt_calculate_color are not available while a lens is set (nt_ray_colors takes any ray)");
    if (s->lens->width != width || s->lens->height != height)
        return fail(NT_E_INVALID, "the lens is for %d x %d pixels, the render is of %d x %d", s->lens->width, s->lens->height, width, height);
    if (s->supersampling > 1) return fail(NT_E_UNSUPPORTED, "supersampling %d is not available while a lens is set", s->supersampling);
    if (b.world > 1) return fail(NT_E_UNSUPPORTED, "row bands (band_world %d) are not available while a lens is set", b.world);
    if (stats) return fail(NT_E_UNSUPPORTED, "collect_stats is not available while a lens is set");
    return NT_OK;
}

// the lens's table on the device of `ds`: uploaded on first use there and kept
int lens_table(NtLensData *ld, DeviceState *ds, const float *&dev_ptr) {
    std::lock_guard<std::mutex> g(ld->mu);
    auto it = ld->dev.find(ds->device);
    if (it == ld->dev.end()) {
        void *p = nullptr;
        const size_t bytes = ld->coeffs.size() * sizeof(float);
        HIP_TRY(hipMalloc(&p, bytes));
        if (hipMemcpy(p, ld->coeffs.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(p);
            return fail(NT_E_DEVICE, "lens table upload failed");
        }
        it = ld->dev.emplace(ds->device, p).first;
    }
    dev_ptr = (const float *)it->second;
    return NT_OK;
}

int rays_image_target(const nt_scene *s, DeviceState *ds, const Format *fmt, void *dest_dev, const int *abort_word, hipStream_t stream, NtTarget &tg);
int rays_enqueue(nt_scene *s, DeviceState *ds, const NtRayJob &job, float *rgb, const Format *fmt, void *dest_dev, bool strict,
                 const int *abort_word, hipStream_t stream);

// the cap of the ray route's direction scratch, a device: the default of the supersampling scratch
const long long kLensDirsCap = (long long)1024 << 20;

// A render job with a lens set.  Opaque composite scenes that launch_composite_fixed would give the packet walk keep it
// (nt_launch_lens: the LENS instantiation of the walk into hit records, then lens_shade); every other scene -- transparent
// materials, the reference's normals for Solids, run-time n, NTRACER_COMPOSITE_KERNEL set, a tree deeper than the packet
// stack, BoxScene -- is rendered frame by frame by the ray-colour kernels (rays_enqueue) from directions that lens_expand
// writes for a band of whole rows at a time, and lens_mask_fill paints the masked pixels afterwards.  Enqueue only.
int enqueue_lens(nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw) {
    NtLensData *ld = s->lens.get();
    if (int r = lens_check(s, job.colors_out ? job.view_w : job.fmt->width, job.colors_out ? job.view_h : job.fmt->height, job.bands, job.stats,
                           job.colors_out != nullptr)) return r;
    const Format &f = *job.fmt;
    if (job.row_begin != 0 || job.row_count != f.height) return fail(NT_E_UNSUPPORTED, "a row range is not available while a lens is set");
    if (f.bpp == 0) return NT_OK;                                       // nothing to draw
    const float *table = nullptr;
    if (int r = lens_table(ld, ds, table)) return r;
    const int n = s->n;
    const float *cams;
    if (int e = device_camera(s, ds, job.cam_buf, job.stream, cams)) return e;
    NtLaunchInfo li = launch_info(s, ds, sw, job.nframes, job.stream);
    if (s->composite && composite_route(s, sw).packet_walk) {
        FrameJob pj = job;
        pj.cam_buf = cams;
        NtTarget tg;
        if (int r = fill_target(s, ds, pj, tg)) return r;
        NtCamera cam{};
        cam.buf = cams;
        cam.n = n;
        NtCompositeDev c;
        if (int e = plan_composite(s, ds, pj, sw, tg, cam, li, c)) return e;      // (the counter, numerators, tile order)
        // the records between the walk and the shading pass, for every scene: the two-pass route's own scratch and rule
        if (int e = hit_record_scratch(ds, sw, (size_t)16 * f.width * f.height, job.nframes, li)) return e;
        NtLens ln{};
        ln.table = table;
        ln.cams = cams;
        if (int r = nt_launch_lens(li, c, tg, ln)) return launch_failed(r);
        return NT_OK;
    }
    // the ray route: bands of whole rows whose directions fit the cap
    const long long row_bytes = (long long)f.width * n * sizeof(float);
    const int band = (int)std::max<long long>(1, std::min<long long>(f.height, kLensDirsCap / row_bytes));
    if (int e = ds->lens_dirs.ensure((size_t)band * row_bytes)) return e;
    for (int fr = 0; fr < job.nframes; ++fr) {
        const float *cam = cams + (size_t)fr * 4 * n;
        for (int r0 = 0; r0 < f.height; r0 += band) {
            const int rows = std::min(band, f.height - r0);
            const long long first = (long long)r0 * f.width, count = (long long)rows * f.width;
            void *dest = (char *)job.dest_dev + (size_t)fr * job.frame_stride + (size_t)r0 * f.pitch;
            if (int r = nt_launch_lens_expand(li, table, cam, first, count, (float *)ds->lens_dirs.p)) return launch_failed(r);
            NtRayJob rj{};
            rj.count = (int)count;
            rj.shared_origin = 1;
            rj.origins = cam;                                           // (the camera's first row)
            rj.directions = (const float *)ds->lens_dirs.p;
            if (int e = rays_enqueue(s, ds, rj, nullptr, &f, dest, job.strict, job.abort_word, job.stream)) return e;
            if (ld->masked) {
                NtTarget tg;
                if (int e = rays_image_target(s, ds, &f, dest, job.abort_word, job.stream, tg)) return e;
                if (int r = nt_launch_lens_mask(li, table, first, count, tg)) return launch_failed(r);
            }
        }
    }
    return NT_OK;
}

// ---------------------------------------------------------------------------------------------
// renders under the parallel projection (nt_scene_set_parallel; kernels in nt_parallel.hpp and nt_var.hip)
// ---------------------------------------------------------------------------------------------

// What a parallel render refuses, checked by the entry points before a device is touched (and by enqueue_parallel again, for
// every way in), as lens_check does it
int parallel_check(const nt_scene *s, const Bands &b, bool stats, bool probes) {
    if (!(s->parallel > 0.0f)) return NT_OK;
    if (probes) return fail(NT_E_UNSUPPORTED, "nt_colors_at / nt_calculate_color are not available while the parallel projection is set (nt_ray_colors takes any ray)");
    if (s->supersampling > 1) return fail(NT_E_UNSUPPORTED, "supersampling %d is not available while the parallel projection is set", s->supersampling);
    if (b.world > 1) return fail(NT_E_UNSUPPORTED, "row bands (band_world %d) are not available while the parallel projection is set", b.world);
    if (stats) return fail(NT_E_UNSUPPORTED, "collect_stats is not available while the parallel projection is set");
    return NT_OK;
}

// A render job with the parallel projection set: enqueue_lens's two routes.  Opaque composite scenes that
// launch_composite_fixed would give the packet walk get the shared-direction walk (nt_launch_parallel: parallel_packet into hit
// records, then parallel_shade); every other scene is rendered frame by frame by the ray-colour kernels (rays_enqueue, one
// origin a ray) from what parallel_expand writes for a band of whole rows at a time.  Enqueue only.
int enqueue_parallel(nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw) {
    if (int r = parallel_check(s, job.bands, job.stats, job.colors_out != nullptr)) return r;
    const Format &f = *job.fmt;
    if (job.row_begin != 0 || job.row_count != f.height) return fail(NT_E_UNSUPPORTED, "a row range is not available while the parallel projection is set");
    if (f.bpp == 0) return NT_OK;                                       // nothing to draw
    const int n = s->n;
    const float *cams;
    if (int e = device_camera(s, ds, job.cam_buf, job.stream, cams)) return e;
    NtLaunchInfo li = launch_info(s, ds, sw, job.nframes, job.stream);
    const float half_w = float(f.width) / float(2), half_h = float(f.height) / float(2);
    const float k = s->parallel / half_w;                               // (once, in fp32, as fill_view forms fovI)
    if (s->composite && composite_route(s, sw).packet_walk) {
        FrameJob pj = job;
        pj.cam_buf = cams;
        NtTarget tg;
        if (int r = fill_target(s, ds, pj, tg)) return r;
        tg.fovI = k;
        NtCamera cam{};
        cam.buf = cams;
        cam.n = n;
        NtCompositeDev c;
        // (the counter and the tile order; plan_composite also ensures the numerator scratch, which this walk never reads)
        if (int e = plan_composite(s, ds, pj, sw, tg, cam, li, c)) return e;
        // the records between the walk and the shading pass, for every scene: the two-pass route's own scratch and rule
        if (int e = hit_record_scratch(ds, sw, (size_t)16 * f.width * f.height, job.nframes, li)) return e;
        NtParallel pl{};
        pl.cams = cams;
        if (int r = nt_launch_parallel(li, c, tg, pl)) return launch_failed(r);
        return NT_OK;
    }
    // the ray route: bands of whole rows whose origins and directions fit the cap
    const long long row_bytes = (long long)f.width * n * sizeof(float) * 2;
    const int band = (int)std::max<long long>(1, std::min<long long>(f.height, kLensDirsCap / row_bytes));
    if (int e = ds->lens_dirs.ensure((size_t)band * row_bytes)) return e;
    for (int fr = 0; fr < job.nframes; ++fr) {
        const float *cam = cams + (size_t)fr * 4 * n;
        for (int r0 = 0; r0 < f.height; r0 += band) {
            const int rows = std::min(band, f.height - r0);
            const long long first = (long long)r0 * f.width, count = (long long)rows * f.width;
            void *dest = (char *)job.dest_dev + (size_t)fr * job.frame_stride + (size_t)r0 * f.pitch;
            float *scratch = (float *)ds->lens_dirs.p;
            if (int r = nt_launch_parallel_expand(li, cam, f.width, k, half_w, half_h, first, count, scratch)) return launch_failed(r);
            NtRayJob rj{};
            rj.count = (int)count;
            rj.shared_origin = 0;
            rj.origins = scratch;
            rj.directions = scratch + (size_t)count * n;
            if (int e = rays_enqueue(s, ds, rj, nullptr, &f, dest, job.strict, job.abort_word, job.stream)) return e;
        }
    }
    return NT_OK;
}

// ---------------------------------------------------------------------------------------------
// view stacks (nt_scene_set_view_stack; kernels in nt_stack.hpp)
// ---------------------------------------------------------------------------------------------

// the K cameras the rule gives for one camera (ntracer_hip.h), operation by operation: stack_cameras is its copy on the device
void stack_cameras_host(const nt_scene *s, const float *origin, const float *axes, float *origins_out, float *axes_out) {
    const int n = s->n;
    for (int k = 0; k < s->stack_count; ++k) {
        const float *e = s->stack_offsets.data() + (size_t)k * n;
        float *o = origins_out + (size_t)k * n, *a = axes_out + (size_t)k * n * n;
        std::memcpy(a, axes, sizeof(float) * n * n);
        for (int j = 0; j < n; ++j) {
            float sj = e[0] * axes[j];
            for (int i = 1; i < n; ++i) sj = sj + (e[i] * axes[(size_t)i * n + j]);
            o[j] = origin[j] + sj;
            a[2 * n + j] = axes[2 * n + j] - (sj * s->stack_r);
        }
    }
}

// A render with a view stack on.  stack_cameras expands the job's cameras -- the scene's own, which goes to device memory here
// with all its axes, a `frames` array or a camera table -- into K sample cameras a frame.  BoxScene up to NT_MAX_FIXED_BOX_DIM
// dimensions: box_stack<N>, one launch, no scratch (nt_scene_set_view_stack_route and NTRACER_FORCE_VAR=1 send it the other way).
// Every other scene, the frames route: the plain render of the sample cameras in the plain fp32 x 3 format into scratch under the
// supersampling cap -- every route of a plain render comes with it -- and stack_resolve into the caller's image, per chunk of
// whole frames; when the K samples of one frame do not fit, frame by frame in chunks of consecutive k through an fp32 accumulator
// frame, the sum still in the order of k.  Enqueue only.
int enqueue_stack(nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw) {
    const char *noun = "a view stack";
    ViewPass vp;
    if (int r = begin_view_pass(s, ds, job, &kViewSettings[VS_STACK], noun, vp)) return r;
    if (vp.nothing) return NT_OK;
    const int n = s->n, K = s->stack_count, F = job.nframes;
    const long long px = vp.px;
    const bool fused = !s->composite && n <= NT_MAX_FIXED_BOX_DIM && !sw.force_var && s->stack_route != NT_STACK_ROUTE_FRAMES;
    // the frames route's plan, before anything is launched
    const long long cap = (long long)s->ss_scratch_mb << 20, frame_bytes = px * 12;
    long long chunk_frames = F, chunk_k = K;
    bool through_acc = false;
    if (!fused) {
        if (K * frame_bytes <= cap) {
            // whole frames, K samples each, as the other passes plan them; a launch's grid holds 65535 frames in its z, and the
            // kernels' pixel indices reach vp.px_limit over all K samples of a chunk's frames
            const long long limit = std::min<long long>(std::min<long long>(65535 / K, std::max(sw.chunk_frames, 1)), std::max<long long>(1, vp.px_limit / (px * K)));
            if (int r = plan_scratch_frames(vp, F, noun, "the samples of one frame", K * frame_bytes, cap, limit, chunk_frames)) return r;
        } else {
            // one frame at a time, its samples in chunks of consecutive k behind an accumulator frame: the helper's refusal when
            // not even the accumulator and one sample fit
            if (int r = plan_scratch_frames(vp, 1, noun, "the accumulator and one sample", 2 * frame_bytes, cap, 1, chunk_frames)) return r;
            through_acc = true;
            chunk_k = std::min<long long>(std::min<long long>(K, cap / frame_bytes - 1), std::max<long long>(1, vp.px_limit / px));
        }
    }
    // the sample cameras
    const size_t cam_floats = (size_t)F * K * 4 * n;
    if (int e = ds->stack_cams.ensure((cam_floats + (size_t)F * K * 4) * sizeof(float))) return e;
    float *scams = (float *)ds->stack_cams.p, *sdots = scams + cam_floats;
    const float *cams = job.cam_buf, *axes = job.cam_axes;
    if (!cams) {
        float packed[4 * NT_DEV_MAX_DIM];
        pack_camera(n, s->origin.data(), s->axes.data(), packed);
        if (int e = ds->stack_in.ensure(sizeof(float) * (4 * n + n * n))) return e;
        float *in = (float *)ds->stack_in.p;
        HIP_TRY(hipMemcpyAsync(in, packed, sizeof(float) * 4 * n, hipMemcpyHostToDevice, job.stream));
        HIP_TRY(hipMemcpyAsync(in + 4 * n, s->axes.data(), sizeof(float) * n * n, hipMemcpyHostToDevice, job.stream));
        cams = in;
        axes = in + 4 * n;
    } else if (!axes) {
        return fail(NT_E_INVALID, "internal: a view stack render whose cameras came without their axes");
    }
    if (int r = nt_launch_stack_cameras(job.stream, n, F, cams, axes, (const float *)ds->stack_offsets.p, K, s->stack_r, scams, sdots)) return launch_failed(r);
    NtStack sk{};
    sk.count = K;
    sk.cams = scams;
    sk.dots = sdots;
    for (int k = 0; k < 3 * K; ++k) sk.weights[k] = s->stack_weights[k];
    if (fused) {
        const NtLaunchInfo li = launch_info(s, ds, sw, F, job.stream);
        if (int r = nt_launch_box_stack(li, vp.tg, sk)) return launch_failed(r);
        return NT_OK;
    }
    Scratch at;
    if (int e = at.open(ds, (size_t)(chunk_frames * chunk_k * frame_bytes + (through_acc ? frame_bytes : 0)))) return e;
    char *samples = at.take<char>((size_t)(chunk_frames * chunk_k * frame_bytes));
    float *acc = through_acc ? at.take<float>((size_t)frame_bytes) : nullptr;
    for (int f0 = 0; f0 < F; f0 += (int)chunk_frames) {
        const int nf = (int)std::min<long long>(chunk_frames, F - f0);
        for (int k0 = 0; k0 < K; k0 += (int)chunk_k) {
            const int kc = (int)std::min<long long>(chunk_k, K - k0);
            // the plain frames of sample cameras [f0 * K + k0, ... + nf * kc): consecutive, as a chunk of k is of one frame alone
            FrameJob bj = base_frame_job(s, job, vp.bf, 0, nf * kc, samples, (size_t)frame_bytes);
            bj.cam_buf = scams + ((size_t)f0 * K + k0) * 4 * n;
            bj.cam_dots = sdots + ((size_t)f0 * K + k0) * 4;
            bj.cam_span = nullptr;
            bj.cam_axes = nullptr;
            if (int e = enqueue(s, ds, bj)) return e;
            NtStackChunk ch{};
            ch.samples = (const uint32_t *)samples;
            ch.k0 = k0;
            ch.kc = kc;
            ch.nframes = nf;
            ch.acc_in = through_acc && k0 > 0 ? acc : nullptr;
            ch.acc_out = through_acc && k0 + kc < K ? acc : nullptr;
            NtTarget ft = vp.tg;
            ft.dest = vp.tg.dest + (long long)f0 * vp.tg.frame_stride;
            if (int r = nt_launch_stack_resolve(job.stream, sk, ch, ft)) return launch_failed(r);
        }
    }
    return NT_OK;
}

// ---------------------------------------------------------------------------------------------
// X-ray views (nt_scene_set_xray, nt_crossing_counts; kernels in nt_xray.hpp and nt_var.hip)
// ---------------------------------------------------------------------------------------------

static_assert(NT_XRAY_PACKET_ITEMS == NT_DEV_XRAY_PACKET_ITEMS, "the packet walk's item limit of the ABI is the launcher's");

// what the entry points that do not honour the setting say while it is on
int xray_refuses(const nt_scene *s, const char *what) {
    if (s && s->composite && s->xray) return fail(NT_E_UNSUPPORTED, "X-ray is on: %s is not available under it", what);
    return NT_OK;
}

// The frames of a render with the setting on, or without job.fmt the counts of one view of job.view_w x job.view_h into
// `counts_dev` -- with that nullptr into scratch under the supersampling cap: *counts_out.  One launch either way: the packet
// walk where nt_xray_packet_route says so, with its numerators and quad order, else xray_var with the `checked` columns of as
// many blocks as fit 512 MB.  Enqueue only.
int enqueue_xray(nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw, int *counts_dev, int **counts_out) {
    const char *noun = "X-ray";
    ViewPass vp;
    if (int r = begin_view_pass(s, ds, job, job.fmt ? &kViewSettings[VS_XRAY] : nullptr, noun, vp)) return r;
    if (vp.nothing) return NT_OK;
    const bool draw = vp.draw;
    if (!draw && !counts_dev) {
        long long chunk_frames;
        if (int r = plan_scratch_frames(vp, 1, noun, "the counts of one frame", vp.px * 4, (long long)s->ss_scratch_mb << 20, LLONG_MAX, chunk_frames)) return r;
        Scratch at;
        if (int e = at.open(ds, (size_t)vp.px * 4)) return e;
        counts_dev = at.take<int>((size_t)vp.px * 4);
    }
    if (counts_out) *counts_out = counts_dev;
    NtCompositeDev c;
    scene_dev(s, ds, sw, job.strict, false, c);
    NtLaunchInfo li = launch_info(s, ds, sw, job.nframes, job.stream);
    NtXray xr{};
    if (int e = device_camera(s, ds, job.cam_buf, job.stream, xr.cams)) return e;
    xr.trans = draw ? (const float *)ds->xr_table.p : nullptr;
    xr.live = (const uint8_t *)ds->live.p;
    xr.counts = draw ? nullptr : counts_dev;
    if (nt_xray_packet_route(li, c)) {
        if (int e = packet_records(s, ds, sw, vp.W, vp.H, job.nframes, nullptr, li)) return e;
    } else {
        const long long tiles = (long long)((vp.W + 7) / 8) * ((vp.H + 7) / 8) * job.nframes;
        long long blocks = std::min<long long>(std::max<long long>(tiles, 1), 8192);
        if (int e = checked_scratch(s, ds, sw, c, 64, blocks, 1, 0, (long long)512 << 20)) return e;
    }
    if (int r = nt_launch_xray(li, c, vp.tg, xr)) return launch_failed(r);
    return NT_OK;
}

// ---------------------------------------------------------------------------------------------
// hit layers (nt_hit_layers; kernels in nt_layers.hpp and nt_var.hip)
// ---------------------------------------------------------------------------------------------

static_assert(NT_LAYERS_MAX == NT_DEV_LAYERS_MAX, "the layer limit of the ABI is the launcher's");

// The job.layers planes of records of one view of job.view_w x job.view_h into `recs_dev` -- with that nullptr into scratch under
// the supersampling cap: *recs_out.  No view setting plays a part.  One launch, on enqueue_xray's routes: the packet walk where
// nt_xray_packet_route says so, with its numerators and quad order, else layers_var with the `checked` columns of as many blocks
// as fit 512 MB.  Enqueue only.
int enqueue_layers(nt_scene *s, DeviceState *ds, const FrameJob &job, const RenderSwitches &sw, nt_ray_hit *recs_dev, nt_ray_hit **recs_out) {
    const char *noun = "the hit layers";
    ViewPass vp;
    if (int r = begin_view_pass(s, ds, job, nullptr, noun, vp)) return r;
    const size_t bytes = (size_t)vp.px * job.layers * sizeof(nt_ray_hit);
    if (!recs_dev) {
        long long chunk_frames;
        if (int r = plan_scratch_frames(vp, 1, noun, "the records of the view", (long long)bytes, (long long)s->ss_scratch_mb << 20, LLONG_MAX, chunk_frames)) return r;
        Scratch at;
        if (int e = at.open(ds, bytes)) return e;
        recs_dev = at.take<nt_ray_hit>(bytes);
    }
    if (recs_out) *recs_out = recs_dev;
    NtCompositeDev c;
    scene_dev(s, ds, sw, job.strict, false, c);
    NtLaunchInfo li = launch_info(s, ds, sw, 1, job.stream);
    NtLayers ly{};
    if (int e = device_camera(s, ds, job.cam_buf, job.stream, ly.cams)) return e;
    ly.live = (const uint8_t *)ds->live.p;
    ly.records = recs_dev;
    ly.layers = job.layers;
    if (nt_xray_packet_route(li, c)) {
        if (int e = packet_records(s, ds, sw, vp.W, vp.H, 1, nullptr, li)) return e;
    } else {
        const long long tiles = (long long)((vp.W + 7) / 8) * ((vp.H + 7) / 8);
        long long blocks = std::min<long long>(std::max<long long>(tiles, 1), 8192);
        if (int e = checked_scratch(s, ds, sw, c, 64, blocks, 1, 0, (long long)512 << 20)) return e;
    }
    if (int r = nt_launch_layers(li, c, vp.tg, ly)) return launch_failed(r);
    return NT_OK;
}

int enqueue(nt_scene *s, DeviceState *ds, const FrameJob &job_in) {
    const RenderSwitches sw = read_switches();
    FrameJob job = job_in;
    // the caller's own render: not the probes, nor a stage that another route has sent back here
    const bool whole = !job.colors_out && !job.samples_pass && !job.counters_pass;
    // the whole-view settings, one line a row of kViewSettings and in its order: the first that is on draws, as the first that is
    // on refuses (tests/test_view_setting_refusals.py holds the refusals to that order, the settings' host tests these lines)
    if (s->xray && s->composite && whole) return enqueue_xray(s, ds, job, sw, nullptr, nullptr);
    if (s->stack_count > 0 && whole) return enqueue_stack(s, ds, job, sw);
    if (s->clip_count > 0 && s->composite && whole) return enqueue_clip(s, ds, job, sw);
    if (s->cue && s->composite && whole) return enqueue_cue(s, ds, job, sw, nullptr, false, nullptr);
    if (s->outlines && s->composite && whole) return enqueue_outlines(s, ds, job, sw, nullptr, false, nullptr);
    if (s->ao_count > 0 && s->composite && whole) return enqueue_ao(s, ds, job, sw, nullptr, nullptr);
    if (s->box_shading && !s->composite && whole) return enqueue_box_shading(s, ds, job, sw);     // (and the lines, when both are on)
    if (s->box_lines && !s->composite && whole) return enqueue_box_lines(s, ds, job, sw, nullptr, false, nullptr);
    if (s->lens) return enqueue_lens(s, ds, job, sw);
    if (s->parallel > 0.0f) return enqueue_parallel(s, ds, job, sw);
    if (s->supersampling > 1 && s->adaptive && whole) return enqueue_adaptive(s, ds, job, sw, nullptr, false, nullptr);
    if (s->supersampling > 1 && whole) return enqueue_supersampled(s, ds, job);
    if (s->composite && job.stats && !job.counters_pass && !job.colors_out) {
        // Scenes with transparent materials or Solids are drawn by the kernels that reproduce the reference's o_hit.normal
        // handling (below), which keep no counters.  Asking for statistics must not change the pixels: the frame is drawn as
        // always, and the counters come from a launch of their own -- the counting kernel (a hit keeps the normal of what
        // was hit, 16-slot mailbox) into a scratch frame.  They describe THAT traversal: the same tree and cells, a few
        // repeated tests after mailbox evictions.  Transparent materials have no counting kernel at all: refused.
        if (s->n > NT_MAX_FIXED_DIM) return fail(NT_E_UNSUPPORTED, "collect_stats is not available above %d dimensions (the run-time-n kernels keep no counters)", NT_MAX_FIXED_DIM);
        if (!s->all_opaque)
            return fail(NT_E_UNSUPPORTED, "collect_stats is not available for scenes with transparent materials (their kernels keep no counters)");
        if (s->n_solids > 0 && !sw.clean_normals) {
            const size_t bytes = (size_t)job.fmt->pitch * (size_t)(job.bands.compact ? job.bands.owned_rows : job.fmt->height);
            if (int e = ds->stats_frame.ensure(std::max<size_t>(bytes, 16))) return e;
            FrameJob cj = job;
            cj.counters_pass = true;
            cj.dest_dev = ds->stats_frame.p;
            cj.frame_stride = 0;
            if (job.nframes > 1) return fail(NT_E_UNSUPPORTED, "collect_stats on a multi-frame launch is not available for scenes with Solids");
            if (int e = enqueue(s, ds, cj)) return e;
            job.stats = false;
        }
    }
    NtTarget tg;
    if (int r = fill_target(s, ds, job, tg)) return r;
    if (!job.colors_out && (tg.row_count <= 0 || tg.bpp == 0)) return NT_OK;      // nothing to draw
    NtCamera cam;
    cam.buf = job.cam_buf;
    cam.dots = job.cam_dots;
    cam.span = job.cam_buf ? job.cam_span : nullptr;
    cam.n = s->n;
    if (!job.cam_buf) pack_camera(s->n, s->origin.data(), s->axes.data(), cam.inl);
    camera_dots(s->n, s->origin.data(), s->axes.data(), cam.odots);
    NtLaunchInfo li = launch_info(s, ds, sw, job.nframes, job.stream);
    int r;
    if (s->composite) {
        NtCompositeDev c;
        if (int e = plan_composite(s, ds, job, sw, tg, cam, li, c)) return e;
        r = nt_launch_composite(li, cam, c, tg);
    } else {
        if (int e = plan_box(s, ds, job, sw, tg, li)) return e;
        r = nt_launch_box(li, cam, tg);
    }
    if (r) return launch_failed(r);
    return NT_OK;
}

int prepare_stats(DeviceState *ds, hipStream_t st, bool on) {
    if (!on) return NT_OK;
    if (int r = ds->stats.ensure(8 * sizeof(unsigned long long))) return r;
    HIP_TRY(hipMemsetAsync(ds->stats.p, 0, 8 * sizeof(unsigned long long), st));
    return NT_OK;
}

// what the scene's settings refuse of a render, in the order the render entry points say it, before they touch a device
int render_checks(const nt_scene *s, const Format &f, const Bands &b, bool stats) {
    for (const ViewSetting &row : kViewSettings) {
        if (int r = whole_view_check(s, row, b, stats, 0, b.owned_rows, f.height)) return r;
    }
    if (int r = lens_check(s, f.width, f.height, b, stats, false)) return r;
    if (int r = parallel_check(s, b, stats, false)) return r;
    return adaptive_check(s, b, stats);
}

// What a job takes from the caller's options.  abort_device and overlapped are the device forms' (`device_form`): a host form
// has its own abort word or none, and waits for its launch.
void job_options(FrameJob &job, const nt_render_opts *opts, bool device_form) {
    job.strict = opts && opts->strict_reference;
    if (!device_form) return;
    job.abort_word = opts ? (const int *)opts->abort_device : nullptr;
    job.overlapped = opts ? opts->overlapped : 0;
}

// the job of a render entry point: the owned rows of `nframes` whole images at `dest_dev`, `frame_stride` bytes apart
FrameJob render_job(const Format &f, const Bands &b, void *dest_dev, size_t frame_stride, int nframes, hipStream_t stream, bool stats,
                    const nt_render_opts *opts, bool device_form) {
    FrameJob job{};
    job.fmt = &f;
    job.bands = b;
    job.dest_dev = dest_dev;
    job.frame_stride = frame_stride;
    job.nframes = nframes;
    job.stream = stream;
    job.stats = stats;
    job_options(job, opts, device_form);
    job.row_begin = 0;
    job.row_count = b.owned_rows;
    return job;
}

// ... and of the entry points that draw nothing (nt_adaptive_mask, nt_ambient_occlusion, nt_outline_mask,
// nt_depth_cue_factors, nt_box_line_mask): one whole view of w x h
FrameJob view_job(int w, int h, hipStream_t stream, const nt_render_opts *opts, bool device_form) {
    FrameJob job{};
    job.nframes = 1;
    job.stream = stream;
    job_options(job, opts, device_form);
    job.view_w = w;
    job.view_h = h;
    job.row_count = h;
    job.bands.owned_rows = h;
    return job;
}

int validate_desc(const nt_scene_desc *d) {
    if (!d) return fail(NT_E_INVALID, "scene description is NULL");
    const int n = d->dimension;
    if (n < 3 || n > NT_MAX_DIM) return fail(NT_E_INVALID, "dimension must be between 3 and %d", NT_MAX_DIM);
    if (d->n_nodes < 0 || d->n_items < 0 || d->n_batches < 0 || d->n_triangles < 0 || d->n_solids < 0 || d->n_materials < 0)
        return fail(NT_E_INVALID, "negative count in scene description");
    if (d->root < -1 || d->root >= d->n_nodes) return fail(NT_E_INVALID, "root index out of range");
    if (!d->aabb_start || !d->aabb_end) return fail(NT_E_INVALID, "scene boundary is required");
    if (d->n_nodes && (!d->node_axis || !d->node_split || !d->node_left || !d->node_right)) return fail(NT_E_INVALID, "node arrays are NULL");
    if (d->n_items && !d->items) return fail(NT_E_INVALID, "items array is NULL");
    if (d->n_batches && (!d->batch_recs || !d->batch_mats)) return fail(NT_E_INVALID, "batch arrays are NULL");
    if (d->n_triangles && (!d->tri_recs || !d->tri_mats)) return fail(NT_E_INVALID, "triangle arrays are NULL");
    if (d->n_solids && (!d->solid_recs || !d->solid_types || !d->solid_mats)) return fail(NT_E_INVALID, "solid arrays are NULL");
    if ((d->n_batches || d->n_triangles || d->n_solids) && (!d->materials || d->n_materials < 1)) return fail(NT_E_INVALID, "materials are required");
    for (int i = 0; i < d->n_nodes; ++i) {
        const int ax = d->node_axis[i];
        if (ax >= n || ax < -1) return fail(NT_E_INVALID, "node %d: axis %d out of range", i, ax);
        if (ax < 0) {
            const long st = d->node_left[i], cnt = d->node_right[i];
            if (st < 0 || cnt < 1 || st + cnt > d->n_items) return fail(NT_E_INVALID, "leaf %d: item range out of bounds", i);
        } else {
            const int l = d->node_left[i], r = d->node_right[i];
            if (l < -1 || l >= d->n_nodes || r < -1 || r >= d->n_nodes) return fail(NT_E_INVALID, "branch %d: child index out of range", i);
            if (l < 0 && r < 0) return fail(NT_E_INVALID, "branch %d: both children are empty", i);
        }
    }
    for (int i = 0; i < d->n_items; ++i) {
        const int it = d->items[i];
        const int kind = it & 3, idx = it >> 2;
        const int lim = kind == NT_KIND_BATCH ? d->n_batches : kind == NT_KIND_TRIANGLE ? d->n_triangles : kind == NT_KIND_SOLID ? d->n_solids : -1;
        if (it < 0 || idx >= lim) return fail(NT_E_INVALID, "item %d: primitive reference out of range", i);
    }
    auto check_mats = [&](const int32_t *m, long cnt) {
        for (long i = 0; i < cnt; ++i) if (m[i] < 0 || m[i] >= d->n_materials) return false;
        return true;
    };
    if (!check_mats(d->batch_mats, (long)d->n_batches * NT_BATCH_SIZE) || !check_mats(d->tri_mats, d->n_triangles) || !check_mats(d->solid_mats, d->n_solids))
        return fail(NT_E_INVALID, "material index out of range");
    for (int i = 0; i < d->n_solids; ++i)
        if (d->solid_types[i] != NT_SOLID_CUBE && d->solid_types[i] != NT_SOLID_SPHERE) return fail(NT_E_INVALID, "solid %d: unknown type", i);
    return NT_OK;
}

// depth of the tree + cycle check (every node reachable at most once)
int tree_depth(const nt_scene_desc *d, int &depth_out) {
    depth_out = 0;
    if (d->root < 0) return NT_OK;
    std::vector<char> seen((size_t)d->n_nodes, 0);
    std::vector<std::pair<int, int>> stack;
    stack.emplace_back(d->root, 1);
    while (!stack.empty()) {
        auto [node, dep] = stack.back();
        stack.pop_back();
        if (seen[node]) return fail(NT_E_INVALID, "node %d is referenced more than once (the k-d tree must be a tree)", node);
        seen[node] = 1;
        depth_out = std::max(depth_out, dep);
        if (d->node_axis[node] >= 0) {
            if (d->node_left[node] >= 0) stack.emplace_back(d->node_left[node], dep + 1);
            if (d->node_right[node] >= 0) stack.emplace_back(d->node_right[node], dep + 1);
        }
    }
    return NT_OK;
}

void pad_records(const float *src, long count, int rec_len, int stride, std::vector<float> &out) {
    out.assign((size_t)count * stride, 0.0f);
    for (long i = 0; i < count; ++i) std::memcpy(out.data() + (size_t)i * stride, src + (size_t)i * rec_len, sizeof(float) * rec_len);
}

// ---------------------------------------------------------------------------------------------
// ray queries: KDNode.intersects / KDNode.occludes batched (src/ntracer_body.hpp:1412-1496; kernels in nt_query.hpp)
// ---------------------------------------------------------------------------------------------

// what can be refused without a device
int query_validate(const nt_scene *s, const nt_ray_batch *rays, const nt_ray_results *out) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (!rays || !out || !out->hits || !rays->origins || !rays->directions) return fail(NT_E_INVALID, "NULL argument");
    if (rays->count < 0) return fail(NT_E_INVALID, "invalid ray count");
    if (out->max_transparent < 0 || out->max_transparent > NT_TH_MAX)
        return fail(NT_E_INVALID, "max_transparent must lie in 0..%d", NT_TH_MAX);
    if (out->transparent && out->max_transparent == 0) return fail(NT_E_INVALID, "a transparent list with max_transparent == 0");
    if (!s->composite) return fail(NT_E_INVALID, "not a composite scene");
    return NT_OK;
}

// the launch of one query: `q` holds device pointers.  The `checked` scratch of the walks with transparent hits is sized by the
// grid: a column per resident lane, at most 256 MB of it, the blocks striding over the rays.
int query_enqueue(nt_scene *s, DeviceState *ds, NtQuery &q, bool strict, hipStream_t stream) {
    const RenderSwitches sw = read_switches();
    NtCompositeDev c;
    scene_dev(s, ds, sw, strict, false, c);
    const CompositeRoute rt = composite_route(s, sw);
    // closest hits of scenes with transparent materials or Solids: the walk that keeps the transparent hits and the
    // reference's o_hit.normal, on the exact `checked` list (see CompositeRoute); occlusion walks keep no such list
    const bool faithful = !q.occlusion && rt.faithful;
    if (faithful) {
        // (a query keeps no ray_color frames: a quarter of the renderer's blocks are more than are resident, and half its bytes)
        const long long lpb = rt.var ? 64 : 256;
        long long blocks = std::min<long long>(((long long)q.count + lpb - 1) / lpb, rt.var ? 4096 : 1024);
        if (int e = checked_scratch(s, ds, sw, c, lpb, blocks, 1, 0, (long long)256 << 20)) return e;
    }
    if (int r = nt_launch_query(launch_info(s, ds, sw, 1, stream), c, q)) return launch_failed(r);
    return NT_OK;
}

int query_host(nt_scene *s, const nt_ray_batch *rays, const nt_ray_results *out, int device, bool occlusion) {
    if (int r = query_validate(s, rays, out)) return r;
    if (rays->count == 0) return NT_OK;
    if (int r = check_renderable(s)) return r;
    RenderGuard guard(s);
    if (int r = guard.acquire()) return r;
    DeviceState *ds;
    if (int r = scene_on_device(s, nullptr, device, ds)) return r;
    if (int r = use_own_stream(ds)) return r;
    // one slab of the probe scratch: rays | per-ray parameters | normals | records | lists, each 16-byte aligned
    const size_t count = (size_t)rays->count, n = (size_t)s->n;
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t vlen = count * n * sizeof(float), flen = count * sizeof(float);
    const size_t rbytes = count * sizeof(nt_ray_hit);
    const size_t lbytes = out->transparent ? rbytes * (size_t)out->max_transparent : 0;
    const float *distance = occlusion ? rays->distance : nullptr;
    float *normal_origin = occlusion ? nullptr : out->normal_origin, *normal_dir = occlusion ? nullptr : out->normal_dir;
    size_t total = 2 * al(vlen) + rbytes + lbytes;
    for (const void *p : {(const void *)rays->t_near, (const void *)rays->t_far, (const void *)distance, (const void *)rays->skip_item,
                          (const void *)rays->skip_lane})
        if (p) total += al(flen);
    if (normal_origin) total += al(vlen);
    if (normal_dir) total += al(vlen);
    if (int r = ds->probes.ensure(total)) return r;
    char *at = (char *)ds->probes.p;
    hipStream_t st = ds->stream;
    // an array of the caller's, copied to the next free piece of the slab (nullptr stays nullptr)
    auto up = [&](const void *src, size_t bytes, void *&dst) -> hipError_t {
        dst = nullptr;
        if (!src) return hipSuccess;
        dst = at;
        at += al(bytes);
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    };
    NtQuery q{};
    q.count = rays->count;
    q.occlusion = occlusion ? 1 : 0;
    void *d;
    HIP_TRY(up(rays->origins, vlen, d)); q.origins = (const float *)d;
    HIP_TRY(up(rays->directions, vlen, d)); q.directions = (const float *)d;
    HIP_TRY(up(rays->t_near, flen, d)); q.t_near = (const float *)d;
    HIP_TRY(up(rays->t_far, flen, d)); q.t_far = (const float *)d;
    HIP_TRY(up(distance, flen, d)); q.distance = (const float *)d;
    HIP_TRY(up(rays->skip_item, flen, d)); q.skip_item = (const int *)d;
    HIP_TRY(up(rays->skip_lane, flen, d)); q.skip_lane = (const int *)d;
    // (the kernels do not write the normal rows of rays without an opaque hit: the caller's rows travel through)
    HIP_TRY(up(normal_origin, vlen, d)); q.normal_origin = (float *)d;
    HIP_TRY(up(normal_dir, vlen, d)); q.normal_dir = (float *)d;
    q.hits = at;
    at += rbytes;
    q.transparent = out->transparent ? at : nullptr;
    q.max_transparent = out->max_transparent;
    if (int r = query_enqueue(s, ds, q, false, st)) { (void)hipStreamSynchronize(st); return r; }
    HIP_TRY(hipMemcpyAsync(out->hits, q.hits, rbytes, hipMemcpyDeviceToHost, st));
    if (q.normal_origin) HIP_TRY(hipMemcpyAsync(normal_origin, q.normal_origin, vlen, hipMemcpyDeviceToHost, st));
    if (q.normal_dir) HIP_TRY(hipMemcpyAsync(normal_dir, q.normal_dir, vlen, hipMemcpyDeviceToHost, st));
    if (q.transparent) HIP_TRY(hipMemcpyAsync(out->transparent, q.transparent, lbytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NT_OK;
}

int query_device(nt_scene *s, const nt_ray_batch *rays, const nt_ray_results *out, const nt_render_opts *opts, void *hip_stream,
                 bool occlusion) {
    if (int r = query_validate(s, rays, out)) return r;
    if (int r = only_device_strict_abort(opts, "a ray query reads")) return r;
    if (rays->count == 0) return NT_OK;
    if (int r = check_renderable(s)) return r;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->busy) return fail(NT_E_BUSY, "the renderer is already running");
    DeviceState *ds;
    if (int r = scene_on_device(s, opts, -1, ds)) return r;
    if (int r = use_stream(ds, (hipStream_t)hip_stream)) return r;
    NtQuery q{};
    q.count = rays->count;
    q.occlusion = occlusion ? 1 : 0;
    q.origins = rays->origins;
    q.directions = rays->directions;
    q.t_near = rays->t_near;
    q.t_far = rays->t_far;
    q.distance = occlusion ? rays->distance : nullptr;
    q.skip_item = rays->skip_item;
    q.skip_lane = rays->skip_lane;
    q.hits = out->hits;
    q.normal_origin = occlusion ? nullptr : out->normal_origin;
    q.normal_dir = occlusion ? nullptr : out->normal_dir;
    q.transparent = out->transparent;
    q.max_transparent = out->max_transparent;
    q.abort_word = opts ? (const int *)opts->abort_device : nullptr;
    return query_enqueue(s, ds, q, opts && opts->strict_reference, (hipStream_t)hip_stream);
}

// ---------------------------------------------------------------------------------------------
// primary-hit buffers: ray_color at depth 0 up to where shading starts, for every pixel (kernels in nt_hits.hpp)
// ---------------------------------------------------------------------------------------------

// what can be refused without a device
int hits_validate(const nt_scene *s, int width, int height, const nt_hit_buffers *out, long long frame_stride, long long nframes) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (!out || !out->hits) return fail(NT_E_INVALID, "NULL argument");
    if (width < 1 || height < 1) return fail(NT_E_INVALID, "invalid view size");
    if (!s->composite) return fail(NT_E_INVALID, "not a composite scene");
    if (s->lens) return fail(NT_E_UNSUPPORTED, "primary-hit buffers are not available while a lens is set");
    if (s->parallel > 0.0f) return fail(NT_E_UNSUPPORTED, "primary-hit buffers are not available while the parallel projection is set");
    if (s->clip_count > 0 && s->n_solids > 0)
        return fail(NT_E_UNSUPPORTED, "clip planes are not available for a scene with Solids (a Solid cut open has no cap)");
    if ((long long)width * height > INT_MAX) return fail(NT_E_INVALID, "a view of %d x %d pixels is beyond 2^31 - 1 records", width, height);
    if (frame_stride < (long long)width * height) return fail(NT_E_INVALID, "frame_stride_records is smaller than one frame");
    if (frame_stride > INT_MAX || nframes * frame_stride > INT_MAX)
        return fail(NT_E_INVALID, "%lld frames of %lld records are beyond 2^31 - 1 records", nframes, frame_stride);
    return NT_OK;
}

// The launch of one pass: `out` holds device pointers, `cam_buf` the frames' cameras in device memory (nullptr: the scene's
// current camera, one frame).  The scene goes the way a render of it would go (plan_composite): the walks with the exact
// `checked` list for transparent materials and the reference's o_hit.normal, the packet walk -- with its numerators and its
// quad order -- for the opaque scenes the fixed-n kernels draw.
int hits_enqueue(nt_scene *s, DeviceState *ds, int width, int height, const nt_hit_buffers *out, long long frame_stride, const float *cam_buf,
                 int nframes, bool strict, const int *abort_word, hipStream_t stream) {
    const RenderSwitches sw = read_switches();
    NtCompositeDev c;
    scene_dev(s, ds, sw, strict, false, c);
    NtTarget tg;
    view_target(s, width, height, abort_word, tg);
    tg.frame_stride = frame_stride * (long long)sizeof(nt_ray_hit);
    NtLaunchInfo li = launch_info(s, ds, sw, nframes, stream);
    const CompositeRoute rt = composite_route(s, sw);
    const bool clip = s->clip_count > 0;       // under clip planes every scene off the packet walk takes the run-time-n kernels
    if (rt.faithful) {
        // (no ray_color frames are kept: the grid of a ray query, see query_enqueue)
        const bool var = rt.var || clip;
        const long long lpb = var ? 64 : 256, tw = var ? 8 : 16;
        const long long tiles = ((width + tw - 1) / tw) * ((height + tw - 1) / tw) * nframes;
        long long blocks = std::min<long long>(tiles, var ? 4096 : 1024);
        if (int e = checked_scratch(s, ds, sw, c, lpb, blocks, 1, 0, (long long)256 << 20)) return e;
    }
    NtHits h{};
    h.nframes = nframes;
    h.frame_stride = frame_stride;
    h.hits = out->hits;
    h.normal_origin = out->normal_origin;
    h.normal_dir = out->normal_dir;
    if (int e = device_camera(s, ds, cam_buf, stream, h.cams)) return e;
    if (rt.packet_walk) {                                               // (of a composite scene: no other comes here)
        // the packet walk's plane numerators and quad order
        if (int e = numerator_scratch(s, ds, sw, nframes, li)) return e;
        if (sw.tile_order) {
            if (int e = tile_order_for(ds, width, height, li.tile_order)) return e;
        }
    }
    if (clip) {
        // the same walks with the planes: what is under a pixel of the cutaway (nt_launch_clip, kept apart from nt_launch_hits)
        NtClip cl{};
        cl.planes = (const float *)ds->clip.p;
        cl.count = s->clip_count;
        cl.cams = h.cams;
        cl.nframes = nframes;
        cl.hits = h.hits;
        cl.frame_stride = h.frame_stride;
        cl.normal_origin = h.normal_origin;
        cl.normal_dir = h.normal_dir;
        NtCamera cam{};
        cam.n = s->n;
        cam.buf = h.cams;
        if (int r = nt_launch_clip(li, cam, c, tg, cl, false)) return launch_failed(r);
        return NT_OK;
    }
    if (int r = nt_launch_hits(li, c, tg, h)) return launch_failed(r);
    return NT_OK;
}

int hits_host(nt_scene *s, int width, int height, const nt_hit_buffers *out, int device) {
    if (int r = hits_validate(s, width, height, out, (long long)width * height, 1)) return r;
    if (int r = check_renderable(s)) return r;
    RenderGuard guard(s);
    if (int r = guard.acquire()) return r;
    DeviceState *ds;
    if (int r = scene_on_device(s, nullptr, device, ds)) return r;
    if (int r = use_own_stream(ds)) return r;
    // one slab of the probe scratch: records | normal origins | normal directions (16-byte aligned each)
    const size_t count = (size_t)width * height;
    const size_t rbytes = count * sizeof(nt_ray_hit), vlen = (count * s->n * sizeof(float) + 15) & ~(size_t)15;
    if (int r = ds->probes.ensure(rbytes + (out->normal_origin ? vlen : 0) + (out->normal_dir ? vlen : 0))) return r;
    hipStream_t st = ds->stream;
    char *at = (char *)ds->probes.p;
    nt_hit_buffers d{};
    d.hits = (nt_ray_hit *)at;
    at += rbytes;
    // (the kernels do not write the normal rows of pixels without an opaque hit: the caller's rows travel through)
    if (out->normal_origin) {
        d.normal_origin = (float *)at;
        at += vlen;
        HIP_TRY(hipMemcpyAsync(d.normal_origin, out->normal_origin, count * s->n * sizeof(float), hipMemcpyHostToDevice, st));
    }
    if (out->normal_dir) {
        d.normal_dir = (float *)at;
        HIP_TRY(hipMemcpyAsync(d.normal_dir, out->normal_dir, count * s->n * sizeof(float), hipMemcpyHostToDevice, st));
    }
    if (int r = hits_enqueue(s, ds, width, height, &d, (long long)count, nullptr, 1, false, nullptr, st)) { (void)hipStreamSynchronize(st); return r; }
    HIP_TRY(hipMemcpyAsync(out->hits, d.hits, rbytes, hipMemcpyDeviceToHost, st));
    if (d.normal_origin) HIP_TRY(hipMemcpyAsync(out->normal_origin, d.normal_origin, count * s->n * sizeof(float), hipMemcpyDeviceToHost, st));
    if (d.normal_dir) HIP_TRY(hipMemcpyAsync(out->normal_dir, d.normal_dir, count * s->n * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NT_OK;
}

// `cams`: the cameras of the `count` frames in memory of device `cams_device`, or nullptr for the scene's current camera
int hits_device(nt_scene *s, int width, int height, const nt_hit_buffers *out, long long frame_stride, const float *cams, int cams_device,
                int count, const nt_render_opts *opts, void *hip_stream) {
    if (int r = check_renderable(s)) return r;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->busy) return fail(NT_E_BUSY, "the renderer is already running");
    DeviceState *ds;
    if (int r = scene_on_device(s, opts, -1, ds, cams ? cams_device : -1, "pass")) return r;
    if (int r = use_stream(ds, (hipStream_t)hip_stream)) return r;
    return hits_enqueue(s, ds, width, height, out, frame_stride, cams, count, opts && opts->strict_reference,
                        opts ? (const int *)opts->abort_device : nullptr, (hipStream_t)hip_stream);
}

// ---------------------------------------------------------------------------------------------
// BoxScene hit buffers: the face of the cube under every pixel and its distance (kernels in nt_boxhits.hpp)
// ---------------------------------------------------------------------------------------------

// what can be refused without a device
int box_hits_validate(const nt_scene *s, int width, int height, const void *hits, long long frame_stride, long long nframes) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (!hits) return fail(NT_E_INVALID, "NULL argument");
    if (width < 1 || height < 1) return fail(NT_E_INVALID, "invalid view size");
    if (s->composite) return fail(NT_E_INVALID, "not a box scene");
    if (s->lens) return fail(NT_E_UNSUPPORTED, "BoxScene hit buffers are not available while a lens is set");
    if (s->parallel > 0.0f) return fail(NT_E_UNSUPPORTED, "BoxScene hit buffers are not available while the parallel projection is set");
    if ((long long)width * height > INT_MAX) return fail(NT_E_INVALID, "a view of %d x %d pixels is beyond 2^31 - 1 records", width, height);
    if (frame_stride < (long long)width * height) return fail(NT_E_INVALID, "frame_stride_records is smaller than one frame");
    if (frame_stride > INT_MAX || nframes * frame_stride > INT_MAX)
        return fail(NT_E_INVALID, "%lld frames of %lld records are beyond 2^31 - 1 records", nframes, frame_stride);
    return NT_OK;
}

// the device forms take two fields of their options; `reader` is the subject of the refusal
int only_device_abort(const nt_render_opts *opts, const char *reader) {
    if (opts && (opts->band_rank || opts->band_world || opts->band_rows || opts->compact || opts->strict_reference || opts->collect_stats ||
                 opts->overlapped))
        return fail(NT_E_INVALID, "%s reads device and abort_device of its options: every other field must be 0", reader);
    return NT_OK;
}

// The launch of one pass: `recs_dev` is device memory, `cam_buf` / `cam_dots` the frames' cameras and their dot products in
// device memory (nullptr: the scene's current camera, one frame, in the kernel arguments as for a render).
int box_hits_enqueue(nt_scene *s, DeviceState *ds, int width, int height, void *recs_dev, long long frame_stride, const float *cam_buf,
                     const float *cam_dots, int nframes, const int *abort_word, hipStream_t stream) {
    const RenderSwitches sw = read_switches();
    NtTarget tg;
    view_target(s, width, height, abort_word, tg);
    tg.frame_stride = frame_stride * (long long)sizeof(nt_ray_hit);
    NtCamera cam;
    box_camera(s, cam_buf, cam_dots, 0, cam);
    const NtLaunchInfo li = launch_info(s, ds, sw, nframes, stream);
    NtBoxFaces bf{};
    bf.mode = NT_BOX_FACES_RECORDS;
    bf.recs = recs_dev;
    bf.frame_stride = frame_stride;
    if (int r = nt_launch_box_faces(li, cam, tg, bf)) return launch_failed(r);
    return NT_OK;
}

int box_hits_host(nt_scene *s, int width, int height, nt_ray_hit *hits, int device) {
    if (int r = box_hits_validate(s, width, height, hits, (long long)width * height, 1)) return r;
    RenderGuard guard(s);   // held like nt_colors_at holds it
    if (int r = guard.acquire()) return r;
    DeviceState *ds;
    if (int r = scene_on_device(s, nullptr, device, ds)) return r;
    if (int r = use_own_stream(ds)) return r;
    const size_t rbytes = (size_t)width * height * sizeof(nt_ray_hit);
    if (int r = ds->probes.ensure(rbytes)) return r;
    hipStream_t st = ds->stream;
    if (int r = box_hits_enqueue(s, ds, width, height, ds->probes.p, (long long)width * height, nullptr, nullptr, 1, nullptr, st)) {
        (void)hipStreamSynchronize(st);
        return r;
    }
    HIP_TRY(hipMemcpyAsync(hits, ds->probes.p, rbytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NT_OK;
}

// `cams` / `dots`: the cameras of the `count` frames in memory of device `cams_device`, or nullptr for the scene's current camera
int box_hits_device(nt_scene *s, int width, int height, void *hits_dev, long long frame_stride, const float *cams, const float *dots,
                    int cams_device, int count, const nt_render_opts *opts, void *hip_stream) {
    std::lock_guard<std::mutex> g(s->mu);
    if (s->busy) return fail(NT_E_BUSY, "the renderer is already running");
    DeviceState *ds;
    if (int r = scene_on_device(s, opts, -1, ds, cams ? cams_device : -1, "pass")) return r;
    if (int r = use_stream(ds, (hipStream_t)hip_stream)) return r;
    return box_hits_enqueue(s, ds, width, height, hits_dev, frame_stride, cams, dots, count, opts ? (const int *)opts->abort_device : nullptr,
                            (hipStream_t)hip_stream);
}

// ---------------------------------------------------------------------------------------------
// colours of the caller's rays: ray_color / box_scene::calculate_color for rays from memory (kernels in nt_rays.hpp)
// ---------------------------------------------------------------------------------------------

// what can be refused without a device; `host`: the rays can be looked at
int rays_validate(const nt_scene *s, const nt_rays *rays, const void *out, bool host) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (!rays || !out || !rays->origins || !rays->directions) return fail(NT_E_INVALID, "NULL argument");
    if (rays->count < 0) return fail(NT_E_INVALID, "invalid ray count");
    if (int r = clip_refuses(s, "the colour of a caller's ray (nt_ray_colors / nt_render_rays)")) return r;
    if (int r = xray_refuses(s, "the colour of a caller's ray (nt_ray_colors / nt_render_rays)")) return r;
    if (!host) return NT_OK;
    const size_t n = (size_t)s->n;
    for (size_t r = 0; r < (size_t)rays->count; ++r) {
        const float *d = rays->directions + r * n;
        const float *o = rays->shared_origin ? (r == 0 ? rays->origins : nullptr) : rays->origins + r * n;
        bool finite = true, zero = true;
        for (size_t k = 0; k < n; ++k) {
            finite = finite && std::isfinite(d[k]) && (!o || std::isfinite(o[k]));
            zero = zero && d[k] == 0.0f;
        }
        if (!finite) return fail(NT_E_INVALID, "ray %zu has a non-finite component", r);
        if (zero) return fail(NT_E_INVALID, "ray %zu has an all-zero direction", r);
    }
    return NT_OK;
}

// the format and the buffer of the image forms, as nt_render checks them, and the count against the format
int rays_image_validate(const nt_image_format *fmt, const nt_rays *rays, size_t dest_len, Format &f) {
    if (int r = parse_format(fmt, f)) return r;
    if ((long long)rays->count != (long long)f.width * f.height)
        return fail(NT_E_INVALID, "%d rays do not fill an image of %d x %d pixels", rays->count, f.width, f.height);
    if (dest_len < required_len(f, Bands())) return fail(NT_E_INVALID, "the buffer is too small for an image with the given dimensions");
    return NT_OK;
}

// The launch of one batch: `job` holds device pointers; the colours go to `rgb` ([count][3], device), or with rgb == nullptr
// into the image `fmt` describes at `dest_dev`.  The scene goes the way a render of it would go (plan_composite), minus the
// packet walk: the `checked` list and, at run-time n or beyond the fixed kernels' frame stack, the ray_color frames in
// global scratch for transparent materials and the reference's o_hit.normal, a column per resident lane -- at most 1024
// blocks of 256 lanes, 4096 of 64 -- the blocks striding over the rays.
// the image of the image forms as a launch target: ray y * width + x is pixel (x, y) of the whole image at dest_dev
int rays_image_target(const nt_scene *s, DeviceState *ds, const Format *fmt, void *dest_dev, const int *abort_word, hipStream_t stream, NtTarget &tg) {
    FrameJob fj{};
    fj.fmt = fmt;
    fj.dest_dev = dest_dev;
    fj.frame_stride = 0;
    fj.nframes = 1;
    fj.stream = stream;
    fj.abort_word = abort_word;
    fj.row_begin = 0;
    fj.row_count = fmt->height;
    if (int r = fill_target(s, ds, fj, tg)) return r;
    // consecutive lanes hold consecutive rays, not the aligned groups of one row that emit_pixel's shared dword stores
    // of 3- and 6-byte pixels count on: those formats go out pixel by pixel
    if (tg.bpp == 3 || tg.bpp == 6) tg.aligned4 = 0;
    return NT_OK;
}

// the scene of a ray-colour launch over `count` rays, and its per-lane scratch: `lpb_fixed` lanes a block of the compile-time-N
// kernels (the run-time-n ones have 64), at most `max_fixed` blocks of them
int rays_scene(const nt_scene *s, DeviceState *ds, const RenderSwitches &sw, bool strict, long long count, long long lpb_fixed, long long max_fixed,
               NtCompositeDev &c) {
    scene_dev(s, ds, sw, strict, false, c);
    const CompositeRoute rt = composite_route(s, sw);
    if (rt.faithful) {
        const long long lpb = rt.var_t ? 64 : lpb_fixed;
        long long blocks = std::min<long long>((count + lpb - 1) / lpb, rt.var_t ? 4096 : max_fixed);
        if (int e = checked_scratch(s, ds, sw, c, lpb, blocks, 1, rt.var_t ? rt.frame_stack : 0, (long long)512 << 20)) return e;
    }
    return NT_OK;
}

int rays_enqueue(nt_scene *s, DeviceState *ds, const NtRayJob &job, float *rgb, const Format *fmt, void *dest_dev, bool strict,
                 const int *abort_word, hipStream_t stream) {
    const RenderSwitches sw = read_switches();
    NtTarget tg;
    if (rgb) {
        std::memset(&tg, 0, sizeof(tg));
        tg.colors_out = rgb;
        tg.probe_count = job.count;
        tg.band_world = 1;
        tg.band_rows = NT_RENDER_CHUNK_SIZE;
        tg.abort_word = abort_word;
    } else {
        if (int r = rays_image_target(s, ds, fmt, dest_dev, abort_word, stream, tg)) return r;
        if (tg.bpp == 0) return NT_OK;                                 // nothing to draw
    }
    NtCompositeDev c;
    if (s->composite) {
        if (int e = rays_scene(s, ds, sw, strict, job.count, 256, 1024, c)) return e;
    }
    if (int r = nt_launch_rays(launch_info(s, ds, sw, 1, stream), s->composite ? &c : nullptr, job, tg)) return launch_failed(r);
    return NT_OK;
}

// the host forms: rays (and the image's bytes, for its padding) up, colours or image down, on the library's own stream
int rays_host(nt_scene *s, const nt_rays *rays, float *rgb, void *dest, size_t dest_len, const nt_image_format *fmt, int device) {
    if (int r = rays_validate(s, rays, rgb ? (const void *)rgb : (const void *)dest, false)) return r;
    Format f;
    if (!rgb) {
        if (int r = rays_image_validate(fmt, rays, dest_len, f)) return r;
    }
    if (int r = rays_validate(s, rays, rgb ? (const void *)rgb : (const void *)dest, true)) return r;
    if (rays->count == 0) return NT_OK;
    if (int r = check_renderable(s)) return r;
    RenderGuard guard(s);
    if (int r = guard.acquire()) return r;
    DeviceState *ds;
    if (int r = scene_on_device(s, nullptr, device, ds)) return r;
    if (int r = use_own_stream(ds)) return r;
    // one slab of the probe scratch: directions | origins | colours, each 16-byte aligned
    const size_t count = (size_t)rays->count, n = (size_t)s->n;
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t dlen = count * n * sizeof(float), olen = (rays->shared_origin ? 1 : count) * n * sizeof(float);
    const size_t cbytes = rgb ? count * 3 * sizeof(float) : 0;
    const size_t need = rgb ? 0 : required_len(f, Bands());
    if (!rgb && need == 0) return NT_OK;                               // a format without channels: nothing to draw
    if (int r = ds->probes.ensure(al(dlen) + al(olen) + cbytes)) return r;
    hipStream_t st = ds->stream;
    char *at = (char *)ds->probes.p;
    NtRayJob job{};
    job.count = rays->count;
    job.shared_origin = rays->shared_origin ? 1 : 0;
    job.directions = (const float *)at;
    job.origins = (const float *)(at + al(dlen));
    float *rgb_dev = rgb ? (float *)(at + al(dlen) + al(olen)) : nullptr;
    HIP_TRY(hipMemcpyAsync(at, rays->directions, dlen, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(at + al(dlen), rays->origins, olen, hipMemcpyHostToDevice, st));
    if (!rgb) {
        if (int r = ds->framebuffer.ensure(std::max<size_t>(need, 16))) return r;
        // pitch padding bytes are not written by the kernels: carry the caller's bytes through
        if (f.pitch != f.width * f.bpp) HIP_TRY(hipMemcpyAsync(ds->framebuffer.p, dest, need, hipMemcpyHostToDevice, st));
    }
    if (int r = rays_enqueue(s, ds, job, rgb_dev, &f, ds->framebuffer.p, false, nullptr, st)) { (void)hipStreamSynchronize(st); return r; }
    if (rgb) HIP_TRY(hipMemcpyAsync(rgb, rgb_dev, cbytes, hipMemcpyDeviceToHost, st));
    else HIP_TRY(hipMemcpyAsync(dest, ds->framebuffer.p, need, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return NT_OK;
}

// the device forms: every pointer is device memory; enqueue only
int rays_device(nt_scene *s, const nt_rays *rays, float *rgb, void *dest_dev, size_t dest_len, const nt_image_format *fmt,
                const nt_render_opts *opts, void *hip_stream) {
    if (int r = rays_validate(s, rays, rgb ? (const void *)rgb : (const void *)dest_dev, false)) return r;
    Format f;
    if (!rgb) {
        if (int r = rays_image_validate(fmt, rays, dest_len, f)) return r;
    }
    if (int r = only_device_strict_abort(opts, "a ray-colour call reads")) return r;
    if (rays->count == 0) return NT_OK;
    if (int r = check_renderable(s)) return r;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->busy) return fail(NT_E_BUSY, "the renderer is already running");
    DeviceState *ds;
    if (int r = scene_on_device(s, opts, -1, ds)) return r;
    if (int r = use_stream(ds, (hipStream_t)hip_stream)) return r;
    NtRayJob job{};
    job.count = rays->count;
    job.shared_origin = rays->shared_origin ? 1 : 0;
    job.origins = rays->origins;
    job.directions = rays->directions;
    return rays_enqueue(s, ds, job, rgb, &f, dest_dev, opts && opts->strict_reference, opts ? (const int *)opts->abort_device : nullptr,
                        (hipStream_t)hip_stream);
}

// ---------------------------------------------------------------------------------------------
// the buffer of a setting alone, of one view of the scene's camera: nt_adaptive_mask, nt_ambient_occlusion, nt_outline_mask,
// nt_depth_cue_factors, nt_box_line_mask and their _device forms
// ---------------------------------------------------------------------------------------------

// what tells the five apart; T is the buffer's element type
template <typename T>
struct ViewQuery {
    size_t elem;                         // bytes a pixel
    int kind;                            // the scenes it is of: 1 composite, 0 BoxScene, -1 either
    const char *clip_what;               // clip_refuses' phrase of it (nullptr: not asked)
    bool (*off)(const nt_scene *s);
    const char *off_message;
    const char *what;                    // subject and verb of the lens / projection refusal
    bool adaptive_terms;                 // row bands and collect_stats, refused in the adaptive mask's words
    bool pixel_term;                     // more than 2^31 - 1 pixels, refused here (face lines: no check_renderable term follows)
    int (*device_options)(const nt_render_opts *opts);      // what the device form refuses of its options (nullptr: nothing)
    // the setting's enqueue: into `dev`, or with `kept` into scratch, whose place it tells there
    int (*enqueue)(nt_scene *s, DeviceState *ds, const FrameJob &job, T *dev, T **kept);
    bool under_xray = false;             // answered while X-ray is on as well (the crossing counts, the hit layers)
    const char *layered = nullptr;       // not nullptr: the call brings a `layers` factor, 1..NT_LAYERS_MAX planes of `elem` bytes a
                                         // pixel, and this is the noun of its refusals (the hit layers alone)
};

const ViewQuery<uint8_t> kAdaptiveMask = {
    1, -1, "the adaptive mask", [](const nt_scene *s) { return !s->adaptive; }, "the adaptive threshold is off (nt_scene_set_adaptive_supersampling)",
    "the adaptive mask is", true, false, nullptr,
    [](nt_scene *s, DeviceState *ds, const FrameJob &job, uint8_t *dev, uint8_t **kept) {
        return enqueue_adaptive(s, ds, job, read_switches(), dev, kept != nullptr, kept);
    }};
const ViewQuery<int> kAoCounts = {
    sizeof(int32_t), 1, "the ambient occlusion count", [](const nt_scene *s) { return s->ao_count <= 0; }, "ambient occlusion is off (nt_scene_set_ambient_occlusion)",
    "the ambient occlusion counts are", false, false,
    [](const nt_render_opts *opts) { return only_device_strict_abort(opts, "the ambient occlusion counts read", "their"); },
    [](nt_scene *s, DeviceState *ds, const FrameJob &job, int *dev, int **kept) { return enqueue_ao(s, ds, job, read_switches(), dev, kept); }};
const ViewQuery<uint8_t> kOutlineMask = {
    1, 1, "the outline mask", [](const nt_scene *s) { return !s->outlines; }, "outlines are off (nt_scene_set_outlines)",
    "the outline mask is", false, false, [](const nt_render_opts *opts) { return only_device_strict_abort(opts, "the outline mask reads"); },
    [](nt_scene *s, DeviceState *ds, const FrameJob &job, uint8_t *dev, uint8_t **kept) {
        return enqueue_outlines(s, ds, job, read_switches(), dev, kept != nullptr, kept);
    }};
const ViewQuery<float> kCueFactors = {
    2 * sizeof(float), 1, "the depth cue factors", [](const nt_scene *s) { return !s->cue; }, "the depth cue is off (nt_scene_set_depth_cue)",
    "the depth cue factors are", false, false,
    [](const nt_render_opts *opts) { return only_device_strict_abort(opts, "the depth cue factors read", "their"); },
    [](nt_scene *s, DeviceState *ds, const FrameJob &job, float *dev, float **kept) {
        return enqueue_cue(s, ds, job, read_switches(), dev, kept != nullptr, kept);
    }};
const ViewQuery<uint8_t> kBoxLineMask = {
    1, 0, nullptr, [](const nt_scene *s) { return !s->box_lines; }, "face lines are off (nt_scene_set_box_lines)",
    "the face-line mask is", false, true, [](const nt_render_opts *opts) { return only_device_abort(opts, "the face-line mask"); },
    [](nt_scene *s, DeviceState *ds, const FrameJob &job, uint8_t *dev, uint8_t **kept) {
        return enqueue_box_lines(s, ds, job, read_switches(), dev, kept != nullptr, kept);
    }};

const ViewQuery<int> kCrossingCounts = {
    sizeof(int32_t), 1, "the crossing count", [](const nt_scene *) { return false; }, "", "the crossing counts are", false, true,
    [](const nt_render_opts *opts) { return only_device_strict_abort(opts, "the crossing counts read", "their"); },
    [](nt_scene *s, DeviceState *ds, const FrameJob &job, int *dev, int **kept) { return enqueue_xray(s, ds, job, read_switches(), dev, kept); },
    true};

const ViewQuery<nt_ray_hit> kHitLayers = {
    sizeof(nt_ray_hit), 1, "the hit layers", [](const nt_scene *) { return false; }, "", "the hit layers are", false, false,      // (the records term of `layered` covers the pixels)
    [](const nt_render_opts *opts) { return only_device_strict_abort(opts, "the hit layers read", "their"); },
    [](nt_scene *s, DeviceState *ds, const FrameJob &job, nt_ray_hit *dev, nt_ray_hit **kept) { return enqueue_layers(s, ds, job, read_switches(), dev, kept); },
    true, "the hit layers"};

// what both forms check before a device is touched; `layers`: the call's factor where q.layered (else 1)
template <typename T>
int view_query_validate(const nt_scene *s, int width, int height, int layers, const void *out, const nt_render_opts *opts, const ViewQuery<T> &q) {
    if (!s || !out) return fail(NT_E_INVALID, "NULL argument");
    if (width < 1 || height < 1) return fail(NT_E_INVALID, "invalid view size");
    if (q.layered && (layers < 1 || layers > NT_LAYERS_MAX)) return fail(NT_E_INVALID, "%s take 1 to %d layers (%d)", q.layered, NT_LAYERS_MAX, layers);
    if (q.kind == 1 && !s->composite) return fail(NT_E_INVALID, "not a composite scene");
    if (q.kind == 0 && s->composite) return fail(NT_E_INVALID, "not a box scene");
    if (q.clip_what) {
        if (int r = clip_refuses(s, q.clip_what)) return r;
        if (!q.under_xray) {
            if (int r = xray_refuses(s, q.clip_what)) return r;
        }
    }
    if (q.off(s)) return fail(NT_E_INVALID, "%s", q.off_message);
    if (q.adaptive_terms) {
        if (opts && opts->band_world > 1)
            return fail(NT_E_UNSUPPORTED, "the adaptive mask is of the whole image: row bands (band_world %d) are not available", opts->band_world);
        if (opts && opts->collect_stats) return fail(NT_E_UNSUPPORTED, "the adaptive mask keeps no counters: collect_stats is not available");
    }
    if (s->lens || s->parallel > 0.0f) return fail(NT_E_UNSUPPORTED, "%s not available while a lens or the parallel projection is set", q.what);
    // (a key of the layers' sorted lists keeps an item code and its lane in 32 bits)
    if (q.layered && std::max(std::max(s->n_batches, s->n_triangles), s->n_solids) > NT_DEV_LAYERS_INDEX_MAX)
        return fail(NT_E_UNSUPPORTED, "%s take scenes of up to 2^26 batches, triangles or Solids each", q.layered);
    if (q.layered && (long long)width * height * layers > INT_MAX)
        return fail(NT_E_INVALID, "%d layers of %d x %d pixels are beyond 2^31 - 1 records", layers, width, height);
    if (q.pixel_term && (long long)width * height > INT_MAX)
        return fail(NT_E_INVALID, "a view of %d x %d pixels is beyond 2^31 - 1 pixels", width, height);
    return check_renderable(s);
}

// The host form: the renderer protocol (`guard` is the caller's, so that it holds while the caller reads more), the enqueue into
// scratch on the scene's own stream, and the buffer's way back.  *ds_out: where it ran.
template <typename T>
int view_query_host(RenderGuard &guard, const ViewQuery<T> &q, int width, int height, T *out, const nt_render_opts *opts, DeviceState **ds_out = nullptr,
                    int layers = 1) {
    nt_scene *s = guard.s;
    if (int r = view_query_validate(s, width, height, layers, out, opts, q)) return r;
    if (int r = guard.acquire()) return r;
    DeviceState *ds;
    if (int r = scene_on_device(s, opts, -1, ds)) return r;
    if (int r = use_own_stream(ds)) return r;
    FrameJob job = view_job(width, height, ds->stream, opts, false);
    job.layers = layers;
    T *kept = nullptr;
    if (int r = q.enqueue(s, ds, job, nullptr, &kept)) { (void)hipStreamSynchronize(ds->stream); return r; }
    HIP_TRY(hipMemcpyAsync(out, kept, (size_t)width * height * layers * q.elem, hipMemcpyDeviceToHost, ds->stream));
    HIP_TRY(hipStreamSynchronize(ds->stream));
    if (ds_out) *ds_out = ds;
    return NT_OK;
}

// the device form: `out_dev` is device memory; enqueue only
template <typename T>
int view_query_device(nt_scene *s, const ViewQuery<T> &q, int width, int height, void *out_dev, const nt_render_opts *opts, void *hip_stream,
                      int layers = 1) {
    if (int r = view_query_validate(s, width, height, layers, out_dev, opts, q)) return r;
    if (q.device_options) {
        if (int r = q.device_options(opts)) return r;
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->busy) return fail(NT_E_BUSY, "the renderer is already running");
    DeviceState *ds;
    if (int r = scene_on_device(s, opts, -1, ds)) return r;
    if (int r = use_stream(ds, (hipStream_t)hip_stream)) return r;
    FrameJob job = view_job(width, height, (hipStream_t)hip_stream, opts, true);      // (overlapped: where options are refused, 0)
    job.layers = layers;
    return q.enqueue(s, ds, job, (T *)out_dev, nullptr);
}

// the pixels of a mask that are marked
long long marked_pixels(const uint8_t *mask, size_t count) { return (long long)(count - (size_t)std::count(mask, mask + count, (uint8_t)0)); }

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char *nt_version(void) { return "ntracer_hip 0.1 (gfx950)"; }

const char *nt_last_error(void) { return g_error.c_str(); }

int nt_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

nt_scene_t *nt_box_scene_create(int dimension) {
    if (dimension < 3 || dimension > NT_MAX_DIM) {
        fail(NT_E_INVALID, "dimension must be between 3 and %d", NT_MAX_DIM);
        return nullptr;
    }
    nt_scene *s = new (std::nothrow) nt_scene();
    if (!s) { fail(NT_E_NOMEM, "out of memory"); return nullptr; }
    s->composite = false;
    s->n = dimension;
    s->origin.assign(dimension, 0.0f);                 // camera(d): origin 0, identity axes (camera.hpp:11)
    s->axes.assign((size_t)dimension * dimension, 0.0f);
    for (int i = 0; i < dimension; ++i) s->axes[(size_t)i * dimension + i] = 1.0f;
    return s;
}

nt_scene_t *nt_composite_scene_create(const nt_scene_desc *d) {
    if (validate_desc(d)) return nullptr;
    int depth = 0;
    if (tree_depth(d, depth)) return nullptr;
    nt_scene *s = new (std::nothrow) nt_scene();
    if (!s) { fail(NT_E_NOMEM, "out of memory"); return nullptr; }
    const int n = d->dimension;
    s->composite = true;
    s->n = n;
    s->origin.assign(n, 0.0f);
    s->axes.assign((size_t)n * n, 0.0f);
    for (int i = 0; i < n; ++i) s->axes[(size_t)i * n + i] = 1.0f;
    s->root = d->root;
    s->depth = depth;
    s->nodes.resize((size_t)d->n_nodes);
    for (int i = 0; i < d->n_nodes; ++i) {
        s->nodes[i].split = d->node_split[i];
        s->nodes[i].axis = d->node_axis[i];
        s->nodes[i].left = d->node_left[i];
        s->nodes[i].right = d->node_right[i];
    }
    s->items.assign(d->items, d->items + d->n_items);
    s->rec_len = n * n + n + 1;
    s->rec_stride = (s->rec_len + 3) / 4 * 4;
    s->n_batches = d->n_batches;
    s->n_triangles = d->n_triangles;
    s->n_solids = d->n_solids;
    s->n_materials = d->n_materials;
    pad_records(d->batch_recs, (long)d->n_batches * NT_BATCH_SIZE, s->rec_len, s->rec_stride, s->batch_recs);
    pad_records(d->tri_recs, d->n_triangles, s->rec_len, s->rec_stride, s->tri_recs);
    s->batch_mats.assign(d->batch_mats, d->batch_mats + (size_t)d->n_batches * NT_BATCH_SIZE);
    s->tri_mats.assign(d->tri_mats, d->tri_mats + d->n_triangles);
    s->solid_recs.assign(d->solid_recs, d->solid_recs + (size_t)d->n_solids * (2 * n * n + n));
    s->solid_types.assign(d->solid_types, d->solid_types + d->n_solids);
    s->solid_mats.assign(d->solid_mats, d->solid_mats + d->n_solids);
    s->materials.resize((size_t)d->n_materials * 10);
    for (int i = 0; i < d->n_materials; ++i) {
        const nt_material &m = d->materials[i];
        float *o = s->materials.data() + (size_t)i * 10;
        o[0] = m.color[0]; o[1] = m.color[1]; o[2] = m.color[2];
        o[3] = m.specular[0]; o[4] = m.specular[1]; o[5] = m.specular[2];
        o[6] = m.opacity; o[7] = m.reflectivity; o[8] = m.specular_intensity; o[9] = m.specular_exp;
        if (!(m.opacity >= 1.0f)) s->all_opaque = false;       // primitive::opaque (tracer.hpp:187)
        if (m.reflectivity != 0.0f) s->any_reflective = true;
    }
    s->has_scalar = false;
    for (int i = 0; i < d->n_items; ++i) if ((d->items[i] & 3) != NT_KIND_BATCH) s->has_scalar = true;
    // the X-ray rule's live masks: a lane whose record is bytewise equal to an earlier lane of its batch is padding
    s->live_masks.assign((size_t)d->n_batches, 0);
    for (int b = 0; b < d->n_batches; ++b) {
        const float *recs = d->batch_recs + (size_t)b * NT_BATCH_SIZE * s->rec_len;
        for (int l = 0; l < NT_BATCH_SIZE; ++l) {
            bool dup = false;
            for (int e = 0; e < l && !dup; ++e)
                dup = std::memcmp(recs + (size_t)l * s->rec_len, recs + (size_t)e * s->rec_len, sizeof(float) * s->rec_len) == 0;
            if (!dup) s->live_masks[b] |= (uint8_t)(1u << l);
        }
    }
    s->aabb.assign(d->aabb_start, d->aabb_start + n);
    s->aabb.insert(s->aabb.end(), d->aabb_end, d->aabb_end + n);
    return s;
}

void nt_scene_destroy(nt_scene_t *s) {
    if (!s) return;
    for (auto &kv : s->devs) {
        DeviceState *ds = kv.second.get();
        if (hipSetDevice(ds->device) != hipSuccess) continue;
        (void)hipDeviceSynchronize();
        for (DevBuf *b : {&ds->nodes, &ds->items, &ds->batch_recs, &ds->batch_mats, &ds->tri_recs, &ds->tri_mats, &ds->solid_recs,
                          &ds->solid_types, &ds->solid_mats, &ds->materials, &ds->aabb, &ds->lights, &ds->framebuffer, &ds->cams, &ds->counter,
                          &ds->probes, &ds->stats, &ds->hits, &ds->stats_frame, &ds->samples, &ds->numer, &ds->cull, &ds->checked, &ds->tframes, &ds->ties, &ds->lens_dirs, &ds->live, &ds->xr_table})
            b->release();
        for (auto &t : ds->chan_tables) if (t->dev) (void)hipFree(t->dev);
        for (auto &t : ds->row_tables) if (t->dev) (void)hipFree(t->dev);
        for (auto &t : ds->tile_orders) t->buf.release();
        for (auto &st : ds->stage) {
            if (st.host) (void)hipHostFree(st.host);
            if (st.done) (void)hipEventDestroy(st.done);
        }
        if (ds->stream) (void)hipStreamDestroy(ds->stream);
        ds->abort_word.release();
        if (ds->abort_one) (void)hipHostFree(ds->abort_one);
        if (ds->side_stream) (void)hipStreamDestroy(ds->side_stream);
        if (ds->frame_done) (void)hipEventDestroy(ds->frame_done);
    }
    delete s;
}

int nt_scene_dimension(const nt_scene_t *s) { return s ? s->n : fail(NT_E_INVALID, "scene is NULL"); }
int nt_scene_is_composite(const nt_scene_t *s) { return s ? (s->composite ? 1 : 0) : fail(NT_E_INVALID, "scene is NULL"); }

int nt_scene_set_camera(nt_scene_t *s, const float *origin, const float *axes) {
    if (!s || !origin || !axes) return fail(NT_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->origin.assign(origin, origin + s->n);
    s->axes.assign(axes, axes + (size_t)s->n * s->n);
    return NT_OK;
}

int nt_scene_get_camera(const nt_scene_t *s, float *origin, float *axes) {
    if (!s || !origin || !axes) return fail(NT_E_INVALID, "NULL argument");
    std::memcpy(origin, s->origin.data(), sizeof(float) * s->n);
    std::memcpy(axes, s->axes.data(), sizeof(float) * s->n * s->n);
    return NT_OK;
}

namespace {
nt_lens_t *lens_new(int width, int height) {
    if (width < 1 || height < 1 || (long long)width * height > INT_MAX / 3) {
        fail(NT_E_INVALID, "invalid lens size %d x %d", width, height);
        return nullptr;
    }
    nt_lens *l = new (std::nothrow) nt_lens();
    if (!l) { fail(NT_E_NOMEM, "out of memory"); return nullptr; }
    l->d = std::make_shared<NtLensData>();
    l->d->width = width;
    l->d->height = height;
    l->d->coeffs.resize((size_t)width * height * 3);
    return l;
}
void lens_count_masked(NtLensData *d) {
    d->masked = 0;
    for (size_t i = 0; i < d->coeffs.size(); i += 3) {
        const float a = d->coeffs[i], b = d->coeffs[i + 1], c = d->coeffs[i + 2];
        if (!(a == a && b == b && c == c) || (a == 0.0f && b == 0.0f && c == 0.0f)) ++d->masked;
    }
}
}  // namespace

nt_lens_t *nt_lens_create(int width, int height, const float *coeffs) {
    if (!coeffs) { fail(NT_E_INVALID, "NULL argument"); return nullptr; }
    nt_lens *l = lens_new(width, height);
    if (!l) return nullptr;
    std::memcpy(l->d->coeffs.data(), coeffs, l->d->coeffs.size() * sizeof(float));
    lens_count_masked(l->d.get());
    return l;
}

nt_lens_t *nt_lens_create_pinhole(int width, int height, float fov) {
    nt_lens *l = lens_new(width, height);
    if (!l) return nullptr;
    // fill_view's constants and primary_dir's coefficients, expression for expression
    const float half_w = float(width) / float(2), half_h = float(height) / float(2);
    const float fovI = std::tan(fov / 2) / half_w;
    float *c = l->d->coeffs.data();
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x, c += 3) {
            c[0] = fovI * ((float)x - half_w);
            c[1] = fovI * ((float)y - half_h);
            c[2] = 1.0f;
        }
    lens_count_masked(l->d.get());
    return l;
}

void nt_lens_destroy(nt_lens_t *lens) { delete lens; }
int nt_lens_width(const nt_lens_t *lens) { return lens ? lens->d->width : fail(NT_E_INVALID, "lens is NULL"); }
int nt_lens_height(const nt_lens_t *lens) { return lens ? lens->d->height : fail(NT_E_INVALID, "lens is NULL"); }

int nt_lens_coeffs(const nt_lens_t *lens, float *out) {
    if (!lens || !out) return fail(NT_E_INVALID, "NULL argument");
    std::memcpy(out, lens->d->coeffs.data(), lens->d->coeffs.size() * sizeof(float));
    return NT_OK;
}

int nt_scene_set_lens(nt_scene_t *s, const nt_lens_t *lens) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    std::shared_ptr<NtLensData> old;               // (released outside the lock: the last owner waits for the device)
    {
        std::lock_guard<std::mutex> g(s->mu);
        if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
        if (lens && s->parallel > 0.0f) return fail(NT_E_INVALID, "a lens and the parallel projection exclude each other: take the parallel projection off first");
        old = std::move(s->lens);
        s->lens = lens ? lens->d : nullptr;
    }
    return NT_OK;
}

nt_lens_t *nt_scene_get_lens(const nt_scene_t *cs) {
    nt_scene *s = const_cast<nt_scene *>(cs);
    if (!s) { fail(NT_E_INVALID, "scene is NULL"); return nullptr; }
    std::lock_guard<std::mutex> g(s->mu);
    if (!s->lens) return nullptr;
    nt_lens *l = new (std::nothrow) nt_lens();
    if (!l) { fail(NT_E_NOMEM, "out of memory"); return nullptr; }
    l->d = s->lens;
    return l;
}

int nt_scene_set_parallel(nt_scene_t *s, float half_width) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (!(half_width >= 0.0f) || std::isinf(half_width)) return fail(NT_E_INVALID, "half_width must be a finite number >= 0");
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    if (half_width > 0.0f && s->lens) return fail(NT_E_INVALID, "the parallel projection and a lens exclude each other: take the lens off first");
    s->parallel = half_width > 0.0f ? half_width : 0.0f;
    return NT_OK;
}

float nt_scene_get_parallel(const nt_scene_t *cs) {
    nt_scene *s = const_cast<nt_scene *>(cs);
    if (!s) { fail(NT_E_INVALID, "scene is NULL"); return 0.0f; }
    std::lock_guard<std::mutex> g(s->mu);
    return s->parallel;
}

int nt_scene_set_fov(nt_scene_t *s, float fov) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->fov = fov;
    return NT_OK;
}

float nt_scene_get_fov(const nt_scene_t *s) { return s ? s->fov : 0.0f; }

int nt_scene_set_supersampling(nt_scene_t *s, int factor) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (factor < 1 || factor > 8) return fail(NT_E_INVALID, "the supersampling factor must be between 1 and 8");
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->supersampling = factor;
    return NT_OK;
}

int nt_scene_get_supersampling(const nt_scene_t *s) { return s ? s->supersampling : fail(NT_E_INVALID, "scene is NULL"); }

int nt_scene_set_supersampling_scratch_mb(nt_scene_t *s, int mib) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (mib < 1 || mib > (1 << 20)) return fail(NT_E_INVALID, "the supersampling scratch cap must be between 1 and %d MiB", 1 << 20);
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->ss_scratch_mb = mib;
    return NT_OK;
}

int nt_scene_get_supersampling_scratch_mb(const nt_scene_t *s) { return s ? s->ss_scratch_mb : fail(NT_E_INVALID, "scene is NULL"); }

int nt_scene_set_adaptive_supersampling(nt_scene_t *s, int enabled, float threshold) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (enabled && !std::isfinite(threshold)) return fail(NT_E_INVALID, "the adaptive threshold must be a finite number");
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->adaptive = enabled != 0;
    s->adaptive_t = enabled ? threshold : 0.0f;
    return NT_OK;
}

int nt_scene_get_adaptive_supersampling(const nt_scene_t *s, int *enabled, float *threshold) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (enabled) *enabled = s->adaptive ? 1 : 0;
    if (threshold) *threshold = s->adaptive_t;
    return NT_OK;
}

int nt_scene_set_ambient_occlusion(nt_scene_t *s, int count, const float *directions, float radius, float bias, float strength) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (!s->composite) return fail(NT_E_INVALID, "BoxScene has no ambient occlusion");
    if (count < 0 || count > 256) return fail(NT_E_INVALID, "the number of ambient occlusion samples must be between 0 and 256");
    if (count > 0) {
        if (!directions) return fail(NT_E_INVALID, "the ambient occlusion directions are NULL");
        for (int k = 0; k < count; ++k) {
            bool zero = true;
            for (int j = 0; j < s->n; ++j) {
                const float v = directions[(size_t)k * s->n + j];
                if (!std::isfinite(v)) return fail(NT_E_INVALID, "ambient occlusion direction %d has a component that is not finite", k);
                zero = zero && v == 0.0f;
            }
            if (zero) return fail(NT_E_INVALID, "ambient occlusion direction %d is all zero", k);
        }
        if (!(radius > 0.0f) || !std::isfinite(radius)) return fail(NT_E_INVALID, "the ambient occlusion radius must be positive and finite");
        if (!(bias >= 0.0f) || !std::isfinite(bias)) return fail(NT_E_INVALID, "the ambient occlusion bias must be finite and not negative");
        if (!(strength >= 0.0f && strength <= 1.0f)) return fail(NT_E_INVALID, "the ambient occlusion strength must lie in [0, 1]");
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->ao_count = count;
    if (count > 0) s->ao_dirs.assign(directions, directions + (size_t)count * s->n);
    else s->ao_dirs.clear();
    s->ao_radius = count > 0 ? radius : 0.0f;
    s->ao_bias = count > 0 ? bias : 0.0f;
    s->ao_strength = count > 0 ? strength : 0.0f;
    ++s->ao_version;
    return NT_OK;
}

int nt_scene_get_ambient_occlusion(const nt_scene_t *s, int *count, float *directions, float *radius, float *bias, float *strength) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (count) *count = s->ao_count;
    if (directions && s->ao_count > 0) std::memcpy(directions, s->ao_dirs.data(), s->ao_dirs.size() * sizeof(float));
    if (radius) *radius = s->ao_radius;
    if (bias) *bias = s->ao_bias;
    if (strength) *strength = s->ao_strength;
    return NT_OK;
}

int nt_scene_set_outlines(nt_scene_t *s, int enabled, float crease_cos, float depth_gap, const float color[3], float strength) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (!s->composite) return fail(NT_E_INVALID, "BoxScene has no outlines: its lines are nt_scene_set_box_lines");
    if (enabled) {
        if (!color) return fail(NT_E_INVALID, "the outline colour is NULL");
        if (!(crease_cos >= 0.0f && crease_cos <= 1.0f)) return fail(NT_E_INVALID, "the outlines' crease_cos must lie in [0, 1]");
        if (!(depth_gap >= 0.0f) || !std::isfinite(depth_gap)) return fail(NT_E_INVALID, "the outlines' depth_gap must be finite and not negative");
        for (int k = 0; k < 3; ++k)
            if (!(color[k] >= 0.0f && color[k] <= 1.0f)) return fail(NT_E_INVALID, "the outline colour's components must lie in [0, 1]");
        if (!(strength >= 0.0f && strength <= 1.0f)) return fail(NT_E_INVALID, "the outlines' strength must lie in [0, 1]");
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->outlines = enabled != 0;
    s->ol_crease_cos = enabled ? crease_cos : 0.0f;
    s->ol_depth_gap = enabled ? depth_gap : 0.0f;
    for (int k = 0; k < 3; ++k) s->ol_color[k] = enabled ? color[k] : 0.0f;
    s->ol_strength = enabled ? strength : 0.0f;
    return NT_OK;
}

int nt_scene_get_outlines(const nt_scene_t *s, int *enabled, float *crease_cos, float *depth_gap, float color[3], float *strength) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (enabled) *enabled = s->outlines ? 1 : 0;
    if (crease_cos) *crease_cos = s->ol_crease_cos;
    if (depth_gap) *depth_gap = s->ol_depth_gap;
    if (color) for (int k = 0; k < 3; ++k) color[k] = s->ol_color[k];
    if (strength) *strength = s->ol_strength;
    return NT_OK;
}

int nt_scene_set_box_lines(nt_scene_t *s, int kinds, const float color[3], float strength) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (s->composite) return fail(NT_E_INVALID, "not a box scene: CompositeScene has outlines (nt_scene_set_outlines)");
    if (kinds) {
        if (kinds & ~(NT_OUTLINE_SILHOUETTE | NT_OUTLINE_CREASE))
            return fail(NT_E_INVALID, "the face lines' kinds are an OR of NT_OUTLINE_SILHOUETTE and NT_OUTLINE_CREASE (%d)", kinds);
        if (!color) return fail(NT_E_INVALID, "the face lines' colour is NULL");
        for (int k = 0; k < 3; ++k)
            if (!(color[k] >= 0.0f && color[k] <= 1.0f)) return fail(NT_E_INVALID, "the face lines' colour components must lie in [0, 1]");
        if (!(strength >= 0.0f && strength <= 1.0f)) return fail(NT_E_INVALID, "the face lines' strength must lie in [0, 1]");
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->box_lines = kinds;
    for (int k = 0; k < 3; ++k) s->bl_color[k] = kinds ? color[k] : 0.0f;
    s->bl_strength = kinds ? strength : 0.0f;
    return NT_OK;
}

int nt_scene_get_box_lines(const nt_scene_t *s, int *kinds, float color[3], float *strength) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (s->composite) return fail(NT_E_INVALID, "not a box scene");
    if (kinds) *kinds = s->box_lines;
    if (color) for (int k = 0; k < 3; ++k) color[k] = s->bl_color[k];
    if (strength) *strength = s->bl_strength;
    return NT_OK;
}

namespace {
bool cue_unit(float v) { return v >= 0.0f && v <= 1.0f; }          // (false for a NaN)

// what nt_scene_set_depth_cue and nt_scene_set_box_shading check of a cue and its tint axis, and what they keep of them: the cue
// with fog_background 0 or 1 and the tint's fields zero without a tint, the axis, the two reciprocals
int cue_validate(int n, const nt_depth_cue *cue, const float *tint_axis, nt_depth_cue &set, std::vector<float> &axis, float &inv_fog, float &inv_tint) {
    set = *cue;
    set.fog_background = cue->fog_background != 0;
    if (!std::isfinite(set.fog_near) || !std::isfinite(set.fog_far) || !(set.fog_near >= 0.0f) || !(set.fog_far > set.fog_near))
        return fail(NT_E_INVALID, "the depth cue's fog range must be finite with 0 <= fog_near < fog_far");
    inv_fog = 1.0f / (set.fog_far - set.fog_near);
    if (!std::isfinite(inv_fog)) return fail(NT_E_INVALID, "the depth cue's fog range is too narrow: 1 / (fog_far - fog_near) is not finite");
    for (int k = 0; k < 3; ++k)
        if (!cue_unit(set.fog_color[k])) return fail(NT_E_INVALID, "the depth cue's fog colour components must lie in [0, 1]");
    if (!cue_unit(set.fog_strength)) return fail(NT_E_INVALID, "the depth cue's fog_strength must lie in [0, 1]");
    if (tint_axis) {
        if (!std::isfinite(set.tint_lo) || !std::isfinite(set.tint_hi) || !(set.tint_hi > set.tint_lo))
            return fail(NT_E_INVALID, "the depth cue's tint range must be finite with tint_lo < tint_hi");
        inv_tint = 1.0f / (set.tint_hi - set.tint_lo);
        if (!std::isfinite(inv_tint)) return fail(NT_E_INVALID, "the depth cue's tint range is too narrow: 1 / (tint_hi - tint_lo) is not finite");
        for (int k = 0; k < 3; ++k)
            if (!cue_unit(set.tint_color_lo[k]) || !cue_unit(set.tint_color_hi[k]))
                return fail(NT_E_INVALID, "the depth cue's tint colour components must lie in [0, 1]");
        axis.assign(tint_axis, tint_axis + n);
        bool any = false;
        for (float v : axis) {
            if (!std::isfinite(v)) return fail(NT_E_INVALID, "the depth cue's tint_axis must be finite");
            any = any || v != 0.0f;
        }
        if (!any) return fail(NT_E_INVALID, "the depth cue's tint_axis must not be all zero");
    } else {
        set.tint_lo = set.tint_hi = 0.0f;
        for (int k = 0; k < 3; ++k) set.tint_color_lo[k] = set.tint_color_hi[k] = 0.0f;
    }
    return NT_OK;
}
}  // namespace

int nt_scene_set_depth_cue(nt_scene_t *s, const nt_depth_cue *cue, const float *tint_axis) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (!s->composite) return fail(NT_E_INVALID, "BoxScene has no depth cue");
    nt_depth_cue set{};
    std::vector<float> axis;
    float inv_fog = 0.0f, inv_tint = 0.0f;
    if (cue) {
        if (int r = cue_validate(s->n, cue, tint_axis, set, axis, inv_fog, inv_tint)) return r;
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->cue = cue != nullptr;
    s->cue_tint = cue && tint_axis;
    s->cue_set = set;
    s->cue_axis = std::move(axis);
    s->cue_inv_fog = inv_fog;
    s->cue_inv_tint = inv_tint;
    return NT_OK;
}

int nt_scene_get_depth_cue(const nt_scene_t *s, int *enabled, nt_depth_cue *cue, int *has_tint, float *tint_axis) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (enabled) *enabled = s->cue ? 1 : 0;
    if (cue) *cue = s->cue_set;
    if (has_tint) *has_tint = s->cue_tint ? 1 : 0;
    if (tint_axis) for (int k = 0; k < s->n; ++k) tint_axis[k] = s->cue_tint ? s->cue_axis[k] : 0.0f;
    return NT_OK;
}

int nt_scene_set_box_shading(nt_scene_t *s, const float *face_colors, const nt_depth_cue *cue, const float *tint_axis) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (s->composite) return fail(NT_E_INVALID, "not a box scene: CompositeScene has depth cues (nt_scene_set_depth_cue)");
    std::vector<float> table, axis;
    nt_depth_cue set{};
    float inv_fog = 0.0f, inv_tint = 0.0f;
    if (face_colors) {
        table.assign(face_colors, face_colors + (size_t)s->n * 6);
        for (float v : table)
            if (!cue_unit(v)) return fail(NT_E_INVALID, "the face colours' components must lie in [0, 1]");
    }
    if (cue) {
        if (int r = cue_validate(s->n, cue, tint_axis, set, axis, inv_fog, inv_tint)) return r;
    } else if (tint_axis) {
        return fail(NT_E_INVALID, "face shading: a tint_axis needs a cue, which holds the tint's range and colours");
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->box_shading = face_colors || cue;
    s->bs_colors = face_colors != nullptr;
    s->bs_cue = cue != nullptr;
    s->bs_tint = cue && tint_axis;
    s->bs_table = std::move(table);
    s->bs_set = set;
    s->bs_axis = std::move(axis);
    s->bs_inv_fog = inv_fog;
    s->bs_inv_tint = inv_tint;
    return NT_OK;
}

int nt_scene_get_box_shading(const nt_scene_t *s, int *enabled, int *has_colors, float *face_colors, int *has_cue, nt_depth_cue *cue,
                             int *has_tint, float *tint_axis) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (s->composite) return fail(NT_E_INVALID, "not a box scene");
    if (enabled) *enabled = s->box_shading ? 1 : 0;
    if (has_colors) *has_colors = s->bs_colors ? 1 : 0;
    if (face_colors)
        for (int k = 0; k < 6 * s->n; ++k) face_colors[k] = s->bs_colors ? s->bs_table[k] : (k % 3 == 0 ? 1.0f : 0.5f);
    if (has_cue) *has_cue = s->bs_cue ? 1 : 0;
    if (cue) *cue = s->bs_set;
    if (has_tint) *has_tint = s->bs_tint ? 1 : 0;
    if (tint_axis) for (int k = 0; k < s->n; ++k) tint_axis[k] = s->bs_tint ? s->bs_axis[k] : 0.0f;
    return NT_OK;
}

int nt_scene_set_clip_planes(nt_scene_t *s, int count, const float *normals, const float *offsets) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (!s->composite) return fail(NT_E_INVALID, "BoxScene has no clip planes");
    if (count < 0 || count > NT_CLIP_MAX) return fail(NT_E_INVALID, "the number of clip planes must lie in [0, %d] (%d)", NT_CLIP_MAX, count);
    if (!normals || !offsets) count = 0;
    const int n = s->n;
    std::vector<float> planes((size_t)count * (n + 1));
    for (int k = 0; k < count; ++k) {
        bool any = false;
        for (int j = 0; j < n; ++j) {
            const float v = normals[(size_t)k * n + j];
            if (!std::isfinite(v)) return fail(NT_E_INVALID, "the normal of clip plane %d must be finite", k);
            any = any || v != 0.0f;
            planes[(size_t)k * (n + 1) + j] = v;
        }
        if (!any) return fail(NT_E_INVALID, "the normal of clip plane %d must not be all zero", k);
        if (!std::isfinite(offsets[k])) return fail(NT_E_INVALID, "the offset of clip plane %d must be finite", k);
        planes[(size_t)k * (n + 1) + n] = offsets[k];
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->clip_count = count;
    s->clip_planes = std::move(planes);
    ++s->clip_version;
    return NT_OK;
}

int nt_scene_get_clip_planes(const nt_scene_t *s, int *count, float *normals, float *offsets) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    std::lock_guard<std::mutex> g(const_cast<nt_scene_t *>(s)->mu);      // (the setter swaps the vector under it)
    if (count) *count = s->clip_count;
    const int n = s->n;
    for (int k = 0; k < s->clip_count; ++k) {
        if (normals) std::memcpy(normals + (size_t)k * n, s->clip_planes.data() + (size_t)k * (n + 1), sizeof(float) * n);
        if (offsets) offsets[k] = s->clip_planes[(size_t)k * (n + 1) + n];
    }
    return NT_OK;
}

int nt_scene_set_view_stack(nt_scene_t *s, int count, const float *offsets, float focus, const float *weights) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (count < 0 || count > NT_STACK_MAX) return fail(NT_E_INVALID, "a view stack has between 0 and %d samples (%d)", NT_STACK_MAX, count);
    if (count > 0 && !offsets) return fail(NT_E_INVALID, "the offsets of a view stack are NULL");
    const int n = s->n;
    std::vector<float> off, wts;
    float r = 0.0f;
    // (the focus is checked whatever the count: a call that takes the setting off with a bad focus is a mistake too)
    if (!(focus >= 0.0f) || !std::isfinite(focus)) return fail(NT_E_INVALID, "the focus of a view stack must be finite and not negative (0: none)");
    if (count > 0) {
        if (focus > 0.0f) {
            r = 1.0f / focus;
            if (!std::isfinite(r)) return fail(NT_E_INVALID, "the focus of a view stack is too small: 1 / focus must be finite");
        }
        off.assign(offsets, offsets + (size_t)count * n);
        for (size_t i = 0; i < off.size(); ++i)
            if (!std::isfinite(off[i])) return fail(NT_E_INVALID, "offset %d of the view stack has a component that is not finite", (int)(i / n));
        wts.assign((size_t)count * 3, 1.0f / (float)count);
        if (weights) {
            wts.assign(weights, weights + (size_t)count * 3);
            for (size_t i = 0; i < wts.size(); ++i)
                if (!std::isfinite(wts[i])) return fail(NT_E_INVALID, "weight %d of the view stack has a component that is not finite", (int)(i / 3));
        }
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->stack_count = count;
    s->stack_offsets = std::move(off);
    s->stack_weights = std::move(wts);
    s->stack_focus = count > 0 ? focus : 0.0f;
    s->stack_r = r;
    ++s->stack_version;
    return NT_OK;
}

int nt_scene_get_view_stack(const nt_scene_t *s, int *count, float *offsets, float *focus, float *weights) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    std::lock_guard<std::mutex> g(const_cast<nt_scene_t *>(s)->mu);      // (the setter swaps the vectors under it)
    if (count) *count = s->stack_count;
    if (focus) *focus = s->stack_focus;
    if (offsets && s->stack_count) std::memcpy(offsets, s->stack_offsets.data(), sizeof(float) * s->stack_offsets.size());
    if (weights && s->stack_count) std::memcpy(weights, s->stack_weights.data(), sizeof(float) * s->stack_weights.size());
    return NT_OK;
}

int nt_scene_set_view_stack_route(nt_scene_t *s, int route) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (route != NT_STACK_ROUTE_AUTO && route != NT_STACK_ROUTE_FRAMES) return fail(NT_E_INVALID, "the route of a view stack is NT_STACK_ROUTE_AUTO or NT_STACK_ROUTE_FRAMES (%d)", route);
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->stack_route = route;
    return NT_OK;
}

int nt_scene_get_view_stack_route(const nt_scene_t *s) { return s ? s->stack_route : fail(NT_E_INVALID, "scene is NULL"); }

int nt_scene_set_xray(nt_scene_t *s, int enabled, float absorbance, float tint) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (!s->composite) return fail(NT_E_INVALID, "BoxScene has no X-ray: a ray crosses exactly two of its faces (nt_box_hits)");
    std::vector<float> table;
    if (enabled) {
        if (!(absorbance >= 0.0f && absorbance <= 1.0f)) return fail(NT_E_INVALID, "the X-ray's absorbance must lie in [0, 1]");
        if (!(tint >= 0.0f && tint <= 1.0f)) return fail(NT_E_INVALID, "the X-ray's tint must lie in [0, 1]");
        // T[m][c] = clamp01(1.0f - absorbance * (1.0f - tint * color_m[c])), every operation rounded on its own
        table.resize((size_t)s->n_materials * 3);
        for (int m = 0; m < s->n_materials; ++m)
            for (int c = 0; c < 3; ++c) {
                const float tc = tint * s->materials[(size_t)m * 10 + c];
                const float in = 1.0f - tc;
                const float ab = absorbance * in;
                float t = 1.0f - ab;
                t = t > 0.0f ? t : 0.0f;
                t = t < 1.0f ? t : 1.0f;
                table[(size_t)m * 3 + c] = t;
            }
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->xray = enabled != 0;
    s->xr_absorbance = enabled ? absorbance : 0.0f;
    s->xr_tint = enabled ? tint : 0.0f;
    s->xr_table = std::move(table);
    ++s->xr_version;
    return NT_OK;
}

int nt_scene_get_xray(const nt_scene_t *s, int *enabled, float *absorbance, float *tint, float *table) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    std::lock_guard<std::mutex> g(const_cast<nt_scene_t *>(s)->mu);      // (the setter swaps the vector under it)
    if (enabled) *enabled = s->xray ? 1 : 0;
    if (absorbance) *absorbance = s->xr_absorbance;
    if (tint) *tint = s->xr_tint;
    if (table && s->xray && !s->xr_table.empty()) std::memcpy(table, s->xr_table.data(), sizeof(float) * s->xr_table.size());
    return NT_OK;
}

int nt_scene_batch_live_masks(const nt_scene_t *s, uint8_t *masks) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    if (!s->composite) return fail(NT_E_INVALID, "not a composite scene");
    if (masks && !s->live_masks.empty()) std::memcpy(masks, s->live_masks.data(), s->live_masks.size());
    return s->n_batches;
}

int nt_view_stack_cameras(const nt_scene_t *s, const float *origin, const float *axes, float *origins_out, float *axes_out) {
    if (!s || !origins_out || !axes_out) return fail(NT_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<nt_scene_t *>(s)->mu);
    if (s->stack_count < 1) return fail(NT_E_INVALID, "the view stack is off (nt_scene_set_view_stack)");
    stack_cameras_host(s, origin ? origin : s->origin.data(), axes ? axes : s->axes.data(), origins_out, axes_out);
    return NT_OK;
}

int nt_scene_set_params(nt_scene_t *s, const nt_scene_params *p) {
    if (!s || !p) return fail(NT_E_INVALID, "NULL argument");
    if (!s->composite) return fail(NT_E_INVALID, "BoxScene has no lighting parameters");
    if (p->bg_gradient_axis < 0 || p->bg_gradient_axis >= s->n) return fail(NT_E_INVALID, "bg_gradient_axis out of range");
    if (p->n_point_lights < 0 || p->n_global_lights < 0) return fail(NT_E_INVALID, "negative light count");
    if ((p->n_point_lights && (!p->point_light_pos || !p->point_light_color)) || (p->n_global_lights && (!p->global_light_dir || !p->global_light_color)))
        return fail(NT_E_INVALID, "light arrays are NULL");
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked) return fail(NT_E_LOCKED, "the scene is locked for reading");
    s->shadows = p->shadows ? 1 : 0;
    s->camera_light = p->camera_light ? 1 : 0;
    s->max_reflect_depth = p->max_reflect_depth;
    s->bg_axis = p->bg_gradient_axis;
    for (int k = 0; k < 3; ++k) { s->ambient[k] = p->ambient[k]; s->bg1[k] = p->bg1[k]; s->bg2[k] = p->bg2[k]; s->bg3[k] = p->bg3[k]; }
    const int n = s->n;
    s->pl_pos.assign(p->point_light_pos, p->point_light_pos + (size_t)p->n_point_lights * n);
    s->pl_color.assign(p->point_light_color, p->point_light_color + (size_t)p->n_point_lights * 3);
    s->gl_dir.assign(p->global_light_dir, p->global_light_dir + (size_t)p->n_global_lights * n);
    s->gl_color.assign(p->global_light_color, p->global_light_color + (size_t)p->n_global_lights * 3);
    ++s->lights_version;
    return NT_OK;
}

int nt_scene_lock(nt_scene_t *s) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    std::lock_guard<std::mutex> g(s->mu);
    ++s->locked;
    return NT_OK;
}

int nt_scene_unlock(nt_scene_t *s) {
    if (!s) return fail(NT_E_INVALID, "scene is NULL");
    std::lock_guard<std::mutex> g(s->mu);
    if (s->locked <= 0) return fail(NT_E_INVALID, "the scene is not locked");
    --s->locked;
    return NT_OK;
}

int nt_scene_locked(const nt_scene_t *s) { return s ? (s->locked > 0 ? 1 : 0) : fail(NT_E_INVALID, "scene is NULL"); }

int nt_format_bytes_per_pixel(const nt_image_format *fmt) {
    Format f;
    if (int r = parse_format(fmt, f)) return r;
    return f.bpp;
}

int nt_render(nt_scene_t *s, void *dest, size_t dest_len, const nt_image_format *fmt, const nt_render_opts *opts, volatile int *abort_flag) {
    if (!s || !dest) return fail(NT_E_INVALID, "NULL argument");
    Format f;
    if (int r = parse_format(fmt, f)) return r;
    Bands b;
    if (int r = parse_bands(opts, f.height, b)) return r;
    const size_t need = required_len(f, b);
    if (dest_len < need) return fail(NT_E_INVALID, "the buffer is too small for an image with the given dimensions");
    if (int r = check_renderable(s)) return r;
    RenderGuard guard(s);
    if (int r = guard.acquire()) return r;
    const bool stats = opts && opts->collect_stats;
    if (int r = render_checks(s, f, b, stats)) return r;
    if (abort_flag && *abort_flag) return NT_ABORTED;           // (before anything touches `dest` or the device)
    DeviceState *ds;
    if (int r = scene_on_device(s, opts, -1, ds)) return r;
    if (int r = use_own_stream(ds)) return r;
    if (int r = ds->framebuffer.ensure(std::max<size_t>(need, 16))) return r;
    if (int r = prepare_stats(ds, ds->stream, stats)) return r;
    // pitch padding bytes are not written by the kernels: carry the caller's bytes through
    if (f.pitch != f.width * f.bpp || (b.world > 1 && !b.compact)) HIP_TRY(hipMemcpyAsync(ds->framebuffer.p, dest, need, hipMemcpyHostToDevice, ds->stream));

    FrameJob job = render_job(f, b, ds->framebuffer.p, 0, 1, ds->stream, stats, opts, false);
    // Abort (the reference's workers poll renderer::CANCEL per pixel, render.cpp:412): ONE launch for the frame -- cutting it
    // into slabs cost a 120-cell frame a kernel tail per slab (9.3 ms instead of 1.2) -- whose blocks read a dword in device
    // memory when they start, and the packet kernel's waves every few dozen nodes (NtTarget::abort_word).  The host waits for the
    // frame with an eye on the caller's flag and raises that word when the flag goes up: what has not started leaves at once,
    // so an abort costs what the waves in flight need to reach their next look at the word.  An aborted frame is incomplete
    // in no particular order; nothing of it is copied back -- the caller's buffer stays as it was.
    if (abort_flag) {
        if (!ds->abort_one) {
            if (int r = ds->abort_word.ensure(64)) return r;
            void *p = nullptr;
            HIP_TRY(hipHostMalloc(&p, 64, hipHostMallocDefault));
            ds->abort_one = (int *)p;
            *ds->abort_one = 1;
            HIP_TRY(hipStreamCreateWithFlags(&ds->side_stream, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&ds->frame_done, hipEventDisableTiming));
        }
        HIP_TRY(hipMemsetAsync(ds->abort_word.p, 0, 4, ds->stream));
        job.abort_word = (const int *)ds->abort_word.p;
    }
    if (int r = enqueue(s, ds, job)) { (void)hipStreamSynchronize(ds->stream); return r; }
    bool aborted = false;
    if (abort_flag) {
        HIP_TRY(hipEventRecord(ds->frame_done, ds->stream));
        while (hipEventQuery(ds->frame_done) == hipErrorNotReady) {
            if (!aborted && *abort_flag) {
                (void)hipMemcpyAsync(ds->abort_word.p, ds->abort_one, 4, hipMemcpyHostToDevice, ds->side_stream);
                aborted = true;
            }
            std::this_thread::yield();
        }
    }
    if (!aborted && need) HIP_TRY(hipMemcpyAsync(dest, ds->framebuffer.p, need, hipMemcpyDeviceToHost, ds->stream));
    HIP_TRY(hipStreamSynchronize(ds->stream));
    if (aborted) HIP_TRY(hipStreamSynchronize(ds->side_stream));
    if (stats) {
        unsigned long long v[8];
        HIP_TRY(hipMemcpy(v, ds->stats.p, sizeof(v), hipMemcpyDeviceToHost));
        s->last_stats.rays = v[0]; s->last_stats.shadow_rays = v[1]; s->last_stats.branches = v[2]; s->last_stats.leaves = v[3];
        s->last_stats.simplex_tests = v[4]; s->last_stats.solid_tests = v[5]; s->last_stats.hits = v[6]; s->last_stats.aabb_enter = v[7];
        s->have_stats = true;
    }
    return aborted ? NT_ABORTED : NT_OK;
}

int nt_render_device(nt_scene_t *s, void *dest_dev, size_t dest_len, const nt_image_format *fmt, const nt_render_opts *opts, void *hip_stream) {
    if (!s || !dest_dev) return fail(NT_E_INVALID, "NULL argument");
    Format f;
    if (int r = parse_format(fmt, f)) return r;
    Bands b;
    if (int r = parse_bands(opts, f.height, b)) return r;
    if (dest_len < required_len(f, b)) return fail(NT_E_INVALID, "the buffer is too small for an image with the given dimensions");
    if (int r = check_renderable(s)) return r;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->busy) return fail(NT_E_BUSY, "the renderer is already running");
    const bool stats = opts && opts->collect_stats;
    if (int r = render_checks(s, f, b, stats)) return r;
    DeviceState *ds;
    if (int r = scene_on_device(s, opts, -1, ds)) return r;
    if (int r = use_stream(ds, (hipStream_t)hip_stream)) return r;
    if (int r = prepare_stats(ds, (hipStream_t)hip_stream, stats)) return r;
    if (stats) { s->have_stats = false; s->stats_device = ds->device; }
    return enqueue(s, ds, render_job(f, b, dest_dev, 0, 1, (hipStream_t)hip_stream, stats, opts, true));
}

int nt_render_frames_device(nt_scene_t *s, void *dest_dev, size_t frame_stride, int nframes, const float *origins, const float *axes,
                            const nt_image_format *fmt, const nt_render_opts *opts, void *hip_stream) {
    if (!s || !dest_dev || !origins || !axes) return fail(NT_E_INVALID, "NULL argument");
    if (nframes < 1 || nframes > 65535) return fail(NT_E_INVALID, "nframes must be between 1 and 65535");
    Format f;
    if (int r = parse_format(fmt, f)) return r;
    Bands b;
    if (int r = parse_bands(opts, f.height, b)) return r;
    if (frame_stride < required_len(f, b)) return fail(NT_E_INVALID, "frame_stride is smaller than one frame");
    if (int r = check_renderable(s)) return r;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->busy) return fail(NT_E_BUSY, "the renderer is already running");
    const bool stats = opts && opts->collect_stats;
    if (int r = render_checks(s, f, b, stats)) return r;
    DeviceState *ds;
    if (int r = scene_on_device(s, opts, -1, ds)) return r;
    {
        // This entry point stages the caller's host arrays in a pinned slot that later calls reuse: a graph would replay the
        // launch, not the staging.  Refused while `hip_stream` is being captured -- a camera table (nt_render_table_device), whose
        // cameras live in device memory, is what a graph wants (tests: test_render_calls_captured_in_a_hip_graph).
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)hip_stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return fail(NT_E_UNSUPPORTED, "nt_render_frames_device stages host cameras per call and cannot be captured into a graph: use a camera table");
    }
    if (int r = use_stream(ds, (hipStream_t)hip_stream)) return r;
    const int n = s->n;
    // (under a view stack all the axes travel behind the table: stack_cameras reads the hidden rows too)
    const size_t table_floats = (size_t)nframes * 4 * n + (size_t)nframes * 4;
    const size_t cam_floats = table_floats + (s->stack_count > 0 ? (size_t)nframes * n * n : 0);
    DeviceState::Stage *st = nullptr;
    if (int r = stage_slot(ds, cam_floats * sizeof(float), st)) return r;
    float *packed = (float *)st->host;
    pack_cameras(n, nframes, origins, axes, packed);
    if (s->stack_count > 0) std::memcpy(packed + table_floats, axes, sizeof(float) * nframes * n * n);
    // a camera table that earlier launches may still read must not be overwritten: grow-only buffer,
    // refilled only after the stream that used it has drained (same-stream ordering)
    if (int r = ds->cams.ensure(cam_floats * sizeof(float))) return r;
    // a copy kernel on the launch stream reads the pinned slot in place; the event keeps the slot from reuse until it has
    // (removed: NTRACER_CAM_UPLOAD=memcpy, and NTRACER_STAGE_EVENT=0, which skipped the event: unsafe beyond 8 calls in flight)
    if (int r = nt_launch_upload(hip_stream, packed, (float *)ds->cams.p, (int)cam_floats)) return launch_failed(r);
    HIP_TRY(hipEventRecord(st->done, (hipStream_t)hip_stream));
    st->in_flight = true;
    if (int r = prepare_stats(ds, (hipStream_t)hip_stream, stats)) return r;
    if (stats) { s->have_stats = false; s->stats_device = ds->device; }
    FrameJob job = render_job(f, b, dest_dev, frame_stride, nframes, (hipStream_t)hip_stream, stats, opts, true);
    job.cam_buf = (const float *)ds->cams.p;
    job.cam_dots = job.cam_buf + (size_t)nframes * 4 * s->n;
    if (s->stack_count > 0) job.cam_axes = job.cam_buf + table_floats;
    return enqueue(s, ds, job);
}

struct nt_camera_table {
    int n = 0, nframes = 0, device = -1;
    float *dev = nullptr;                // [nframes][4][n] camera rows, then [nframes][4] dot products (NtCamera::buf), then
                                         // [nframes][2] spans (NtCamera::span), then [nframes][n][n], all the axes of the
                                         // cameras, which a view stack's hidden offsets need (FrameJob::cam_axes)
};

nt_camera_table_t *nt_camera_table_create(int dimension, int nframes, const float *origins, const float *axes, int device) {
    if (dimension < 3 || dimension > NT_MAX_DIM || nframes < 1 || nframes > 65535 || !origins || !axes) {
        fail(NT_E_INVALID, "invalid camera table arguments");
        return nullptr;
    }
    int dev;
    if (pick_device(nullptr, device, dev)) return nullptr;
    const int n = dimension;
    const size_t span_at = (size_t)nframes * 4 * n + (size_t)nframes * 4;
    const size_t axes_at = span_at + (size_t)nframes * 2;
    const size_t cam_floats = axes_at + (size_t)nframes * n * n;
    std::vector<float> packed(cam_floats);
    pack_cameras(n, nframes, origins, axes, packed.data());
    std::memcpy(packed.data() + axes_at, axes, sizeof(float) * nframes * n * n);
    // the span of every camera (nt_box_span.hpp): once here, a few microseconds each, for the 510 waves of every frame that would
    // each work it out again in their stretch codes.  (The table does not know its scene: only BoxScene's tile kernel reads them.)
    for (int f = 0; f < nframes; ++f) {
        const float *o = origins + (size_t)f * n, *ax = axes + (size_t)f * n * n;
        const NtBoxSpan sp = nt_box_strip_span(n, o, ax, ax + n, ax + 2 * n);
        packed[span_at + 2 * (size_t)f] = sp.lo;
        packed[span_at + 2 * (size_t)f + 1] = sp.hi;
    }
    void *p = nullptr;
    if (hipMalloc(&p, cam_floats * sizeof(float)) != hipSuccess) { fail(NT_E_NOMEM, "hipMalloc failed for the camera table"); return nullptr; }
    if (hipMemcpy(p, packed.data(), cam_floats * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p);
        fail(NT_E_DEVICE, "camera table upload failed");
        return nullptr;
    }
    nt_camera_table *t = new (std::nothrow) nt_camera_table();
    if (!t) { (void)hipFree(p); fail(NT_E_NOMEM, "out of memory"); return nullptr; }
    t->n = n; t->nframes = nframes; t->device = dev; t->dev = (float *)p;
    return t;
}

void nt_camera_table_destroy(nt_camera_table_t *t) {
    if (!t) return;
    if (t->dev && hipSetDevice(t->device) == hipSuccess) { (void)hipDeviceSynchronize(); (void)hipFree(t->dev); }
    delete t;
}

int nt_camera_table_frames(const nt_camera_table_t *t) { return t ? t->nframes : fail(NT_E_INVALID, "table is NULL"); }

int nt_render_table_device(nt_scene_t *s, void *dest_dev, size_t frame_stride, const nt_camera_table_t *table, int first, int count,
                           const nt_image_format *fmt, const nt_render_opts *opts, void *hip_stream) {
    if (!s || !dest_dev || !table) return fail(NT_E_INVALID, "NULL argument");
    if (table->n != s->n) return fail(NT_E_INVALID, "the camera table is for %d dimensions, the scene has %d", table->n, s->n);
    if (first < 0 || count < 1 || first > table->nframes - count) return fail(NT_E_INVALID, "frames %d..%d are not in a table of %d", first, first + count - 1, table->nframes);
    Format f;
    if (int r = parse_format(fmt, f)) return r;
    Bands b;
    if (int r = parse_bands(opts, f.height, b)) return r;
    if (frame_stride < required_len(f, b)) return fail(NT_E_INVALID, "frame_stride is smaller than one frame");
    if (int r = check_renderable(s)) return r;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->busy) return fail(NT_E_BUSY, "the renderer is already running");
    const bool stats = opts && opts->collect_stats;
    if (int r = render_checks(s, f, b, stats)) return r;
    DeviceState *ds;
    if (int r = scene_on_device(s, opts, -1, ds, table->device, "render")) return r;
    if (int r = use_stream(ds, (hipStream_t)hip_stream)) return r;
    if (int r = prepare_stats(ds, (hipStream_t)hip_stream, stats)) return r;
    if (stats) { s->have_stats = false; s->stats_device = ds->device; }
    FrameJob job = render_job(f, b, dest_dev, frame_stride, count, (hipStream_t)hip_stream, stats, opts, true);
    job.cam_buf = table->dev + (size_t)first * 4 * table->n;                                  // (the table: all cameras, then all dot products)
    job.cam_dots = table->dev + (size_t)table->nframes * 4 * table->n + (size_t)first * 4;
    job.cam_span = table->dev + (size_t)table->nframes * (4 * table->n + 4) + (size_t)first * 2;
    job.cam_axes = table->dev + (size_t)table->nframes * (4 * table->n + 6) + (size_t)first * table->n * table->n;
    return enqueue(s, ds, job);
}

int nt_adaptive_mask(nt_scene_t *s, int width, int height, uint8_t *mask, long long *flagged, const nt_render_opts *opts) {
    RenderGuard guard(s);
    DeviceState *ds;
    if (int r = view_query_host(guard, kAdaptiveMask, width, height, mask, opts, &ds)) return r;
    int count = 0;
    HIP_TRY(hipMemcpyAsync(&count, ds->refine_count.p, sizeof(int), hipMemcpyDeviceToHost, ds->stream));
    HIP_TRY(hipStreamSynchronize(ds->stream));
    if (flagged) *flagged = count;
    return NT_OK;
}

int nt_adaptive_mask_device(nt_scene_t *s, int width, int height, void *mask_dev, const nt_render_opts *opts, void *hip_stream) {
    return view_query_device(s, kAdaptiveMask, width, height, mask_dev, opts, hip_stream);
}

int nt_ambient_occlusion(nt_scene_t *s, int width, int height, int32_t *blocked, const nt_render_opts *opts) {
    RenderGuard guard(s);
    return view_query_host(guard, kAoCounts, width, height, blocked, opts);
}

int nt_ambient_occlusion_device(nt_scene_t *s, int width, int height, void *blocked_dev, const nt_render_opts *opts, void *hip_stream) {
    return view_query_device(s, kAoCounts, width, height, blocked_dev, opts, hip_stream);
}

int nt_outline_mask(nt_scene_t *s, int width, int height, uint8_t *mask, long long *marked, const nt_render_opts *opts) {
    RenderGuard guard(s);
    if (int r = view_query_host(guard, kOutlineMask, width, height, mask, opts)) return r;
    if (marked) *marked = marked_pixels(mask, (size_t)width * height);
    return NT_OK;
}

int nt_outline_mask_device(nt_scene_t *s, int width, int height, void *mask_dev, const nt_render_opts *opts, void *hip_stream) {
    return view_query_device(s, kOutlineMask, width, height, mask_dev, opts, hip_stream);
}

int nt_crossing_counts(nt_scene_t *s, int width, int height, int32_t *counts, const nt_render_opts *opts) {
    RenderGuard guard(s);
    return view_query_host(guard, kCrossingCounts, width, height, counts, opts);
}

int nt_crossing_counts_device(nt_scene_t *s, int width, int height, void *counts_dev, const nt_render_opts *opts, void *hip_stream) {
    return view_query_device(s, kCrossingCounts, width, height, counts_dev, opts, hip_stream);
}

int nt_hit_layers(nt_scene_t *s, int width, int height, int layers, nt_ray_hit *records, const nt_render_opts *opts) {
    RenderGuard guard(s);
    return view_query_host(guard, kHitLayers, width, height, records, opts, nullptr, layers);
}

int nt_hit_layers_device(nt_scene_t *s, int width, int height, int layers, void *records_dev, const nt_render_opts *opts, void *hip_stream) {
    return view_query_device(s, kHitLayers, width, height, records_dev, opts, hip_stream, layers);
}

int nt_depth_cue_factors(nt_scene_t *s, int width, int height, float *factors, const nt_render_opts *opts) {
    RenderGuard guard(s);
    return view_query_host(guard, kCueFactors, width, height, factors, opts);
}

int nt_depth_cue_factors_device(nt_scene_t *s, int width, int height, void *factors_dev, const nt_render_opts *opts, void *hip_stream) {
    return view_query_device(s, kCueFactors, width, height, factors_dev, opts, hip_stream);
}

int nt_box_line_mask(nt_scene_t *s, int width, int height, uint8_t *mask, long long *marked, const nt_render_opts *opts) {
    RenderGuard guard(s);
    if (int r = view_query_host(guard, kBoxLineMask, width, height, mask, opts)) return r;
    if (marked) *marked = marked_pixels(mask, (size_t)width * height);
    return NT_OK;
}

int nt_box_line_mask_device(nt_scene_t *s, int width, int height, void *mask_dev, const nt_render_opts *opts, void *hip_stream) {
    return view_query_device(s, kBoxLineMask, width, height, mask_dev, opts, hip_stream);
}

int nt_colors_at(nt_scene_t *s, int width, int height, int count, const int32_t *xs, const int32_t *ys, float *rgb, int device) {
    if (!s || (count > 0 && (!xs || !ys || !rgb))) return fail(NT_E_INVALID, "NULL argument");
    if (width < 1 || height < 1 || count < 0) return fail(NT_E_INVALID, "invalid view size or count");
    if (int r = clip_refuses(s, "the colour of single pixels (nt_colors_at / nt_calculate_color)")) return r;
    if (int r = xray_refuses(s, "the colour of single pixels (nt_colors_at / nt_calculate_color)")) return r;
    if (count == 0) return NT_OK;
    if (int r = check_renderable(s)) return r;
    RenderGuard guard(s);   // Scene.calculate_color locks the scene for the call (render.cpp:599-603)
    if (int r = guard.acquire()) return r;
    if (int r = lens_check(s, width, height, Bands(), false, true)) return r;
    if (int r = parallel_check(s, Bands(), false, true)) return r;
    DeviceState *ds;
    if (int r = scene_on_device(s, nullptr, device, ds)) return r;
    if (int r = use_own_stream(ds)) return r;
    const size_t ibytes = (size_t)count * sizeof(int32_t);
    const size_t cbytes = (size_t)count * 3 * sizeof(float);
    if (int r = ds->probes.ensure(2 * ibytes + cbytes)) return r;
    char *base = (char *)ds->probes.p;
    HIP_TRY(hipMemcpyAsync(base, xs, ibytes, hipMemcpyHostToDevice, ds->stream));
    HIP_TRY(hipMemcpyAsync(base + ibytes, ys, ibytes, hipMemcpyHostToDevice, ds->stream));
    FrameJob job{};
    job.nframes = 1;
    job.stream = ds->stream;
    job.colors_out = (float *)(base + 2 * ibytes);
    job.xs = (const int *)base;
    job.ys = (const int *)(base + ibytes);
    job.probe_count = count;
    job.view_w = width;
    job.view_h = height;
    if (int r = enqueue(s, ds, job)) { (void)hipStreamSynchronize(ds->stream); return r; }
    HIP_TRY(hipMemcpyAsync(rgb, base + 2 * ibytes, cbytes, hipMemcpyDeviceToHost, ds->stream));
    HIP_TRY(hipStreamSynchronize(ds->stream));
    return NT_OK;
}

int nt_calculate_color(nt_scene_t *s, int x, int y, int width, int height, float rgb[3]) {
    const int32_t xs = x, ys = y;
    return nt_colors_at(s, width, height, 1, &xs, &ys, rgb, -1);
}

int nt_intersect_rays(nt_scene_t *s, const nt_ray_batch *rays, const nt_ray_results *out, int device) {
    return query_host(s, rays, out, device, false);
}

int nt_occludes_rays(nt_scene_t *s, const nt_ray_batch *rays, const nt_ray_results *out, int device) {
    return query_host(s, rays, out, device, true);
}

int nt_intersect_rays_device(nt_scene_t *s, const nt_ray_batch *rays, const nt_ray_results *out, const nt_render_opts *opts, void *hip_stream) {
    return query_device(s, rays, out, opts, hip_stream, false);
}

int nt_occludes_rays_device(nt_scene_t *s, const nt_ray_batch *rays, const nt_ray_results *out, const nt_render_opts *opts, void *hip_stream) {
    return query_device(s, rays, out, opts, hip_stream, true);
}

int nt_primary_hits(nt_scene_t *s, int width, int height, const nt_hit_buffers *out, int device) {
    return hits_host(s, width, height, out, device);
}

int nt_primary_hits_device(nt_scene_t *s, int width, int height, const nt_hit_buffers *out, const nt_render_opts *opts, void *hip_stream) {
    if (int r = hits_validate(s, width, height, out, (long long)width * height, 1)) return r;
    if (int r = only_device_strict_abort(opts, "a primary-hit pass reads")) return r;
    return hits_device(s, width, height, out, (long long)width * height, nullptr, -1, 1, opts, hip_stream);
}

int nt_primary_hits_table_device(nt_scene_t *s, int width, int height, const nt_hit_buffers *out, size_t frame_stride_records,
                                 const nt_camera_table_t *table, int first, int count, const nt_render_opts *opts, void *hip_stream) {
    if (!s || !table) return fail(NT_E_INVALID, "NULL argument");
    if (table->n != s->n) return fail(NT_E_INVALID, "the camera table is for %d dimensions, the scene has %d", table->n, s->n);
    if (first < 0 || count < 1 || first > table->nframes - count) return fail(NT_E_INVALID, "frames %d..%d are not in a table of %d", first, first + count - 1, table->nframes);
    if (frame_stride_records > (size_t)INT_MAX) return fail(NT_E_INVALID, "frame_stride_records is beyond 2^31 - 1 records");
    if (int r = hits_validate(s, width, height, out, (long long)frame_stride_records, count)) return r;
    if (int r = only_device_strict_abort(opts, "a primary-hit pass reads")) return r;
    return hits_device(s, width, height, out, (long long)frame_stride_records, table->dev + (size_t)first * 4 * table->n, table->device, count, opts, hip_stream);
}

int nt_box_hits(nt_scene_t *s, int width, int height, nt_ray_hit *hits, int device) {
    return box_hits_host(s, width, height, hits, device);
}

int nt_box_hits_device(nt_scene_t *s, int width, int height, void *hits_dev, const nt_render_opts *opts, void *hip_stream) {
    if (int r = box_hits_validate(s, width, height, hits_dev, (long long)width * height, 1)) return r;
    if (int r = only_device_abort(opts, "a BoxScene hit pass")) return r;
    return box_hits_device(s, width, height, hits_dev, (long long)width * height, nullptr, nullptr, -1, 1, opts, hip_stream);
}

int nt_box_hits_table_device(nt_scene_t *s, int width, int height, void *hits_dev, size_t frame_stride_records, const nt_camera_table_t *table,
                             int first, int count, const nt_render_opts *opts, void *hip_stream) {
    if (!s || !table) return fail(NT_E_INVALID, "NULL argument");
    if (table->n != s->n) return fail(NT_E_INVALID, "the camera table is for %d dimensions, the scene has %d", table->n, s->n);
    if (first < 0 || count < 1 || first > table->nframes - count) return fail(NT_E_INVALID, "frames %d..%d are not in a table of %d", first, first + count - 1, table->nframes);
    if (frame_stride_records > (size_t)INT_MAX) return fail(NT_E_INVALID, "frame_stride_records is beyond 2^31 - 1 records");
    if (int r = box_hits_validate(s, width, height, hits_dev, (long long)frame_stride_records, count)) return r;
    if (int r = only_device_abort(opts, "a BoxScene hit pass")) return r;
    return box_hits_device(s, width, height, hits_dev, (long long)frame_stride_records, table->dev + (size_t)first * 4 * table->n,
                           table->dev + (size_t)table->nframes * 4 * table->n + (size_t)first * 4, table->device, count, opts, hip_stream);
}

int nt_ray_colors(nt_scene_t *s, const nt_rays *rays, float *rgb, int device) {
    if (!rgb) return fail(NT_E_INVALID, "NULL argument");
    return rays_host(s, rays, rgb, nullptr, 0, nullptr, device);
}

int nt_ray_colors_device(nt_scene_t *s, const nt_rays *rays, float *rgb, const nt_render_opts *opts, void *hip_stream) {
    if (!rgb) return fail(NT_E_INVALID, "NULL argument");
    return rays_device(s, rays, rgb, nullptr, 0, nullptr, opts, hip_stream);
}

int nt_render_rays(nt_scene_t *s, void *dest, size_t dest_len, const nt_image_format *fmt, const nt_rays *rays, int device) {
    if (!dest) return fail(NT_E_INVALID, "NULL argument");
    return rays_host(s, rays, nullptr, dest, dest_len, fmt, device);
}

int nt_render_rays_device(nt_scene_t *s, void *dest_dev, size_t dest_len, const nt_image_format *fmt, const nt_rays *rays,
                          const nt_render_opts *opts, void *hip_stream) {
    if (!dest_dev) return fail(NT_E_INVALID, "NULL argument");
    return rays_device(s, rays, nullptr, dest_dev, dest_len, fmt, opts, hip_stream);
}

int nt_scene_last_stats(const nt_scene_t *cs, nt_stats *out) {
    nt_scene *s = const_cast<nt_scene *>(cs);
    if (!s || !out) return fail(NT_E_INVALID, "NULL argument");
    if (!s->have_stats) {
        if (s->stats_device < 0) return fail(NT_E_INVALID, "no render with collect_stats has run on this scene");
        auto it = s->devs.find(s->stats_device);
        if (it == s->devs.end() || !it->second->stats.p) return fail(NT_E_INVALID, "no statistics available");
        HIP_TRY(hipSetDevice(s->stats_device));
        HIP_TRY(hipDeviceSynchronize());
        unsigned long long v[8];
        HIP_TRY(hipMemcpy(v, it->second->stats.p, sizeof(v), hipMemcpyDeviceToHost));
        s->last_stats.rays = v[0]; s->last_stats.shadow_rays = v[1]; s->last_stats.branches = v[2]; s->last_stats.leaves = v[3];
        s->last_stats.simplex_tests = v[4]; s->last_stats.solid_tests = v[5]; s->last_stats.hits = v[6]; s->last_stats.aabb_enter = v[7];
        s->have_stats = true;
    }
    *out = s->last_stats;
    return NT_OK;
}

}  // extern "C"
