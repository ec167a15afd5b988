// nt_device.hpp -- structures shared by the host API (nt_api.cpp) and the HIP kernels
// (nt_box.hpp, nt_composite.hpp, nt_var.hip).  gfx950 only.
#pragma once
#include <stdint.h>

#define NT_DEV_MAX_DIM 64
#define NT_DEV_MAX_FIXED 10
#define NT_DEV_MAX_FIXED_BOX 24        // BoxScene kernels are also compiled for N = 11..24
#define NT_DEV_BATCH 4
#define NT_DEV_MAX_REFLECT 16

// reference: ROUNDING_FUZZ = numeric_limits<float>::epsilon()*10 (src/tracer.hpp:25)
#define NT_FUZZ (1.1920928955078125e-07f * 10.0f)
// reference: LIGHT_THRESHOLD (src/tracer.hpp:31)
#define NT_LIGHT_THRESHOLD (1.0f / 512.0f)

struct NtChanDev {          // render.cpp:95-99 channel, plus host-precomputed packing constants
    float f_r, f_g, f_b, f_c;
    uint32_t bits;
    uint32_t tfloat;
    uint32_t offset;        // first bit of the channel, counted from the pixel's most significant bit
    uint32_t maxval;        // 0xffffffff >> (32 - bits): the integer scale of render.cpp:439
};

// how a pixel is assembled (chosen on the host from the format)
#define NT_PACK_GENERIC 0   // up to 128 bits, any number of channels
#define NT_PACK_WORD32 1    // <= 32 bits and <= 4 live channels: one 32-bit container, unrolled
#define NT_PACK_WORD64 2    // <= 64 bits and <= 4 live channels: one 64-bit container, unrolled

// Where the pixels of one launch go.  Rows are dealt to ranks in bands of `band_rows`
// (RENDER_CHUNK_SIZE, render.cpp:43): owned row r -> image row
//   y = ((r / band_rows) * band_world + band_rank) * band_rows + r % band_rows.
struct NtTarget {
    uint8_t *dest;
    long long frame_stride;   // bytes between frames (blockIdx.z)
    const NtChanDev *chans;
    int nchannels, bpp, reversed, pitch;
    int pack_mode;            // NT_PACK_*; channels whose value is identically 0 are dropped from `chans`
    // plain RGB layouts in one dword (RGBX8, BGRA8, ...): plain_bits != 0, and component k goes to the fields
    // plain_mul[k] marks (a quantised component times plain_mul[k] is that component shifted into all of them)
    uint32_t plain_bits, plain_maxval, plain_mul[3];
    // ... and for 8-bit fields on byte boundaries (RGBX8, BGRA8, ...): the v_perm_b32 selector that builds the dword as it
    // lies in memory from (src0 = quantised R, src1 = quantised G = B); 0 when the layout is not of that kind
    uint32_t plain_sel;
    int plain_f32[3];         // 12-byte pixels of three fp32 channels that are plain components: component of float k; else -1
    int width, height;        // view size: set_view_size(w,h) (tracer.hpp:65-69)
    float half_w, half_h, fovI;
    int band_rank, band_world, band_rows, compact;
    int row_begin, row_count; // owned-row range rendered by this launch
    int aligned4;             // dest, pitch and frame_stride are 4-byte aligned
    // probe mode (nt_colors_at / nt_calculate_color): fp32 colours of listed pixels
    float *colors_out;
    const int *probe_xs, *probe_ys;
    int probe_count;
    // two-pass renders of lit scenes: primary hits found by the packet kernel, [frame][row][x] records of 16 bytes
    // (dist, item, lane, -); nullptr otherwise
    const void *hits;
    // BoxScene: four bits per (frame, owned row, 64-pixel stretch), eight stretches to a dword, from box_cull_kernel:
    //   0: no ray of the stretch can reach the cube; 1..13: every ray of it clearly hits face K = code - 1;
    //   14 (a near-tie), 15: look at each ray.  box_kernel<N> reads them.  [frame][row][cull_words] dwords, or nullptr
    const uint32_t *cull;
    int cull_words;
    // the fused route's redo bitmap, one bit per stretch, [frame][row][redo_words] dwords: box_tile_kernel (packed RGB, N > 8)
    // sets the bit of a stretch it leaves to box_redo_kernel (code 14, or a lane needed the reference's own face-by-face
    // arithmetic), and box_redo_kernel clears it
    uint32_t *redo;
    int redo_words;
    // BoxScene tile kernel: per owned row (index = owned-row number; 64 entries of padding) 16 bytes {float sy = fovI*(y -
    // half_h); uint32 y < height; int64 byte offset of the row within a frame}, read with scalar loads; or nullptr
    const void *rowtab;
    // box_tile_kernel, interleaved rows: 0 = a wave renders ROWS consecutive rows (table entry = owned-row number); W > 0 = the
    // W waves of a column strip (W = gridDim.y * WAVES) deal the rows out among themselves, wave w renders rows w, w + W,
    // w + 2W, ... -- every wave of a strip then holds the same share of the rows that need ray-by-ray work -- and the row
    // table is in SLOT order: entry w * ROWS + rr belongs to row w + W * rr (valid = 0 past the last row).
    int row_il;
    // Abort word (renderer::CANCEL, polled per pixel by the reference: render.cpp:412): nullptr, or a dword the device can read
    // while the kernels run -- best in device memory (pinned host memory works too, but every look at it is then a PCIe round
    // trip) -- that the kernels read past the caches when a block (or a tile of a striding block) starts; non-zero: the block
    // leaves without drawing
    const int *abort_word;
    // box_tile_kernel: the middle columns of the image are started `lead_frames` frames ahead of the outer ones (see the kernel); 0: off
    int lead_frames;
};

// Camera rows used by the ray source (camera.hpp:40-45): origin, right, up, forward.
// Either inline in the kernel arguments (single frame) or from a device buffer
// [frame][4][n] (multi-frame launches).
// Four ray-independent dot products travel with the camera for BoxScene's circumsphere rejection (conservative,
// not part of the exact predicate): |origin|^2, origin.right, origin.up, origin.forward -- `odots` for the inline
// camera, four floats per frame after the last camera of a table.
struct NtCamera {
    const float *buf;         // nullptr => use `inl`; else [nframes][4][n] cameras of the launch's frames
    const float *dots;        // with buf: [nframes][4] dot products of the same frames (|o|^2, o.right, o.up, o.forward)
    // with buf, or nullptr: [nframes][2], sx_lo and sx_hi of the same frames -- outside them no ray of the frame can hit BoxScene's
    // cube (nt_box_span.hpp; box_tile_kernel, NT_BOX_STRIP_SPAN).  Only a camera table has them: nullptr says nothing about any frame.
    const float *span = nullptr;
    int n;
    float odots[4];
    float inl[4 * NT_DEV_MAX_DIM];
};
struct NtCameraFixed {        // N <= 8: 4*8 floats inline
    const float *buf;
    const float *dots;
    const float *span = nullptr;   // (NtCamera::span)
    int n;
    float odots[4];
    float inl[4 * NT_DEV_MAX_FIXED_BOX];
};

struct NtNode {               // 16-byte k-d node record
    float split;
    int axis;                 // -1: leaf
    int left;                 // branch: child or -1; leaf: first item
    int right;                // branch: child or -1; leaf: item count
};

struct NtCompositeDev {
    const NtNode *nodes;
    const int *items;
    const float *batch_recs;  // [n_batches*4][rec_stride]
    const int *batch_mats;
    const float *tri_recs;    // [n_triangles][rec_stride]
    const int *tri_mats;
    const float *solid_recs;  // [n_solids][2*n*n+n]
    const int *solid_types;
    const int *solid_mats;
    const float *materials;   // [n_materials][10]
    const float *aabb;        // start[n], end[n]
    int rec_stride;           // floats per simplex record, multiple of 4
    int root;
    int stack_depth;          // LDS stack entries per lane
    int shadows, camera_light, max_reflect_depth, bg_axis;
    float ambient[3], bg1[3], bg2[3], bg3[3];
    int n_point_lights;
    const float *pl_pos;
    const float *pl_color;
    int n_global_lights;
    const float *gl_dir;
    const float *gl_color;
    int all_opaque;           // every material has opacity >= 1
    int any_reflective;
    int has_scalar_prims;     // leaves hold unbatched triangles or solids
    int n_batches, n_solids;
    int prune;                // 1: closest-hit walks drop subtrees that start clearly beyond the current hit (nt_beyond_hit)
    unsigned long long *stats;  // nullptr or 8 counters (nt_stats order)
    // Reference-faithful normals (composite_kernel_t<N, true>): the reference's first leaf loop hands o_hit.normal itself to
    // the primitive tests (tracer.hpp:1001,1020), so which tests run -- its exact `checked` list (:782,:832) -- matters.
    // One bit per (resident lane, primitive): checked[word * checked_lanes + lane slot]; nullptr selects the "clean"
    // semantics with the 16-slot mailbox.
    uint32_t *checked;
    int alias_normals;        // 1: the reference's o_hit.normal handling; 0: a hit keeps the normal of what was hit (NTRACER_CLEAN_NORMALS)
    int checked_words;        // ceil((n_batches + n_triangles + n_solids) / 32)
    int checked_lanes;        // lane slots = blocks of the launch * 256
    int n_triangles;
    // run-time-n transparency kernel (composite_kernel_var_t): the ray_color frame stacks in global scratch,
    // tframes[(frame * words + word) * checked_lanes + lane slot], words = var_frame_words(n); nullptr = not that kernel
    float *tframes;
    int tframe_count;         // frames per lane slot: max_reflect_depth + 1 if anything reflects, else 1
};

// ---- launchers implemented in nt_var.hip (dispatch) over nt_inst_box.hip / nt_inst_composite.hip ----
struct NtLaunchInfo {
    int n;                    // dimension
    int nframes;
    void *stream;             // hipStream_t
    // persistent composite kernel (optional): a zeroed 8-byte work counter, the camera table
    // [nframes][4][n] in device memory, and the CU count of the device
    void *persist_counter;
    const float *persist_cams;
    int cu_count;
    int kernel_choice;        // 0: default (packet kernel for lean scenes), 1: persistent per-lane kernel, 2: tile kernel
    const int *tile_order;    // packet kernel: device permutation of the 16x16-pixel quads of the launch (or nullptr)
    void *hit_buf;            // scratch for two-pass renders: hit_frames * width * rows * 16 bytes (or nullptr)
    int hit_frames;
    float *numer_buf;         // scratch for the packet kernel's plane numerators: numer_frames * n_batches * 4 floats
    int numer_frames;
    int tile_rows, tile_waves; // BoxScene, fused path: box_tile_kernel's block shape (nt_box_tile_geom; the row table follows it)
    int cull_clean;           // cull_buf is all zero (the fused path's redo bitmap lives at its start)
    int frame_major;          // packet kernel: PacketArgs::frame_major (0: the frames of a multi-frame launch interleaved)
    int force_var;            // the run-time-n kernels at every dimension
    int box_var_rows;         // BoxScene, run-time n: box_rows_kernel_var for packed RGB (0: box_kernel_var for every format)
    uint32_t *cull_buf;       // BoxScene: scratch, (4 * nframes * row_count + 64) * ceil(ceil(width/64)/32) dwords: box_cull_kernel's stretch codes and
                              // 16 rows of padding, or the fused route's redo bitmap at its start (or nullptr)
};

// box_tile_kernel's block shape for a launch, decided in one place because the host's row table (nt_api.cpp) follows it:
// 64 rows a wave and one wave a block for tall launches with waves to spare; otherwise 16 rows a wave (8 in small launches),
// four waves a block, or three when that leaves fewer idle waves below the last row (see launch_box_fixed).
// `overlapped` (nt_render_opts::overlapped): the caller keeps two or more streams busy with calls like this one, so the
// ramp and the tail of a call are filled by its neighbours.  Long waves -- whose tail is what makes them lose on a short
// launch that runs alone -- are then the better shape from 64 rows up: a rank's 136 rows of the 160 headline frames take
// 66 us alone with 16 x 3 and 86 with 64 x 1, 54 and 48 when consecutive calls alternate between two streams.
struct NtBoxTileGeom { int rows, waves; };
static inline NtBoxTileGeom nt_box_tile_geom(int width, int row_count, int nframes, int overlapped) {
    const long long cols = (width + 63) / 64;
    const long long waves8 = cols * ((row_count + 31) / 32) * nframes * 4;
    const bool r16 = waves8 >= 64 * 1024;
    int wpb = 4;
    if (r16) {
        const int groups = (row_count + 15) / 16;                   // waves with rows, per column
        if ((groups + 2) / 3 * 3 < (groups + 3) / 4 * 4) wpb = 3;
    }
    const long long waves64 = cols * ((row_count + 63) / 64) * nframes;
    bool r64 = r16 && row_count >= 512 && waves64 >= 32 * 1024;
    if (overlapped && r16 && row_count >= 64 && waves64 >= 8 * 1024) r64 = true;
    NtBoxTileGeom g;
    g.rows = r64 ? 64 : (r16 ? 16 : 8);
    g.waves = r64 ? 1 : wpb;
    return g;
}

// One batched ray query (nt_query.hpp, nt_var.hip): `count` rays from device memory, one 16-byte record a ray out.
// Every pointer is device memory; the optional ones are nullptr when the caller left them out.
struct NtQuery {
    int count;
    int occlusion;            // 0: closest hit (KDNode.intersects), 1: KDNode.occludes
    const float *origins;     // [count][n]
    const float *directions;  // [count][n], used as given
    const float *t_near, *t_far;          // nullptr (-FLT_MAX / FLT_MAX) or [count]
    const float *distance;                // occlusion: nullptr (FLT_MAX) or [count]
    const int *skip_item, *skip_lane;     // nullptr (none) or [count]
    void *hits;               // [count] records {float dist; int item, lane, n_transparent} (nt_ray_hit)
    float *normal_origin, *normal_dir;    // nullptr or [count][n]; rows of rays without an opaque hit are not written
    void *transparent;        // nullptr or [count][max_transparent] records: the transparent hits in the walk's order
    int max_transparent;
    const int *abort_word;    // as NtTarget::abort_word
};

// One primary-hit pass (nt_hits.hpp, nt_var.hip): the record of every pixel of `nframes` views of tg.width x tg.height, the view
// and the abort word in the NtTarget that travels with it.  Every pointer is device memory.  A pixel's record index is
// frame * frame_stride + y * width + x, and its normal rows lie at that index too.
struct NtHits {
    const float *cams;        // [nframes][4][n] camera rows: origin, right, up, forward (NtCamera::buf)
    int nframes;
    long long frame_stride;   // records between frames, >= width * height
    void *hits;               // records {float dist; int item, lane, n_transparent} (nt_ray_hit)
    float *normal_origin, *normal_dir;    // nullptr or [record][n]; rows of pixels without an opaque hit are not written
};

// One batch of the caller's rays to colour (nt_rays.hpp, nt_var.hip): `count` rays from device memory.  Where the colours go is
// in the NtTarget that travels with it: colors_out = rgb [count][3], or an image whose pixel (x, y) is ray y * width + x.
struct NtRayJob {
    int count;
    int shared_origin;        // 1: `origins` is one origin [n] for every ray
    const float *origins;     // [count][n], or [n]
    const float *directions;  // [count][n], any non-zero finite length: normalised as primary_dir does it
};

// A lens (nt_lens.hpp): per-pixel coefficients (sx, sy, sz) of the primary ray in the camera's frame, in place of the pinhole's
// fovI * (x - half_w), fovI * (y - half_h), 1.  Every pointer is device memory.
struct NtLens {
    const float *table;       // [height][width][3], the size of the view
    const float *cams;        // [nframes][4][n] camera rows of the launch's frames (NtCamera::buf)
    const void *hits;         // packet route: the 16-byte records between the walk and the shading pass (the launcher's own)
};

// The parallel projection (nt_parallel.hpp): its scale k = half_width / half_w travels in NtTarget::fovI.  Device memory.
struct NtParallel {
    const float *cams;        // [nframes][4][n] camera rows of the launch's frames (NtCamera::buf)
    const void *hits;         // packet route: the 16-byte records between the walk and the shading pass (the launcher's own)
};

// Adaptive supersampling (nt_adaptive.hpp, nt_var.hip): what lies between the base frame and the caller's image.  Every pointer
// is device memory.  A flagged pixel's list entry is frame * height * width + y * width + x, frames counted within the launch.
struct NtAdaptive {
    const uint32_t *base;     // the base frame: [nframes][height][width] pixels of three big-endian floats, clamped to [0, 1]
    int nframes;
    float threshold;          // contrast > threshold flags the pixel
    uint32_t *list;           // the flagged pixels; room for every pixel of the launch
    int *count;               // their number: zeroed in stream order in front of the flag kernel (adaptive_reset)
    uint8_t *mask;            // nullptr, or [nframes][height][width] bytes: 1 flagged, 0 not
    int draw;                 // 1: unflagged pixels go into tg.dest; 0: the mask alone is wanted
};
struct NtRefine {
    const uint32_t *list;     // NtAdaptive::list
    const int *count;         // NtAdaptive::count
    long long max_count;      // pixels of the launch: what the list could hold (the grid is sized by it)
    const float *cams;        // [nframes][4][n] camera rows of the launch's frames (NtCamera::buf)
    int s;                    // s x s samples a pixel
    float half_w, half_h, fovI;   // the s * width x s * height view (fill_view)
};

// Ambient occlusion (nt_ao.hpp, nt_var.hip): K short rays from the primary hit of every pixel, counted.  Every
// pointer is device memory; a pixel's index is frame * height * width + y * width + x, frames counted within the launch, and its
// hit record and normal rows (a primary-hit pass with normals, NtHits) lie at that index.
struct NtAo {
    const float *cams;        // [nframes][4][n] camera rows of the launch's frames (NtCamera::buf)
    int nframes;
    const void *recs;         // the pixels' 16-byte hit records
    const float *normal_origin, *normal_dir;   // [pixel][n]; rows of pixels without an opaque hit are never read
    const float *dirs;        // the setting's table, [count][n], used as given
    int count;                // K
    float radius, bias;
    int *blocked;             // [pixel]: -1 without an opaque hit, else the number of blocked samples
};
// the ray route's arrays for pixels [first, first + pixels): pixels * K rays, ray k of pixel i at i * K + k
struct NtAoRays {
    long long first, pixels;
    float *origins, *directions;          // [pixels * K][n]
    float *t_near, *t_far;                // [pixels * K]
    int *skip_item, *skip_lane;           // [pixels * K]
    const void *results;                  // [pixels * K] 16-byte records, what the closest-hit query wrote
};

// Outlines (nt_outline.hpp, nt_var.hip): the mask bytes of every pixel from its hit record and those of its four
// neighbours.  Every pointer is device memory; a pixel's index is frame * height * width + y * width + x, frames counted within
// the launch, and its hit record, normal row and mask byte lie at that index.
#define NT_DEV_OUTLINE_SILHOUETTE 1   // the mask bits (NT_OUTLINE_* of ntracer_hip.h)
#define NT_DEV_OUTLINE_CREASE 2
#define NT_DEV_OUTLINE_DEPTH 4
struct NtOutline {
    const float *cams;        // fast route: [nframes][4][n] camera rows of the launch's frames (NtCamera::buf)
    int nframes;
    const void *recs;         // the pixels' 16-byte hit records (fast route: the launcher's own, li.hit_buf)
    const float *normal_dir;  // general route: [pixel][n]; rows of pixels without an opaque hit are never read
    float cc;                 // crease_cos * crease_cos, formed once by the host in fp32
    float depth_gap;
    float color[3], strength;
    uint8_t *mask;            // [pixel] (the mask-only launches and the general route)
};

// Depth cues (nt_cue.hpp, nt_var.hip; the rule in full: ntracer_hip.h): the factors (f, g) of a pixel from its
// own hit record, its primary ray and the camera's origin.  Every pointer is device memory; a pixel's index is
// frame * height * width + y * width + x, frames counted within the launch.  The tint axis travels in the kernel arguments.
struct NtCue {
    const float *cams;        // [nframes][4][n] camera rows of the launch's frames (NtCamera::buf)
    int nframes;
    const void *recs;         // the pixels' 16-byte hit records {dist, item, lane, n_transparent}
    float fog_near, inv_fog;  // inv_fog = 1.0f / (fog_far - fog_near), formed once by the host in fp32
    float fog_color[3], fog_strength;
    int fog_background;
    int tint;                 // 0: no tint, g = -1 everywhere
    float tint_lo, inv_tint;  // inv_tint = 1.0f / (tint_hi - tint_lo), likewise
    float tint_color_lo[3], tint_color_hi[3];
    float tint_axis[NT_DEV_MAX_DIM];
    float *factors;           // [pixel][2] (the factor launches)
};

// Clip planes (nt_clip.hpp, nt_var.hip; the rule in full: ntracer_hip.h): the keep-region a . x <= b of up to
// NT_DEV_CLIP_MAX planes, which every ray of the launch honours.  Device memory, read at uniform addresses.
#define NT_DEV_CLIP_MAX 8
struct NtClipPlanes {        // what the run-time-n walk kernels take as their last argument: {nullptr, 0} without the setting
    const float *planes;      // [count][n + 1]: a plane's normal, then its offset
    int count;                // 0: no clip
};
struct NtClip {
    const float *planes;      // [count][n + 1]: a plane's normal, then its offset
    int count;                // 0: no clip
    const float *cams;        // [nframes][4][n] camera rows of the launch's frames (NtCamera::buf)
    int nframes;
    void *hits;               // renders on the packet route: li.hit_buf; primary-hit passes: the caller's records (NtHits::hits)
    long long frame_stride;   // primary-hit passes: records between frames (NtHits::frame_stride)
    float *normal_origin, *normal_dir;    // primary-hit passes: as NtHits has them
};

// BoxScene hit buffers and face lines (nt_boxhits.hpp, nt_var.hip; the rules in full: ntracer_hip.h): the face
// record of every pixel of li.nframes views of tg.width x tg.height, or what follows from the records of a pixel and its four
// neighbours -- the mask bytes, or the frame with the lines drawn.  Every pointer is device memory; a pixel's record index is
// frame * frame_stride + y * width + x, its mask byte lies at frame * height * width + y * width + x.
#define NT_BOX_FACES_RECORDS 0        // the records into `recs`
#define NT_BOX_FACES_MASK 1           // the mask bytes into `mask`
#define NT_BOX_FACES_DRAW 2           // the plain frame with the lines drawn, into the NtTarget that travels with it
struct NtBoxFaces {
    int mode;                 // NT_BOX_FACES_*
    void *recs;               // records {float dist; int item, lane, n_transparent} (nt_ray_hit): item = axis, lane = side.  MASK and
                              // DRAW: scratch for the run-time-n kernels alone (the compile-time-N kernel keeps its records in LDS)
    long long frame_stride;   // records between frames, >= width * height
    uint8_t *mask;            // MASK: [frame][height][width]
    int kinds;                // MASK, DRAW: the setting's OR of NT_DEV_OUTLINE_SILHOUETTE and NT_DEV_OUTLINE_CREASE
    float color[3], strength; // DRAW
};

// BoxScene face shading (nt_boxshade.hpp, nt_var.hip; the rule in full: ntracer_hip.h): the frame shaded from
// the face record of every pixel -- a colour of its own for each of the 2n faces, the depth cues' fog and tint from the same
// record, and the face lines of NtBoxFaces on top.  The table and the tint axis travel in the kernel arguments; the kernels read
// the table from LDS, where a block stages it once (a by-value array indexed by a lane's face would go to scratch).
struct NtBoxShade {
    NtCue cue;                // the depth cues' constants; recs, cams, nframes and factors are not read
    int cue_on;               // 0: f = g = -1 everywhere
    int gb_equal;             // the table, the tint colours and the fog colour all have g == b: so has every unmarked pixel
    int kinds;                // != 0: face lines as NtBoxFaces has them, with ...
    float line_color[3], line_strength;
    void *recs;               // run-time n alone: scratch for box_hits_var's records, li.nframes frames of ...
    long long frame_stride;   // ... this many records
    float colors[NT_DEV_MAX_DIM * 6];     // T[axis][side][channel]; (1, 0.5, 0.5) everywhere without a table of the caller's
};

// A view stack (nt_stack.hpp; the rule in full: ntracer_hip.h): K sample cameras a frame, whose plain pictures
// are clamped, weighted and summed in the order of k.  Every pointer is device memory.  The sample cameras are stack_cameras'
// output: camera f * count + k is sample k of frame f of the launch.
#define NT_DEV_STACK_MAX 64
struct NtStack {
    int count;                // K
    const float *cams;        // [nframes * count][4][n] camera rows of the samples (NtCamera::buf)
    const float *dots;        // [nframes * count][4] their dot products (NtCamera::dots)
    float weights[NT_DEV_STACK_MAX * 3];  // w_k[c]
};
// One chunk of the frames route: samples [k0, k0 + kc) of `nframes` frames, each a plain fp32 x 3 frame (NtAdaptive::base's
// layout) of tg.width x tg.height pixels, sample kk of frame f at ((f * kc + kk) * width * height) pixels.  acc_in: nullptr (the
// sum starts at 0.0f) or the running sums of the samples before k0, three native floats a pixel; acc_out: nullptr (the pixel goes
// through the packer into tg, the whole image of every frame, no bands) or where the running sums go.  With either, nframes is 1.
struct NtStackChunk {
    const uint32_t *samples;
    int k0, kc, nframes;
    const float *acc_in;
    float *acc_out;
};
// stack_cameras: the K sample cameras of each of `nframes` cameras -- rows `cams` [nframes][4][n], all their axes `axes`
// [nframes][n][n] -- under the offsets [count][n] and r = 1 / focus (0: none), and their dot products, into out_cams / out_dots
int nt_launch_stack_cameras(void *stream, int n, int nframes, const float *cams, const float *axes, const float *offsets, int count, float r,
                            float *out_cams, float *out_dots);
int nt_launch_stack_resolve(void *stream, const NtStack &sk, const NtStackChunk &ch, const NtTarget &tg);
// box_stack<N> of the scene's dimension, N = 3..NT_DEV_MAX_FIXED_BOX (the host sends every other BoxScene through the frames
// route): tg is the whole image of every frame (no bands)
int nt_launch_box_stack(const NtLaunchInfo &li, const NtTarget &tg, const NtStack &sk);

// X-ray views (nt_xray.hpp, nt_var.hip; the rule in full: ntracer_hip.h): every primitive a primary ray crosses,
// counted, and the background times the product of their materials' transmittances.  Every pointer is device memory.
#define NT_DEV_XRAY_PACKET_ITEMS 65536    // the packet walk's seen bitset: 8 KiB a wave, four waves a SIMD in 160 KiB of LDS
struct NtXray {
    const float *cams;        // [nframes][4][n] camera rows of the launch's frames (NtCamera::buf)
    const float *trans;       // [n_materials][3] transmittances T (a render; the counts read none)
    const uint8_t *live;      // [n_batches] live masks: bit l set when lane l of the batch counts
    int *counts;              // not nullptr: the counts [frame][height][width] go here and nothing is drawn
};
// tg: the whole image of every frame (no bands), or with xr.counts the view and the abort word.  The packet walk xray_packet of
// the scene's dimension where n <= 10, the tree's stack <= 32, kernel_choice 0, no force_var and at most NT_DEV_XRAY_PACKET_ITEMS
// items; else xray_var, which needs sc.checked (with checked_lanes = blocks of the launch * 64)
int nt_launch_xray(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtXray &xr);
// the rule that picks the packet walk, for the host to size the scratch by
static inline bool nt_xray_packet_route(const NtLaunchInfo &li, const NtCompositeDev &sc) {
    return li.n <= NT_DEV_MAX_FIXED && sc.stack_depth <= 32 && li.kernel_choice == 0 && !li.force_var &&
           (long long)sc.n_batches + sc.n_triangles + sc.n_solids <= NT_DEV_XRAY_PACKET_ITEMS;
}

// Hit layers (nt_layers.hpp, nt_var.hip; the rule in full: ntracer_hip.h): the `layers` nearest crossings of every
// pixel's primary ray, ordered by (t, item, lane), as nt_ray_hit records whose fourth word is the pixel's crossing count.  Every
// pointer is device memory.
#define NT_DEV_LAYERS_MAX 8
#define NT_DEV_LAYERS_INDEX_MAX (1 << 26)      // an item code and its lane share the 32 low bits of a key: (item << 3) | (lane + 1)
struct NtLayers {
    const float *cams;        // [4][n] camera rows of the view (NtCamera::buf)
    const uint8_t *live;      // [n_batches] live masks, as NtXray has them
    void *records;            // nt_ray_hit [layers][height][width]
    int layers;               // 1..NT_DEV_LAYERS_MAX
};
// tg: the view and the abort word; one frame.  The routes are nt_launch_xray's: layers_packet where nt_xray_packet_route says so,
// else layers_var, which needs sc.checked (with checked_lanes = blocks of the launch * 64)
int nt_launch_layers(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtLayers &ly);

int nt_launch_box(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg);
// BoxScene face shading: box_shaded<N, LINES> of the scene's dimension, or box_hits_var into bs.recs and box_shaded_var behind
// it.  tg is the whole image of every frame (no bands).  The cameras travel as for nt_launch_box.
int nt_launch_box_shade(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg, const NtBoxShade &bs);
// BoxScene hit buffers and face lines: the kernels of nt_boxhits.hpp at the scene's dimension, or box_hits_var (and, behind it,
// box_lines_var on bf.recs).  RECORDS, MASK: tg is the view and the abort word; DRAW: the whole image of every frame (no bands).
// The cameras travel as for nt_launch_box.
int nt_launch_box_faces(const NtLaunchInfo &li, const NtCamera &cam, const NtTarget &tg, const NtBoxFaces &bf);
// Outlines, fast route (opaque scenes, n <= 10, stack depth <= 32): the packet walk into li.hit_buf (li.hit_frames frames of
// tg.width * tg.height records), then outline_shade into tg, the whole image of every frame (no bands) ...
int nt_launch_outline(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtOutline &ol);
// ... or outline_mark_fixed into ol.mask (tg: the view and the abort word)
int nt_launch_outline_mask(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtOutline &ol);
// general route: ol.recs and ol.normal_dir (a primary-hit pass, NtHits) into ol.mask at run-time n ...
int nt_launch_outline_mark(const NtLaunchInfo &li, const NtTarget &tg, const NtOutline &ol);
// ... and the base frame (NtAdaptive::base's layout) blended with the colour where the mask is set, into tg.dest, the whole image
// of ol.nframes frames (no bands)
int nt_launch_outline_apply(void *stream, const uint32_t *base, const NtOutline &ol, const NtTarget &tg);
// Depth cues, fast route (opaque scenes, n <= 10, stack depth <= 32): the packet walk into li.hit_buf (li.hit_frames frames of
// tg.width * tg.height records), then cue_shade into tg, the whole image of every frame (no bands) ...
int nt_launch_cue(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtCue &cu);
// ... or cue_factors_fixed into cu.factors (tg: the view and the abort word)
int nt_launch_cue_factors_fixed(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtCue &cu);
// general route, at run-time n behind a primary-hit pass (cu.recs): the factors of every pixel of cu.nframes frames into
// cu.factors ...
int nt_launch_cue_factors(const NtLaunchInfo &li, const NtTarget &tg, const NtCue &cu);
// ... or the base frame (NtAdaptive::base's layout) blended by them into tg.dest, the whole image of cu.nframes frames (no bands)
int nt_launch_cue_apply(const NtLaunchInfo &li, const uint32_t *base, const NtCue &cu, const NtTarget &tg);
int nt_launch_composite(const NtLaunchInfo &li, const NtCamera &cam, const NtCompositeDev &sc, const NtTarget &tg);
// Renders and primary-hit passes under clip planes, kept apart from every launcher above.  draw: tg is the whole image of every
// frame (no bands); otherwise tg is the view and the abort word and the records go to cl.hits (normal rows: cl.normal_*).
// Opaque scenes the packet walk takes (n <= 10, stack depth <= 32, kernel_choice 0, no force_var): composite_packet<..., CLIP>
// into records -- a render's in li.hit_buf, li.hit_frames frames of them -- and clip_shade, or hits_normals.  Every other
// scene: the run-time-n kernels with cl in their arguments, sc.checked / sc.tframes as for nt_launch_composite / nt_launch_hits
int nt_launch_clip(const NtLaunchInfo &li, const NtCamera &cam, const NtCompositeDev &sc, const NtTarget &tg, const NtClip &cl, bool draw);
// resolve_kernel<s> (nt_resolve.hpp): the s x s samples of every pixel of owned rows [tg.row_begin, tg.row_begin + tg.row_count)
// of `nframes` frames -- 12-byte fp32 x 3 pixels as the render kernels write them, s * tg.row_count rows of `pitch_bytes` a frame
// -- averaged and packed into tg.dest
int nt_launch_resolve(int s, void *stream, const void *samples, long long frame_stride_bytes, long long pitch_bytes, int nframes, const NtTarget &tg);
// the query kernels; sc.checked (with checked_lanes = blocks of the launch * lanes a block) selects the walks with transparent
// hits and the reference's o_hit.normal handling, as for a render
int nt_launch_query(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtQuery &q);
// the primary-hit kernels; li carries what the packet walk wants (kernel_choice, tile_order, numer_buf, frame_major), sc.checked
// selects the walks with transparent hits as for nt_launch_query, and tg.frame_stride is h.frame_stride in bytes
int nt_launch_hits(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtHits &h);
// the colours of the caller's rays; sc == nullptr: BoxScene.  sc->checked / sc->tframes select the walks with transparent hits
// as for a render, their grid what that scratch has lane columns for; tg.abort_word is honoured when a block or a stride step starts
int nt_launch_rays(const NtLaunchInfo &li, const NtCompositeDev *sc, const NtRayJob &job, const NtTarget &tg);
// A render through a lens on the packet walk (opaque scenes, n <= 10, stack depth <= 32): li as for nt_launch_composite, with
// li.hit_buf holding li.hit_frames frames of tg.width * tg.height records; tg is the whole image (no bands)
int nt_launch_lens(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtLens &ln);
// ... and for every other scene, around nt_launch_rays: the unnormalised directions of pixels [first, first + count) of the
// view under the camera `cam` ([4][n], device) into out[count][n], zero for a masked pixel; and (0, 0, 0) into the masked ones
// among those pixels of the image at tg.dest, whose first pixel is pixel `first`
int nt_launch_lens_expand(const NtLaunchInfo &li, const float *table, const float *cam, long long first, long long count, float *out);
int nt_launch_lens_mask(const NtLaunchInfo &li, const float *table, long long first, long long count, const NtTarget &tg);
// A render under the parallel projection on the packet walk (opaque scenes, n <= 10, stack depth <= 32): as nt_launch_lens,
// with tg.fovI = half_width / half_w
int nt_launch_parallel(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtParallel &pl);
// ... and for every other scene, in front of nt_launch_rays: the origins o' of pixels [first, first + count) of a view `width`
// pixels wide under the camera `cam` ([4][n], device) into out[count][n], and the unnormalised forward row into the `count`
// rows behind them; k, half_w and half_h as NtTarget has them
int nt_launch_parallel_expand(const NtLaunchInfo &li, const float *cam, int width, float k, float half_w, float half_h, long long first,
                              long long count, float *out);
// adaptive_flag: tg is the whole image of ad.nframes frames (no bands); see NtAdaptive
int nt_launch_adaptive_flag(void *stream, const NtAdaptive &ad, const NtTarget &tg);
// the refine kernels: the scene as for nt_launch_rays (sc == nullptr: BoxScene; sc->checked / sc->tframes with lane columns for
// blocks of 64 lanes); tg is the whole image the list's pixels belong to
int nt_launch_refine(const NtLaunchInfo &li, const NtCompositeDev *sc, const NtRefine &rf, const NtTarget &tg);
// ambient occlusion, fast route: ao_kernel<N, SCALP> of the scene's dimension (opaque scenes the fixed-n kernels draw); tg is
// the view and the abort word
int nt_launch_ao(const NtLaunchInfo &li, const NtCompositeDev &sc, const NtTarget &tg, const NtAo &ao);
// ... and the ray route's two kernels around nt_launch_query (run-time n): the rays of a chunk of pixels, and their counts
int nt_launch_ao_expand(const NtLaunchInfo &li, const NtTarget &tg, const NtAo &ao, const NtAoRays &ar);
int nt_launch_ao_reduce(const NtLaunchInfo &li, const NtTarget &tg, const NtAo &ao, const NtAoRays &ar);
// ao_apply: the base frame (NtAdaptive::base's layout) times 1 - strength * blocked / K into tg.dest, the whole image of
// `nframes` frames (no bands)
int nt_launch_ao_apply(void *stream, const uint32_t *base, const int *blocked, int count, float strength, int nframes, const NtTarget &tg);
int nt_launch_upload(void *stream, const float *src_pinned, float *dst, int count);
int nt_var_frame_words(int n);   // floats per ray_color frame of composite_kernel_var_t
const char *nt_launch_error();
