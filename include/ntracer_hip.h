/*
 * ntracer_hip.h -- C ABI of libntracer_hip.so, the MI355X-native replacement for
 * NTracer's per-pixel ray-cast path.
 *
 * The reference has no C ABI: the path sits behind the in-process C++ plugin
 * interface `class scene` (reference src/render.hpp:8-26) and is driven by
 * `BlockingRenderer.render` / `CallbackRenderer.begin_render` /
 * `Scene.calculate_color` (src/render.cpp:853-909, :651-700, :586-614).
 * Each entry point below names the reference interface it replaces; the
 * reference-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes only; every function returns NT_OK (0)
 * or a negative nt_status (never throws across the ABI); nt_last_error() gives
 * a thread-local message for the last failure on the calling thread.  Inputs
 * are copied -- the caller keeps ownership.  `dest` buffers are borrowed for the
 * duration of the call.  One render at a time per scene handle (NT_E_BUSY
 * otherwise, the reference's already_running_error, render.cpp:87-92); different
 * handles may be used concurrently from different threads.
 */
#ifndef NTRACER_HIP_H
#define NTRACER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NT_MAX_DIM 64            /* run-time-n kernels: n-vectors live in LDS */
#define NT_MAX_FIXED_DIM 10      /* compile-time-N kernels: 3..10 (reference: setup.py --optimize-dimensions, default 3..8) */
#define NT_MAX_FIXED_BOX_DIM 24  /* ... BoxScene's also for 11..24 */
#define NT_BATCH_SIZE 4          /* tracern.BATCH_SIZE of the SSE reference build (tracer.hpp:34-38) */
#define NT_MAX_PIXELSIZE 16      /* bytes per pixel, render.cpp:50 */
#define NT_MAX_BITSIZE 31        /* integer channel bits, render.cpp:48 */
#define NT_RENDER_CHUNK_SIZE 32  /* render.cpp:43 -- also the multi-GPU band height */

typedef enum {
    NT_OK = 0,
    NT_ABORTED = 1,              /* render stopped by the abort flag (BlockingRenderer.render -> False) */
    NT_E_INVALID = -1,           /* ValueError / TypeError in the reference */
    NT_E_BUSY = -2,              /* already_running_error (render.cpp:87-92) */
    NT_E_LOCKED = -3,            /* render.LockedError (ntracer_body.hpp:235-240) */
    NT_E_DEVICE = -4,            /* HIP runtime failure / no GPU: the product path never falls back to CPU */
    NT_E_NOMEM = -5,             /* MemoryError */
    NT_E_UNSUPPORTED = -6
} nt_status;

typedef struct nt_scene nt_scene_t;

/* render.Channel (render.cpp:95-99,120-164) */
typedef struct {
    float f_r, f_g, f_b, f_c;
    uint8_t bit_size;            /* 1..31, or 32 when tfloat */
    uint8_t tfloat;              /* raw IEEE-754 bits of the clamped value */
    uint8_t _pad[2];
} nt_channel;

/* render.ImageFormat (render.cpp:167-172,249-288) */
typedef struct {
    int32_t width, height;
    int32_t pitch;               /* bytes per row; 0 => width * bytes_per_pixel */
    int32_t nchannels;
    const nt_channel *channels;
    int32_t reversed;            /* emit each pixel's bytes in reverse order */
} nt_image_format;

/* render.Material (render.hpp:56-73; defaults render.cpp:1249-1252,1269) */
typedef struct {
    float color[3];
    float specular[3];
    float opacity, reflectivity, specular_intensity, specular_exp;
} nt_material;

/* leaf item encoding: (index << 2) | kind */
#define NT_KIND_BATCH 0          /* tracern.TriangleBatch: index = batch number, 4 simplices */
#define NT_KIND_TRIANGLE 1       /* tracern.Triangle (unbatched leftover) */
#define NT_KIND_SOLID 2          /* tracern.Solid */
#define NT_SOLID_CUBE 1          /* wrapper.CUBE */
#define NT_SOLID_SPHERE 2        /* wrapper.SPHERE */

/*
 * Flat description of a composite_scene (tracer.hpp:1710-1740): the k-d tree of
 * KDBranch/KDLeaf objects, its primitives and materials.
 * Simplex record (n*n + n + 1 floats): d, face_normal[n], p1[n], edge_normal[n-1][n]
 * (tracer.hpp:399-401,539-541).  Solid record (2*n*n + n floats): orientation[n][n],
 * inv_orientation[n][n], position[n] (tracer.hpp:237-239).
 */
typedef struct {
    int32_t dimension;
    int32_t root;                /* node index, or -1 for an empty scene */
    int32_t n_nodes;
    const int32_t *node_axis;    /* branch: split axis; leaf: -1 */
    const float *node_split;
    const int32_t *node_left;    /* branch: child (< split) or -1; leaf: first item */
    const int32_t *node_right;   /* branch: child (>= split) or -1; leaf: item count */
    int32_t n_items;
    const int32_t *items;        /* per leaf: batches first (tracer.hpp:1149) */
    int32_t n_batches;
    const float *batch_recs;     /* [n_batches][NT_BATCH_SIZE][record] */
    const int32_t *batch_mats;   /* [n_batches][NT_BATCH_SIZE] material index */
    int32_t n_triangles;
    const float *tri_recs;
    const int32_t *tri_mats;
    int32_t n_solids;
    const float *solid_recs;
    const int32_t *solid_types;
    const int32_t *solid_mats;
    int32_t n_materials;
    const nt_material *materials;
    const float *aabb_start;     /* scene boundary (tracern.AABB) */
    const float *aabb_end;
} nt_scene_desc;

/* composite_scene attributes (tracer.hpp:1713-1725; setters ntracer_body.hpp:833-933) */
typedef struct {
    int32_t shadows;             /* default 0 */
    int32_t camera_light;        /* default 1 */
    int32_t max_reflect_depth;   /* default 4 */
    int32_t bg_gradient_axis;    /* default 1 */
    float ambient[3];            /* default 0,0,0 */
    float bg1[3], bg2[3], bg3[3];/* default (1,1,1) (0,0,0) (0,1,1) */
    int32_t n_point_lights;
    const float *point_light_pos;    /* [n][dimension] */
    const float *point_light_color;  /* [n][3] */
    int32_t n_global_lights;
    const float *global_light_dir;   /* [n][dimension] */
    const float *global_light_color; /* [n][3] */
} nt_scene_params;

typedef struct {
    int32_t device;              /* HIP device ordinal; -1 => current device */
    int32_t band_rank;           /* this caller renders bands b with b % band_world == band_rank */
    int32_t band_world;          /* 0 or 1 => whole image */
    int32_t band_rows;           /* 0 => NT_RENDER_CHUNK_SIZE */
    int32_t compact;             /* 1: dest holds only the owned rows, packed in band order */
    int32_t strict_reference;    /* 0: closest-hit walks skip k-d cells that start beyond the current hit (same pixels, far fewer
                                    tests).  1: walk exactly the cells the reference walks
                                    (src/tracer.hpp:1179-1243).  NTRACER_STRICT_REFERENCE=1 in the environment forces 1,
                                    also for nt_colors_at / nt_calculate_color, which take no options. */
    int32_t collect_stats;       /* 1: count rays/nodes/tests with device atomics (slower).  Never changes the pixels: scenes whose
                                    frames come from kernels without counters (Solids with the reference's normal handling) are
                                    drawn as always and counted by a launch of their own (the counters then describe the
                                    clean-normal traversal); scenes with transparent materials, and n > 10: NT_E_UNSUPPORTED */
    int32_t overlapped;          /* device entry points: 1 = the caller keeps two or more streams busy with calls like this one
                                    (consecutive calls overlap on the device: the ramp and the tail of a call are filled by its
                                    neighbours), so the library shapes its launches for throughput rather than for the time of a
                                    call that runs alone (BoxScene: longer waves).  Never changes the pixels.  0: default */
    /* Abort for the device entry points (nt_render_device / nt_render_frames_device), which only enqueue: NULL, or a dword
       the DEVICE can read while the kernels run -- best in device memory, raised by a 4-byte copy on another stream
       (pinned host memory works too, but every block's look at it is then a PCIe round trip) -- that the caller sets
       non-zero to cancel; blocks that have not started then leave without drawing (the reference polls its CANCEL state
       per pixel, src/render.cpp:412).  nt_render keeps such a word itself and relays the caller's `abort_flag` to it;
       this field is ignored there. */
    const volatile int32_t *abort_device;
} nt_render_opts;

/* counters gathered when collect_stats is set (SURVEY section 8d byte model) */
typedef struct {
    uint64_t rays;               /* primary + reflection rays */
    uint64_t shadow_rays;
    uint64_t branches;
    uint64_t leaves;
    uint64_t simplex_tests;
    uint64_t solid_tests;
    uint64_t hits;
    uint64_t aabb_enter;
} nt_stats;

/* ---- library ---- */
const char *nt_version(void);
const char *nt_last_error(void);             /* thread-local; "" when none */
int nt_device_count(void);                   /* number of HIP devices, 0 when none */

/* ---- scenes ---- */
/* tracern.BoxScene(dimension): box_scene (tracer.hpp:83-123; ntracer_body.hpp:676-715) */
nt_scene_t *nt_box_scene_create(int dimension);
/* tracern.CompositeScene(boundary,data): composite_scene (tracer.hpp:1710-1740; ntracer_body.hpp:720-933) */
nt_scene_t *nt_composite_scene_create(const nt_scene_desc *desc);
void nt_scene_destroy(nt_scene_t *s);
int nt_scene_dimension(const nt_scene_t *s);
int nt_scene_is_composite(const nt_scene_t *s);

/* Scene.set_camera / get_camera (ntracer_body.hpp:676-700): origin[n], axes row-major [n][n]
   (rows: right, up, forward, ...; camera.hpp:40-45).  NT_E_LOCKED while a render holds the scene. */
int nt_scene_set_camera(nt_scene_t *s, const float *origin, const float *axes);
int nt_scene_get_camera(const nt_scene_t *s, float *origin, float *axes);
/* Scene.set_fov / .fov (radians; default 0.8, tracer.hpp:91,1731) */
int nt_scene_set_fov(nt_scene_t *s, float fov);
float nt_scene_get_fov(const nt_scene_t *s);
/* Supersampling (the reference has no counterpart: it draws one ray a pixel).  factor s = 1..8, default 1 = one ray a pixel,
   nothing changes.  With s > 1 every render entry point draws, for a W x H image in any format, the box-filtered s*W x s*H
   frame of the same scene, camera and fov: sample (i, j) of pixel (x, y) is pixel (s*x + i, s*y + j) of that frame in the
   plain three-channel fp32 format, i.e. calculate_color's result with each component clamped to [0, 1]; the pixel's colour
   is the fp32 sum of its s*s samples taken one after the other in row-major order, divided by (float)(s*s); that colour
   then goes through the format's channel conversion and packing as always.  Both stages run on the device: the samples go
   to a scratch buffer of at most nt_scene_set_supersampling_scratch_mb MiB (1..2^20, default 1024) per scene and device,
   never more than the job needs, and larger jobs are cut into
   frame chunks and, below one frame, into row chunks.  The samples of ONE output row, 12*s*s*W bytes, must fit that
   buffer, and a sample row's 12*s*W bytes and the s*H sample rows must be countable in 31 bits: otherwise the render
   fails with NT_E_UNSUPPORTED before anything is launched.  nt_calculate_color / nt_colors_at answer for one ray and
   ignore the factor.  A view setting like fov: not part of a pickled scene.  NT_E_INVALID for a factor outside 1..8,
   NT_E_LOCKED while a render holds the scene.  No device is needed to set or get it. */
int nt_scene_set_supersampling(nt_scene_t *s, int factor);
int nt_scene_get_supersampling(const nt_scene_t *s);
int nt_scene_set_supersampling_scratch_mb(nt_scene_t *s, int mib);
int nt_scene_get_supersampling_scratch_mb(const nt_scene_t *s);
/* Adaptive supersampling: one more view setting beside the factor, off by default.  enabled != 0 with a finite float `threshold`
   t switches it on.  With it on and a factor s > 1, a W x H render is defined as follows.  Let P be the plain single-sample frame
   of the same scene, camera and fov, each component clamped to [0, 1] as a sample is clamped.  The contrast of pixel (x, y) is the
   largest |P[x,y][c] - P[x',y'][c]| over c in {r, g, b} and over those of its four neighbours (x +- 1, y), (x, y +- 1) that lie
   inside the image; a pixel without a neighbour inside the image has contrast 0.  The pixel is flagged iff contrast > t, in fp32.
   A flagged pixel gets exactly the supersampled pixel defined above (its s*s samples clamped, summed in fp32 in row-major order,
   divided by (float)(s*s)); an unflagged pixel gets P's colour; either goes through the format's conversion and packing as always.
   So t < 0 flags every pixel and the frame is the supersampled frame, t >= 1 flags none and the frame is the plain frame, and with
   s = 1 the setting changes nothing.  What the scheme cannot see: a feature thinner than a pixel that every pixel-centre ray
   misses leaves no contrast in P and is not refined.  All of it runs on the device (a base frame and a list of flagged pixels, 16
   bytes a pixel a frame, under the cap of nt_scene_set_supersampling_scratch_mb; larger jobs are cut into chunks of whole frames,
   and a single frame that does not fit fails with NT_E_UNSUPPORTED before anything is launched).  Refused with NT_E_UNSUPPORTED
   ("adaptive ...") before a device is touched, drawing nothing: row bands (band_world > 1) and collect_stats -- a pixel's
   neighbours across a band are not there, and the refining kernels keep no counters.  A lens and the parallel projection refuse
   any factor above 1 as before.  nt_calculate_color / nt_colors_at, nt_primary_hits*, nt_ray_colors*, nt_render_rays* and the ray
   queries ignore the setting, as they ignore the factor.  Not part of a pickled scene.  NT_E_INVALID for a NaN or infinite
   threshold (the setting stays as it was), NT_E_LOCKED while a render holds the scene.  No device is needed to set or get it;
   the getter writes 0 / 1 and the threshold (0 when off) through whichever pointers are not NULL. */
int nt_scene_set_adaptive_supersampling(nt_scene_t *s, int enabled, float threshold);
int nt_scene_get_adaptive_supersampling(const nt_scene_t *s, int *enabled, float *threshold);
/* The flags of a width x height render of the scene's own camera under the threshold that is set, whatever the factor:
   mask[y * width + x] = 1 for a flagged pixel, 0 otherwise.  The host form also returns their number through `flagged` (may be
   NULL); it reads device, strict_reference of `opts`.  The device form writes width * height bytes of device memory at mask_dev
   and is only enqueued on hip_stream; it also reads abort_device and overlapped.  NT_E_INVALID when the threshold is off;
   NT_E_UNSUPPORTED for bands or collect_stats in `opts`, and while a lens or the parallel projection is set. */
int nt_adaptive_mask(nt_scene_t *s, int width, int height, uint8_t *mask, long long *flagged, const nt_render_opts *opts);
int nt_adaptive_mask_device(nt_scene_t *s, int width, int height, void *mask_dev, const nt_render_opts *opts, void *hip_stream);
/* Ambient occlusion: a view setting of a CompositeScene, off by default, that darkens a pixel by how enclosed its primary hit is.
   count = K (1..256) samples, `directions` a [K][n] table (every component finite, no row all zero, rows used as given, not
   normalised), radius > 0, bias >= 0, strength in [0, 1]; count = 0 takes it off.  Everything below is fp32 without contraction,
   dot products summed left to right.
   The blocked count of pixel (x, y) of a W x H view rests on the record nt_primary_hits defines for that pixel, normal_origin = no
   and normal_dir = nd included.  Without an opaque hit blocked = -1.  Otherwise, with d the primary ray's unit direction,
   side = -dot(d, nd), b = side < 0 ? -bias : bias, o'[j] = no[j] + nd[j] * b; for k = 0..K-1, s = dot(nd, t_k) and
   v = ((s < 0) != (side < 0)) ? -t_k : t_k; sample k is blocked iff the closest-hit walk nt_intersect_rays defines -- origin o',
   direction v, t_near = 0, t_far = radius, (skip_item, skip_lane) the primary hit's (item, lane), strict_reference and the
   NTRACER_* switches as for a query on this scene -- answers item >= 0 && dist <= radius.  The radius is thus in units of |t_k|;
   transparent surfaces do not block; blocked is the number of blocked samples.
   A render with the setting on: P the plain single-sample frame with each component clamped to [0, 1], a = (float)blocked / (float)K
   (0 for blocked = -1), f = 1.0f - strength * a, and the pixel is (P.r * f, P.g * f, P.b * f) through the format's conversion
   and packing as always: with strength = 0, or where nothing blocks, the plain frame byte for byte.  nt_render, nt_render_device,
   nt_render_frames_device and nt_render_table_device honour the setting and refuse with NT_E_UNSUPPORTED ("ambient occlusion
   ...") before a device is touched, drawing nothing: a supersampling factor above 1, row bands (band_world > 1),
   collect_stats, a lens, the parallel projection (and a row range, which only a caller inside the library can ask for).  nt_colors_at / nt_calculate_color, nt_primary_hits*, nt_ray_colors*,
   nt_render_rays* and the ray queries ignore it.  All of it runs on the device under the cap of
   nt_scene_set_supersampling_scratch_mb: 32 + 8 n bytes a pixel a frame, and for scenes with transparent materials, Solids with the
   reference's normals, n > 10 or NTRACER_FORCE_VAR=1 also 8 n + 32 bytes a ray of a chunk of whole pixel rows; larger jobs are cut
   into chunks of whole frames, and a single frame (with one row of rays) that does not fit fails with NT_E_UNSUPPORTED before
   anything is launched.  Not part of a pickled scene.  NT_E_INVALID for a BoxScene, a count outside 0..256, NULL directions with
   count > 0, a non-finite or all-zero row, a radius that is not positive and finite, a negative or non-finite bias, a strength
   outside [0, 1] (the setting stays as it was); NT_E_LOCKED while a render holds the scene.  No device is needed to set or get it;
   the getter writes through whichever pointers are not NULL, the table ([count][n] floats) included. */
int nt_scene_set_ambient_occlusion(nt_scene_t *s, int count, const float *directions, float radius, float bias, float strength);
int nt_scene_get_ambient_occlusion(const nt_scene_t *s, int *count, float *directions, float *radius, float *bias, float *strength);
/* The blocked counts of a width x height view of the scene's current camera, blocked[y * width + x].  The host form holds the
   scene like nt_colors_at and reads device and strict_reference of `opts`.  The device form writes exactly width * height dwords of
   device memory at blocked_dev and is only enqueued on hip_stream; it also reads abort_device, and every other field of `opts`
   must be 0.  NT_E_INVALID when the setting is off; NT_E_UNSUPPORTED while a lens or the parallel projection is set. */
int nt_ambient_occlusion(nt_scene_t *s, int width, int height, int32_t *blocked, const nt_render_opts *opts);
int nt_ambient_occlusion_device(nt_scene_t *s, int width, int height, void *blocked_dev, const nt_render_opts *opts, void *hip_stream);
/* Outlines (the reference has none): a line along the silhouette, along every edge where two facets meet at an angle and along
   every jump in depth, drawn on the device from the primary hits of the render itself.  CompositeScene only.  enabled = 0 takes
   the setting off; else crease_cos in [0, 1], depth_gap >= 0 (0: no depth lines), every color component and strength in [0, 1],
   all finite.  Everything below is fp32 without contraction, dot products summed left to right.
   For a W x H view let R(p) = (dist, item, lane) and nd(p) = normal_dir be what nt_primary_hits defines for pixel p, with the
   strict_reference and NTRACER_* switches of a render of the scene.  The mask byte of p is 0 when item(p) < 0.  Otherwise it is
   the OR, over those of the four neighbours q = (x +- 1, y), (x, y +- 1) that lie inside the image, of
     NT_OUTLINE_SILHOUETTE  if item(q) < 0;
     nothing                if item(q) == item(p) and lane(q) == lane(p);
     nothing                if dist(p) > dist(q): the nearer pixel carries the line, so lines are one pixel wide;
     otherwise, with c = dot(nd(p), nd(q)), la = dot(nd(p), nd(p)), lb = dot(nd(q), nd(q)) and cc = crease_cos * crease_cos
     computed once,
       NT_OUTLINE_CREASE    if c * c < cc * (la * lb),
       NT_OUTLINE_DEPTH     if depth_gap > 0 and (dist(q) - dist(p)) > depth_gap * dist(p).
   Neighbours outside the image do not count (a 1 x 1 view has no lines) and never cross a frame boundary.  The normals are used
   as given: they are not all of unit length (hence la * lb) and are compared up to sign, because neighbouring simplices of one
   facet may be oriented either way.  Transparent surfaces carry no lines: the records are those of opaque hits.
   A render with the setting on: P the plain single-sample frame with each component clamped to [0, 1]; a pixel with mask != 0
   becomes (P.c * (1.0f - strength)) + (color.c * strength) for each component c, every other pixel is P, and either goes through
   the format's conversion and packing as always: with strength = 0 the plain frame byte for byte.  nt_render, nt_render_device,
   nt_render_frames_device and nt_render_table_device honour the setting and refuse with NT_E_UNSUPPORTED ("outlines ...")
   before a device is touched, drawing nothing: a supersampling factor above 1 (adaptive or not), row bands (band_world > 1),
   collect_stats, a lens, the parallel projection, ambient occlusion being on (and a row range, which only a caller inside the
   library can ask for).  nt_colors_at / nt_calculate_color, nt_primary_hits*, nt_ray_colors*, nt_render_rays*, the ray queries,
   nt_adaptive_mask* and nt_ambient_occlusion* ignore it.  Opaque scenes up to 10 dimensions on the renders' packet walk are drawn
   from one walk: 16 bytes of record a pixel a frame.  Every other scene (transparent materials, Solids with the reference's
   normals, n > 10, NTRACER_FORCE_VAR=1, NTRACER_COMPOSITE_KERNEL set) takes 29 + 4 n bytes a pixel a frame -- base frame, record,
   normal row, mask; 17 + 4 n for nt_outline_mask*, which draw no base frame -- under the cap of nt_scene_set_supersampling_scratch_mb, and so does the packet walk's record scratch here:
   larger jobs are cut into chunks of whole frames, and a single frame that does not fit fails with NT_E_UNSUPPORTED before
   anything is launched.  Not part of a pickled scene.  NT_E_INVALID for a BoxScene and for a value outside its range (the
   setting stays as it was); NT_E_LOCKED while a render holds the scene.  No device is needed to set or get it; the getter writes
   through whichever pointers are not NULL. */
#define NT_OUTLINE_SILHOUETTE 1
#define NT_OUTLINE_CREASE 2
#define NT_OUTLINE_DEPTH 4
int nt_scene_set_outlines(nt_scene_t *s, int enabled, float crease_cos, float depth_gap, const float color[3], float strength);
int nt_scene_get_outlines(const nt_scene_t *s, int *enabled, float *crease_cos, float *depth_gap, float color[3], float *strength);
/* The mask bytes of a width x height view of the scene's current camera, mask[y * width + x].  The host form also returns the
   number of non-zero bytes through `marked` (may be NULL); it holds the scene like nt_colors_at and reads device and
   strict_reference of `opts`.  The device form writes exactly width * height bytes of device memory at mask_dev and is only
   enqueued on hip_stream; it also reads abort_device, and every other field of `opts` must be 0.  NT_E_INVALID when the setting
   is off; NT_E_UNSUPPORTED while a lens or the parallel projection is set. */
int nt_outline_mask(nt_scene_t *s, int width, int height, uint8_t *mask, long long *marked, const nt_render_opts *opts);
int nt_outline_mask_device(nt_scene_t *s, int width, int height, void *mask_dev, const nt_render_opts *opts, void *hip_stream);
/* Depth cues (the reference has none): a surface fades towards a fog colour with its distance from the eye, and is tinted by
   where its visible point lies along a direction of n-space ("colour by w"), on the device from the primary hits of the render
   itself.  CompositeScene only.  Everything below is fp32 without contraction, sums left to right,
   clamp01(v) = max(0, min(1, v)).  The host forms two reciprocals once, in fp32: inv_fog = 1.0f / (fog_far - fog_near) and,
   with a tint, inv_tint = 1.0f / (tint_hi - tint_lo).
   For a W x H view let R(p) = (dist, item, lane, n_transparent) be what nt_primary_hits defines for pixel p, with the
   strict_reference and NTRACER_* switches of a render of the scene, o the camera's origin and d the primary ray's unit direction
   as the render forms it.  The pixel's two factors (f, g):
     item >= 0:  t = dist, f = clamp01((t - fog_near) * inv_fog);
                 with a tint x_k = (d_k * t) + o_k, s = tint_axis_0 * x_0, then s = s + (tint_axis_k * x_k) for k = 1 .. n - 1,
                 and g = clamp01((s - tint_lo) * inv_tint); without a tint g = -1;
     item < 0, fog_background set and n_transparent == 0:  f = 1, g = -1;
     otherwise f = -1, g = -1: the pixel is left alone.  Transparent surfaces carry no cue, as they carry no lines.
   A render with the setting on: P the plain single-sample frame with each component clamped to [0, 1], Q = P;
     if g >= 0:  Q.c = P.c * ((tint_color_lo.c * (1.0f - g)) + (tint_color_hi.c * g));
     if f >= 0:  w = f * fog_strength and Q.c = (Q.c * (1.0f - w)) + (fog_color.c * w);
   and Q goes through the format's conversion and packing as always: with fog_strength = 0 and no tint the plain frame byte for
   byte.  nt_render, nt_render_device, nt_render_frames_device and nt_render_table_device honour the setting and refuse with
   NT_E_UNSUPPORTED ("depth cue ...") before a device is touched, drawing nothing: a supersampling factor above 1 (adaptive or
   not), row bands (band_world > 1), collect_stats, a lens, the parallel projection, ambient occlusion, outlines (and a row
   range, which only a caller inside the library can ask for).  nt_colors_at / nt_calculate_color, nt_primary_hits*,
   nt_ray_colors*, nt_render_rays*, the ray queries, nt_adaptive_mask*, nt_ambient_occlusion* and nt_outline_mask* ignore it.
   Opaque scenes up to 10 dimensions on the renders' packet walk are drawn from one walk: 16 bytes of record a pixel a frame.
   Every other scene (transparent materials, Solids with the reference's normals, n > 10, NTRACER_FORCE_VAR=1,
   NTRACER_COMPOSITE_KERNEL set) takes 28 bytes a pixel a frame -- base frame and record; 16 for nt_depth_cue_factors*, which
   draw no base frame -- under the cap of nt_scene_set_supersampling_scratch_mb, and so does the packet walk's record scratch
   here: larger jobs are cut into chunks of whole frames, and a single frame that does not fit fails with NT_E_UNSUPPORTED
   before anything is launched.  Not part of a pickled scene. */
typedef struct nt_depth_cue {
    float fog_near, fog_far;           /* 0 <= fog_near < fog_far, 1 / (fog_far - fog_near) finite */
    float fog_color[3];                /* every colour component and fog_strength in [0, 1] */
    float fog_strength;
    int32_t fog_background;            /* not 0: pixels that hit nothing at all take the fog in full */
    float tint_lo, tint_hi;            /* read with a tint_axis only: tint_lo < tint_hi, 1 / (tint_hi - tint_lo) finite */
    float tint_color_lo[3], tint_color_hi[3];
} nt_depth_cue;
/* cue == NULL takes the setting off; tint_axis == NULL means no tint, else `dimension` floats, finite and not all zero.
   NT_E_INVALID for a BoxScene and for a value that is not finite or outside its range (the setting stays as it was);
   NT_E_LOCKED while a render holds the scene.  No device is needed to set or get it; the getter writes through whichever
   pointers are not NULL: *enabled 0 or 1, *cue (zeroes while off, tint fields zero without a tint), *has_tint 0 or 1,
   tint_axis `dimension` floats (zeroes without a tint). */
int nt_scene_set_depth_cue(nt_scene_t *s, const nt_depth_cue *cue, const float *tint_axis);
int nt_scene_get_depth_cue(const nt_scene_t *s, int *enabled, nt_depth_cue *cue, int *has_tint, float *tint_axis);
/* The factors (f, g) of a width x height view of the scene's current camera, factors[(y * width + x) * 2 + {0, 1}].  The host
   form holds the scene like nt_colors_at and reads device and strict_reference of `opts`.  The device form writes exactly
   width * height * 8 bytes of device memory at factors_dev and is only enqueued on hip_stream; it also reads abort_device, and
   every other field of `opts` must be 0.  NT_E_INVALID when the setting is off; NT_E_UNSUPPORTED while a lens or the parallel
   projection is set. */
int nt_depth_cue_factors(nt_scene_t *s, int width, int height, float *factors, const nt_render_opts *opts);
int nt_depth_cue_factors_device(nt_scene_t *s, int width, int height, void *factors_dev, const nt_render_opts *opts, void *hip_stream);
/* Clip planes (the reference has none): cutaway views.  Up to NT_CLIP_MAX planes; plane k is a normal a_k of `dimension`
   floats, finite and not all zero (it need not be a unit vector), and a finite offset b_k.  The keep-region is the set of
   points x with a_k . x <= b_k for every k: what lies outside it does not exist for any ray the tracer casts.  CompositeScene
   only.  Everything below is fp32 without contraction, sums left to right.
   The window of a ray (o, d), d exactly as the walk that casts the ray uses it:
     t0 = 0, t1 = FLT_MAX, empty = false;
     for k = 0 .. count - 1:  p = a_k0 * o_0, then p = p + a_kj * o_j for j = 1 .. n - 1;  s = p - b_k;
                              r = a_k0 * d_0, then r = r + a_kj * d_j for j = 1 .. n - 1;
         r > 0:             q = (-s) / r, and if q < t1 then t1 = q;
         r < 0:             q = (-s) / r, and if q > t0 then t0 = q;
         r == 0 and s > 0:  empty = true;
     at the end empty = empty or t0 > t1.
   A candidate hit at parameter t of any primitive test is accepted iff the rule without planes accepts it and
   !empty && t0 <= t <= t1.  This holds for every ray: primary rays, shadow rays (beside their light-distance rule), reflection
   rays and the continuation through transparent hits -- the geometry cut away casts no shadow and shows in no mirror.  A
   rejected candidate leaves the walk as if the primitive had never been tested (the hit, the transparent list and which
   subtrees count as having improved it; the walk's record of tested primitives may remember it).  A primary walk starts at
   max(aabb entry, t0) and ends at t1; the walks of the other rays visit the cells they always visit.  Lights keep shining from
   wherever they are.  There are no caps: a cut shell is open and its inner side is seen.
   nt_render, nt_render_device, nt_render_frames_device and nt_render_table_device honour the setting, and so do nt_primary_hits,
   nt_primary_hits_device and nt_primary_hits_table_device, normal rows included: picking under a cutaway answers what is seen.
   Refused with NT_E_UNSUPPORTED ("clip planes ...") before a device is touched, drawing nothing: a supersampling factor above 1
   (adaptive or not), row bands (band_world > 1), collect_stats, a lens, the parallel projection, ambient occlusion, outlines,
   depth cues, and a scene with Solids -- a Solid cut open needs a cap or an inner wall, which nothing here defines -- (and a
   row range, which only a caller inside the library can ask for).  While the
   setting is on nt_colors_at / nt_calculate_color, nt_ray_colors*, nt_render_rays*, nt_adaptive_mask*, nt_ambient_occlusion*,
   nt_outline_mask* and nt_depth_cue_factors* are refused likewise.  The ray queries (nt_intersect_rays*, nt_occludes_rays*) are
   the tree's own methods and ignore the setting.
   Opaque scenes up to 10 dimensions on the renders' packet walk are drawn from one clipped walk into 16 bytes of record a
   pixel and a shading pass; every other scene (transparent materials, n > 10, NTRACER_FORCE_VAR=1, NTRACER_COMPOSITE_KERNEL
   set, trees deeper than the walk's stack) by the run-time-n kernels.  Not part of a pickled scene. */
#define NT_CLIP_MAX 8
/* normals: [count][dimension], offsets: [count].  count == 0 or a NULL pointer takes the setting off.  NT_E_INVALID for a
   BoxScene, a count outside [0, NT_CLIP_MAX] and a non-finite or all-zero normal or a non-finite offset (the setting stays as
   it was); NT_E_LOCKED while a render holds the scene.  No device is needed to set or get it; the getter writes through
   whichever pointers are not NULL: *count, then `count` rows of normals and `count` offsets (room for NT_CLIP_MAX suffices). */
int nt_scene_set_clip_planes(nt_scene_t *s, int count, const float *normals, const float *offsets);
int nt_scene_get_clip_planes(const nt_scene_t *s, int *count, float *normals, float *offsets);
/* CompositeScene.set_shadows/set_camera_light/set_max_reflect_depth/set_ambient_color/
   set_background/add_light rolled into one call */
int nt_scene_set_params(nt_scene_t *s, const nt_scene_params *p);
/* class scene::lock()/unlock() (render.hpp:18-22) and the Python `locked` attribute */
int nt_scene_lock(nt_scene_t *s);
int nt_scene_unlock(nt_scene_t *s);
int nt_scene_locked(const nt_scene_t *s);

/* ---- rendering ---- */
/* ImageFormat.bytes_per_pixel (render.cpp:192-209); negative status on an invalid format */
int nt_format_bytes_per_pixel(const nt_image_format *fmt);

/* BlockingRenderer.render(dest, format, scene) (render.cpp:853-909): dest is HOST memory of at
   least pitch*height bytes (or the compact size).  abort_flag (may be NULL) is polled on the host
   while the frame's one launch runs and relayed to a dword the kernels read when a block starts: blocks that have not
   started leave without drawing.  Returns NT_ABORTED if the flag became non-zero before the frame was finished
   (signal_abort, render.cpp:911-923); an aborted frame is not copied back -- `dest` stays as the caller had it. */
int nt_render(nt_scene_t *s, void *dest, size_t dest_len, const nt_image_format *fmt,
              const nt_render_opts *opts, volatile int *abort_flag);

/* (Streams: the launches of one scene on one device share that scene's scratch buffers and are ordered by the stream they
   are enqueued on.  A call that names another stream than the scene's previous call on that device first waits, on the
   host, for the previous stream to drain -- alternate streams per scene handle, not within one.) */
/* Same frame loop, but dest is DEVICE memory on opts->device and the launch is only enqueued on
   `hip_stream` (a hipStream_t; NULL = the legacy default stream); no host synchronisation.  Used
   by the bench (framebuffer resident in HBM) and by the multi-GPU gather.  The scene must stay
   alive and unmodified until the stream has drained. */
int nt_render_device(nt_scene_t *s, void *dest_dev, size_t dest_len, const nt_image_format *fmt,
                     const nt_render_opts *opts, void *hip_stream);

/* Render `nframes` frames with per-frame cameras in ONE launch (the RotatingCamera loop of the
   reference's scripts/polytope.py:522-556 without a launch per frame).  origins [nframes][n],
   axes [nframes][n][n]; frame f goes to dest_dev + f*frame_stride. */
int nt_render_frames_device(nt_scene_t *s, void *dest_dev, size_t frame_stride, int nframes,
                            const float *origins, const float *axes, const nt_image_format *fmt,
                            const nt_render_opts *opts, void *hip_stream);

/* A camera path resident in device memory: the cameras of a sequence (the RotatingCamera loop of scripts/polytope.py:522-556
   has 160) packed and uploaded ONCE; nt_render_table_device then renders frames [first, first + count) of it exactly like
   nt_render_frames_device, but with nothing to pack or upload per call -- one kernel launch instead of two, which is what a
   render loop over a fixed path, and a rank's small share of a tiled frame, spend a tenth of their time on.
   The table belongs to the scene's dimension and to one device; it may be used by any scene of that dimension.
   After a warm-up call such a call only launches kernels and may be captured into a HIP graph; nt_render_frames_device, which
   stages host memory per call, returns NT_E_UNSUPPORTED on a capturing stream. */
typedef struct nt_camera_table nt_camera_table_t;
nt_camera_table_t *nt_camera_table_create(int dimension, int nframes, const float *origins, const float *axes, int device);
void nt_camera_table_destroy(nt_camera_table_t *t);
int nt_camera_table_frames(const nt_camera_table_t *t);
int nt_render_table_device(nt_scene_t *s, void *dest_dev, size_t frame_stride, const nt_camera_table_t *table, int first, int count,
                           const nt_image_format *fmt, const nt_render_opts *opts, void *hip_stream);

/* Scene.calculate_color(x,y,width,height) (render.cpp:586-614): unpacked fp32 colour of one pixel,
   computed by the same device code as nt_render. */
int nt_calculate_color(nt_scene_t *s, int x, int y, int width, int height, float rgb[3]);
/* batched form: `count` pixels (xs, ys) -> rgb[count][3] */
int nt_colors_at(nt_scene_t *s, int width, int height, int count, const int32_t *xs, const int32_t *ys,
                 float *rgb, int device);

/* ---- ray queries ---------------------------------------------------------------------------------------
   KDNode.intersects / KDNode.occludes of the reference (src/ntracer_body.hpp:1412-1496) on the scene's root, for `count`
   arbitrary rays in one call: a ray in, one record out.  A ray's answer is that of the reference's walk for that ray alone
   (closest hit: kd_node_intersection, src/tracer.hpp:1179-1243, starting from o_hit.dist = max; occlusion: _occludes,
   :1258-1307, its far-child rule included); the caller's t_near / t_far go to the root call and (skip_item, skip_lane) is the
   intersection_target the ray leaves from.  There is no scene-box test in front: the methods have none.
   CompositeScene only (the reference's BoxScene has no tree): a BoxScene handle is NT_E_INVALID.  An empty scene answers
   "no hit / not blocked".  The closest-hit walk skips cells beyond the current hit unless strict_reference is set
   (nt_render_opts, or NTRACER_STRICT_REFERENCE=1), and o_hit.normal is the reference's unless NTRACER_CLEAN_NORMALS=1, both
   exactly as for a render. */
#define NT_TH_MAX 24             /* transparent hits kept per ray */

typedef struct {                 /* 16 bytes: one dwordx4 store a ray */
    float dist;                  /* nearest opaque hit, in units of |direction|; FLT_MAX when none */
    int32_t item;                /* (index << 2) | NT_KIND_*, the leaf-item code; -1: no opaque hit */
    int32_t lane;                /* simplex inside the batch; -1 otherwise */
    int32_t n_transparent;       /* transparent hits left in the reference's list when the walk ends; in the records of
                                    nt_hit_layers this word is `count` (NT_LAYER_COUNT below) */
} nt_ray_hit;

typedef struct {
    int32_t count;
    const float *origins, *directions;      /* [count][n]; directions are used as given, not normalised */
    const float *t_near, *t_far;            /* NULL (= -FLT_MAX / FLT_MAX, the reference's defaults) or [count] */
    const float *distance;                  /* occlusion only: NULL (= FLT_MAX) or [count] */
    const int32_t *skip_item, *skip_lane;   /* NULL (= none) or [count]: the reference's `source` / `batch_index` */
} nt_ray_batch;

typedef struct {
    nt_ray_hit *hits;                       /* [count]; occlusion: item = -1, dist = blocked ? 1 : 0, n_transparent filled */
    float *normal_origin, *normal_dir;      /* NULL or [count][n]: o_hit.normal; rows of rays without an opaque hit are left alone */
    nt_ray_hit *transparent;                /* NULL or [count][max_transparent]: the list itself, in the walk's order (unused
                                               slots: item = -1) */
    int32_t max_transparent;                /* 0..24 (NT_TH_MAX) */
} nt_ray_results;

/* Host memory in, host memory out; returns when the results are in place.  Holds the scene like nt_colors_at (NT_E_BUSY
   while a render runs) and stages through the scene's probe scratch on the library's own stream.  NT_E_INVALID, before any
   device is touched: NULL rays / out / hits / origins / directions, count < 0, max_transparent outside 0..NT_TH_MAX, a
   `transparent` pointer with max_transparent == 0.  count == 0: NT_OK without a device. */
int nt_intersect_rays(nt_scene_t *s, const nt_ray_batch *rays, const nt_ray_results *out, int device);
int nt_occludes_rays(nt_scene_t *s, const nt_ray_batch *rays, const nt_ray_results *out, int device);
/* Every pointer of `rays` and `out` is DEVICE memory on opts->device; the launch is only enqueued on `hip_stream`, with the
   stream and lifetime rules of nt_render_device.  Of `opts` (may be NULL) device, strict_reference and abort_device are
   read -- blocks that start after the abort word is raised leave without writing -- and every other field must be 0, else
   NT_E_INVALID.  After a warm-up call with the same count nothing is allocated.  (The one buffer a query may allocate, the
   per-lane `checked` scratch of scenes with transparent materials or Solids, is shared with the scene's renders on that device
   and only grows: a render in between that needs a larger one reallocates it, which synchronises the device once.) */
int nt_intersect_rays_device(nt_scene_t *s, const nt_ray_batch *rays, const nt_ray_results *out,
                             const nt_render_opts *opts, void *hip_stream);
int nt_occludes_rays_device(nt_scene_t *s, const nt_ray_batch *rays, const nt_ray_results *out,
                            const nt_render_opts *opts, void *hip_stream);

/* ---- primary-hit buffers ----------------------------------------------------------------------------------
   What is under each pixel of a view: composite_scene::ray_color at depth 0 up to the point where shading starts
   (src/tracer.hpp:1856-1868).  For pixel (x, y) of a width x height view with the scene's camera and fov: d = the primary
   ray's unit direction (integer pixel coordinates), t0 = aabb_distance(origin, d); t0 < 0: no hit; otherwise the record of
   kd_node_intersection on the root with t_near = t0, t_far = FLT_MAX and no source.  The record is nt_ray_hit: a pixel
   without an opaque hit gets FLT_MAX, -1, -1, n_transparent (0 when the ray misses the scene box); d is a unit vector, so
   dist is the Euclidean depth.  Every pixel's record is written.  One ray a pixel: the supersampling factor is ignored, as
   by nt_colors_at.  The walk obeys strict_reference and the NTRACER_* switches exactly as a render of the scene does (opaque
   scenes up to 10 dimensions take the render's packet walk).  CompositeScene only: a BoxScene handle is NT_E_INVALID.  An
   empty scene answers "no hit" for every pixel. */
typedef struct {
    nt_ray_hit *hits;                       /* [frame][height][width]; a pixel's record index is
                                               frame * frame_stride_records + y * width + x */
    float *normal_origin, *normal_dir;      /* NULL or [record index][n]: o_hit.normal; the rows of pixels without an opaque
                                               hit are left alone */
} nt_hit_buffers;

/* Host memory out, the scene's current camera, one frame; returns when the records are in place.  Holds the scene like
   nt_colors_at.  NT_E_INVALID, before any device is touched: NULL scene / out / hits, width or height < 1, a BoxScene,
   width * height beyond 2^31 - 1 records. */
int nt_primary_hits(nt_scene_t *s, int width, int height, const nt_hit_buffers *out, int device);
/* Every pointer of `out` is DEVICE memory on opts->device; the launch is only enqueued on `hip_stream`, with the stream and
   lifetime rules of nt_render_device.  Of `opts` (may be NULL) device, strict_reference and abort_device are read -- blocks
   that start after the abort word is raised leave without writing -- and every other field must be 0, else NT_E_INVALID. */
int nt_primary_hits_device(nt_scene_t *s, int width, int height, const nt_hit_buffers *out, const nt_render_opts *opts,
                           void *hip_stream);
/* ... frames [first, first + count) of a camera table in one launch, as nt_render_table_device renders them:
   frame_stride_records >= width * height records lie between the frames (the records and normal rows in between are not
   touched).  NT_E_INVALID also for a table of another dimension or device, a bad first / count, a stride smaller than a
   frame, and count * frame_stride_records beyond 2^31 - 1.  After a warm-up call of the same shape nothing is allocated
   (the `checked` scratch is shared with renders and queries as described above). */
int nt_primary_hits_table_device(nt_scene_t *s, int width, int height, const nt_hit_buffers *out, size_t frame_stride_records,
                                 const nt_camera_table_t *table, int first, int count, const nt_render_opts *opts,
                                 void *hip_stream);

/* ---- colours of the caller's rays -----------------------------------------------------------------------------
   The shaded result for rays the camera did not make.  For ray r with origin o and direction v: the direction is normalised
   exactly as the ray source normalises a primary ray (src/tracer.hpp:71-75) -- |v|^2 summed left to right, sqrtf, one IEEE
   division per component -- and d is that unit direction.  CompositeScene: the colour is ray_color(o, d, depth 0, no source)
   (src/tracer.hpp:1856-1883), i.e. what composite_scene::calculate_color does after the ray source, scene-box test included.
   BoxScene: box_scene::calculate_color's colour for that ray (:101-114).  The walk obeys strict_reference,
   NTRACER_CLEAN_NORMALS and NTRACER_FORCE_VAR exactly as a render of the scene does; the scene's camera, fov and supersampling
   factor are ignored.  An empty composite scene gives the background.  Every dimension a render supports is supported
   (compile-time kernels for n = 3..10, BoxScene to 24; run-time n to 64).  The rays of a batch need not be coherent: the
   packet walk and BoxScene's stretch shortcuts are not used, so a camera's own rays cost more here than a render of them.
   A ray with a non-finite component or an all-zero direction: the host forms refuse the batch; the device forms cannot look
   at the rays, and such a ray's colour is unspecified (every loop of the walks is bounded by the tree and the reflection
   depth whatever the bits are, so the call still ends and the other rays are not affected). */
typedef struct {
    int32_t count;
    const float *origins;        /* [count][n]; or [n], one origin for every ray, when shared_origin != 0 */
    const float *directions;     /* [count][n], any non-zero finite length */
    int32_t shared_origin;
} nt_rays;

/* Host memory in, host memory out: rgb[count][3], the unpacked fp32 colours as nt_colors_at gives them.  Holds the scene like
   nt_colors_at (NT_E_BUSY while a render runs), stages through the scene's probe scratch on the library's own stream and
   returns when the result is in place.  NT_E_INVALID, before any device is touched: NULL scene / rays / rgb / origins /
   directions, count < 0, a ray with a non-finite component or an all-zero direction (the message names the first such
   ray).  count == 0: NT_OK without a device. */
int nt_ray_colors(nt_scene_t *s, const nt_rays *rays, float *rgb, int device);
/* Every pointer is DEVICE memory on opts->device; the launch is only enqueued on `hip_stream`, with the stream and lifetime
   rules of nt_render_device.  Of `opts` (may be NULL) device, strict_reference and abort_device are read -- blocks that start
   after the abort word is raised leave without writing -- and every other field must be 0, else NT_E_INVALID.  After a
   warm-up call of the same count nothing is allocated (the `checked` and frame scratch of scenes with transparent materials
   or Solids is shared with the scene's renders and queries on that device, as described for the ray queries). */
int nt_ray_colors_device(nt_scene_t *s, const nt_rays *rays, float *rgb, const nt_render_opts *opts, void *hip_stream);
/* The same colours as an image in any format: ray y * width + x is pixel (x, y), packed as nt_render packs it (whole image,
   no bands, one ray a pixel); count must equal fmt->width * fmt->height.  `dest` is HOST memory, staged through the scene's
   framebuffer scratch; pitch padding keeps the caller's bytes.  NT_E_INVALID as for nt_ray_colors, and for NULL dest, an
   invalid format (the checks and messages of nt_render), a count that does not match it, dest_len too small. */
int nt_render_rays(nt_scene_t *s, void *dest, size_t dest_len, const nt_image_format *fmt, const nt_rays *rays, int device);
/* ... dest_dev and the rays in DEVICE memory, enqueued on `hip_stream`; `opts` as for nt_ray_colors_device. */
int nt_render_rays_device(nt_scene_t *s, void *dest_dev, size_t dest_len, const nt_image_format *fmt, const nt_rays *rays,
                          const nt_render_opts *opts, void *hip_stream);

/* ---- lenses: fisheye, panoramic and other projections that keep the eye in one point ---------------------------
   A lens is a table of width x height x 3 fp32 coefficients (sx, sy, sz), row-major [y][x].  Set on a scene it replaces the
   pinhole ray source of the render entry points: pixel (x, y)'s ray leaves the camera's origin along
       v[j] = (forward[j] * sz + right[j] * sx) - up[j] * sy,      d = v / |v|
   with d formed as the pinhole's is (|v|^2 summed left to right, sqrtf, one IEEE division a component, no contraction).  The
   pinhole itself is sz = 1, sx = fovI * (x - width / 2), sy = fovI * (y - height / 2), fovI = tan(fov / 2) / (width / 2); with
   sz = 1.0f the direction is the pinhole's bit for bit.  The table does not depend on the camera: it is uploaded to a device
   on first use there and serves every frame.  An entry whose three coefficients are all zero, or that holds a NaN, is a
   masked pixel: no ray is cast and the pixel gets colour (0, 0, 0) through the format.  While a lens is set the scene's fov
   is ignored; strict_reference and the NTRACER_* render switches act as on any render.
   Honoured by nt_render, nt_render_device, nt_render_frames_device and nt_render_table_device, which return NT_E_INVALID --
   before any device is touched -- when the lens is not of the format's width x height, and NT_E_UNSUPPORTED, drawing nothing,
   for what a lens does not do yet: a supersampling factor above 1, row bands (band_world > 1), collect_stats.  With a lens
   set nt_colors_at / nt_calculate_color and nt_primary_hits* are refused with NT_E_UNSUPPORTED as well (never answered with
   the pinhole).  nt_ray_colors*, nt_render_rays* and the ray queries take their rays from the caller and ignore the lens.
   Opaque CompositeScenes up to 10 dimensions keep the packet walk under a lens (two passes: the walk leaves 16-byte hit
   records, a shading pass picks them up); every other scene is rendered by the ray-colour kernels from directions expanded
   on the device, in bands of whole rows of at most 1 GiB. */
typedef struct nt_lens nt_lens_t;
/* `coeffs`: width * height * 3 floats in host memory, copied.  NULL (NT_E_INVALID) for a size < 1 or NULL coeffs. */
nt_lens_t *nt_lens_create(int width, int height, const float *coeffs);
/* the pinhole of a width x height view with the given fov, filled with the very expressions the pinhole ray source uses */
nt_lens_t *nt_lens_create_pinhole(int width, int height, float fov);
void nt_lens_destroy(nt_lens_t *lens);
int nt_lens_width(const nt_lens_t *lens);
int nt_lens_height(const nt_lens_t *lens);
/* copies the table (width * height * 3 floats) to `out` */
int nt_lens_coeffs(const nt_lens_t *lens, float *out);
/* NULL takes the lens off.  The scene shares ownership of the table: the handle may be destroyed while the scene uses it.
   NT_E_LOCKED while a render holds the scene, as nt_scene_set_camera. */
int nt_scene_set_lens(nt_scene_t *s, const nt_lens_t *lens);
/* a new handle on the scene's lens (to be destroyed by the caller), or NULL when none is set */
nt_lens_t *nt_scene_get_lens(const nt_scene_t *s);

/* ---- the parallel (orthographic) projection ----------------------------------------------------------------------
   With half_width > 0 set on a scene, the scene's camera unchanged, pixel (x, y) of a width x height render casts the ray
       k  = half_width / half_w
       sx = k * ((float)x - half_w)
       sy = k * ((float)y - half_h)
       o'[j] = (origin[j] + right[j] * sx) - up[j] * sy
       v = forward,      d = v / |v|
   with half_w = float(width) / 2 and half_h = float(height) / 2, d formed as the pinhole's is (|v|^2 summed left to right,
   sqrtf, one IEEE division a component, no contraction) and k computed once on the host in fp32, as the pinhole's fovI is.
   The image spans 2 * half_width scene units horizontally, with square pixels: half_width plays the part tan(fov / 2) plays
   for the pinhole, and the scene's fov is ignored while the projection is set.  Everything behind the ray source is a
   render's own: the scene-box test, the walk, shading, packing, strict_reference and the NTRACER_* render switches.
   Honoured by nt_render, nt_render_device, nt_render_frames_device and nt_render_table_device, which return
   NT_E_UNSUPPORTED -- before any device is touched, drawing nothing -- for what the projection does not do yet: a
   supersampling factor above 1, row bands (band_world > 1), collect_stats.  While it is set nt_colors_at /
   nt_calculate_color and nt_primary_hits* are refused with NT_E_UNSUPPORTED as well (never answered with the pinhole).
   nt_ray_colors*, nt_render_rays* and the ray queries take their rays from the caller and ignore the setting.
   Opaque CompositeScenes up to 10 dimensions are rendered by a packet walk for rays that share their direction (two
   passes: the walk leaves 16-byte hit records, a shading pass picks them up); every other scene by the ray-colour kernels
   from origins expanded on the device, in bands of whole rows of at most 1 GiB.
   half_width 0 takes the projection off; negative, NaN or infinite: NT_E_INVALID.  NT_E_LOCKED while a render holds the
   scene, as nt_scene_set_camera.  A lens and the parallel projection exclude each other: setting either while the other
   is set is NT_E_INVALID and changes nothing. */
int nt_scene_set_parallel(nt_scene_t *s, float half_width);
/* the half_width set, 0 when the projection is off */
float nt_scene_get_parallel(const nt_scene_t *s);

/* statistics of the last render on this scene that had collect_stats set */
int nt_scene_last_stats(const nt_scene_t *s, nt_stats *out);

/* ---- scene construction (host only, no device needed) --------------------------------------------------
   build_kdtree / build_composite_scene of the reference (src/tracer.hpp:1965-2455; Python entry points
   src/ntracer_body.hpp:3250-3357).  Items are primitives or batches: a bounding box each, plus -- for
   simplices -- their vertices, simplex_first[i] .. simplex_first[i+1] indexing simplex_verts [count][n][n]
   (an item without simplices, e.g. a Solid, is placed by its box).  The tree comes back in the flat layout of
   nt_scene_desc (leaf: axis -1, left = first entry of leaf_items, right = count); leaf_items holds ITEM
   indices.  Arrays are malloc'ed; release with nt_kdtree_free. */
typedef struct {
    int32_t root;
    int32_t n_nodes;
    int32_t n_leaf_items;
    int32_t *node_axis;
    float *node_split;
    int32_t *node_left;
    int32_t *node_right;
    int32_t *leaf_items;
    float *aabb;                 /* start[n], end[n] */
} nt_kdtree;

/* kd_tree_params (tracer.hpp:1948-1961).  Zero / negative fields select the defaults: depth 25, threshold 2,
   costs 1 : 1 (the reference's per-dimension constants, :1933-1946, were tuned for its CPU walk; on the GPU a
   branch step is cheap next to a 4-simplex batch test). */
typedef struct {
    int32_t max_depth;           /* <= 64 */
    int32_t split_threshold;
    float traversal_cost;
    float intersection_cost;
} nt_kdtree_params;

int nt_kdtree_build(int dimension, int n_items, const float *item_lo, const float *item_hi, const int32_t *simplex_first,
                    const float *simplex_verts, const nt_kdtree_params *params, nt_kdtree *out);
void nt_kdtree_free(nt_kdtree *t);

/* aabb::intersects(prototype) of the reference (src/tracer.hpp:1465-1700), done by exact clipping: a convex polytope
   -- `n_verts` vertices [n_verts][dimension], each with the set of its facets' ids as a 192-bit mask `tight`
   [n_verts][3]; two vertices span an edge when they share `shared_for_edge` facets -- is cut by the 2*dimension
   half-spaces of the box [lo, hi] (which get the facet ids first_free_bit ...).  Returns the number of vertices of
   what is left (0: disjoint; out_lo / out_hi then untouched, else its bounding box), or a negative status.
   dimension <= 16.  A simplex: vertex i is on every facet but i, shared_for_edge = dimension-2; a parallelotope
   (solid cube): vertex on one facet of each of the dimension pairs, shared_for_edge = dimension-1. */
int nt_polytope_clip_box(int dimension, int n_verts, const float *verts, const uint64_t *tight, int shared_for_edge, int first_free_bit,
                         const float *lo, const float *hi, float *out_lo, float *out_hi);

/* ---- BoxScene hit buffers and face lines ---------------------------------------------------------------------------
   Which face of the cube [-1, 1]^n a pixel sees, and how far away it is: hypercube_intersects (src/tracer.hpp:115-152) taken
   one step further than the colour needs it.  For pixel (x, y) of a width x height view with the scene's camera and fov let o
   be the camera's origin and d the primary ray's unit direction exactly as the BoxScene renders form it (integer pixel
   coordinates): sx = fovI * (x - half_w), sy = fovI * (y - half_h), v = (forward + right * sx) - up * sy, |v|^2 summed left to
   right, sqrtf, one IEEE division a component.  Then, in fp32 without contraction:
     for i = 0 .. n - 1 in ascending order, skipping d_i == 0:
       s = d_i < 0 ? 1.0f : -1.0f;  dist = (s - o_i) / d_i;
       if dist > 0 and for every j != i:  !(fabsf((d_j * dist) + o_j) > 1.0f + ROUNDING_FUZZ), ROUNDING_FUZZ = FLT_EPSILON * 10:
         dist >= FLT_MAX: no hit (tracer.hpp:142 with the default cutoff); else: the hit is face (i, s) at dist.  Stop.
     no face passes: no hit.
   The record is nt_ray_hit: dist, the Euclidean depth (d is a unit vector); item = i, the axis the face is perpendicular to;
   lane = 1 for the face at +1 and 0 for the face at -1; n_transparent = 0.  A pixel without a hit gets FLT_MAX, -1, -1, 0.
   Every pixel's record is written.  The outward normal is s * e_i and is not stored.  An origin inside the cube sees nothing,
   as in the reference.  One ray a pixel: the supersampling factor is ignored, as by nt_colors_at, and so is the face-line
   setting below.  BoxScene only: a CompositeScene handle is NT_E_INVALID ("not a box scene"); nt_primary_hits* is its
   counterpart there.  NT_E_UNSUPPORTED while a lens or the parallel projection is set.  Up to 24 dimensions the kernel is
   compiled for the dimension; above, and at every dimension under NTRACER_FORCE_VAR=1, the run-time-n kernel answers. */

/* Host memory out ([height][width] records), the scene's current camera, one frame; returns when the records are in place.
   Holds the scene like nt_colors_at.  NT_E_INVALID, before any device is touched: NULL scene / hits, width or height < 1, a
   CompositeScene, width * height beyond 2^31 - 1 records. */
int nt_box_hits(nt_scene_t *s, int width, int height, nt_ray_hit *hits, int device);
/* `hits_dev` is DEVICE memory on opts->device; the launch is only enqueued on `hip_stream`, with the stream and lifetime rules
   of nt_render_device.  Of `opts` (may be NULL) device and abort_device are read -- blocks that start after the abort word is
   raised leave without writing -- and every other field must be 0, else NT_E_INVALID. */
int nt_box_hits_device(nt_scene_t *s, int width, int height, void *hits_dev, const nt_render_opts *opts, void *hip_stream);
/* ... frames [first, first + count) of a camera table in one launch: a pixel's record index is
   frame * frame_stride_records + y * width + x, and the records between the frames are not touched.  NT_E_INVALID also for a
   table of another dimension or device, a bad first / count, a stride smaller than a frame, and count * frame_stride_records
   beyond 2^31 - 1.  Nothing is allocated. */
int nt_box_hits_table_device(nt_scene_t *s, int width, int height, void *hits_dev, size_t frame_stride_records,
                             const nt_camera_table_t *table, int first, int count, const nt_render_opts *opts, void *hip_stream);

/* Face lines: a line along the cube's silhouette and along every edge where two of its faces meet, drawn inside the render.
   `kinds` = 0 takes the setting off; otherwise it is an OR of NT_OUTLINE_SILHOUETTE and NT_OUTLINE_CREASE (a convex body has no
   depth lines: NT_OUTLINE_DEPTH is refused), every colour component and `strength` finite and in [0, 1].  NT_E_INVALID for a
   CompositeScene (nt_scene_set_outlines is its counterpart) and for a value out of range -- the setting stays as it was;
   NT_E_LOCKED while a render holds the scene.  No device is needed.  The setting is not part of a pickled scene.

   With R(p) = (dist, item, lane) the record above, the mask byte of pixel p of a W x H view is 0 when item(p) < 0, and
   otherwise the OR, over those of the four neighbours q = (x +- 1, y), (x, y +- 1) that lie inside the image (and the frame:
   lines never cross a frame boundary), of
     NT_OUTLINE_SILHOUETTE  if item(q) < 0;
     nothing                if item(q) == item(p) and lane(q) == lane(p);
     nothing                if dist(p) > dist(q): the nearer pixel carries the line, so lines are one pixel wide (both carry it
                            on an exact tie);
     NT_OUTLINE_CREASE      otherwise,
   ANDed with `kinds`.  This is the outline rule with the crease test always true: two different faces of a cube are
   perpendicular or opposite.

   A render with the setting on: P = the plain single-sample colour with each component clamped to [0, 1]; a pixel with a
   non-zero mask becomes (P.c * (1.0f - strength)) + (color.c * strength), every other pixel is P, and either goes through the
   format's conversion and packing as always.  With strength = 0 the frame is the plain frame byte for byte, in every format.
   nt_render, nt_render_device, nt_render_frames_device and nt_render_table_device honour the setting, and refuse with
   NT_E_UNSUPPORTED ("face lines ...") before a device is touched, drawing nothing, for a supersampling factor above 1 (adaptive
   or not), row bands, collect_stats, a lens, the parallel projection (and a row range, which only a caller inside the library
   can ask for).  nt_colors_at / nt_calculate_color, nt_ray_colors*, nt_render_rays*, nt_adaptive_mask* and nt_box_hits* ignore
   it.  Up to 24 dimensions one kernel computes the records of a 64 x 32 tile and its one-pixel halo into LDS, marks and draws:
   no record crosses device memory and nothing is allocated.  Above (and under NTRACER_FORCE_VAR=1) the records of whole frames
   go through a scratch of 16 bytes a pixel and frame under the cap of nt_scene_set_supersampling_scratch_mb, larger jobs in
   chunks of whole frames; a single frame that does not fit is NT_E_UNSUPPORTED before anything is launched. */
int nt_scene_set_box_lines(nt_scene_t *s, int kinds, const float color[3], float strength);
/* any out pointer may be NULL */
int nt_scene_get_box_lines(const nt_scene_t *s, int *kinds, float color[3], float *strength);
/* The mask bytes alone, [height][width], one sample a pixel of the scene's current camera.  Host memory out, `marked` (may be
   NULL) the number of non-zero bytes; of `opts` (may be NULL) device is read.  NT_E_INVALID when the setting is off, as
   nt_outline_mask; NT_E_UNSUPPORTED under a lens or the parallel projection. */
int nt_box_line_mask(nt_scene_t *s, int width, int height, uint8_t *mask, long long *marked, const nt_render_opts *opts);
/* `mask_dev` is DEVICE memory on opts->device; only enqueued on `hip_stream`.  Of `opts` device and abort_device are read and
   every other field must be 0. */
int nt_box_line_mask_device(nt_scene_t *s, int width, int height, void *mask_dev, const nt_render_opts *opts, void *hip_stream);

/* ---- BoxScene face shading ---------------------------------------------------------------------------------------------
   A colour of its own for each of the 2n faces of the cube, and the depth cues of CompositeScene -- distance fog and a
   coordinate tint ("colour by w") -- from the face record of the render itself.  BoxScene only.  Everything below is fp32
   without contraction, sums left to right, clamp01(v) = max(0, min(1, v)).  The host forms two reciprocals once, in fp32:
   inv_fog = 1.0f / (fog_far - fog_near) and, with a tint, inv_tint = 1.0f / (tint_hi - tint_lo).
   For pixel p of a W x H view let R(p) = (dist, i, l) be the record that nt_box_hits defines (item = i, lane = l), d the unit
   direction formed there, o the camera's origin and T the face-colour table [n][2][3], T[i][l] the colour of the face at +1
   (l = 1) or -1 (l = 0) of axis i; without a table of the caller's own every entry is (1.0f, 0.5f, 0.5f).
     hit (i >= 0):  shade = fabsf(d_i) and B.c = shade * T[i][l][c];
     no hit:        B = the plain background colour of d_0: d_0 > 0 ? (d_0, d_0, d_0) : (0, -d_0, -d_0);
     P.c = clamp01(B.c), a zero as +0 (the background's -d_0 is -0 where d_0 is +0; the plain frame stores +0 there too);
     the factors (f, g), the depth cues' rule with "item >= 0" read as "hit", n_transparent = 0 and t = dist:
       hit:     f = clamp01((t - fog_near) * inv_fog); with a tint x_k = (d_k * t) + o_k, s = tint_axis_0 * x_0, then
                s = s + (tint_axis_k * x_k) for k = 1 .. n - 1, and g = clamp01((s - tint_lo) * inv_tint); without a tint g = -1;
       no hit:  with fog_background set f = 1, g = -1; otherwise f = -1, g = -1;
       without a cue f = g = -1 everywhere;
     Q = P;  if g >= 0:  Q.c = P.c * ((tint_color_lo.c * (1.0f - g)) + (tint_color_hi.c * g));
             if f >= 0:  w = f * fog_strength and Q.c = (Q.c * (1.0f - w)) + (fog_color.c * w);
     with face lines on as well (nt_scene_set_box_lines): the mask byte is exactly the face-line rule's, and a pixel with a
     non-zero mask becomes (Q.c * (1.0f - strength)) + (color.c * strength) with the lines' own colour and strength;
   and the result goes through the format's conversion and packing as always.  With no table, no tint and fog_strength = 0
   the frame is the plain frame byte for byte, in every format -- with lines on, the face-line frame -- and likewise with only
   a table equal to the default.
   nt_render, nt_render_device, nt_render_frames_device and nt_render_table_device honour the setting, and refuse with
   NT_E_UNSUPPORTED ("face shading is not available ...") before a device is touched, drawing nothing, for a supersampling
   factor above 1 (adaptive or not), row bands, collect_stats, a lens, the parallel projection (and a row range, which only a
   caller inside the library can ask for); with face lines on as well, that setting's words answer.  nt_colors_at /
   nt_calculate_color, nt_ray_colors*, nt_render_rays*, nt_adaptive_mask*, nt_box_hits* and nt_box_line_mask* ignore it.  There
   is no buffer entry point of its own: the render in the plain fp32 format is the buffer.
   Up to 24 dimensions one kernel forms the records and draws from them -- in registers, or with face lines in LDS as the
   face-line kernel does: no record crosses device memory and nothing is allocated.  Above (and under NTRACER_FORCE_VAR=1) the
   records of whole frames go through a scratch of 16 bytes a pixel and frame under the cap of
   nt_scene_set_supersampling_scratch_mb, larger jobs in chunks of whole frames; a single frame that does not fit is
   NT_E_UNSUPPORTED before anything is launched.

   face_colors: [dimension][2][3] floats, finite and in [0, 1], or NULL for the default table.  cue and tint_axis are validated
   exactly as nt_scene_set_depth_cue validates them (tint_axis == NULL means no tint; a tint_axis without a cue, which holds the
   tint's range and colours, is NT_E_INVALID).  face_colors == NULL && cue == NULL takes the setting off.  NT_E_INVALID for a
   CompositeScene ("not a box scene": nt_scene_set_depth_cue is its counterpart) and for a bad value -- the setting stays as it
   was; NT_E_LOCKED while a render holds the scene.  No device is needed to set or get it.  The setting is not part of a
   pickled scene. */
int nt_scene_set_box_shading(nt_scene_t *s, const float *face_colors /* [n][2][3] or NULL */,
                             const nt_depth_cue *cue /* or NULL */, const float *tint_axis /* or NULL */);
/* any out pointer may be NULL: *enabled, *has_colors, *has_cue, *has_tint 0 or 1; face_colors [dimension][2][3] floats (the
   default table without one of the caller's); *cue zeroes without a cue, its tint fields zero without a tint; tint_axis
   `dimension` floats (zeroes without a tint) */
int nt_scene_get_box_shading(const nt_scene_t *s, int *enabled, int *has_colors, float *face_colors,
                             int *has_cue, nt_depth_cue *cue, int *has_tint, float *tint_axis);

/* ---- view stacks: depth of field, slabs and anaglyphs summed on the device -------------------------------------------------
   One picture from K cameras that differ from the scene's camera by a small offset: the K plain pictures are added with weights.
   A view setting of BoxScene and CompositeScene alike, off by default.  K = count, 1 <= K <= NT_STACK_MAX; sample k has an offset
   e_k of `dimension` floats in the camera's own frame and a weight w_k of three floats; `focus` > 0, or 0 for none.  Everything
   below is fp32, every product and sum rounded on its own (no fma).
   For a camera (o, rows a_0 right, a_1 up, a_2 forward, a_3 ...) sample k is an ordinary camera:
     s_k = e_k[0] * a_0, then for j = 1 .. n - 1: s_k = s_k + (e_k[j] * a_j), component by component;
     o_k = o + s_k;
     f_k = a_2 - (s_k * r), r = 1.0f / focus, one IEEE division done once by the setter; r = 0.0f without a focus;
     every other row of the axes unchanged.
   With a focus all K rays of pixel (x, y) pass through o + focus * (a_2 + c_x a_0 - c_y a_1): the sharp plane of a lens, the
   zero-parallax plane of a stereo pair.  Without one the samples are translations: along a hidden axis (row 3 and up) they are
   the neighbouring 3-D slices of n-space, a slab.  The sample cameras are sheared, not orthonormal; the renders take them as
   they are.
   c_k is the colour a plain render gives the pixel under camera k, each component clamped to [0, 1] as the fp32 packer clamps
   it (clamping before the sum is deliberate: a view stack adds pictures, as a caller adding fp32 frames would).  The pixel is
     acc = 0.0f;  for k = 0 .. K - 1:  acc.c = acc.c + (w_k[c] * c_k.c)
   and goes through the format's conversion and packing as always.  K = 1 with a zero offset and weight 1 is the plain frame byte
   for byte.
   nt_render, nt_render_device, nt_render_frames_device and nt_render_table_device honour the setting (for a frame of a `frames`
   array or a camera table the rule starts from that frame's camera) and refuse with NT_E_UNSUPPORTED ("a view stack is not
   available ...") before a device is touched, drawing nothing: a supersampling factor above 1 (adaptive or not), row bands,
   collect_stats, a lens, the parallel projection, clip planes, depth cues, outlines, ambient occlusion, BoxScene's face lines and
   face shading (and a row range, which only a caller inside the library can ask for).  nt_colors_at / nt_calculate_color,
   nt_primary_hits*, nt_box_hits*, nt_ray_colors*, nt_render_rays*, the ray queries and the other settings' masks ignore it.
   All of it runs on the device.  BoxScene up to 24 dimensions: one kernel keeps the K samples of a pixel in registers; no sample
   crosses device memory and no scratch is needed (nt_scene_set_view_stack_route sends it the other way).  Every
   other scene: the plain render of the sample cameras into fp32 x 3 scratch, 12 K bytes a pixel a frame under the cap of
   nt_scene_set_supersampling_scratch_mb, and a resolve pass; larger jobs are cut into chunks of whole frames, and when the K
   samples of one frame do not fit, into chunks of consecutive k whose sums pass through an fp32 accumulator frame -- the sum
   stays in the order of k and not one bit changes.  When not even the accumulator and one sample fit (24 bytes a pixel) the
   render fails with NT_E_UNSUPPORTED ("a view stack ...") before anything is launched.  Not part of a pickled scene. */
#define NT_STACK_MAX 64
/* offsets: [count][dimension]; weights: [count][3], or NULL for 1.0f / (float)count each; count == 0 takes the setting off.
   NT_E_INVALID for a count outside 0..NT_STACK_MAX, NULL offsets with count > 0, an offset, weight or focus that is not
   finite, a negative focus (both also with count == 0) and one whose reciprocal is not finite (the setting stays as it was); NT_E_LOCKED while a render
   holds the scene.  No device is needed to set or get it. */
int nt_scene_set_view_stack(nt_scene_t *s, int count, const float *offsets, float focus, const float *weights);
/* any out pointer may be NULL: *count (0 when off), `count` rows of offsets, *focus (0: none), `count` rows of weights (room
   for NT_STACK_MAX rows suffices) */
int nt_scene_get_view_stack(const nt_scene_t *s, int *count, float *offsets, float *focus, float *weights);
/* The K cameras the rule gives for one camera: origins_out [K][dimension], axes_out [K][dimension][dimension].  origin / axes
   NULL: the scene's own.  Runs on the host, needs no device, and is bit for bit what the renders use.  NT_E_INVALID when the
   setting is off. */
int nt_view_stack_cameras(const nt_scene_t *s, const float *origin, const float *axes, float *origins_out, float *axes_out);
/* A TESTING AND MEASURING HOOK, not a feature: applications have no reason to call it.  Which of the two routes a BoxScene of up
   to 24 dimensions takes with a stack on: NT_STACK_ROUTE_AUTO (the default), the fused kernel; NT_STACK_ROUTE_FRAMES, the scratch
   and the resolve pass of every other scene.  Same bytes either way: the hook lets the suite and tools/view_stack_time.py hold
   the routes against each other (a setting of the scene, because the environment switches are a closed list).
   Every other scene takes the frames route whatever is set.  NT_E_INVALID for another value, NT_E_LOCKED while a render holds
   the scene.  Not part of a pickled scene. */
#define NT_STACK_ROUTE_AUTO 0
#define NT_STACK_ROUTE_FRAMES 1
int nt_scene_set_view_stack_route(nt_scene_t *s, int route);
int nt_scene_get_view_stack_route(const nt_scene_t *s);

/* ---- X-ray views: every surface a primary ray crosses, counted on the device ------------------------------------------------
   A picture of the inside: every primitive the ray of a pixel crosses multiplies the background behind it by a per-material
   transmittance.  A product commutes, so there is no hit list, no cap, no order and no nearest-hit cutoff.  A view setting of
   CompositeScene, off by default.  Everything below is fp32, every product and sum rounded on its own (no fma).
   For pixel (x, y) of a W x H view take (o, d), the pinhole's primary ray exactly as a render forms it, and dist0 =
   aabb_distance(o, d) as a render forms it.  The crossing set S is empty when dist0 < 0; otherwise it is every primitive of the
   scene -- whatever the k-d tree says, which only culls -- whose own test accepts the ray without a cutoff and with t != 0,
   each primitive once:
     a lane of a batch (the batch rule): denom = N[0] * d[0], then + N[k] * d[k] for k = 1 .. n - 1; no likewise from o;
       t = -(no + dd) / denom, accepted when denom != 0 && t >= 0; pside = p1 - (o + t * d) component by component; every edge
       coordinate area_e = E_e[0] * pside[0], then + E_e[k] * pside[k], is >= -NT_FUZZ, and tot = 0.0f + area_0 + area_1 + ...
       is <= 1 + NT_FUZZ.  Every lane of a batch that passes counts (the reference's "nearest lane of a batch alone" is a
       nearest-hit matter).  A lane whose record is bytewise equal to an earlier lane of the same batch is padding (the builder
       fills the last batch by repeating its last simplex) and never counts: the library forms a 4-bit live mask a batch when
       the scene is made (nt_scene_batch_live_masks);
     an unbatched triangle (the scalar rule, with the cutoff FLT_MAX): denom != 0, 0 < t < FLT_MAX, every edge coordinate in
       [-NT_FUZZ, 1 + NT_FUZZ] and their sum <= 1 + NT_FUZZ;
     a Solid: the Solid's own intersection test with the cutoff FLT_MAX; it counts 1 or 0, and from inside it is not there, as in
       a render.
   Opacity, lights, shadows and reflections play no part.  From S:
     count(x, y) = |S|, int32;
     colour(x, y) = B(o, d) * prod over p in S of T[material(p)], per channel: f = 1.0f; f = f * T[m][c] for every crossing, in
       no specified order; then B * f, and the format's conversion and packing as always.  B is the colour a render gives a ray
       that hits nothing (the background gradient).
     T[m][c] = clamp01(1.0f - absorbance * (1.0f - tint * color_m[c])), computed once a material by the setter, in that order.
   tint = 0 is the grey X-ray (1 - absorbance)^count; tint = 1 is stained glass.
   With the setting on nt_render, nt_render_device, nt_render_frames_device and nt_render_table_device draw this colour instead
   of the shaded one, and refuse with NT_E_UNSUPPORTED ("X-ray is not available ...") before a device is touched, drawing
   nothing: a supersampling factor above 1 (adaptive or not), row bands, collect_stats, a lens, the parallel projection, a view
   stack, clip planes (a cut-away X-ray is not drawn without the cut), depth cues, outlines and ambient occlusion.
   nt_colors_at / nt_calculate_color, nt_ray_colors*, nt_render_rays*, nt_adaptive_mask*, nt_ambient_occlusion*,
   nt_outline_mask* and nt_depth_cue_factors* are refused while it is on; nt_primary_hits* and the ray queries ignore it.
   All of it runs on the device.  Up to 10 dimensions, a tree of depth <= 32 and NT_XRAY_PACKET_ITEMS batches + triangles +
   Solids: one wave-uniform packet walk a tile with an exact "seen" bit an item in LDS.  Every other scene, and
   NTRACER_FORCE_VAR=1: a per-lane walk with an exact bit a lane and item in scratch (shared with the scene's renders on that
   device).  Not part of a pickled scene. */
#define NT_XRAY_PACKET_ITEMS 65536
/* CompositeScene only.  NT_E_INVALID for a BoxScene, and with `enabled` for an absorbance or tint that is not finite or outside
   [0, 1] (the setting stays as it was); NT_E_LOCKED while a render holds the scene.  No device is needed to set or get it. */
int nt_scene_set_xray(nt_scene_t *s, int enabled, float absorbance, float tint);
/* any out pointer may be NULL; `table`: the [n_materials][3] transmittances T as the kernels read them (untouched when off) */
int nt_scene_get_xray(const nt_scene_t *s, int *enabled, float *absorbance, float *tint, float *table);
/* The live masks of the rule: `masks` (may be NULL) receives one byte a batch, bit l set when lane l counts.  Returns the number
   of batches, or NT_E_INVALID for a BoxScene.  No device is needed. */
int nt_scene_batch_live_masks(const nt_scene_t *s, uint8_t *masks);
/* The counts alone of one width x height view of the scene's camera, [height][width] int32, whether or not the setting is on (a
   count has no parameters).  Host form: holds the scene like nt_colors_at; of `opts` (may be NULL) device is read and
   strict_reference accepted and ignored (there is no pruning to switch).  Device form: `counts_dev` is device memory and the
   call is only enqueued on hip_stream; it also reads abort_device, and every other field of `opts` must be 0.  NT_E_INVALID,
   before any device is touched and leaving the buffer alone: NULL arguments, width or height < 1, a BoxScene, more than
   2^31 - 1 pixels; NT_E_UNSUPPORTED while clip planes, a lens or the parallel projection are set. */
int nt_crossing_counts(nt_scene_t *s, int width, int height, int32_t *counts, const nt_render_opts *opts);
int nt_crossing_counts_device(nt_scene_t *s, int width, int height, void *counts_dev, const nt_render_opts *opts, void *hip_stream);

/* ---- hit layers: the K nearest surfaces of every pixel, in order -------------------------------------------------------------
   What lies under a pixel behind the first surface: the crossings of the pixel's primary ray, nearest first, with their
   identity.  CompositeScene only.  Everything below is fp32, every product and sum rounded on its own (no fma).
   For pixel (x, y) of a W x H view take (o, d), dist0 and the crossing set S exactly as the X-ray rule above defines them: the
   batch rule with the live mask, the scalar rule for unbatched triangles with the cutoff FLT_MAX, a Solid's own test with the
   cutoff FLT_MAX, S empty for dist0 < 0, and t != 0.  Each member of S carries
     t:    the rule's own quotient -(no + dd) / denom for a simplex (one IEEE division); for a Solid its entering distance: a
           cube's as the Solid's own fp32 test gives it; a sphere's, once that test has accepted it, evaluated again in float64
           on the fp32 ray and record -- local ray lo = O^-1 o - p, ld = O^-1 d, a = ld.ld, b = 2 ld.lo, c = lo.lo - 1,
           t = (-b - sqrt(b b - 4 a c)) / (2 a), sums in ascending index, no fma -- and rounded to fp32 once (the fp32 quadratic
           cancels nearly all its digits from many radii away; without an entering root in float64 the fp32 distance stays);
     item: the leaf-item code (index << 2) | NT_KIND_* of nt_ray_hit;
     lane: 0..3 inside a batch, -1 otherwise.
   Order S by t ascending; ties by item ascending, then lane ascending (t > 0, so the bits of t order as t does: the key is
   (bits of t, item, lane)).  Layer l, l = 0 .. layers - 1, is the l-th member.  Its record is an nt_ray_hit
     {dist = t, item, lane, count}
   whose fourth word is count = |S|, the pixel's full crossing count -- nt_crossing_counts' number -- the same in every layer of
   the pixel: count > layers says the list was cut.  A layer beyond |S| is {FLT_MAX, -1, -1, count}.  Every record of every
   pixel is written.  Opacity, lights, shadows, reflections and the X-ray setting play no part; one ray a pixel.
   `records` is planar, [layers][height][width]: the record of layer l of pixel (x, y) is at index (l * height + y) * width + x,
   so a layer is a contiguous image.
   Host form: holds the scene like nt_colors_at; of `opts` (may be NULL) device is read and strict_reference accepted and ignored
   (there is no pruning to switch).  Device form: `records_dev` is device memory and the call is only enqueued on hip_stream; it
   also reads abort_device, and every other field of `opts` must be 0.  Both are answered whether or not X-ray is on.  After a
   warm-up call of the same shape nothing is allocated.  Before any device is touched and leaving the buffer alone:
   NT_E_INVALID for NULL arguments, width or height < 1, `layers` outside 1..NT_LAYERS_MAX, a BoxScene, more than 2^31 - 1
   records, and NT_E_UNSUPPORTED while clip planes, a lens or the parallel projection are set, and for a scene with more than
   2^26 batches, triangles or Solids (the key keeps an item and its lane in 32 bits).
   The routes are the X-ray's: up to 10 dimensions, a tree of depth <= 32 and NT_XRAY_PACKET_ITEMS items take the wave-uniform
   packet walk, each lane keeping its 2, 4 or 8 nearest in registers; every other scene, and NTRACER_FORCE_VAR=1, the per-lane
   walk.  Same bytes either way. */
#define NT_LAYERS_MAX 8
#define NT_LAYER_COUNT(rec) ((rec).n_transparent)      /* count = |S| of a hit-layer record */
int nt_hit_layers(nt_scene_t *s, int width, int height, int layers, nt_ray_hit *records, const nt_render_opts *opts);
int nt_hit_layers_device(nt_scene_t *s, int width, int height, int layers, void *records_dev, const nt_render_opts *opts, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* NTRACER_HIP_H */
