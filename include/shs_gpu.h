/*
 * shs_gpu.h -- C ABI of libshs_gpu.so, the MI355X (gfx950) replacement for the shs_renderer
 * triangle scan-conversion hot path.
 *
 * The reference has no C ABI/FFI; it has three C++ seams, and every entry point
 * below names the seam it replaces.  Paths are relative to /root/reference/cpp-folders/src/.
 *
 *   Seam 1 (legacy draw-call seam): RendererSystem::process(dt) -> draw_triangle_tile(Canvas&,
 *     ZBuffer&, verts, norms, std::function VS, std::function FS, tile_min, tile_max)
 *     hello-3d-primitives/hello_pipeline_blinn_phong_shading.cpp:189-313 (and the Phong :204,
 *     Gouraud :186-236, Flat :194-247 copies).  Replaced by shs_render_legacy(): the std::function
 *     shaders become the shading-model enum + POD uniform block of shs_legacy_draw, the per-tile job
 *     loop becomes one enqueue on the context's HIP stream.
 *   Seam 2 (library rasterize_mesh) and Seam 3 (the PassShadowMap / PassPBRForward IRenderPass
 *     bodies, Forward+ light culling): the "Library path" section below.
 *
 * Conventions: every function returns int status (0 = SHS_OK), never throws; a
 * context is used by one host thread at a time; host buffers are caller-owned and use the exact
 * reference layouts (RGBA8 canvas rows bottom-up, f32 depth in screen rows for the legacy path);
 * matrices are column-major float[16] exactly as glm::mat4 stores them.  No torch types cross.
 */
#ifndef SHS_GPU_H
#define SHS_GPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHS_OK 0
#define SHS_ERR_INVALID (-1)     /* bad argument (null pointer, bad size, unknown id)      */
#define SHS_ERR_HIP (-2)         /* HIP runtime error (message via shs_last_error)         */
#define SHS_ERR_NO_DEVICE (-3)   /* no gfx950 device / device index out of range           */
#define SHS_ERR_OVERFLOW (-4)    /* internal bin capacity exceeded; frame re-issued        */

/* Shading models of the legacy pipelines (the FS/VS pairs each hello_pipeline_* demo binds). */
#define SHS_SHADING_FLAT 0         /* hello_pipeline_flat_shading.cpp:46-98         */
#define SHS_SHADING_GOURAUD 1      /* hello_pipeline_gouraud_shading.cpp:46-89       */
#define SHS_SHADING_PHONG 2        /* hello_pipeline_phong_shading.cpp:47-108        */
#define SHS_SHADING_BLINN_PHONG 3  /* hello_pipeline_blinn_phong_shading.cpp:48-97   */
/* The other fragment shaders the reference binds to the same draw_triangle_tile.  Their vertex shader
 * and Uniforms are the Blinn-Phong pipeline's (model, world light_dir, camera_pos, color). */
#define SHS_SHADING_TOON 4         /* hello_pipeline_toon_shading.cpp:56-90          */
#define SHS_SHADING_GOOCH 5        /* hello_pipeline_gooch_shading.cpp:56-95         */
#define SHS_SHADING_OREN_NAYAR 6   /* hello_pipeline_oren_nayar_shading.cpp:57-99    */
#define SHS_SHADING_NORMAL_VIS 7   /* hello_pipeline_normal_zbuffer_debug.cpp:57-69  */
#define SHS_SHADING_DEPTH_VIS 8    /* hello_pipeline_normal_zbuffer_debug.cpp:105-120 (reads the clip z) */
/* The texture-mapping pipeline: the Blinn-Phong shader with baseColor from sample_nearest, and its own
 * draw_triangle_tile -- perspective-correct depth, world position and UV from the corners' 1 / w, pixels
 * with invw_sum <= 0 skipped.  Reads the mesh's UVs (shs_mesh_upload_soup_uv) and the draw's texture
 * (shs_render_legacy_batch_tex, the one render call that takes it). */
#define SHS_SHADING_TEXTURED 9     /* hello_pipeline_texture_mapping.cpp:66-116, 205-294 */

typedef struct shs_ctx shs_ctx;

/* One legacy draw = one object of the scene loop (blinn_phong_shading.cpp:272-305): the
 * reference's `Uniforms` POD (:36-42) plus the mesh handle and shading model.
 *   model      : Uniforms::model; for SHS_SHADING_FLAT this is Uniforms::mv (flat_shading.cpp:35)
 *   light_dir  : Uniforms::light_dir (world); for SHS_SHADING_FLAT: Uniforms::light_dir_view      */
typedef struct shs_legacy_draw {
    int32_t mesh_id;
    int32_t shading;
    float mvp[16];
    float model[16];
    float light_dir[3];
    float camera_pos[3];
    uint8_t color[4];
} shs_legacy_draw;

/* Per-frame description.  ref_tile_w/h are the reference's tile-job size (TILE_SIZE_X/Y = 80,
 * blinn_phong_shading.cpp:29-30): the legacy raster clamps each triangle's bounding box to the
 * tile that runs it, and the GPU path reproduces that visited-pixel set exactly.
 * shard_rank/shard_count select the GPU tiles (shs_gpu_tile_size() px square, row-major) this
 * device owns (tile % count == rank);
 * (0,1) renders the whole frame. */
typedef struct shs_frame_desc {
    int32_t width, height;
    int32_t ref_tile_w, ref_tile_h;
    int32_t shard_rank, shard_count;
    uint32_t flags;               /* SHS_FRAME_* */
    uint8_t clear_color[4];       /* Canvas::fill_pixel colour, {0,0,0,255} in every demo      */
} shs_frame_desc;

#define SHS_FRAME_PREQUANT 1u     /* also keep the shader's pre-truncation floats (tests)     */
#define SHS_FRAME_PRESENT 2u      /* also write the SDL present staging (shs_resolve_present)  */

typedef struct shs_raster_stats {
    uint64_t tri_input;           /* triangles submitted (rasterizer.hpp:208 tri_input)        */
    uint64_t tri_setup;           /* triangles surviving setup culls (area<=0, |denom|<1e-5)   */
    uint64_t tri_ghost;           /* slivers whose tile-clamp pixels near the bbox are tested   */
    uint64_t bin_entries;         /* (tile, triangle) pairs binned                              */
    uint64_t covered_pixels;      /* final pixels with depth != clear (shaded Mpix/s numerator) */
    uint64_t tri_ghost_unbounded; /* ... with no error bound: every visited pixel tested        */
    uint64_t spilled;             /* bin entries beyond the per-tile capacity                    */
    uint64_t max_tile_bin;        /* fullest 32x32 tile's triangle count                         */
    uint64_t ghost_fragments;     /* passing tile-clamp pixels of unbounded slivers outside bbox */
} shs_raster_stats;

/* ---- context ---------------------------------------------------------------------------- */
int shs_create(int device, shs_ctx **out);
int shs_destroy(shs_ctx *ctx);
const char *shs_last_error(shs_ctx *ctx);
/* Run on a caller-provided hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL
 * restores the context's own stream. */
int shs_set_stream(shs_ctx *ctx, void *hip_stream);
void *shs_get_stream(shs_ctx *ctx);
int shs_synchronize(shs_ctx *ctx);

/* ---- geometry (replaces the ModelGeometry vectors the tile jobs read,
 *      shs_renderer.hpp:1296-1298; uploaded once, device resident) ------------------------ */
int shs_mesh_upload_soup(shs_ctx *ctx, const float *positions, const float *normals, int32_t n_tris,
                         int32_t *mesh_id);
/* ... with the third vertex stream, ModelGeometry::uvs: uvs[6 * n_tris], (u, v) per corner.  A mesh
 * uploaded without UVs (uvs NULL, or shs_mesh_upload_soup) and drawn with SHS_SHADING_TEXTURED reads
 * vec2(0) per corner, as ModelGeometry stores for a mesh without texture coordinates
 * (shs_renderer.hpp:1285-1290).  The other shading models ignore the UVs. */
int shs_mesh_upload_soup_uv(shs_ctx *ctx, const float *positions, const float *normals, const float *uvs, int32_t n_tris,
                            int32_t *mesh_id);
int shs_mesh_release(shs_ctx *ctx, int32_t mesh_id);
/* A handle in dst to src's uploaded mesh (legacy soup or library MeshData), on the same device, without
 * a copy: frames in flight on several contexts read one device copy of each mesh.  The buffers stay
 * src's: src must not release the mesh, nor be destroyed, while dst may still read it; releasing the
 * shared handle in dst (or destroying dst) frees nothing. */
int shs_mesh_share(shs_ctx *dst, shs_ctx *src, int32_t src_mesh_id, int32_t *mesh_id);

/* ---- the hot path (Seam 1) --------------------------------------------------------------- */
/* Clears the frame (Canvas::fill_pixel + ZBuffer::clear) and rasterises all draws in order,
 * asynchronously on the context stream.  Results stay in device memory until shs_resolve. */
int shs_render_legacy(shs_ctx *ctx, const shs_frame_desc *frame, const shs_legacy_draw *draws, int32_t n_draws);

/* Superseding: a render call while the previous batch is still in flight does not wait for it, but
 * it reads that batch's capacity-overflow word first (final once the batch's setup is, copied to
 * pinned memory beside its raster); an overflowed batch is finished -- re-issued with grown
 * capacities -- before the new one is enqueued, so work queued behind a batch on the stream never
 * sees an incomplete frame. */
/* A batch of n_frames frames (1 <= n_frames <= SHS_MAX_BATCH_FRAMES) of one frame description, e.g.
 * the next n_frames camera poses of a render-ahead host or the views of a multi-view capture: frame f
 * draws draws[f * n_draws .. f * n_draws + n_draws - 1], in that order, and every frame must submit
 * the same number of triangles.  Each frame has its own device framebuffers (frame f's colour at
 * byte f*W*H*4 of the colour plane shs_device_framebuffers returns, its depth at float f*W*H); the
 * frames are independent -- each equals the frame shs_render_legacy renders from its draws.  One
 * k_setup + one k_raster launch cover the whole batch.  shs_render_legacy(ctx, frame, draws, n) is
 * shs_render_legacy_batch(ctx, frame, draws, n, 1).  Statistics (shs_get_stats) are batch totals. */
#define SHS_MAX_BATCH_FRAMES 1024
int shs_render_legacy_batch(shs_ctx *ctx, const shs_frame_desc *frame, const shs_legacy_draw *draws, int32_t n_draws,
                            int32_t n_frames);

/* shs_render_legacy_batch with the textured draws' albedo textures: albedo_tex[n_frames * n_draws], parallel
 * to draws, shs_texture_upload ids -- texel (x, y) at byte 4 * (y * w + x), the layout Texture2D::texels
 * holds after the host's loader has run (its flip included).  Read only for draws of
 * SHS_SHADING_TEXTURED; id 0 takes the shader's else branch (Uniforms::color), an unknown id is
 * SHS_ERR_INVALID.  albedo_tex NULL: every id 0.  This is the entry point of SHS_SHADING_TEXTURED:
 * shs_render_legacy[_batch] take the models they have always taken, SHS_SHADING_FLAT .. SHS_SHADING_DEPTH_VIS,
 * and answer a textured draw, like any other model they do not know, with SHS_ERR_INVALID ("bad shading
 * model").  For every other batch the two calls are the same.  shs_texture_release of a texture a batch in
 * flight samples finishes the batch first. */
int shs_render_legacy_batch_tex(shs_ctx *ctx, const shs_frame_desc *frame, const shs_legacy_draw *draws, const int32_t *albedo_tex,
                                int32_t n_draws, int32_t n_frames);

/* sample_nearest alone (synchronous), through the function the rasters call: uv[2n] -> rgba[4n], the
 * texel's r, g, b with alpha 255 (the shader does not read alpha).  The textured model's counterpart of
 * shs_legacy_shade_samples, which rejects SHS_SHADING_TEXTURED (its inputs are not that pipeline's). */
int shs_legacy_sample_nearest(shs_ctx *ctx, int32_t tex_id, int32_t n, const float *uv, uint8_t *rgba);

/* The legacy fragment shaders alone, for n samples (synchronous): the kernel shades each sample with
 * the function the rasters shade a winning pixel with.  uniforms: light_dir, camera_pos, color and
 * shading are read (mesh_id and mvp are ignored); shading is any model but SHS_SHADING_FLAT and
 * SHS_SHADING_GOURAUD, whose varyings differ (SHS_ERR_INVALID).  normal_sum[3n]: the barycentric sum of
 * the corners' normals, before draw_triangle_tile normalises it; world_pos[3n]: the interpolated world
 * position; clip_z[n]: the interpolated clip-space z (read by SHS_SHADING_DEPTH_VIS alone).  rgba[4n]:
 * the colour bytes; prequant[4n]: the pre-truncation floats (r, g, b, 1) as SHS_FRAME_PREQUANT keeps
 * them.  Either output may be NULL. */
int shs_legacy_shade_samples(shs_ctx *ctx, const shs_legacy_draw *uniforms, int32_t n, const float *normal_sum,
                             const float *world_pos, const float *clip_z, uint8_t *rgba, float *prequant);

/* Copy the frame into caller-owned host buffers (blocking).  color: W*H*4 bytes, canvas rows
 * (Canvas::buffer() layout); depth: W*H floats, screen rows (ZBuffer::buffer() as the legacy
 * pipelines index it).  Either pointer may be NULL.  shs_resolve = frame 0 of the last batch. */
int shs_resolve(shs_ctx *ctx, uint8_t *color, float *depth);
int shs_resolve_frame(shs_ctx *ctx, int32_t frame_index, uint8_t *color, float *depth);
/* Present staging (SHS_FRAME_PRESENT), written by the same launch as the canvas: the RGBA32 surface
 * Canvas::copy_to_SDLSurface fills (shs_renderer.hpp:833-848) -- surface row h-1-y holds canvas row
 * y, SDL_MapRGBA into create_sdl_surface's little-endian RGBA32 masks (:850-856) is the Color bytes.
 * shs_resolve_present copies it into a caller surface (pixels + pitch in bytes >= W*4), replacing
 * the per-pixel copy loop; shs_present_device returns the device pointer (W*H words, rows top-down).
 * shs_present_device and shs_device_framebuffers first finish the batch (wait for it; a capacity
 * overflow re-issues it), so the pointer holds the final frame.  The pointer aliases the context's
 * buffers: it is valid until the next shs_render_legacy* call on this context (which rewrites them,
 * and reallocates them when the frame or batch grows); call again per batch. */
int shs_resolve_present(shs_ctx *ctx, int32_t frame_index, uint8_t *pixels, int32_t pitch);
int shs_present_device(shs_ctx *ctx, int32_t frame_index, void **present_dev);
/* Pre-truncation shader floats, W*H*4 (canvas rows), only when SHS_FRAME_PREQUANT was set:
 * shs_resolve_prequant_frame for frame frame_index of the batch, shs_resolve_prequant for frame 0. */
int shs_resolve_prequant(shs_ctx *ctx, float *prequant);
int shs_resolve_prequant_frame(shs_ctx *ctx, int32_t frame_index, float *prequant);
/* Device pointers of the current batch's colour / depth planes (zero-copy hand-off to torch / RCCL);
 * finished and valid as for shs_present_device.
 * The pointers are writable and the library cannot see what is done through them, so the next legacy
 * batch after shs_device_framebuffers or shs_present_device clears every idle tile again
 * (SHS_OPT_LEGACY_STALE_CLEAR below): a render loop that takes the pointers every batch gets full
 * clears every batch. */
int shs_device_framebuffers(shs_ctx *ctx, void **color_dev, void **depth_dev);
int shs_get_stats(shs_ctx *ctx, shs_raster_stats *stats);
/* The 32x8 raster tiles the last legacy batch's clear strips wrote the clear values into (a batch
 * total; finishes the batch first, as shs_get_stats).  Busy tiles, which the raster writes whole, are
 * not counted.  Under SHS_OPT_LEGACY_STALE_CLEAR it is every idle owned tile of every frame for a batch
 * that clears fully, and only the tiles an earlier batch left non-clear otherwise (0 for a batch that
 * repeats the previous one). */
int shs_legacy_cleared_tiles(shs_ctx *ctx, uint64_t *tiles);

/* Per-kernel device timing of the last frame, recorded with HIP events on the context stream
 * (k_setup, k_ghost, unused, k_raster) in milliseconds.  Enabled by shs_enable_timing(ctx, 1). */
int shs_enable_timing(shs_ctx *ctx, int enable);
int shs_last_kernel_ms(shs_ctx *ctx, float *ms4);
/* Sums of the same four kernel durations over every frame enqueued since shs_timing_reset
 * (events recorded on the context stream around each kernel, harvested lazily). */
int shs_timing_reset(shs_ctx *ctx);
int shs_timing_read(shs_ctx *ctx, double *sum_ms4, int64_t *n_frames);

/* ---- host helpers: GLM restatements the reference host code computes with glm -----------
 * (Camera3D::update shs_renderer.hpp:1224-1236; MonkeyObject::get_world_matrix
 *  blinn_phong_shading.cpp:122-128).  The drop-in host keeps its own glm code; these exist so
 *  non-C++ callers (tests, bench) can build identical uniforms. */
int shs_camera3d(const float position[3], float horizontal_angle, float vertical_angle, float fov_deg,
                 float z_near, float z_far, float view16[16], float proj16[16]);
int shs_model_trs(const float position[3], float rotation_deg_y, const float scale[3], float out16[16]);
int shs_mat4_mul(const float a16[16], const float b16[16], float out16[16]);
int shs_mat4_inverse(const float m16[16], float out16[16]);

/* Debug / test hook: copy the last frame's per-triangle raster records (64 B each, layout
 * shs_dev::TriHot in csrc/shs_device.hpp: the pixel-independent barycentric terms, screen z, a
 * draw | flags << 29 word and the packed bin box) into caller memory; returns the count via n_out.
 * Records of culled triangles are not written by the legacy setup (stale entries). */
int shs_debug_records(shs_ctx *ctx, void *out, int64_t capacity, int64_t *n_out);

/* Tuning knobs.  SHS_OPT_BIN_CAPACITY: initial per-tile bin capacity (entries past it spill to a
 * global list and stay exact; the context grows the capacity to the fullest tile it observes). */
#define SHS_OPT_BIN_CAPACITY 1
/* SHS_OPT_RASTER_MODE: 0 auto (small scenes scan every triangle's bin box per tile, large scenes
 * build per-tile bins), 1 force scan, 2 force bins.  Results are identical in every mode. */
#define SHS_OPT_RASTER_MODE 2
/* SHS_OPT_TIMELINE: 1 = record every workgroup's start / end time (s_memrealtime, 100 MHz) of the
 * frames that follow (profiling aid; read with shs_debug_timeline / shs_lib_debug_timeline), 2 = the
 * same, with the library's shadow-pass raster recorded instead of the camera pass's, 0 = off. */
#define SHS_OPT_TIMELINE 3
/* SHS_OPT_RASTER_LOOP: 1 = (candidate, pixel) pair tasks dealt over the waves (default), 0 = each
 * thread loops over the tile's candidates for its own pixel.  Results are identical in both. */
#define SHS_OPT_RASTER_LOOP 4
/* SHS_OPT_SPILL_CAPACITY / SHS_OPT_FRAG_CAPACITY (tests): reallocate the legacy workspaces' global
 * bin-spill list / ghost-fragment list to `value` entries.  A batch that needs more raises its
 * overflow flag and is re-issued with grown lists when it is finished (synchronise, resolve, present,
 * superseded); results are identical. */
#define SHS_OPT_SPILL_CAPACITY 5
#define SHS_OPT_FRAG_CAPACITY 6
/* SHS_OPT_LIB_PART: library camera passes split a busy 32x8 raster tile whose candidate list holds more
 * than `value` entries into ceil(n / value) parts (at most 16) rendered by several workgroups at once,
 * part j over list positions [j n / k, (j + 1) n / k) of the whole tile; the parts merge their keys
 * with 64-bit atomicMin and the last one writes the winners (results identical).  -1: 512 for
 * tile-sharded passes, off otherwise; 0 (default): off (measured slower). */
#define SHS_OPT_LIB_PART 7
/* SHS_OPT_SHARD_CULL: 1 = each setup workgroup of a tile-sharded camera pass first keeps the triangles
 * of its inputs that can reach the rank's tiles (positions only) and sets up only those; 0 (default) =
 * every rank sets up every triangle, dropping the ones off its tiles after the transform.  Results
 * identical. */
#define SHS_OPT_SHARD_CULL 8
/* SHS_OPT_SHARD_LAYOUT: which 32x32 bin tiles a tile-sharded library frame's rank owns.
 * SHS_SHARD_INTERLEAVED (default): tile % count == rank.  SHS_SHARD_REGIONS: one rectangle per rank,
 * from a recursive bisection of the bin grid at equal predicted cost, predicted from the context's
 * previous camera pass (the bin-tile bounds of its 256-triangle setup blocks; the first pass, or one
 * after a resize, splits by pixels).  Every rank derives the same rectangles from the same frames, with
 * no exchange; a rank then skips whole setup blocks whose bounds miss its rectangle.  Applies to
 * shs_light_cull, shs_render_pbr_forward, shs_tonemap and shs_tiles_* of sharded library frames (the
 * legacy path stays interleaved).  Images identical; a region-sharded pass's statistics count only the
 * setup blocks that reach the rank. */
#define SHS_OPT_SHARD_LAYOUT 9
#define SHS_SHARD_INTERLEAVED 0
#define SHS_SHARD_REGIONS 1
/* SHS_OPT_SHARD_ROOT_SHARE: rank 0's share of a region layout's predicted cost, in permille of the other
 * ranks' (default 1000).  Rank 0 also unpacks every peer's tiles of the gathered frame; a smaller share
 * leaves it room for that.  Every rank must use the same value. */
#define SHS_OPT_SHARD_ROOT_SHARE 10
/* SHS_OPT_SHADOW_FOOTPRINT: 1 = shs_render_shadow_map records the pass (light camera computed and
 * returned as before) and the next shs_render_pbr_forward enqueues it over only the 32x32 shadow-map
 * tiles that pass's pixels can read: for each draw with `shadow`, the light-space bounds of (its world
 * box) ∩ (the camera frustum slice of the pixels the rank shades -- its region, or the whole frame),
 * widened by the PCF reach (shadow_sample.hpp:65-104) -- so a region-sharded rank renders only its own
 * shadow footprint and no shadow map crosses between ranks.  Texels outside are not written that pass;
 * the frame's images are identical.  A later camera pass that samples the same map (another view or
 * region) and reads beyond the rendered tiles enqueues the shadow pass again over the union first;
 * releasing a caster mesh of a footprint-restricted map renders the map whole first.
 * shs_resolve_shadow_map of a recorded pass renders it whole.
 * 0 (default): every shadow pass renders the whole map when it is called. */
#define SHS_OPT_SHADOW_FOOTPRINT 11
/* SHS_OPT_LEGACY_PIPELINE: 1 = multi-draw scan-mode legacy batches (shs_render_legacy_batch with more
 * than 6 draws in all, scenes up to 4096 triangles) are pipelined: batch k's raster runs in the same
 * launch as batch k + 1's setup, or at the next call that needs the frames (shs_synchronize, every
 * resolve / present / tiles call, a non-pipelined render, shs_set_stream).  The frames are identical;
 * what changes is that a batch's frames are final only after such a call -- work the caller queues on
 * the context stream right after shs_render_legacy_batch does not see them.  0 (default): off. */
#define SHS_OPT_LEGACY_PIPELINE 12
/* SHS_OPT_LEGACY_STALE_CLEAR: 1 (default) = a legacy batch clears only the raster tiles that an earlier
 * batch of this context left non-clear and that it does not itself draw into.  The context keeps one
 * flag per (frame of the batch, 32x8 raster tile); frame f of every batch lands at the same addresses,
 * so outside the busy tiles the planes already hold the clear values of the previous batch.  A batch
 * clears every idle tile as before whenever the library cannot vouch for the planes: the first batch,
 * another width / height / frame count / clear colour / PRESENT or PREQUANT flag / shard than the
 * previous batch, reallocated planes, after shs_device_framebuffers, shs_present_device or a
 * shs_tiles_unpack* into SHS_TARGET_LEGACY / SHS_TARGET_PRESENT, after a failed render call, and always
 * under SHS_OPT_LEGACY_PIPELINE.  0 = every batch clears every idle tile.  Images are identical either
 * way. */
#define SHS_OPT_LEGACY_STALE_CLEAR 13
/* SHS_OPT_LEGACY_TILE_GROUPS: 1 (default) = a scan-mode legacy batch (scenes up to 4096 triangles) on
 * the pair-task raster deals its busy raster tiles to the persistent raster as 2x2 groups (64x16 px)
 * instead of one by one: the group's workgroup scans the frame's bin boxes and stages the candidates'
 * records once, then rasters each busy tile of the group.  Ignored (tile lists as before) for single
 * frames (fewer busy tiles than raster workgroups: latency, not throughput), for bin-mode batches, under SHS_OPT_LEGACY_PIPELINE for the batches it pipelines, and with SHS_OPT_RASTER_LOOP 0.
 * 0 = every busy tile is its own work item.  Images and statistics are identical either way. */
#define SHS_OPT_LEGACY_TILE_GROUPS 14
/* SHS_OPT_LEGACY_GROUP_SPANS: 1 (default) = a tile group's pair pass (SHS_OPT_LEGACY_TILE_GROUPS, wherever
 * that applies) tests only the pixels inside a conservative span of each row of a candidate's box clipped
 * to the group, instead of the whole clipped box.  0 = whole boxes.  Images and statistics are identical
 * either way. */
#define SHS_OPT_LEGACY_GROUP_SPANS 15
int shs_set_option(shs_ctx *ctx, int option, int64_t value);
/* The regions of the last region-sharded camera pass: rects[4 r .. 4 r + 3] = (bx0, by0, bx1, by1) of
 * rank r, bin tiles, inclusive (bx1 < bx0: rank r owns nothing). */
int shs_get_shard_regions(shs_ctx *ctx, int32_t shard_count, int32_t *rects);
/* Host-only (no device): the region balance itself, for tests -- blocks[4 i .. 4 i + 3] = k_lib_setup's
 * per-block record (bx0 | bx1 << 16, by0 | by1 << 16, triangles, 1 bounded / 2 estimate / 0 none). */
int shs_shard_balance_rects(const uint32_t *blocks, int32_t n_blocks, int32_t width, int32_t height, int32_t shard_count,
                            int32_t root_permille, int32_t *rects);

/* Debug / profiling hook: the last frame's workgroup timeline.  out[0..7] = {k_setup grid, k_raster
 * grid, setup blocks, ghost blocks, clear blocks, stride S, 0, 0} (k_setup's block roles in that
 * order), then S slots per k_setup workgroup followed by S per k_raster workgroup: start, end, and
 * phase marks of the workgroup's thread 0 (0 where a phase did not run). */
int shs_debug_timeline(shs_ctx *ctx, uint64_t *out, int64_t capacity, int64_t *n_out);
/* Debug / profiling hook: the last camera pass's (SHS_OPT_TIMELINE 2: shadow pass's) k_lib_raster workgroup timeline,
 * 24 uint64 per workgroup: start, end, summed ticks of gather / stage + pairs / resolve + shade over
 * its busy tiles, clear ticks, busy tiles, cleared tiles, staging passes, pairs, candidates, longest
 * busy tile, and (deep camera raster) the staging passes' selection + record + span ticks and segment
 * ticks, all busy tiles' ticks, the last busy tile's end (s_memrealtime, 100 MHz).  out = NULL: *n_out = the count only. */
int shs_lib_debug_timeline(shs_ctx *ctx, uint64_t *out, int64_t capacity, int64_t *n_out);
/* The same for the last camera pass's k_lib_setup: 6 uint64 per workgroup -- start, after its
 * triangles, after the deferred marks, end, large primitives, deferred union width x height. */
int shs_lib_debug_setup_timeline(shs_ctx *ctx, uint64_t *out, int64_t capacity, int64_t *n_out);

/* Library/ABI version for integration checks; edge of the square GPU screen tile (shard unit). */
int shs_abi_version(void);
int shs_gpu_tile_size(void);

/* =========================================================================================
 * Library path -- Seam 2 (rasterize_mesh, shs-renderer-lib/include/shs/sw_render/rasterizer.hpp
 * :181-442) and Seam 3 (PassShadowMap, passes/pass_shadow_map.hpp:44-206; PassPBRForward,
 * passes/pass_pbr_forward.hpp:49-214).  The std::function ShaderProgram becomes a program enum
 * + the POD uniform block below.  Paths relative to shs-renderer-lib/include/shs/.
 * ========================================================================================= */
#define SHS_PROGRAM_PBR_MR 0        /* make_pbr_mr_program          shader/builtin_shaders.hpp:154-214 */
#define SHS_PROGRAM_BLINN_PHONG 1   /* make_blinn_phong_program     :105-152                         */
#define SHS_PROGRAM_DEBUG_ALBEDO 2  /* make_debug_view_shader_program(DebugViewMode) :221-245        */
#define SHS_PROGRAM_DEBUG_NORMAL 3
#define SHS_PROGRAM_DEBUG_DEPTH 4

#define SHS_CULL_NONE 0             /* RasterizerCullMode (rasterizer.hpp:26-31) */
#define SHS_CULL_BACK 1
#define SHS_CULL_FRONT 2

/* MeshData (resources/mesh.hpp:23-43): n_verts vec3 positions; normals / uvs may be shorter than
 * positions (missing entries read as (0,1,0) / (0,0), rasterizer.hpp:196-202) or NULL; indices NULL
 * = non-indexed soup (3 consecutive positions per triangle).  Device resident from here on, a mesh of
 * more than 256 triangles stored in the spatial (Morton) order of its triangles' centroids; the
 * submission order -- z ties, clipped fans, draws without a depth target -- stays the MeshData order. */
int shs_mesh_upload(shs_ctx *ctx, const float *positions, int32_t n_verts, const float *normals, int32_t n_normals,
                    const float *uvs, int32_t n_uvs, const uint32_t *indices, int64_t n_indices, int32_t *mesh_id);

/* Texture2DData (resources/texture.hpp:23-49): w * h Color texels (RGBA8, texel (x, y) at byte
 * 4 * (y * w + x)), device resident from here on.  *tex_id is >= 1 (the TextureAssetHandle convention,
 * resource_registry.hpp:62-66: 0 = no texture).  The PBR and Blinn-Phong programs sample it at the
 * perspective-correct UV0 varying with sample_texture2d_bilinear_repeat_linear (shader/
 * builtin_shaders.hpp:25-55; the sRGB decode uses the host's std::pow values).  A texture that fails
 * Texture2DData::valid() is not uploaded: the caller passes 0, as the sampler then returns vec3(1). */
int shs_texture_upload(shs_ctx *ctx, const uint8_t *rgba, int32_t w, int32_t h, int32_t *tex_id);
int shs_texture_release(shs_ctx *ctx, int32_t tex_id);

/* One rasterize_mesh call as PassPBRForward issues it per RenderItem: the ShaderUniforms fields the
 * builtin programs read (shader/types.hpp:87-116) and RasterizerConfig's cull mode / front face.
 * shadow != 0: u.shadow_map = the context's shadow map (last shs_render_shadow_map). */
typedef struct shs_lib_draw {
    int32_t mesh_id;
    int32_t program;              /* SHS_PROGRAM_* */
    int32_t cull_mode;            /* SHS_CULL_* */
    int32_t front_face_ccw;
    float model[16], viewproj[16], prev_model[16], prev_viewproj[16];
    float light_dir_ws[3], light_color[3], light_intensity, camera_pos[3];
    float base_color[3], metallic, roughness, ao;
    int32_t shadow;
    float light_viewproj[16];
    float shadow_bias_const, shadow_bias_slope;
    int32_t shadow_pcf_radius;
    float shadow_pcf_step, shadow_strength;
    int32_t enable_motion_vectors;
    int32_t base_color_tex;       /* u.base_color_tex: a shs_texture_upload id, 0 = none (sample = vec3(1)) */
} shs_lib_draw;

#define SHS_LIB_DEPTH_MOTION 1u   /* RasterizerTarget::depth_motion present: z test, depth + motion */
#define SHS_LIB_BG_GRADIENT 2u    /* PassPBRForward's no-sky background gradient, else clear_hdr     */

/* The pass's render targets: RT_ColorHDR (W*H RGBA32F, rows y-up) and RT_ColorDepthMotion (depth
 * cleared to 1 with zn / zf for the linear depth, motion cleared to 0).  shard_rank / shard_count as
 * in shs_frame_desc (32x32 tiles, tile % count == rank). */
typedef struct shs_lib_frame {
    int32_t width, height;
    int32_t shard_rank, shard_count;
    uint32_t flags;               /* SHS_LIB_* */
    float zn, zf;
    float clear_hdr[4];
} shs_lib_frame;

typedef struct shs_lib_stats {
    uint64_t tri_input;           /* RasterizerStats (rasterizer.hpp:48-53) */
    uint64_t tri_after_clip;
    uint64_t tri_raster;
    uint64_t covered_pixels;      /* pixels whose depth != clear (shaded Mpix/s numerator) */
    uint64_t max_tile_bin;
    uint64_t spilled;
    uint64_t clipped_extra;       /* fan triangles beyond the first of clipped input triangles */
} shs_lib_stats;
/* A tile-sharded pass (shard_count > 1) skips the clipping of triangles whose fans cannot reach its
 * tiles: its tri_after_clip / tri_raster / clipped_extra leave those out. */

/* PassPBRForward::execute: clear (gradient / clear_hdr, depth 1, motion 0) and one rasterize_mesh per
 * draw, in order, asynchronously on the context stream. */
int shs_render_pbr_forward(shs_ctx *ctx, const shs_lib_frame *frame, const shs_lib_draw *draws, int32_t n_draws);
/* Copy the pass's targets into caller-owned buffers: hdr W*H*4 floats, depth W*H, motion W*H*2
 * (row y = bottom-up, exactly PixelBuffer2D::at(x, y)); any pointer may be NULL. */
int shs_resolve_lib(shs_ctx *ctx, float *hdr, float *depth, float *motion);
int shs_get_lib_stats(shs_ctx *ctx, shs_lib_stats *stats);
/* Device pointers of the pass's targets; the pass chain is finished first (a capacity overflow
 * re-issues it), valid until the next shs_render_pbr_forward on this context. */
int shs_lib_device_targets(shs_ctx *ctx, void **hdr_dev, void **depth_dev, void **motion_dev);
/* Kernel durations of the library passes enqueued since shs_lib_timing_reset while
 * shs_enable_timing(ctx, 1) is on (HIP events on the context stream): sum_ms4 = {shadow k_lib_setup,
 * shadow k_lib_raster, camera k_lib_setup, camera k_lib_raster}; n_passes2 = {shadow, camera} passes. */
int shs_lib_timing_reset(shs_ctx *ctx);
int shs_lib_timing_read(shs_ctx *ctx, double sum_ms4[4], int64_t n_passes2[2]);

/* A shadow caster (RenderItem with casts_shadow): mesh + model matrix. */
typedef struct shs_shadow_caster {
    int32_t mesh_id;
    float model[16];
} shs_shadow_caster;

/* PassShadowMap::execute into the context's RT_ShadowDepth (w*h f32, cleared to 1): scene AABB of the
 * casters' mesh bounds, build_dir_light_camera_aabb(sun_dir, aabb, 10, w) (camera/light_camera.hpp
 * :33-98), then the depth pass.  light_viewproj_out (optional) receives ctx.shadow.light_viewproj. */
int shs_render_shadow_map(shs_ctx *ctx, int32_t w, int32_t h, const float sun_dir[3], const shs_shadow_caster *casters,
                          int32_t n_casters, float light_viewproj_out[16]);
int shs_resolve_shadow_map(shs_ctx *ctx, float *depth);
/* The bin tiles (32x32 texels, inclusive) the last enqueued shadow pass rendered: the whole map, or
 * under SHS_OPT_SHADOW_FOOTPRINT the camera pass's footprint (rect[2] < rect[0]: none, or still recorded). */
int shs_get_shadow_region(shs_ctx *ctx, int32_t rect[4]);
/* Host-only (no device): the footprint itself, for tests -- the texels (inclusive; texel_rect[2] <
 * texel_rect[0]: none) of an sm_w x sm_h map, through light_viewproj, that a PCF of `reach` texels reads
 * from points of the world box [world_min, world_max] whose camera_viewproj projection falls on the pixel
 * rectangle px_rect = {x0, y0, x1, y1} (inclusive, rows y up) of a width x height frame. */
int shs_shadow_footprint(const float light_viewproj[16], int32_t sm_w, int32_t sm_h, const float camera_viewproj[16],
                         int32_t width, int32_t height, const int32_t px_rect[4], const float world_min[3],
                         const float world_max[3], int32_t reach, int32_t texel_rect[4]);
/* Host-only, for tests: the same footprint per row of row_h texels (row r: texel rows r * row_h ..
 * r * row_h + row_h - 1, r < n_rows) -- the texel columns [x0[r], x1[r]] (x1[r] < x0[r]: none) read there,
 * from the convex hull of the footprint polytope's light-space image (round 6: a footprint shadow pass
 * renders only these 32-texel rows' spans of its rectangle). */
int shs_shadow_footprint_rows(const float light_viewproj[16], int32_t sm_w, int32_t sm_h, const float camera_viewproj[16],
                              int32_t width, int32_t height, const int32_t px_rect[4], const float world_min[3],
                              const float world_max[3], int32_t reach, int32_t row_h, int32_t n_rows, int32_t *x0,
                              int32_t *x1);

/* ---- Forward+ light-list binning ---------------------------------------
 * CullingLightGPU (lighting/light_types.hpp:141-166), the std430 record the reference uploads for
 * its GPU light culling; 160 B. */
typedef struct shs_culling_light {
    float position_range[4];      /* xyz position, w range                                       */
    float color_intensity[4];
    float direction_spot[4];
    float axis_spot_outer[4];
    float up_shape_x[4];
    float shape_attenuation[4];   /* x shape, y attenuation power, z bias, w cutoff              */
    uint32_t type_shape_flags[4]; /* x LightType, y culling shape, z flags, w attenuation model   */
    float cull_sphere[4];
    float cull_aabb_min[4];
    float cull_aabb_max[4];
} shs_culling_light;

#define SHS_LIGHT_CULL_NONE 0         /* culling_mode of fp_stress_light_cull.comp             */
#define SHS_LIGHT_CULL_TILED 1
#define SHS_LIGHT_CULL_TILED_DEPTH 2  /* tiles + per-tile depth range (fp_stress_depth_reduce) */
#define SHS_LIGHT_CULL_CLUSTERED 3

/* The CameraUBO fields the culling reads.  depth_linear: the depth range of mode 2 is reduced from
 * the context's library depth buffer (linear view depth, rasterizer.hpp:354-357); 0 = perspective
 * LH_NO depth as the Vulkan depth_reduce shader assumes.  shard_rank / shard_count: only the lists of
 * owned 32x32 tiles are built (others get count 0). */
typedef struct shs_light_cull_desc {
    int32_t width, height;
    uint32_t tile_size, max_per_tile, mode, z_slices;
    float view[16], proj[16];
    float zn, zf;
    int32_t depth_linear;
    int32_t shard_rank, shard_count;
} shs_light_cull_desc;

/* Upload the frame's local light set (replaces the LightBuffer SSBO). */
int shs_lights_upload(shs_ctx *ctx, const shs_culling_light *lights, int32_t n_lights);
/* fp_stress_light_cull.comp (+ fp_stress_depth_reduce.comp for mode 2, over the last library depth)
 * into device tile lists: counts[n_lists], indices[n_lists * max_per_tile], ascending light index.
 * Draws with SHS_PROGRAM_FORWARD_PLUS read these lists. */
int shs_light_cull(shs_ctx *ctx, const shs_light_cull_desc *desc);
/* counts: n_lists; indices: n_lists * max_per_tile (entries past the count are undefined); ranges:
 * tiles * 2 floats (mode 2).  Any pointer may be NULL. */
int shs_resolve_light_lists(shs_ctx *ctx, uint32_t *counts, uint32_t *indices, float *ranges);
#define SHS_PROGRAM_FORWARD_PLUS 5  /* per-pixel point lights from the tile lists (light_runtime.hpp:321-333) */

/* ---- typed local lights: spot, rect-area and tube-area shading ----------------------------------
 * LightProperties (lighting/light_runtime.hpp:53-72) with its LightType: what the four
 * ILightModel::sample functions (:321-333, :376-402, :445-471, :514-534) read.  The packed
 * shs_culling_light cannot stand in for it (other angle clamps, inflated rect extents, a negated rect
 * direction).  128 B. */
#define SHS_LIGHT_POINT 1
#define SHS_LIGHT_SPOT 2
#define SHS_LIGHT_RECT_AREA 3
#define SHS_LIGHT_TUBE_AREA 4
typedef struct shs_light_props {
    uint32_t type;                /* SHS_LIGHT_* (LightType 1-4)                                   */
    uint32_t attenuation_model;   /* LightAttenuationModel: 0 linear, 1 smooth, 2 inverse square   */
    uint32_t flags;               /* LightFlags* (bit 0 enabled: read by the culling only)         */
    float range;
    float position_ws[3], intensity;
    float color[3], inner_angle_rad;
    float direction_ws[3], outer_angle_rad;
    float right_ws[3], tube_half_length;
    float up_ws[3], tube_radius;
    float rect_half_extents[2], attenuation_power, attenuation_bias;
    float attenuation_cutoff, reserved[3];
} shs_light_props;

/* ILightModel::pack_for_culling of each record's type (light_runtime.hpp:309-314, 357-367, 425-436,
 * 494-502 through make_*_culling_light, lighting/light_types.hpp:251-435).  Host only, no device.
 * SHS_ERR_INVALID for a type outside 1-4. */
int shs_light_pack_culling(const shs_light_props *props, int32_t n_lights, shs_culling_light *out);
/* Upload the light set for SHS_PROGRAM_FORWARD_PLUS_TYPED: `cull` feeds shs_light_cull as after
 * shs_lights_upload, `props` the per-pixel shading.  SHS_ERR_INVALID (with a message) for a type outside
 * 1-4 and for a rect-area light whose up_ws is parallel to its forward direction (the reference's basis
 * is NaN there). */
int shs_lights_upload_typed(shs_ctx *ctx, const shs_culling_light *cull, const shs_light_props *props, int32_t n_lights);
/* As SHS_PROGRAM_FORWARD_PLUS, each listed light through the sample function of its own type
 * (hello_light_types_culling_sw.cpp:366-418).  Needs shs_lights_upload_typed and a shs_light_cull run
 * after it; program 5 lights any uploaded set as points. */
#define SHS_PROGRAM_FORWARD_PLUS_TYPED 6

/* ---- the software library's CPU light binning -----------------------------
 * build_light_bin_culling (shs-renderer-lib/include/shs/lighting/light_culling_runtime.hpp:266-371):
 * cull_lights_tiled / cull_lights_tiled_view_depth_range / cull_lights_clustered
 * (lighting/jolt_light_culling.hpp:135-412) -- per bin, the cell of make_screen_tile_cell (:95-133)
 * against every camera-frustum-visible light with classify_vs_cell (geometry/jolt_culling.hpp:129-257).
 * The lights are the SceneShapes' world AABBs (min xyz, max xyz; SceneShape::world_aabb()): the
 * binning reads only those and the bounding sphere Jolt derives from them.  Lists hold local light
 * indices in ascending order: counts[bin] = every match, indices[bin * max_per_bin + k] the first
 * max_per_bin (use max_per_bin = n_lights for the reference's unbounded vectors).  Bins are tile-row-
 * major (top-origin tile rows), clusters slice-major; bins_xyz = (bins_x, bins_y, bins_z), all 0 for
 * SHS_LIGHT_CULL_NONE or no lights.  Synchronous: host arrays in, host arrays out. */
typedef struct shs_light_bin_desc {
    int32_t width, height;
    uint32_t tile_size;           /* LightBinCullingConfig::tile_size (16)                        */
    uint32_t mode;                /* SHS_LIGHT_CULL_NONE / _TILED / _TILED_DEPTH / _CLUSTERED       */
    uint32_t z_slices;            /* cluster_depth_slices (16)                                    */
    uint32_t max_per_bin;
    float view_proj[16];
    float z_near, z_far;          /* LightBinCullingConfig::z_near / z_far                         */
    const float *tile_min_view_depth;   /* mode 2: tiles_x * tiles_y linear view depths each, or NULL */
    const float *tile_max_view_depth;
    int32_t n_depth_tiles;
} shs_light_bin_desc;
int shs_light_bin_culling(shs_ctx *ctx, const shs_light_bin_desc *desc, const float *light_aabbs, int32_t n_lights,
                          uint32_t bins_xyz[3], uint32_t *counts, uint32_t *indices);

/* ---- multi-GPU tile shards -------------------------------------------------------
 * A frame rendered with shard_rank / shard_count holds only its own 32x32 tiles (tile % count ==
 * rank, or its region: SHS_OPT_SHARD_LAYOUT).  shs_tiles_pack writes them into a caller-owned DEVICE buffer (e.g. a torch tensor on the
 * context's device) -- one 32x32-padded block per owned tile, planes colour / depth / motion --
 * for an RCCL gather; rank 0 calls shs_tiles_unpack once per peer to compose the full frame.  Both
 * are enqueued on the context stream (see shs_set_stream). */
#define SHS_TARGET_LEGACY 0   /* shs_render_legacy frame: RGBA8 canvas rows + f32 depth  */
#define SHS_TARGET_LIB 1      /* library frame: RGBA32F HDR (+ depth + motion)           */
#define SHS_TARGET_PRESENT 2  /* legacy SDL staging (SHS_FRAME_PRESENT): RGBA8, 4 B/px    */
#define SHS_TARGET_LIB_PRESENT 3 /* tonemap present staging (SHS_TONEMAP_PRESENT): RGBA8  */
int shs_tiles_packed_words(shs_ctx *ctx, int target, int32_t shard_count, int64_t *words_per_rank);   /* the largest rank's */
/* The packed size of one rank's tiles (regions differ in size). */
int shs_tiles_rank_words(shs_ctx *ctx, int target, int32_t shard_rank, int32_t shard_count, int64_t *words);
/* shs_tiles_pack first makes the frame final: it waits for the frame's setup (not its raster) and,
 * if a capacity overflowed, re-issues it; the pack is then enqueued on the context stream behind it,
 * so the packed tiles are final without a host wait for the render. */
int shs_tiles_pack(shs_ctx *ctx, int target, int32_t shard_rank, int32_t shard_count, void *dst_dev);
int shs_tiles_unpack(shs_ctx *ctx, int target, int32_t shard_rank, int32_t shard_count, const void *src_dev);
/* shs_tiles_unpack of several ranks' packed buffers in one launch (rank 0's side of the gather):
 * src_dev[r] = rank r's packed buffer, or NULL to skip rank r (rank 0 itself, empty ranks). */
int shs_tiles_unpack_ranks(shs_ctx *ctx, int target, int32_t count, const void *const *src_dev);

/* Host GLM restatements for non-C++ callers (camera/convention.hpp; pass_pbr_forward.hpp:136-141). */
int shs_look_at_lh(const float eye[3], const float center[3], const float up[3], float out16[16]);
int shs_perspective_lh_no(float fovy_radians, float aspect, float zn, float zf, float out16[16]);
int shs_model_euler(const float pos[3], const float rot_euler[3], const float scl[3], float out16[16]);
int shs_dir_light_camera_aabb(const float sun_dir[3], const float aabb_min[3], const float aabb_max[3], float extra_margin,
                              uint32_t resolution, float view16[16], float proj16[16], float viewproj16[16]);

/* ---- after the path: PassTonemap + present staging ------------------------
 * PassTonemap::execute (shs-renderer-lib/include/shs/passes/pass_tonemap.hpp:36-83) over the last
 * camera pass's HDR target, and the SDL texture staging of upload_ldr_to_rgba8
 * (exp-plumbing/hello_pass_basics.cpp:102-119), in one launch on the context stream.  The bytes are
 * the reference's: the host derives, with its own std::pow / std::lround, the 255 thresholds in
 * x = c / (1 + c) where the byte changes, and the kernel counts thresholds. */
#define SHS_TONEMAP_LDR 1u      /* RT_ColorLDR: W*H RGBA8, rows y up, alpha 255 */
#define SHS_TONEMAP_PRESENT 2u  /* RGBA8 staging for SDL_UpdateTexture: rows top-down, alpha 255 */
typedef struct shs_tonemap_desc {
    float exposure;             /* FrameParams::pass.tonemap.exposure (clamped to >= 0.0001 as the pass does) */
    float gamma;                /* ...gamma (clamped to >= 0.001) */
    uint32_t flags;             /* SHS_TONEMAP_* targets to write (at least one) */
} shs_tonemap_desc;
int shs_tonemap(shs_ctx *ctx, const shs_tonemap_desc *desc);
/* Fused PassTonemap: with desc non-NULL, every later shs_render_pbr_forward also writes desc's
 * targets from its shading kernel (one launch, no HDR re-read; the bytes are shs_tonemap's), and the
 * frame counts as tonemapped (shs_resolve_ldr, shs_motion_blur, SHS_TARGET_LIB_PRESENT tiles) without
 * a shs_tonemap call.  NULL turns it off.  The reference runs PassTonemap as a separate pass
 * (pass_tonemap.hpp:36-83); this only fuses it into the producer. */
int shs_lib_fuse_tonemap(shs_ctx *ctx, const shs_tonemap_desc *desc);
/* The scene's sky model behind the meshes: the first branch of PassPBRForward's background
 * (passes/pass_pbr_forward.hpp:64-73), render_skybox_to_hdr (sky/skybox_renderer.hpp:25-57) over
 * ProceduralSky::sample (sky/procedural_sky.hpp:22-46) or CubemapSky::sample (sky/cubemap_sky.hpp:39-116).
 * Every later shs_render_pbr_forward writes, for each pixel no primitive won, (sample(dir), 1) with
 * dir = normalize(inverse(cam_viewproj) * (ndc, 1, 1) / w - cam_pos), or (0, 0, 0, 1) where |w| < 1e-8 --
 * from its shading kernel, so the HDR target, a fused tonemap and the present staging hold the sky with no
 * further pass.  Such a frame ignores SHS_LIB_BG_GRADIENT and clear_hdr; depth and motion clears are
 * unchanged.  The HDR values are the reference's bit for bit (GLM's operation orders, IEEE / and sqrt, the
 * cubemap's sRGB decode as the host's std::pow(c / 255, 2.2) values).
 * Sticky, like shs_lib_fuse_tonemap: a moving camera calls it per frame (cam_viewproj / cam_pos are the
 * frame's scene.cam); each enqueued camera pass keeps the descriptor it was enqueued with.  NULL or
 * SHS_SKY_NONE: back to the gradient / clear_hdr.
 * SHS_ERR_INVALID: an unknown model, a non-finite field, a cam_viewproj whose glm::inverse is not finite,
 * a zero (or not normalisable) sun direction for SHS_SKY_PROCEDURAL, a face id of SHS_SKY_CUBEMAP that is
 * 0 or no live shs_texture_upload id.  The reference's CubemapSky returns black when a face fails
 * Texture2DData::valid(); such a cubemap is not uploaded (as shs_texture_upload): the caller sets no sky
 * model and a clear_hdr of (0, 0, 0, 1).  Faces may differ in size.  Fields the model does not read
 * (sun_dir_ws of a cubemap; face_tex, intensity of a procedural sky) are ignored.
 * shs_texture_release of a face of the context's current sky fails with SHS_ERR_INVALID: set another sky
 * (or none) first. */
#define SHS_SKY_NONE 0
#define SHS_SKY_PROCEDURAL 1
#define SHS_SKY_CUBEMAP 2
typedef struct shs_sky_desc {
    int32_t model;                        /* SHS_SKY_* */
    float cam_viewproj[16], cam_pos[3];   /* scene.cam.viewproj (column-major) / .pos */
    float sun_dir_ws[3];                  /* ProceduralSky's constructor argument (normalised by the library) */
    int32_t face_tex[6];                  /* shs_texture_upload ids: +X,-X,+Y,-Y,+Z,-Z */
    float intensity;                      /* CubemapSky's intensity */
} shs_sky_desc;
int shs_lib_set_sky(shs_ctx *ctx, const shs_sky_desc *desc);
/* ISkyModel::sample of desc's model for n directions (dirs3: n x 3 floats) into rgb3 (n x 3), through the
 * sampler the camera pass uses; the camera fields of desc are not read.  The loop body of the reference's
 * IBL precompute (resources/ibl.hpp:97-203).  Synchronous; the context's sticky sky is left alone. */
int shs_sky_sample(shs_ctx *ctx, const shs_sky_desc *desc, const float *dirs3, int32_t n, float *rgb3);
/* Copy the tonemapped targets into caller-owned W*H*4-byte buffers (either may be NULL). */
int shs_resolve_ldr(shs_ctx *ctx, uint8_t *ldr, uint8_t *present);
/* Device pointers of the tonemap targets (the pass chain finished first, as shs_lib_device_targets). */
int shs_ldr_device_targets(shs_ctx *ctx, void **ldr_dev, void **present_dev);
/* PassLightShafts::execute (shs-renderer-lib/include/shs/passes/pass_light_shafts.hpp:44-215), the
 * "light_shafts" pass of the standard chain between tonemap and motion blur
 * (pipeline/pass_adapters.hpp:1184-1276), on the last tonemap's RT_ColorLDR (SHS_TONEMAP_LDR; the
 * separate and the fused tonemap both count) IN PLACE, as the adapter runs it (input == output): after
 * the call the shafted bytes are the frame's LDR for shs_resolve_ldr, shs_ldr_device_targets,
 * shs_motion_blur and SHS_TARGET_LIB_PRESENT tile packs (the tonemap's present staging is rewritten
 * too when it has one).  rt_depth_like is the camera pass's depth plane when it has one
 * (SHS_LIB_DEPTH_MOTION) unless SHS_LIGHT_SHAFTS_NO_DEPTH.  The bytes are the reference's.  With
 * enable = 0, or a sun that projects outside the screen (:78-106), the LDR is left untouched.
 * Fields are FrameParams::pass.light_shafts (frame/frame_params.hpp:35-42) and the scene's camera / sun.
 * SHS_ERR_INVALID: no such tonemap since the last camera pass; a second call on the same tonemap, or one
 * after its shs_motion_blur (run shs_tonemap again first); non-finite floats; steps > 1024 (the
 * reference has no upper bound -- an error rather than a clamp, so no accepted input differs from it);
 * a tile-sharded frame (shard_count > 1: the taps cross tile ownership -- in a multi-GPU run the pass
 * belongs after the gather).  A later shs_tonemap or camera pass starts over. */
#define SHS_LIGHT_SHAFTS_NO_DEPTH 1u    /* rt_depth_like absent: s = luma only */
typedef struct shs_light_shafts_desc {
    int32_t enable;             /* FrameParams::pass.light_shafts.enable */
    int32_t steps;              /* 48; the pass takes max(8, steps) */
    float density, weight, decay;   /* 0.8, 0.9, 0.95; clamped as the pass does */
    float cam_pos[3], sun_dir_ws[3];   /* scene.cam.pos, scene.sun.dir_ws */
    float viewproj[16];         /* scene.cam.viewproj, column-major */
    uint32_t flags;             /* SHS_LIGHT_SHAFTS_* */
} shs_light_shafts_desc;
int shs_light_shafts(shs_ctx *ctx, const shs_light_shafts_desc *desc);
/* PassMotionBlur::execute (shs-renderer-lib/include/shs/passes/pass_motion_blur.hpp:38-170) on the
 * last tonemap's RT_ColorLDR (SHS_TONEMAP_LDR) with the camera pass's depth / motion planes
 * (SHS_LIB_DEPTH_MOTION), into a separate RT_ColorLDR (+ its present staging with
 * SHS_MOTION_BLUR_PRESENT).  Fields are FrameParams::pass.motion_blur (frame/frame_params.hpp:49-57)
 * and FrameParams::dt; enable = 0 copies the input, as the pass does. */
#define SHS_MOTION_BLUR_PRESENT 1u
typedef struct shs_motion_blur_desc {
    int32_t enable;
    int32_t samples;            /* default 10, clamped to [4, 32] */
    float strength;             /* 1 */
    float max_velocity_px;      /* 20 */
    float min_velocity_px;      /* 0.25 */
    float depth_reject;         /* 0.08 */
    float dt;                   /* FrameParams::dt, seconds */
    uint32_t flags;             /* SHS_MOTION_BLUR_* */
} shs_motion_blur_desc;
int shs_motion_blur(shs_ctx *ctx, const shs_motion_blur_desc *desc);
/* Copy the blurred RT_ColorLDR (rows y up) and / or its present staging (rows top-down). */
int shs_resolve_motion_blur(shs_ctx *ctx, uint8_t *ldr, uint8_t *present);
/* ---- software occlusion pass ------------------------------------------------
 * culling_sw::run_software_occlusion_pass (shs-renderer-lib/include/shs/geometry/culling_software.hpp
 * :229-331) as scene_culling.hpp:187-219 drives it: the frustum-visible objects in view-depth order
 * (view z of the world AABB centre), each tested against the occlusion depth with its screen rect
 * (project_aabb_to_screen_rect + is_rect_occluded) and, when visible, depth-rasterized into it
 * (rasterize_mesh_depth_transformed).  Synchronous: the visible list feeds the host's draw list. */
typedef struct shs_occluder {
    int32_t mesh_id;            /* indexed shs_mesh_upload mesh (DebugMesh vertices + indices) */
    float model[16];            /* the instance transform (column-major) */
    float aabb_min[3], aabb_max[3];   /* world AABB (SceneElement::geometry.world_aabb()) */
} shs_occluder;
typedef struct shs_occlusion_desc {
    int32_t width, height;      /* occlusion buffer (OCC_W x OCC_H): 1 .. 65535 per side, width * height
                                 * <= 2^31 - 2^16 (SHS_ERR_INVALID beyond either limit, nothing allocated) */
    float view[16], view_proj[16];
    float depth_epsilon;        /* 1e-4 in the reference */
    int32_t enable;             /* 0: every frustum-visible object is visible */
} shs_occlusion_desc;
/* occluded[n_objects] (1 = occluded; 0 for objects not frustum-visible), visible[] in visit order
 * (capacity n_frustum_visible), *n_visible, depth W*H (y * W + x, may be NULL). */
int shs_occlusion_pass(shs_ctx *ctx, const shs_occlusion_desc *desc, const shs_occluder *objects, int32_t n_objects,
                       const uint32_t *frustum_visible, int32_t n_frustum_visible, uint8_t *occluded,
                       uint32_t *visible, int32_t *n_visible, float *depth);

/* ---- debug_draw colour + depth raster ----------------------------------------
 * shs::debug_draw (shs-renderer-lib/include/shs/sw_render/debug_draw.hpp): draw_filled_triangle
 * (:60-109) and draw_mesh_blinn_phong_transformed (:147-203), the lit-surface draw of the culling
 * demos (hello_occlusion_culling_sw.cpp:387-407, hello_culling_sw.cpp:315).  rgba is the RT_ColorLDR
 * (W*H Color, y * W + x, the rows as the canvas holds them) and depth the std::span<float> depth
 * buffer (y * W + x); both are read and written in place, exactly as a sequential draw of the list in
 * submission order leaves them.  Synchronous. */
typedef struct shs_debug_draw_desc {
    int32_t width, height;      /* canvas_w, canvas_h (== rt.w, rt.h) */
    float view_proj[16];        /* vp (column-major) */
    float camera_pos[3];
    float light_dir_ws[3];
} shs_debug_draw_desc;
typedef struct shs_debug_mesh {
    int32_t mesh_id;            /* indexed shs_mesh_upload mesh (DebugMesh vertices + indices) */
    float model[16];            /* column-major */
    float base_color[3];
} shs_debug_mesh;
/* The meshes in order, each draw_mesh_blinn_phong_transformed.  tri_lit (may be NULL): 4 floats per
 * triangle in submission order -- lit.rgb before the byte conversion (0 when the triangle is culled
 * before shading) and 1.0 when the triangle passes draw_filled_triangle's area test (0.0 otherwise). */
int shs_debug_draw_meshes(shs_ctx *ctx, const shs_debug_draw_desc *desc, const shs_debug_mesh *meshes,
                          int32_t n_meshes, uint8_t *rgba, float *depth, float *tri_lit);
typedef struct shs_debug_triangle {
    float p0[2], p1[2], p2[2];  /* screen points (pixels) */
    float z[3];                 /* depths z0, z1, z2 */
    uint8_t rgba[4];            /* Color */
} shs_debug_triangle;
/* draw_filled_triangle for each triangle in order. */
int shs_debug_fill_triangles(shs_ctx *ctx, int32_t width, int32_t height, const shs_debug_triangle *tris,
                             int32_t n_tris, uint8_t *rgba, float *depth);

/* ---- Canvas-API multi-pass extras --------------------------------------------
 * hello-render-target/ demos, paths relative to cpp-folders/src/hello-render-target/.  Colour buffers are
 * shs::Canvas pixels (W*H Color), depth the ZBuffer (view z, FLT_MAX = empty) and velocity the
 * Buffer<glm::vec2>, all indexed y * W + x as the passes index raw().  Host buffers: synchronous;
 * flags SHS_CANVAS_DEVICE: device buffers, enqueued on the context stream (shs_set_stream): the
 * caller orders that stream against whatever produces the inputs and consumes the outputs -- run
 * the context on the producer's stream (as the Python host does with torch's current stream) or
 * make the streams wait on events. */
#define SHS_CANVAS_DEVICE 1u
#define SHS_CANVAS_MAX_AUTOFOCUS_RADIUS 32
typedef struct shs_canvas_motion_blur_desc {
    int32_t width, height;
    float curr_view[16], curr_proj[16], prev_view[16], prev_proj[16];   /* column-major */
    int32_t samples;            /* MB_SAMPLES (12) */
    float strength;             /* MB_STRENGTH (0.85) */
    float w_obj, w_cam;         /* MB_W_OBJ (1), MB_W_CAM (0.35) */
    int32_t soft_knee;          /* MB_SOFT_KNEE (1) */
    float knee_px;              /* MB_KNEE_PIXELS (18) */
    float max_px;               /* MB_MAX_PIXELS (22) */
} shs_canvas_motion_blur_desc;
/* combined_motion_blur_pass (hello_pbr.cpp:1128-1252): src, depth, velocity -> dst. */
int shs_canvas_motion_blur(shs_ctx *ctx, const shs_canvas_motion_blur_desc *desc, const uint8_t *src, const float *depth,
                           const float *velocity, uint8_t *dst, uint32_t flags);
/* gaussian_blur_pass (hello_depth_of_field.cpp:175-251): one 5-tap axis, src -> dst. */
int shs_canvas_gaussian_blur(shs_ctx *ctx, int32_t width, int32_t height, const uint8_t *src, uint8_t *dst,
                             int32_t horizontal, uint32_t flags);
typedef struct shs_canvas_dof_desc {
    int32_t width, height;
    int32_t blur_iterations;    /* BLUR_ITERATIONS (3) */
    int32_t autofocus_radius;   /* AUTOFOCUS_RADIUS (6), at most SHS_CANVAS_MAX_AUTOFOCUS_RADIUS */
    int32_t focus_x, focus_y;   /* the autofocus centre (CANVAS_WIDTH / 2, CANVAS_HEIGHT / 2) */
    float range;                /* dof_range (24) */
    float max_blur;             /* dof_maxblur (0.6) */
} shs_canvas_dof_desc;
/* The depth-of-field step of hello_depth_of_field.cpp:786-812: color (ping.color) is the sharp frame
 * in and the composite out; blur_out (may be NULL) receives the final blur (pong.color); focus_depth
 * (may be NULL, host) the autofocus depth. */
int shs_canvas_dof(shs_ctx *ctx, const shs_canvas_dof_desc *desc, uint8_t *color, const float *depth, uint8_t *blur_out,
                   float *focus_depth, uint32_t flags);
/* light_shafts_pass of hello_pbr_light_shafts.cpp (:1390-1707; PASS1.5 of its frame, :2171-2190): per pixel a
 * volumetric ray march from the camera through height fog with a sine-noise density, the sun's visibility from
 * the shadow map at every step, a Henyey-Greenstein phase, and a soft re-tonemap of the pixel's colour.  The
 * fields after shadow_h are LightShaftParams (:189-218) in its order, bools as int32_t. */
#define SHS_CANVAS_LIGHT_SHAFTS_MAX_STEPS 4096
typedef struct shs_canvas_light_shafts_desc {
    int32_t width, height;
    float cam_pos[3];
    float inv_view_proj[16];    /* glm::inverse(proj * view) (:2171), column-major: the pass inverts nothing */
    float sun_dir_world[3];     /* sun -> scene, not normalised */
    float light_vp[16];
    int32_t shadow_w, shadow_h;
    int32_t enable;             /* 1 */
    int32_t steps;              /* 40 */
    float max_dist;             /* 110 */
    float min_dist;             /* 1 */
    float base_density;         /* 0.18 */
    float height_falloff;       /* 0.10 */
    float noise_scale;          /* 0.65 */
    float noise_strength;       /* 0.60 */
    float jitter_amount;        /* 1 */
    float ambient_strength;     /* 0.08 */
    float sigma_s;              /* 0.030 */
    float sigma_t;              /* 0.065 */
    float g;                    /* 0.82 */
    float intensity;            /* 0.35 */
    int32_t use_shadow;         /* 1 */
    float shadow_bias;          /* 0.0045 */
    int32_t shadow_pcf_2x2;     /* 1 */
} shs_canvas_light_shafts_desc;
/* src, depth -> dst (dst == src is allowed: a pixel reads only its own).  shadow_map: shadow_w * shadow_h floats
 * as shs_rt_resolve_shadow returns them (y down, FLT_MAX = empty); NULL: no map, every step is lit.  prequant (may
 * be NULL): W*H*4 floats -- for a marched pixel the sRGB colour * 255 before the byte truncation and the number of
 * steps that accumulated (those that entered the second `dens > 1e-6f` block), for a pixel the pass only copies
 * (0, 0, 0, -1).  The sin / cos / exp / pow of the march are evaluated in double and rounded once to float; the
 * reference takes them from the host's float libm, so a float may differ from it in its last bit.
 * SHS_ERR_INVALID (nothing is enqueued): a non-positive size, steps above SHS_CANVAS_LIGHT_SHAFTS_MAX_STEPS, a
 * non-finite parameter, matrix or vector, a zero-length sun_dir_world, a map without a positive size. */
int shs_canvas_light_shafts(shs_ctx *ctx, const shs_canvas_light_shafts_desc *desc, const uint8_t *src, const float *depth,
                            const float *shadow_map, uint8_t *dst, float *prequant, uint32_t flags);

/* ---- Canvas-API post passes: velocity blur, fog, outline, FXAA, bloom source, additive, lens flare ----
 * The full-screen passes behind the raster in hello_multi_pass.cpp, hello_camera_and_perobject_motion_blur.cpp
 * and hello_glowing_star.cpp, one thread per pixel, under the conventions of the block above (buffers, flags,
 * SHS_CANVAS_DEVICE).  SHS_ERR_INVALID, with nothing enqueued and the context untouched, for: a null buffer, a
 * non-positive size, an unknown flag, a non-finite parameter, a radius or ghost count outside its range,
 * fog_end - fog_start zero or non-finite, and -- for the four passes that read neighbours (velocity blur, outline,
 * FXAA, lens flare) -- a dst whose W*H*4 bytes overlap src.  Depth is finite or FLT_MAX.  Every pass but the fog
 * and the flare is exact float arithmetic: its bytes are the reference's.  Those two evaluate their one
 * transcendental (std::pow, std::exp) in double and round once to float, where the reference calls the host's
 * float libm: prequant (may be NULL; W*H*4 floats) receives the three floats just before the byte conversion
 * and 1, so that a byte off by one can be explained by its float. */
#define SHS_CANVAS_MAX_OUTLINE_RADIUS 4
#define SHS_CANVAS_MAX_FLARE_GHOSTS 8
typedef struct shs_canvas_velocity_blur_desc {
    int32_t width, height;
    int32_t samples;            /* MB_SAMPLES (12; the glowing star's 8) */
    float strength;             /* MB_STRENGTH (1; the glowing star's 1.5) */
} shs_canvas_velocity_blur_desc;
/* motion_blur_pass (hello_multi_pass.cpp:605-683): velocity * strength, `samples` tent-weighted taps along it;
 * no camera term, no knee, no clamp.  samples <= 1 copies. */
int shs_canvas_velocity_blur(shs_ctx *ctx, const shs_canvas_velocity_blur_desc *desc, const uint8_t *src,
                             const float *velocity, uint8_t *dst, uint32_t flags);
typedef struct shs_canvas_fog_desc {
    int32_t width, height;
    uint8_t fog_color[4];       /* FOG_COLOR (28, 30, 38, 255); the alpha is not used */
    float fog_start, fog_end;   /* FOG_START_Z (20), FOG_END_Z (80); fog_end < fog_start is allowed */
    float fog_power;            /* FOG_POWER (1.25) */
} shs_canvas_fog_desc;
/* fog_pass (hello_multi_pass.cpp:764-819).  dst == src is allowed (a pixel reads only its own).  prequant: the
 * ia * a + t * b sums and 1; (0, 0, 0, -1) for an empty pixel, which the pass copies. */
int shs_canvas_fog(shs_ctx *ctx, const shs_canvas_fog_desc *desc, const uint8_t *src, const float *depth, uint8_t *dst,
                   float *prequant, uint32_t flags);
typedef struct shs_canvas_outline_desc {
    int32_t width, height;
    int32_t radius;             /* EDGE_RADIUS (1): 0 .. SHS_CANVAS_MAX_OUTLINE_RADIUS */
    float threshold;            /* EDGE_THRESHOLD (0.75) */
    float strength;             /* EDGE_STRENGTH (0.15) */
} shs_canvas_outline_desc;
/* outline_pass (hello_multi_pass.cpp:689-758): an empty centre is copied, empty neighbours are skipped. */
int shs_canvas_outline(shs_ctx *ctx, const shs_canvas_outline_desc *desc, const uint8_t *src, const float *depth,
                       uint8_t *dst, uint32_t flags);
typedef struct shs_canvas_fxaa_desc {
    int32_t width, height;
    float reduce_min;           /* FXAA_REDUCE_MIN (1 / 128) */
    float reduce_mul;           /* FXAA_REDUCE_MUL (1 / 8) */
    float span_max;             /* FXAA_SPAN_MAX (8) */
} shs_canvas_fxaa_desc;
/* fxaa_pass (hello_multi_pass.cpp:1000-1114); the 0.02 contrast gate is the reference's constant. */
int shs_canvas_fxaa(shs_ctx *ctx, const shs_canvas_fxaa_desc *desc, const uint8_t *src, uint8_t *dst, uint32_t flags);
typedef struct shs_canvas_spec_bright_desc {
    int32_t width, height;
    float threshold;            /* SPEC_GLOW_THRESHOLD (0.139) */
    float intensity;            /* SPEC_GLOW_INTENSITY (13.25) */
} shs_canvas_spec_bright_desc;
/* build_spec_bright_pass (hello_glowing_star.cpp:700-752): spec01 is the W*H float plane rt_scene.spec; the gold
 * tint is the reference's.  A NaN in the plane gives a black pixel, as std::max(0.0f, NaN) does. */
int shs_canvas_spec_bright(shs_ctx *ctx, const shs_canvas_spec_bright_desc *desc, const float *spec01, uint8_t *dst,
                           uint32_t flags);
/* additive_composite_pass (hello_glowing_star.cpp:754-795): out = base + mul_color(add, strength), clamped.
 * out may be base or add (a pixel reads only its own). */
int shs_canvas_additive(shs_ctx *ctx, int32_t width, int32_t height, const uint8_t *base, const uint8_t *add,
                        float strength, uint8_t *out, uint32_t flags);
typedef struct shs_canvas_lens_flare_desc {
    int32_t width, height;
    float intensity;            /* FLARE_INTENSITY (0.55) */
    float halo_intensity;       /* FLARE_HALO_INTENS (0.35) */
    float chroma_shift_px;      /* FLARE_CHROMA_SHIFT (0.8) */
    int32_t n_ghosts;           /* FLARE_GHOSTS (3): 1 .. SHS_CANVAS_MAX_FLARE_GHOSTS */
    float ghost_scales[SHS_CANVAS_MAX_FLARE_GHOSTS];   /* the first n_ghosts (0.55, 0.85, 1.25) */
} shs_canvas_lens_flare_desc;
/* pseudo_lens_flare_pass (hello_glowing_star.cpp:802-906); the halo scale and the ring's constants are the
 * reference's.  prequant: rr, gg, bb before color_from_rgbaf's clamp, and 1. */
int shs_canvas_lens_flare(shs_ctx *ctx, const shs_canvas_lens_flare_desc *desc, const uint8_t *src, uint8_t *dst,
                          float *prequant, uint32_t flags);
#define SHS_CANVAS_MAX_OBJECT_BLUR_SAMPLES 64
typedef struct shs_canvas_object_blur_desc {
    int32_t width, height;
    float multiplier;           /* BLUR_MULTIPLIER (1.85) */
    float velocity_scale;       /* the host's clampf(target_dt / dt, 0.25f, 4.0f) (:782-784; 1 at 60 frames a second);
                                 * taken as it is, not clamped here */
    float min_vel2;             /* MIN_VEL2_THRESHOLD (0.25): a scaled velocity whose squared length is below it copies */
    int32_t max_samples;        /* MAX_BLUR_SAMPLES (20): 2 .. SHS_CANVAS_MAX_OBJECT_BLUR_SAMPLES */
    float depth_eps;            /* DEPTH_REJECT_EPS (0.15) */
    int32_t depth_rows;         /* 0: depth is in canvas rows like src, read at y; 1: in screen rows, read at
                                 * height - 1 - y -- the demo's case (:508-509, :524-525) and what shs_rt_render_plain leaves */
} shs_canvas_object_blur_desc;
/* post_process_motion_blur (hello_per_object_motion_blur.cpp:461-552): v = velocity * (multiplier * velocity_scale);
 * dot(v, v) < min_vel2 copies; otherwise (int)length(v) samples, clamped to 2 .. max_samples, over a kernel centred on the
 * pixel (offsets -0.5 .. +0.5 of v), each at ((int)(x - v.x * o), (int)(y - v.y * o)); a sample outside the canvas is
 * skipped, one whose depth differs from the pixel's by more than depth_eps is skipped (an empty depth is FLT_MAX, so an
 * empty pixel gathers empty samples only); the mean of the rest through color_from_rgbaf, or the source pixel when none is
 * left.  The (int) conversions are the x86-64 ones: a NaN or Inf velocity gives two samples outside the canvas and the
 * pixel is copied.  Exact float arithmetic: the bytes are the reference's.  src, velocity (W*H*2 floats, +Y up) and dst in
 * canvas rows.  SHS_ERR_INVALID, with nothing enqueued: a null buffer, a non-positive size, an unknown flag, a non-finite
 * parameter, max_samples outside its range, depth_rows other than 0 or 1, a dst whose bytes overlap src. */
int shs_canvas_object_blur(shs_ctx *ctx, const shs_canvas_object_blur_desc *desc, const uint8_t *src, const float *depth,
                           const float *velocity, uint8_t *dst, uint32_t flags);
/* hello_ping_pong.cpp:611-618: `iterations` (BLUR_ITERATIONS, 3) rounds of shs_canvas_gaussian_blur, horizontal from
 * color into a scratch canvas the context owns, vertical back into color; color (W*H*4 bytes) holds the result.
 * iterations 0 leaves color as it is.  SHS_ERR_INVALID: a null buffer, a non-positive size, an unknown flag,
 * iterations < 0. */
int shs_canvas_ping_pong_blur(shs_ctx *ctx, int32_t width, int32_t height, int32_t iterations, uint8_t *color, uint32_t flags);

/* A demo's whole post chain in one call, on scratch canvases the context owns (grown on demand, released by
 * shs_destroy).  The frame's width and height apply to every step: those of the embedded descs are ignored.
 * color, depth and velocity are what the raster left (shs_rt_device_targets, or host copies); color is only read,
 * dst (W*H*4 bytes) receives the presented frame and may be color.  Everything is checked before the first step
 * is enqueued; with SHS_CANVAS_DEVICE the chain never synchronises with the host (the autofocus depth stays on
 * the device). */
#define SHS_CANVAS_BLUR_VELOCITY_FIRST 0   /* hello_multi_pass.cpp:1379-1426 */
#define SHS_CANVAS_BLUR_COMBINED_FIRST 1   /* the same chain with shs_canvas_motion_blur as its first step */
#define SHS_CANVAS_BLUR_COMBINED_LATE  2   /* hello_camera_and_perobject_motion_blur.cpp:1544-1606: DoF, fog,
                                            * outline, then shs_canvas_motion_blur, then FXAA */
typedef struct shs_canvas_multi_pass_frame_desc {
    int32_t width, height;
    int32_t blur_mode;          /* SHS_CANVAS_BLUR_* */
    int32_t enable_dof;         /* ENABLE_DOF (1) */
    int32_t enable_fxaa;        /* ENABLE_FXAA (1) */
    shs_canvas_velocity_blur_desc velocity_blur;   /* blur_mode 0 */
    shs_canvas_motion_blur_desc motion_blur;       /* blur_mode 1, 2 */
    shs_canvas_dof_desc dof;
    shs_canvas_fog_desc fog;
    shs_canvas_outline_desc outline;
    shs_canvas_fxaa_desc fxaa;
} shs_canvas_multi_pass_frame_desc;
/* Blur, the DoF step (shs_canvas_dof), fog, outline, FXAA; a disabled DoF or FXAA passes its input on. */
int shs_canvas_multi_pass_frame(shs_ctx *ctx, const shs_canvas_multi_pass_frame_desc *desc, const uint8_t *color,
                                const float *depth, const float *velocity, uint8_t *dst, uint32_t flags);
typedef struct shs_canvas_glow_frame_desc {
    int32_t width, height;
    int32_t enable_dof;         /* ENABLE_DOF (1) */
    int32_t enable_bloom;       /* ENABLE_BLOOM (1); 0: bloom_out is black, as the reference clears it */
    int32_t enable_flare;       /* ENABLE_FLARE (1); 0: flare_out is black */
    int32_t bloom_iterations;   /* BLOOM_BLUR_ITERS (10): horizontal + vertical shs_canvas_gaussian_blur each, >= 0 */
    shs_canvas_velocity_blur_desc velocity_blur;
    shs_canvas_dof_desc dof;
    shs_canvas_spec_bright_desc spec_bright;
    shs_canvas_lens_flare_desc lens_flare;
} shs_canvas_glow_frame_desc;
/* hello_glowing_star.cpp:1233-1310: velocity blur, DoF, bright pass over spec01, the bloom's Gaussian iterations,
 * flare over the bloom, and the two additive composites (strength 1) onto the DoF's output. */
int shs_canvas_glow_frame(shs_ctx *ctx, const shs_canvas_glow_frame_desc *desc, const uint8_t *color, const float *depth,
                          const float *velocity, const float *spec01, uint8_t *dst, uint32_t flags);

/* ---- Canvas render-target raster: shadow pass and shadowed camera pass ------------------------------
 * The raster the hello-render-target/ demos share, for its simplest complete host
 * hello_shadow_mapping.cpp (paths relative to cpp-folders/src/hello-render-target/):
 *   shs_rt_render_shadow  PASS0: draw_triangle_tile_shadow (:791-834) over the ShadowMap's tile jobs
 *                         (:1320-1411): depth only, ndc z in [0, 1], strict '<', FLT_MAX = empty;
 *   shs_rt_render         PASS1: draw_triangle_tile_color_depth_motion_shadow (:854-1022) with
 *                         vertex_shader_full (:602-620) and fragment_shader_full (:699-750): near-plane
 *                         clipping in clip space, both windings, view-z depth, perspective-correct
 *                         world position and UV, per-pixel velocity, Blinn-Phong with the shadow lookup.
 *   shs_rt_render_shadow_edge  PASS0 of hello_ibl_skybox_xsimd.cpp instead: another raster rule into the same map
 *                         (edge functions, back faces dropped, depth bits that depend on the SIMD width), below.
 * The reference clamps a triangle's bbox to the tile job that runs it, so the pixels it visits depend on
 * the job size (ref_tile_w x ref_tile_h; the demo: 80 x 80 for both passes): the same set is visited here.
 * The planes -- colour (Canvas pixels), depth (ZBuffer: view z, FLT_MAX = empty) and velocity
 * (Buffer<glm::vec2>) -- are in canvas rows at y * W + x, what shs_canvas_motion_blur reads; the shadow
 * map is ShadowMap::depth_ (y down) at y * w + x.  Both calls enqueue on the context stream and return;
 * the resolves and shs_rt_device_targets order themselves after them.  One frame at a time: a render
 * replaces the context's previous render-target frame.
 *
 * shs_rt_frame::shading chooses the camera pass's fragment shader over the same raster:
 *   0  fragment_shader_full of hello_shadow_mapping.cpp, as above;
 *   1  fragment_shader_softshadow of hello_shadow_mapping_soft.cpp (:991-1040; its PASS1 is
 *      draw_triangle_tile_color_depth_softshadow :845-986, tile jobs of 160): Blinn-Phong whose ambient
 *      and diffuse terms take the base colour and whose specular term does not, under
 *      pcss_shadow_factor (:333-445) -- a centre lookup, a blocker search and a variable-radius PCF over
 *      POISSON_32 rotated per screen pixel, with the constants of shs_rt_set_pcss.  That demo has no
 *      motion buffer: the velocity plane is all zeros and prev_mvp is not used.  SHS_RT_PCF has no
 *      effect; SHS_RT_USE_SHADOW and SHS_RT_PREQUANT keep their meaning (the prequant plane's fourth
 *      float is the PCSS factor).  The per-pixel rotations' cos / sin are the host libm's, as the
 *      reference's: the first soft frame of a size builds a width * height table of them (16 B per
 *      pixel, at most 2^26 pixels) and keeps it until the size changes.
 *   2  fragment_shader_pbr of hello_pbr.cpp (:627-727), through shs_rt_render_pbr only (shs_rt_render rejects
 *      it: the shader needs the per-draw uniforms of shs_rt_pbr_draw).  That demo's PASS0 and PASS1 rasters
 *      (:827-870, :883-1045) are hello_shadow_mapping.cpp's, so shs_rt_render_shadow serves it unchanged and
 *      its PASS2 is shs_canvas_motion_blur over shs_rt_device_targets.  Cook-Torrance GGX under the shadow
 *      lookup of shading 0 (SHS_RT_USE_SHADOW, SHS_RT_PCF, bias_base, bias_slope), plus image-based lighting
 *      from the EnvIBL of shs_rt_set_ibl; Reinhard tonemap and gamma 2.2 to bytes.  The velocity plane is
 *      written as for shading 0.  Its skybox_background_pass (:733-799) is shs_rt_set_sky below.  Not built: the
 *      IBL precompute, which stays on the host (its results come in through shs_rt_set_ibl).
 *   3  fragment_shader_pbr of hello_pbr_light_shafts.cpp (:768-850), through shs_rt_render_pbr_soft only.  That
 *      demo's PASS1 raster (:1015-1180) is hello_pbr.cpp's with tile jobs of 160 (:117-118).  The shader is shading
 *      2's with three differences: the shadow factor is pcss_shadow_factor (:650-762, shading 1's text; the
 *      constants of shs_rt_set_pcss, whose defaults are this demo's :135-148 too, and shading 1's rotation table),
 *      so SHS_RT_PCF has no effect; there is no minimum-ambient term; the direct radiance is the literal 3.0,
 *      shs_rt_pbr::direct_intensity's default.  The velocity plane is written as for shading 2; the prequant
 *      plane's fourth float is the PCSS factor.
 *   4  fragment_shader_full of hello_ibl_skybox.cpp (:446-524), through shs_rt_render_skybox_ibl only (the shader
 *      needs the per-draw knobs of shs_rt_skybox_ibl_draw).  That demo's PASS0 and PASS1 rasters (:646-686, :705-860)
 *      are hello_shadow_mapping.cpp's with tile jobs of 160, its skybox_background_pass (:532-611) is shs_rt_set_sky
 *      with SHS_RT_SKY_ENCODE_CLAMP, and its PASS2 is shs_canvas_motion_blur over shs_rt_device_targets.  Blinn-Phong
 *      under the shadow lookup of shading 0 (SHS_RT_USE_SHADOW, SHS_RT_PCF, bias_base, bias_slope) whose ambient and
 *      diffuse terms take the base colour and whose specular term does not, with the ambient term tinted by
 *      sky.sample(N) and a Schlick-weighted sky.sample(reflect(-V, N)) added: u.sky is the sky bound by
 *      shs_rt_set_sky, the one the background pass draws (no sky bound: u.sky == nullptr, tint 1, no reflection).
 *      The velocity plane is written as for shading 0; the prequant plane's fourth float is the shadow factor.
 *   5  the two fragment shaders of hello_water.cpp, through shs_rt_render_water only: fragment_shader_full (:938-994, the
 *      "atmosphere" shader) for the draws whose shs_rt_water_draw::flags is 0 and fragment_shader_water (:1000-1097) for
 *      those with SHS_RT_WATER_SURFACE.  That demo's PASS0 and PASS1 rasters, its vertex shader, velocity and
 *      shadow_uvz_from_world are hello_shadow_mapping.cpp's (tile jobs of 80) and its PASS2 is shs_canvas_motion_blur.
 *      The frame is shadow pass, reflection pass (a camera pass from the camera mirrored at the water plane, every draw
 *      non-water, SHS_RT_WATER_REFLECTION off), shs_rt_keep_reflection, camera pass, blur.  The atmosphere shader is
 *      Blinn-Phong with a sky-coloured ambient term (sky_color_simple along the view ray), exponential fog, Reinhard
 *      and gamma 2.2; the water shader takes its normal and foam from water_flow_normal_and_foam (:862-930, a hash /
 *      value-noise / fbm chain over world x, z and shs_rt_water::time_sec, bit for bit the reference's), mixes the
 *      water's base colour with the reflection canvas's texel under reflection_vp (nearest, distorted by the normal;
 *      the sky where the lookup leaves the canvas or none is held) by Schlick's fresnel, and adds foam, a glossy
 *      highlight and the same fog.  The shadow lookup (:716-751) differs from shading 0's: a uv outside [0, 1] is lit
 *      before the PCF taps, and an empty texel is lit whatever z is.  Both shaders round to the byte
 *      (clampi(lround(c * 255), 0, 255)) where shadings 0 to 4 truncate; the prequant plane holds c * 255 before that
 *      rounding and the shadow factor.  The velocity plane is written as for shading 0.
 *   (6 to 10: the unclipped demos, further down.)
 *   11 fragment_shader_full of hello_ibl_skybox_optimized.cpp (:875-958; the same text in hello_ibl_skybox_xsimd.cpp
 *      :822-911), through shs_rt_render_ibl_phong only (the shader needs the per-draw knobs of shs_rt_ibl_phong_draw).
 *      Both demos' PASS1 raster (optimized :1125-1291) is hello_shadow_mapping.cpp's with tile jobs of 160; the
 *      optimized demo's PASS0 is shs_rt_render_shadow, the xsimd demo's is shs_rt_render_shadow_edge; their
 *      skybox_background_pass is shs_rt_set_sky with SHS_RT_SKY_CUBEMAP and SHS_RT_SKY_ENCODE_CLAMP, and their PASS2 is
 *      shs_canvas_motion_blur over shs_rt_device_targets.  Blinn-Phong with the draw's shininess under the shadow lookup
 *      of shading 0, the specular term not taking the base colour, a legacy ambient of 0.18; plus, from the IBL of
 *      shs_rt_set_ibl, the irradiance along N weighted by kd = 1 - F and the prefiltered specular along reflect(-V, N)
 *      at lod = sqrt(2 / (shininess + 2)) * (mips - 1) weighted by ks = F (Schlick over ibl_f0); the shadow factor
 *      multiplies the direct term only.  The IBL precompute of those demos (irradiance and prefiltered mips from the
 *      skybox) stays with the caller.  pow(., shininess) is one double-precision pow rounded once.  The velocity plane
 *      is written as for shading 0; the prequant plane's fourth float is the shadow factor. */
typedef struct shs_rt_draw {
    int32_t mesh_id;            /* shs_mesh_upload_soup[_uv] soup (without UVs: vec2(0) per corner) */
    int32_t albedo_tex;         /* shs_texture_upload id (use_texture), 0: base_color */
    float model[16];            /* column-major */
    float mvp[16];
    float prev_mvp[16];
    uint8_t base_color[4];
} shs_rt_draw;
#define SHS_RT_USE_SHADOW 1u    /* u.shadow: the map of the last shs_rt_render_shadow (else lit) */
#define SHS_RT_PCF 2u           /* SHADOW_USE_PCF: shadow_factor_pcf_2x2, else shadow_compare */
#define SHS_RT_PREQUANT 4u      /* keep (r, g, b) * 255 before the byte truncation and the shadow factor */
typedef struct shs_rt_frame {
    int32_t width, height;
    int32_t ref_tile_w, ref_tile_h;   /* the reference's tile job size (TILE_SIZE_X, TILE_SIZE_Y) */
    uint8_t clear_color[4];
    float view[16];
    float light_vp[16];
    float light_dir_world[3];
    float camera_pos[3];
    float bias_base, bias_slope;      /* SHADOW_BIAS_BASE (0.0025), SHADOW_BIAS_SLOPE (0.01) */
    float max_velocity_px;            /* MB_MAX_PIXELS (22) */
    uint32_t flags;                   /* SHS_RT_* */
    int32_t shading;                  /* 0: fragment_shader_full, 1: fragment_shader_softshadow,
                                         2: fragment_shader_pbr (shs_rt_render_pbr),
                                         3: hello_pbr_light_shafts.cpp's fragment_shader_pbr :768-850 over
                                            pcss_shadow_factor :650-762 (shs_rt_render_pbr_soft),
                                         4: hello_ibl_skybox.cpp's fragment_shader_full :446-524
                                            (shs_rt_render_skybox_ibl),
                                         5: hello_water.cpp's fragment_shader_full :938-994 and
                                            fragment_shader_water :1000-1097 per draw (shs_rt_render_water),
                                         6: hello_multi_pass.cpp's blinn_phong_fragment_shader :207-237,
                                         7: hello_glowing_star.cpp's star_fragment_shader :269-308
                                            (both shs_rt_render_motion),
                                         8: hello_per_object_motion_blur.cpp's velocity_fragment_shader :139-177,
                                         9: hello_depth_of_field.cpp's and 10: hello_ping_pong.cpp's
                                            blinn_phong_fragment_shader (all three shs_rt_render_plain, whose depth
                                            plane is in screen rows),
                                         11: hello_ibl_skybox_optimized.cpp's and hello_ibl_skybox_xsimd.cpp's
                                            fragment_shader_full, optimized :875-958 (shs_rt_render_ibl_phong) */
} shs_rt_frame;
/* The PCSS constants of shading 1 (hello_shadow_mapping_soft.cpp:101-116), kept in the context. */
typedef struct shs_rt_pcss {
    float light_uv_radius;        /* LIGHT_UV_RADIUS_BASE (0.0035) */
    float search_radius_texels;   /* PCSS_BLOCKER_SEARCH_RADIUS_TEXELS (18) */
    float min_filter_texels;      /* PCSS_MIN_FILTER_RADIUS_TEXELS (1) */
    float max_filter_texels;      /* PCSS_MAX_FILTER_RADIUS_TEXELS (28) */
    float epsilon;                /* PCSS_EPSILON (1e-5) */
    int32_t blocker_samples;      /* PCSS_BLOCKER_SAMPLES (12), 0..64 */
    int32_t pcf_samples;          /* PCSS_PCF_SAMPLES (24), 0..64 */
} shs_rt_pcss;
/* NULL: the demo's constants, also the default.  SHS_ERR_INVALID: a non-finite float or a count outside
 * 0..64 (the context keeps what it had).  Counts above 32 wrap through POISSON_32[i & 31], as the reference. */
int shs_rt_set_pcss(shs_ctx *ctx, const shs_rt_pcss *pcss);
/* pcss_shadow_factor for n samples with the context's PCSS constants, through the device function the
 * raster calls: map is a host w x h ShadowMap (y down, FLT_MAX = empty), uv 2n, z and bias n each, pxpy
 * 2n screen pixels (the rotation's seed), out n factors.  Synchronous; for tests of the edge cases. */
int shs_rt_pcss_samples(shs_ctx *ctx, const float *map, int32_t w, int32_t h, int32_t n, const float *uv, const float *z,
                        const float *bias, const int32_t *pxpy, float *out);
typedef struct shs_rt_stats {
    int64_t input_tris;         /* triangles submitted */
    int64_t polys3, polys4;     /* clipped polygons of 3 and of 4 vertices */
    int64_t sub_tris;           /* sub-triangles that reach the raster (w and area tests passed) */
} shs_rt_stats;
/* Only mesh_id and model of a caster are read.  SHS_ERR_INVALID: an unknown mesh id, a non-positive size. */
int shs_rt_render_shadow(shs_ctx *ctx, int32_t w, int32_t h, int32_t ref_tile_w, int32_t ref_tile_h, const float light_vp[16],
                         const shs_rt_draw *casters, int32_t n_casters);
/* SHS_ERR_INVALID: an unknown mesh or texture id, a non-positive size, unknown flags, a shading other than
 * 0 or 1 (2 goes through shs_rt_render_pbr, 3 through shs_rt_render_pbr_soft, 4 through shs_rt_render_skybox_ibl, 5 through shs_rt_render_water, 6 and 7 through shs_rt_render_motion, 8 to 10 through shs_rt_render_plain, 11 through shs_rt_render_ibl_phong), or SHS_RT_USE_SHADOW without a shadow map rendered before. */
int shs_rt_render(shs_ctx *ctx, const shs_rt_frame *frame, const shs_rt_draw *draws, int32_t n_draws);
/* Host copies of the last camera pass (any pointer may be NULL): color W*H*4 bytes, depth W*H floats,
 * velocity W*H*2 floats.  Synchronous. */
int shs_rt_resolve(shs_ctx *ctx, uint8_t *color, float *depth, float *velocity);
int shs_rt_resolve_shadow(shs_ctx *ctx, float *shadow_map);
/* W*H*4 floats (r, g, b, shadow factor) of a SHS_RT_PREQUANT frame, zeros where nothing was shaded. */
int shs_rt_resolve_prequant(shs_ctx *ctx, float *prequant);
/* Per pixel the sub-triangle whose fragment it shows (2 * triangle + fan index over the whole submission,
 * -1 none): W*H int32.  For the parity tests. */
int shs_rt_resolve_ids(shs_ctx *ctx, int32_t *tri_id);
int shs_rt_get_stats(shs_ctx *ctx, shs_rt_stats *stats);
/* The last camera pass's device planes, final in the context stream's order (as shs_device_framebuffers):
 * valid until the next shs_rt_render of another size or shs_destroy. */
int shs_rt_device_targets(shs_ctx *ctx, void **color_dev, void **depth_dev, void **velocity_dev);
/* The device map of the last shs_rt_render_shadow (w * h floats, what shs_rt_resolve_shadow copies), final in the
 * context stream's order: shs_canvas_light_shafts chains after the raster without a resolve.  Any pointer may be
 * NULL.  Valid until the next shs_rt_render_shadow of another size or shs_destroy.  SHS_ERR_INVALID: no shadow map. */
int shs_rt_device_shadow_map(shs_ctx *ctx, void **map_dev, int32_t *w, int32_t *h);
/* hello_pbr.cpp's per-object uniforms that fragment_shader_pbr and vertex_shader_full read beside shs_rt_draw
 * (whose base_color is MaterialPBR::baseColor_srgb): element i goes with shs_rt_draw[i]. */
typedef struct shs_rt_pbr_draw {
    float normal_mat[9];              /* u.normal_mat, column-major mat3, supplied by the caller as the demo does
                                         (:1482 mat3(1) for the floor, :1557 transpose(inverse(mat3(model)))) */
    float metallic, roughness, ao;    /* MaterialPBR :474-482 */
    float ibl_diffuse_intensity, ibl_specular_intensity, ibl_reflection_strength;   /* :516-518 */
} shs_rt_pbr_draw;
/* The shader's constants (hello_pbr.cpp:150-155), kept in the context. */
typedef struct shs_rt_pbr {
    float exposure;                   /* PBR_EXPOSURE 1.75 */
    float min_roughness;              /* PBR_MIN_ROUGHNESS 0.04 */
    float direct_intensity;           /* DIRECT_LIGHT_INTENSITY 3.0 */
} shs_rt_pbr;
/* NULL: the demo's constants, also the default.  SHS_ERR_INVALID: a non-finite constant (the context keeps
 * what it had). */
int shs_rt_set_pbr(shs_ctx *ctx, const shs_rt_pbr *pbr);
/* EnvIBL (shs/resources/ibl.hpp:21-59) from host floats: irr = 6 faces of irr_size^2 rgb; spec = mip
 * 0..mip_count-1 concatenated, mip m = 6 faces of max(1, spec_base >> m)^2 rgb (ibl.hpp:168); texel (x, y) of a
 * face at y * size + x.  irr == NULL: no IBL (u.ibl == nullptr), also the default.  Kept in the context until
 * the next call.  Synchronous.  SHS_ERR_INVALID: a size <= 0 (or above 8192), mip_count outside 1..16, spec
 * NULL (the context keeps what it had). */
int shs_rt_set_ibl(shs_ctx *ctx, int32_t irr_size, const float *irr, int32_t spec_base, int32_t mip_count, const float *spec);
/* PASS1 of hello_pbr.cpp: the raster of shs_rt_render with fragment_shader_pbr.  frame->shading must be 2.
 * SHS_ERR_INVALID as shs_rt_render, and for any other shading. */
int shs_rt_render_pbr(shs_ctx *ctx, const shs_rt_frame *frame, const shs_rt_draw *draws, const shs_rt_pbr_draw *pbr_draws,
                      int32_t n_draws);
/* PASS1 of hello_pbr_light_shafts.cpp: the raster of shs_rt_render_pbr with that demo's fragment_shader_pbr (PBR
 * under PCSS, no minimum ambient).  frame->shading must be 3.  SHS_ERR_INVALID as shs_rt_render_pbr, and for any other
 * shading; a frame of more than 2^26 pixels (the rotation table of shading 1). */
int shs_rt_render_pbr_soft(shs_ctx *ctx, const shs_rt_frame *frame, const shs_rt_draw *draws, const shs_rt_pbr_draw *pbr_draws,
                           int32_t n_draws);
/* sample_cubemap_linear_vec(env_irradiance, dir) and sample_prefiltered_spec_trilinear(spec, dir, lod)
 * (ibl.hpp:236-286) of the context's IBL for n directions through the device functions the raster calls: dirs3
 * 3n, lod n, both outputs 3n.  Synchronous; for tests of the edge cases.  SHS_ERR_INVALID without an IBL. */
int shs_rt_ibl_samples(shs_ctx *ctx, int32_t n, const float *dirs3, const float *lod, float *irr_rgb3, float *spec_rgb3);
/* skybox_background_pass (hello_pbr.cpp:733-799; the same routine in hello_pbr_light_shafts.cpp:856-921 and
 * hello_ibl_skybox.cpp:532-611) over the legacy AbstractSky models of hello-shs-renderer/shs_renderer.hpp: AnalyticSky
 * (:552-611) and CubeMapSky with sample_face_bilinear (:432-517).  (These are not the library path's ProceduralSky /
 * CubemapSky of shs_lib_set_sky; the legacy ProceduralSky :520-549 is not built: no render-target demo constructs it.)
 * The reference draws the sky first and the triangles over it.  Here, with a sky bound, every camera pass
 * (shs_rt_render, shs_rt_render_pbr, shs_rt_render_pbr_soft, shs_rt_render_skybox_ibl, shs_rt_render_water, shs_rt_render_motion, shs_rt_render_plain, whatever the shading) is followed on the context stream by a background pass
 * that colours each pixel that shows no fragment (shs_rt_resolve_ids: -1) -- also one whose fragment kept its depth
 * but not its colour -- from the direction through the pixel's centre (:769-780; canvas x, y with y up).  Such a
 * pixel's prequant floats are (r, g, b) * 255 before the truncation and 1; depth and velocity stay as the raster
 * left them. */
#define SHS_RT_SKY_NONE 0
#define SHS_RT_SKY_ANALYTIC 1
#define SHS_RT_SKY_CUBEMAP 2
#define SHS_RT_SKY_ENCODE_REINHARD 0   /* * exposure, x / (1 + x), linear_to_srgb, rgb01_to_color (hello_pbr.cpp:785-789) */
#define SHS_RT_SKY_ENCODE_CLAMP 1      /* clamp(c, 0, 1), linear_to_srgb, rgb01_to_color (hello_ibl_skybox.cpp:598-601) */
typedef struct shs_rt_sky {
    int32_t model, encode;       /* SHS_RT_SKY_*, SHS_RT_SKY_ENCODE_* */
    float sun_dir[3];            /* AnalyticSky::sun_direction */
    float intensity;             /* CubeMapSky::intensity_ */
    int32_t face_tex[6];         /* +X -X +Y -Y +Z -Z, shs_texture_upload ids (any sizes, not necessarily square) */
    float cam_forward[3], cam_right[3], cam_up[3];   /* Camera3D vectors, normalised by the host as the pass does */
    float fov_degrees;           /* cam.field_of_view */
    float exposure;              /* SKY_EXPOSURE 1.85 */
} shs_rt_sky;
/* NULL or SHS_RT_SKY_NONE: no sky, also the default: uncovered pixels keep clear_color.  Kept in the context for every
 * later camera pass; no device work, cheap enough to call per frame as the camera moves.  SHS_ERR_INVALID (the
 * context keeps what it had): an unknown model or encode, a non-finite float, a camera vector (or, for the analytic
 * model, sun direction) that cannot be normalised, an unknown face id.  shs_texture_release of a face of the bound
 * sky fails with SHS_ERR_INVALID: set another sky first. */
int shs_rt_set_sky(shs_ctx *ctx, const shs_rt_sky *sky);
/* sky.sample(dir), the linear radiance, of the bound sky for n directions through the device function the
 * background pass calls: dirs3 and rgb3 3n.  Synchronous; for tests of the edge cases.  SHS_ERR_INVALID without a
 * sky. */
int shs_rt_sky_samples(shs_ctx *ctx, int32_t n, const float *dirs3, float *rgb3);
/* hello_ibl_skybox.cpp's per-object knobs that its fragment_shader_full reads beside shs_rt_draw (Uniforms :336-339;
 * set per object :1299-1302, :1362-1365, :1414-1417): element i goes with shs_rt_draw[i].  The shader saturates
 * ibl_ambient, ibl_refl and ibl_refl_mix; ibl_f0 is used as given. */
typedef struct shs_rt_skybox_ibl_draw {
    float ibl_ambient;     /* how far the ambient term is tinted by sky.sample(N) (0.25) */
    float ibl_refl;        /* the reflection's strength (0.35) */
    float ibl_f0;          /* Schlick's reflectivity at normal incidence (0.04) */
    float ibl_refl_mix;    /* per-object multiplier of the reflection (1) */
} shs_rt_skybox_ibl_draw;
/* PASS1 of hello_ibl_skybox.cpp: the raster of shs_rt_render with that demo's fragment_shader_full, which samples the
 * sky bound by shs_rt_set_sky per shaded pixel; the background pass follows as after every camera pass.
 * frame->shading must be 4.  SHS_ERR_INVALID as shs_rt_render, for any other shading, for a null ibl_draws with
 * n_draws > 0 and for a non-finite knob (nothing is enqueued). */
int shs_rt_render_skybox_ibl(shs_ctx *ctx, const shs_rt_frame *frame, const shs_rt_draw *draws,
                             const shs_rt_skybox_ibl_draw *ibl_draws, int32_t n_draws);
/* hello_ibl_skybox_optimized.cpp's and hello_ibl_skybox_xsimd.cpp's per-object knobs that their fragment_shader_full reads
 * beside shs_rt_draw (Uniforms, optimized :757-764; set per object :1737-1741, :1805-1809, :1862-1866): element i goes
 * with shs_rt_draw[i].  The shader saturates ibl_ambient, ibl_refl and ibl_refl_mix; ibl_f0 is used as given. */
typedef struct shs_rt_ibl_phong_draw {
    float ibl_ambient;     /* the weight of the diffuse irradiance term (0.30) */
    float ibl_refl;        /* the weight of the prefiltered-specular term (0.35) */
    float ibl_f0;          /* Schlick's reflectivity at normal incidence (0.04) */
    float ibl_refl_mix;    /* per-object multiplier of the specular term (1) */
    float shininess;       /* the direct specular exponent and, through sqrt(2 / (shininess + 2)), the IBL lod's roughness
                              (64); >= 0 */
} shs_rt_ibl_phong_draw;
/* PASS1 of hello_ibl_skybox_optimized.cpp and of hello_ibl_skybox_xsimd.cpp (shading 11): the raster of shs_rt_render with
 * those demos' fragment_shader_full (optimized :875-958), which reads the IBL bound by shs_rt_set_ibl (none bound:
 * u.ibl == nullptr, both IBL terms 0); the background pass follows as after every camera pass.  frame->shading must be
 * 11.  SHS_ERR_INVALID as shs_rt_render, for any other shading, for a null ibl_draws with n_draws > 0, for a non-finite
 * knob and for shininess < 0 (nothing is enqueued).  The reference would take a negative exponent; no demo passes one,
 * and sqrt(2 / (shininess + 2)) stops being a number at -2. */
int shs_rt_render_ibl_phong(shs_ctx *ctx, const shs_rt_frame *frame, const shs_rt_draw *draws,
                            const shs_rt_ibl_phong_draw *ibl_draws, int32_t n_draws);
/* PASS0 of hello_ibl_skybox_xsimd.cpp (draw_triangle_tile_shadow_xsimd :1016-1191) into the map shs_rt_render_shadow fills:
 * shs_rt_resolve_shadow, shs_rt_device_shadow_map, SHS_RT_USE_SHADOW and shs_canvas_light_shafts serve it unchanged.  Not
 * that pass's rule: edge functions with inclusive tests (E >= 0), so back faces (area <= 0) are dropped; a box of
 * (int)floor / (int)ceil of the corners' extent clamped to the tile job and then to the map; the depth from E / area
 * weights.  simd_lanes is the reference build's xsimd::batch<float>::size (8 for AVX2, 4 for SSE2 / NEON, 16 for AVX-512):
 * a row of a job is walked from the box's first column in groups of simd_lanes texels while a whole group fits, which
 * sum an edge function as A x + (B y + C), and the rest of the row as (A x + B y) + C, so a texel's depth depends on
 * simd_lanes and on the tile job size.  (int)floor / (int)ceil of a value that is not finite or does not fit an int is
 * undefined in the reference: a triangle with a screen corner that is not finite or is at least 2^31 in magnitude is
 * dropped.  SHS_ERR_INVALID: what shs_rt_render_shadow rejects, a simd_lanes other than 1, 2, 4, 8, 16. */
int shs_rt_render_shadow_edge(shs_ctx *ctx, int32_t w, int32_t h, int32_t ref_tile_w, int32_t ref_tile_h, const float light_vp[16],
                              const shs_rt_draw *casters, int32_t n_casters, int32_t simd_lanes);
/* hello_water.cpp (shading 5): which of that demo's two fragment shaders a draw runs; element i goes with shs_rt_draw[i]. */
#define SHS_RT_WATER_SURFACE 1u      /* fragment_shader_water (:1000-1097); 0: fragment_shader_full (:938-994) */
typedef struct shs_rt_water_draw {
    uint32_t flags;                  /* SHS_RT_WATER_SURFACE or 0 */
} shs_rt_water_draw;
/* The frame's part of hello_water.cpp's Uniforms (:653-655), passed per call because it changes every frame. */
#define SHS_RT_WATER_REFLECTION 1u   /* u.reflection_color is bound: the context's reflection canvas */
typedef struct shs_rt_water {
    float reflection_vp[16];         /* u.reflection_vp: the mirrored camera's proj * view, column-major */
    float time_sec;                  /* u.time_sec */
    uint32_t flags;                  /* SHS_RT_WATER_REFLECTION or 0 (refl_col = sky, :1020-1021) */
} shs_rt_water;
/* PASS1A / PASS1B of hello_water.cpp: the raster of shs_rt_render with that demo's two fragment shaders, chosen per
 * draw by water_draws[i].flags.  frame->shading must be 5.  The background pass follows as after every camera pass.
 * SHS_ERR_INVALID as shs_rt_render, for any other shading, for a null water or a null water_draws with n_draws > 0,
 * for unknown bits in either flags word, for SHS_RT_WATER_REFLECTION with no reflection canvas held and for a
 * non-finite time_sec (nothing is enqueued). */
int shs_rt_render_water(shs_ctx *ctx, const shs_rt_frame *frame, const shs_rt_draw *draws, const shs_rt_water_draw *water_draws,
                        const shs_rt_water *water, int32_t n_draws);
/* The last camera pass's colour plane, at its own size and after its background pass if a sky is bound, becomes the
 * context's reflection canvas: one device-to-device copy on the context stream, no host synchronise (but the first
 * call of a larger size, which allocates).  Valid until replaced, cleared or shs_destroy; later camera passes do not
 * touch it.  SHS_ERR_INVALID: no camera pass before it. */
int shs_rt_keep_reflection(shs_ctx *ctx);
/* The same canvas from a host image, w * h RGBA in canvas rows (y up), for hosts that draw the reflection elsewhere.
 * The reflection's size is its own, not the frame's (:1029-1038).  rgba NULL: no reflection canvas.  Synchronous.
 * SHS_ERR_INVALID: a size outside 1 .. 32767 (the context keeps what it had). */
int shs_rt_set_reflection(shs_ctx *ctx, const uint8_t *rgba, int32_t w, int32_t h);
/* water_flow_normal_and_foam (:862-930) for n points through the device function the raster calls: world_pos3 and
 * normal3 3n, foam n.  Synchronous; for tests of the hash chain, which is bit for bit the reference's.
 * SHS_ERR_INVALID: a non-finite time_sec. */
int shs_rt_water_samples(shs_ctx *ctx, int32_t n, const float *world_pos3, float time_sec, float *normal3, float *foam);
/* The camera pass of hello_multi_pass.cpp, hello_camera_and_perobject_motion_blur.cpp (shading 6) and
 * hello_glowing_star.cpp (shading 7): draw_triangle_tile_color_depth_motion (hello_multi_pass.cpp:525-599, the same text
 * at hello_camera_and_perobject_motion_blur.cpp:542-615) and draw_triangle_color_depth_velocity_spec
 * (hello_glowing_star.cpp:354-435).  It is not the raster of shs_rt_render: there is no near-plane clip and no w test (a
 * corner behind the camera projects mirrored), back faces are culled (area <= 0), the world position is interpolated
 * screen-linearly like every other varying, the velocity clamp's second threshold is 0.0001, and a fragment that wins the
 * strict depth test always writes its colour.  Shading 6 is blinn_phong_fragment_shader (:207-237: ambient 0.35,
 * specular 0.5 * pow(., 64)); shading 7 is star_fragment_shader (:269-308: ambient 0.20, spec01 = clampf(3.85 *
 * pow(., 256), 0, 1), (ambient + diffuse) * (colour * 0.85) + spec01 * (1, 0.90, 0.55)), which also fills the spec plane
 * below.  Read of the frame: width, height, ref_tile_w/h (80 x 80 in the two blur demos; the star's single job is the
 * whole frame: pass width, height), clear_color, view, light_dir_world, camera_pos, max_velocity_px (40, 22 and 30 in the
 * three demos), flags, shading; of a draw: mesh_id, model, mvp, prev_mvp, base_color.  light_vp and bias_* are not read.
 * With SHS_RT_PREQUANT the plane's fourth float is 1 for shading 6 and spec01 for shading 7.  A pixel's id is 2 * triangle
 * (one record per triangle, fan index 0); shs_rt_stats: polys3 = polys4 = 0, sub_tris counts the triangles for which
 * area <= 0 is false.  shs_rt_resolve*, shs_rt_device_targets and shs_rt_get_stats serve this pass like any other camera
 * pass, and with a sky bound the background pass follows it as after every camera pass (the three demos bind none).
 * SHS_ERR_INVALID, with nothing enqueued: another shading, a non-positive size or tile, unknown flags, SHS_RT_USE_SHADOW
 * or SHS_RT_PCF (these demos have no shadow map), a non-zero albedo_tex (the shaders read the base colour only), an
 * unknown mesh id, a non-finite or negative max_velocity_px. */
int shs_rt_render_motion(shs_ctx *ctx, const shs_rt_frame *frame, const shs_rt_draw *draws, int32_t n_draws);
/* RT_ColorDepthVelocitySpec::spec (hello_glowing_star.cpp:314-341) of the last camera pass, if it was a shading-7 frame:
 * W*H floats in canvas rows, spec01 where a fragment is shown and 0 elsewhere.  shs_rt_resolve_spec copies it to the host
 * (synchronous); shs_rt_device_spec returns the device plane, final in the context stream's order, for
 * shs_canvas_glow_frame with SHS_CANVAS_DEVICE.  The plane is allocated by the first shading-7 frame of a size.
 * SHS_ERR_INVALID after any other camera pass. */
int shs_rt_resolve_spec(shs_ctx *ctx, float *spec);
int shs_rt_device_spec(shs_ctx *ctx, void **spec_dev);
/* The camera pass of the three plain demos, the unclipped raster of shs_rt_render_motion again (no clip, no w test,
 * area <= 0 culled, every varying screen-linear, strict '<' depth with the first of equal depths winning, a winning
 * fragment always shows; ids 2 * triangle, polys3 = polys4 = 0, sub_tris the triangles the area rule keeps), for
 * frame->shading
 *   8: hello_per_object_motion_blur.cpp's draw_triangle_velocity_tile :391-455 with velocity_fragment_shader :139-177:
 *      view-z depth; velocity = (vec2(pos) / pos.w - vec2(prev) / prev.w) * 0.5f * vec2(W, H) on the clip positions
 *      interpolated to the pixel, +Y up, not clamped (max_velocity_px is not read): where an interpolated w is 0 the Inf
 *      or NaN is stored as it comes;
 *   9: hello_depth_of_field.cpp's draw_triangle_tile :524-574: view-z depth, the velocity plane all zero;
 *  10: hello_ping_pong.cpp's draw_triangle_tile :352-400: depth clip.z / clip.w per corner, interpolated
 *      screen-linearly; the velocity plane all zero; frame->view is not read.
 * The colour of all three is shading 6's Blinn-Phong with an ambient term of 0.15 (0.35 there).
 * THE DEPTH PLANE IS IN SCREEN ROWS: after this pass, and after this pass only, the depth of screen pixel (px, py), py
 * counted from the top, is at py * W + px -- the reference's three demos hand ZBuffer::test_and_set_depth the screen row,
 * so that is what their ZBuffer holds -- while colour, velocity, ids and prequant are in canvas rows, (H - 1 - py) * W + px,
 * as after every other camera pass.  hello_per_object_motion_blur.cpp turns the row over when it reads
 * (shs_canvas_object_blur with depth_rows = 1); hello_depth_of_field.cpp does not, and shs_canvas_dof over this plane as
 * it is reproduces that demo's frame, its autofocus and composite reading a depth upside down against the colour.
 * Pixels nothing covers keep FLT_MAX, the clear colour, zero velocity and id -1.  shs_rt_resolve*,
 * shs_rt_device_targets, shs_rt_get_stats and the sky background pass serve this pass like any other camera pass;
 * shs_rt_resolve_spec and shs_rt_device_spec answer SHS_ERR_INVALID after it.
 * SHS_ERR_INVALID, with nothing enqueued: another shading (and shadings 8 to 10 through every other shs_rt_render*
 * entry), a non-positive size or tile, unknown flags, SHS_RT_USE_SHADOW or SHS_RT_PCF, a non-zero albedo_tex, an unknown
 * mesh id. */
int shs_rt_render_plain(shs_ctx *ctx, const shs_rt_frame *frame, const shs_rt_draw *draws, int32_t n_draws);
/* ortho_lh_zo (hello_shadow_mapping.cpp:128-140): LH, z in [0, 1]. */
int shs_ortho_lh_zo(float left, float right, float bottom, float top, float znear, float zfar, float out16[16]);

/* ---- multi-GPU from one host process (SURVEY.md 5 "Distributed communication backend", 8e) ---------
 * The reference host is one C++ process driving one render loop (hello_pipeline_blinn_phong_shading.cpp
 * :369-455; PluggablePipeline::execute, pipeline/pluggable_pipeline.hpp:980).  A group is n contexts
 * in this process, context r on devices[r] (a device may repeat), each rendering the 32x32 tiles with
 * tile % n == r of every frame.  Per-rank work (uploads, passes) runs on one host worker thread per
 * rank, so the enqueue cost does not serialise over the GPUs.  shs_group_gather composes a frame on
 * rank 0's context: every rank packs its tiles on its own stream, copies them to rank 0's device
 * (hipMemcpyPeerAsync: xGMI between MI355X peers) and rank 0 unpacks them -- all stream-ordered, no
 * host wait, receive buffers double-buffered so the next frame's render overlaps this one's transfer.
 * Rank 0's context then resolves the full frame with the single-context calls (shs_resolve_lib,
 * shs_resolve_ldr, shs_resolve, shs_resolve_present).  Geometry, textures and lights are uploaded to
 * every rank (the ids agree across ranks when every rank uploads the same sequence). */
typedef struct shs_group shs_group;
int shs_group_create(const int32_t *devices, int32_t n, shs_group **out);
int shs_group_destroy(shs_group *g);
const char *shs_group_last_error(shs_group *g);
int shs_group_size(shs_group *g);
/* The rank's context (for the single-context calls; do not destroy it). */
int shs_group_context(shs_group *g, int32_t rank, shs_ctx **ctx);
/* Replicated uploads: the same call on every rank; *id is the (common) id. */
int shs_group_mesh_upload(shs_group *g, const float *positions, int32_t n_verts, const float *normals, int32_t n_normals,
                          const float *uvs, int32_t n_uvs, const uint32_t *indices, int64_t n_indices, int32_t *mesh_id);
int shs_group_mesh_upload_soup(shs_group *g, const float *positions, const float *normals, int32_t n_tris, int32_t *mesh_id);
int shs_group_mesh_upload_soup_uv(shs_group *g, const float *positions, const float *normals, const float *uvs, int32_t n_tris,
                                  int32_t *mesh_id);
int shs_group_texture_upload(shs_group *g, const uint8_t *rgba, int32_t w, int32_t h, int32_t *tex_id);
int shs_group_lights_upload(shs_group *g, const shs_culling_light *lights, int32_t n_lights);
int shs_group_lights_upload_typed(shs_group *g, const shs_culling_light *cull, const shs_light_props *props, int32_t n_lights);
/* shs_set_option on every rank's context (e.g. SHS_OPT_SHARD_LAYOUT). */
int shs_group_set_option(shs_group *g, int option, int64_t value);
int shs_group_lib_fuse_tonemap(shs_group *g, const shs_tonemap_desc *desc);
/* shs_lib_set_sky on every rank's context (face_tex: shs_group_texture_upload ids). */
int shs_group_lib_set_sky(shs_group *g, const shs_sky_desc *desc);
/* Sharded passes: rank r runs the call with shard_rank = r, shard_count = n (the frame's own shard
 * fields are ignored).  The shadow map is rendered whole on every rank (every rank's PCF reads all of it). */
int shs_group_light_cull(shs_group *g, const shs_light_cull_desc *desc);
int shs_group_render_shadow_map(shs_group *g, int32_t w, int32_t h, const float sun_dir[3], const shs_shadow_caster *casters,
                                int32_t n_casters, float light_viewproj_out[16]);
int shs_group_render_pbr_forward(shs_group *g, const shs_lib_frame *frame, const shs_lib_draw *draws, int32_t n_draws);
int shs_group_render_legacy(shs_group *g, const shs_frame_desc *frame, const shs_legacy_draw *draws, int32_t n_draws);
/* ... with albedo_tex[n_draws] (shs_group_texture_upload ids, or NULL) as shs_render_legacy_batch_tex: the
 * group call that takes SHS_SHADING_TEXTURED. */
int shs_group_render_legacy_tex(shs_group *g, const shs_frame_desc *frame, const shs_legacy_draw *draws, const int32_t *albedo_tex,
                                int32_t n_draws);
/* Compose the last frame's target (SHS_TARGET_*) on rank 0's context, asynchronously. */
int shs_group_gather(shs_group *g, int target);
int shs_group_synchronize(shs_group *g);

/* Host-only (no device): the byte thresholds for gamma (thr[0] = 0; +inf where a byte is never
 * reached).  Exposed for the parity tests. */
int shs_tonemap_thresholds(float gamma, float thr[256]);
/* Host-only: PassLightShafts' sun projection (pass_light_shafts.hpp:78-92) as shs_light_shafts runs it.
 * sun_uv keeps the pass's initial (0.5, 0.2) when |clip.w| <= 1e-6.  Exposed for the parity tests. */
int shs_light_shafts_sun_uv(const float cam_pos[3], const float sun_dir_ws[3], const float viewproj[16],
                            float sun_uv[2], int32_t *valid);

#ifdef __cplusplus
}
#endif
#endif
