/* vrt.h -- C ABI of the MI355X voxel ray-march library (python_raytracer_amd/_vrt.so).
 *
 * The reference (MirceaKitsune/python_raytracer) is pure Python and has no FFI of its own; its
 * boundary for this path is the object API `Camera.tile(thread, t)` / `Camera.trace(...)`
 * (reference init.py:126-150, 37-121) reading `Camera.pos/rot/lens/chunks` (init.py:14-33),
 * `data.settings` (data.py:18-77) and `data.Material` attributes (data.py:85-93).  This header is
 * what a binding for that path calls instead of the Python loops; python_raytracer_amd/camera.py
 * is that binding (ctypes).  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions: plain C, no exceptions; every function returns 0 or a negative vrt_status.
 * All `d_` pointers are DEVICE pointers owned by the caller (e.g. PyTorch-ROCm tensors) and are
 * only borrowed for the duration of the call; `stream` is a hipStream_t passed as void*.
 * Device memory is allocated only by vrt_pow_memo_create() and freed only by vrt_release_caches(); no other
 * function allocates, frees or synchronises (vrt_profile_end() waits for its events), so a frame may be captured
 * into a hipGraph.
 */
#ifndef VRT_H
#define VRT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRT_ABI_VERSION 9

typedef enum {
    VRT_OK = 0,
    VRT_ERR_ARG = -1,        /* null pointer / bad size / unsupported setting */
    VRT_ERR_HIP = -2,        /* a HIP runtime call failed (vrt_last_hip_error) */
    VRT_ERR_WORKSPACE = -3,  /* workspace / plan buffer too small */
    VRT_ERR_NO_DEVICE = -4,
    VRT_ERR_PLAN = -5,       /* the tile plan was built for other pixels / settings */
} vrt_status;

/* Render settings: the subset of data.settings the path reads (reference data.py:26-50, 64-68). */
typedef struct vrt_settings {
    int32_t width, height;     /* settings.width / height */
    int32_t samples;           /* settings.samples */
    int32_t chunk_size;        /* settings.chunk_size: power of two >= 8 */
    int32_t chunk_radius;      /* round(chunk_size / 2) */
    int32_t has_background;    /* 1: data.background is lib.material_background, 0: None (init.py:119) */
    uint64_t seed_nonce;       /* 0 = settings.static: seed = (1+x)(1+y)(1+s) (init.py:137).  Non-zero = a non-static
                                  frame (init.py:147 re-seeds from OS entropy, no parity requirement): every ray slot
                                  gets its own stream, seed = (y * width + x) * max_samples + s + seed_nonce */
    double proportions;        /* settings.proportions (data.py:66) */
    double shutter, falloff, dof, dist_min, dist_max, max_light, max_bounces;
    double lod_bounces, lod_samples, lod_random, lod_edge;
} vrt_settings;

/* Camera state (reference init.py:15-17). */
typedef struct vrt_camera {
    double pos[3];
    double rot[4];             /* quaternion x, y, z, w */
    double lens;               /* fov * pi / 8 */
} vrt_camera;

/* Packed scene = what Camera.chunks holds (reference init.py:18), flattened.
 *   chunk_table[(cx*dims[1] + cy)*dims[2] + cz], chunk (cx,cy,cz) at world origin + c*chunk_size:
 *       0                      -> no Frame for this chunk (void)
 *       slot+1 | (res << 24)   -> voxel block `slot`, Frame.resolution `res` (1..255)
 *   voxels: n_slots blocks of chunk_size^3 bytes, material id per voxel (0 = empty), stored at WORLD
 *       coordinates q*res (reference data.py:136-138, 163-175).  Inside a block voxels are bricked:
 *       8^3 bricks ordered [bx][by][bz], each brick 512 B = 8 micro-bricks [mx][my][mz] of 4^3 voxels
 *       (64 B, [x][y][z]).  vrt_voxel_offset() gives the byte offset.
 *   materials: n_materials records of 8 doubles {r, g, b, roughness, absorption, ior, energy, 0};
 *       material id = record index + 1 (reference data.py:85-93 attributes read by lib.py:448-460). */
typedef struct vrt_scene {
    int64_t origin[3];         /* world coords of chunk (0,0,0); multiples of chunk_size */
    int32_t dims[3];           /* chunks per axis */
    int32_t chunk_size;
    int32_t n_slots;
    int32_t n_materials;       /* <= 255 */
    const uint32_t* d_chunk_table;
    const uint8_t* d_voxels;
    const double* d_materials;
    const uint64_t* d_occupancy; /* n_slots * chunk_size^3 / 64 words, bit b of word w = (d_voxels[64 w + b] != 0): one
                                    word per 4^3 micro-brick, eight consecutive words (one 64-byte line) per 8^3 brick.
                                    Derived from d_voxels by vrt_occupancy_build; only the measurement variants of the
                                    march (VRT_LOOKUP=1|2) read it, the shipped kernels read the bytes */
    int32_t max_resolution;      /* largest Frame.resolution in d_chunk_table if known (1, 2, ...), 0 = unknown (the
                                    generic kernel).  Selects the kernel variant: an OVERSTATED value only costs speed, an
                                    UNDERSTATED one gives wrong results (the resolution-1 and resolution <= 2 variants
                                    leave out the snapping larger resolutions need) */
    int32_t flags;               /* VRT_SCENE_* bits, 0 if nothing is known (ABI 5 called this field `pad`) */
    const uint32_t* d_world_tables; /* NULL, or the world-axis offset tables of a VRT_SCENE_LAYOUT_DENSE scene
                                    (vrt_world_tables_build: a function of dims and chunk_size only) */
} vrt_scene;
/* vrt_scene.flags: d_chunk_table[i] == (i + 1) | (1 << 24) for every cell -- a dense world, every chunk present at
 * resolution 1, its voxel blocks in table order (what vrt_synth_volume writes; n_slots must equal the number of cells).
 * A chunk table beyond the size the march keeps in LDS (4 096 cells) is otherwise read from memory at every chunk
 * border a ray crosses; with this bit the march computes the entry instead.  Only set it for a table that was checked. */
#define VRT_SCENE_TABLE_IS_IDENTITY 1
/* vrt_scene.flags: the voxel blocks lie in TABLE ORDER -- n_slots equals the number of cells and the block of cell i is
 * block i, whether or not the table lists the cell (d_chunk_table[i] is 0 or (i + 1) | res << 24; the bytes of an unlisted
 * cell's block are never interpreted).  The voxel address of a world cell is then a sum of three per-axis terms, so the
 * march can look ahead ACROSS chunk borders without reading the table (world-axis offset tables in LDS; DESIGN.md
 * section 4) and replays the reference's re-snaps (init.py:67-73) for the borders a ray really crossed afterwards.
 * vrt_voxelize / vrt_synth_volume / vrt_select_chunks produce and keep this layout; PackedScene builds it for small
 * scene boxes.  Implied by VRT_SCENE_TABLE_IS_IDENTITY.  Only set it for a table that was checked.  The look-ahead also
 * needs d_world_tables, at most 2^30 bytes of voxels, and tables that fit the march's LDS (vrt_world_tables_bytes says). */
#define VRT_SCENE_LAYOUT_DENSE 2

/* Box of chunk cells in which visited chunks are recorded (the `traversed` list of init.py:72-73, 143).
 * d_keys[(cx*dims[1]+cy)*dims[2]+cz] receives min over rays of (ray_index << 12 | resnap_index), or
 * UINT64_MAX if never visited; the caller fills it with 0xFF bytes before the call, or sets `reset` and vrt_render_tile
 * (and vrt_trace_rays) does (in the launch that clears the frame's counters: one kernel less per frame).  Sorting the visited
 * cells by key reproduces the reference's order-preserving union.  Visits outside the box are only counted
 * (d_stats[VRT_S_TRAV_OUTSIDE]): size the box for the rays' reach, (dist_max + 1 + chunk_size / 2) * max |vel|_inf
 * around the camera -- the primary velocity of a ROTATED camera can exceed 1 per component, because the
 * reference's quaternion product (lib.py:353-358) is not norm-preserving; see Camera._velocity_bound. */
typedef struct vrt_traversed {
    int64_t origin[3];         /* world coords of cell (0,0,0); multiples of chunk_size */
    int32_t dims[3];
    int32_t reset;             /* vrt_render_tile: nonzero = set every key to UINT64_MAX before the frame's rays record theirs
                                  (0: the keys are the caller's -- e.g. several tiles recorded into one box) */
    uint64_t* d_keys;          /* may be NULL: do not record */
} vrt_traversed;

/* Per-ray end state (the `ray` store returned by Camera.trace, init.py:50-59, plus event counters).
 * Only written when requested; 152 bytes. */
enum { VRT_C_LOOKUP = 0, VRT_C_NBR, VRT_C_RESNAP, VRT_C_CHUNK_GET, VRT_C_HIT, VRT_C_DRAW, VRT_C_ADV, VRT_C_BROKE,
       VRT_NCOUNTERS };
typedef struct vrt_ray {
    int32_t x, y, s;
    int32_t color[3];
    int32_t alpha;
    int32_t ntrav;
    int32_t counters[VRT_NCOUNTERS];
    double detail, energy, step, life, bounces;
    double pos[3], vel[3];
} vrt_ray;

/* Frame statistics written by vrt_render_tile into d_stats (16 x uint64, zeroed by the callee):
 *   [0..7] event counters summed over rays (VRT_C_*), [8] primary rays traced to their end, [9] those of them that needed
 *   more random draws than the fast table held and were re-traced (a ray counted in [10] is in neither), [10] rays whose
 *   draws exceeded every table or that found a re-trace list full -- vrt_workspace_bytes has the capacities --
 *   (result invalid -> the Python wrapper raises), [11] chunk visits outside the traversed box, [12] workgroups of the
 *   frame's march that ran march_pool_kernel (rays regrouped between lanes through LDS; 0: march_kernel, one ray per lane
 *   -- which one runs is the library's choice by launch size and LDS room, and never changes a result).  Bits 32 and up of
 *   the same word count those of them that took their rays as square pixel tiles in Morton order, one eighth of the window
 *   per XCD, instead of in list order (VRT_TILED=1, a measured variant: whole-window launches over scenes beyond the caches). */
enum { VRT_S_RAYS = 8, VRT_S_RNG_RETRACED = 9, VRT_S_RNG_EXHAUSTED = 10, VRT_S_TRAV_OUTSIDE = 11, VRT_S_POOL_GROUPS = 12,
       VRT_S_STALLED = 13,  /* waves of march_pool_kernel that found nothing to run for 4096 passes in a row and gave up
                               (internal error: the frame is invalid, the Python wrapper raises) */
       VRT_S_LOOKAHEAD_GROUPS = 14,  /* workgroups of the frame's march whose look-ahead crossed chunk borders (march_step_w:
                                        VRT_SCENE_LAYOUT_DENSE scenes) */
       VRT_S_RAYGEN_GROUPS = 15,  /* workgroups of the frame's march that worked out their rays' lens quaternions and lives
                                     themselves (vrt_render_tile without d_ray_table: no ray table is written then) */
       VRT_S_CAST_REJECTED = 9,  /* vrt_cast_rays only (which re-traces nothing: the index is free there): rays the device
                                    refused -- see vrt_cast_ray */
       VRT_S_PATH_TRUNCATED = 12,  /* vrt_path_rays only (which has no ray pool): completed rays with more hits than max_hits */
       VRT_S_PATH_RECORDS = 13,    /* vrt_path_rays only: hit records written for completed rays */
       VRT_NSTATS = 16 };

int vrt_abi_version(void);
const char* vrt_status_string(int status);
int vrt_last_hip_error(void);           /* hipError_t of the last failing HIP call on this thread */
int vrt_device_count(int* count);

/* The shader's pow (lib.py:450, 465) has one exponent per frame, 1 + falloff, and a handful of bases: it is memoised.
 * vrt_pow_memo_create allocates (hipMalloc + a synchronous clear, so not inside a stream capture) a 4-KiB table for
 * (current device, falloff) that the library keeps and every later frame with that falloff reuses; without it a frame
 * memoises into its workspace and starts cold (about 0.3 ms per frame).  At most 64 tables per process (then
 * VRT_ERR_WORKSPACE).  vrt_release_caches synchronises each device that owns one and frees them all. */
int vrt_pow_memo_create(double falloff);
int vrt_release_caches(void);

/* d_occupancy of a vrt_scene from its voxel bytes: n_bytes = n_slots * chunk_size^3 (a multiple of 64). */
int vrt_occupancy_build(const uint8_t* d_voxels, int64_t n_bytes, uint64_t* d_occupancy, void* stream);

/* World-axis offset tables of a scene whose voxel blocks lie in table order (VRT_SCENE_LAYOUT_DENSE): three arrays
 * X | Y | Z of (dims[a] * chunk_size + 64) words -- 32 guard cells either side of the world -- such that the voxel of
 * world cell (x, y, z) is byte X[x] + Y[y] + Z[z] of d_voxels.  This is what replaces Frame.get_voxel's "which chunk,
 * then which cell" (reference data.py:136-145, init.py:67-77) for the positions the march reads ahead: no chunk table
 * lookup between a position and its voxel.  vrt_world_tables_bytes: *bytes = size of the three tables, or 0 when the
 * march could not use them (more than 2^30 bytes of voxels, or tables beyond its LDS budget). */
int vrt_world_tables_bytes(const int32_t* dims, int32_t chunk_size, int64_t* bytes);
int vrt_world_tables_build(const int32_t* dims, int32_t chunk_size, uint32_t* d_tables, int64_t bytes, void* stream);

/* Byte offset of voxel (lx,ly,lz) inside a chunk block (host helper; same function the kernels use). */
int64_t vrt_voxel_offset(int32_t chunk_size, int32_t lx, int32_t ly, int32_t lz);

/* Maximum samples per pixel for these settings (init.py:133-134). */
int32_t vrt_max_samples(const vrt_settings* st);

/* ---- tile plan ---------------------------------------------------------------------------------------
 * A static index over a pixel list, built once per (pixel list, width, height, samples, lod_edge) like the
 * reference builds settings.pixels once at start-up (data.py:70-77): the per-sample seeds
 * (1+x)(1+y)(1+s) (init.py:137) collide heavily (a 4K x 8 spp frame has 62.7 M rays but 7.8 M distinct seeds),
 * and equal seeds give equal random streams, so every frame seeds MT19937 once per DISTINCT seed.
 * The plan holds the sorted distinct seeds and, per ray slot, the index of its seed.
 *   layout of d_plan: 64-byte header {u64 magic, n_px, n_slots, n_distinct, settings_hash, n_words, full_frame, 0}
 *                     (full_frame = 1: the pixel list is the whole window in x-major order, pixel p = (p / height,
 *                     p % height); vrt_render_tile then resolves in 16 x 16 tiles, writing whole image-row segments),
 *                     u32 seed_list[n_slots], u32 ray_seedidx[n_slots]   (0xFFFFFFFF = unused sample slot)
 * Requires (width * height * max_samples) < 2^32.  vrt_plan_build is asynchronous; read the first 64 bytes of
 * d_plan back (after the stream has finished) to learn n_distinct (header word 3). */
int vrt_plan_bytes(const vrt_settings* st, int64_t n_px, int64_t* plan_bytes, int64_t* scratch_bytes);
int vrt_plan_build(const vrt_settings* st, const int32_t* d_pixels_xy, int64_t n_px, void* d_plan, int64_t plan_bytes,
                   void* d_scratch, int64_t scratch_bytes, void* stream);

/* Workspace bytes vrt_render_tile needs: the frame's draw table (n_distinct rows of fast_draws doubles) and ray table
 * (64 bytes per ray slot) unless the caller passes its own (external: VRT_WS_* bits), 4 bytes per ray slot for the
 * per-sample results and the retrace tables (1/64 of the ray slots, between 2^18 and 2^22 rays, times 912 bytes, plus
 * 32 MiB for the third tier).  BASELINE config 3 (62.7 M rays): 7.5 GB, or 1.25 GB with both tables external.
 * fast_draws: random draws kept per distinct seed in the frame's table, 32 or 64; rays that consume more are re-traced
 * with a private 113-draw row (and the few that outrun that, with a 1024-draw row from a full-state MT19937), so the
 * choice changes speed only, never results (32 suits max_bounces <= ~4; scenes where many rays take > 9 rough hits
 * want 64) -- as long as the re-trace lists hold the rays: per march launch (at most 2^28 ray slots) the first re-trace list
 * holds 1/64 of the launch's ray slots, held between 2^18 and 2^22 (the whole launch if it has fewer than 2^18), and the
 * second 4096 rays.  A ray that finds its list full, or that outruns the 1024-draw row, is not completed: its outputs are
 * undefined and it is counted in d_stats[VRT_S_RNG_EXHAUSTED] instead of d_stats[VRT_S_RAYS]. */
enum { VRT_WS_DRAW_TABLE = 1, VRT_WS_RAY_TABLE = 2 };
int vrt_workspace_bytes(const vrt_settings* st, int64_t n_px, int64_t n_distinct, int32_t fast_draws, int32_t external,
                        int64_t* bytes);

/* ---- draw table -------------------------------------------------------------------------------------
 * table[i * fast_draws + k] = k-th random.random() after random.seed(seed_list[i] + st->seed_nonce)
 * (init.py:137, 139; lib.py:434), for every distinct seed of the plan.  With static seeds (init.py:136-137) the
 * table depends only on the plan, fast_draws and seed_nonce, not on the frame: build it once with
 * vrt_draw_table_build and pass it to every vrt_render_tile call, or pass NULL there and the frame seeds its own
 * table into the workspace (what a non-static run, whose nonce changes every frame, needs anyway). */
int vrt_draw_table_bytes(int64_t n_distinct, int32_t fast_draws, int64_t* bytes);
int vrt_draw_table_build(const vrt_settings* st, const int32_t* d_pixels_xy, int64_t n_px, const void* d_plan,
                         int64_t n_distinct, int32_t fast_draws, double* d_table, int64_t table_bytes, void* stream);

/* ---- ray table --------------------------------------------------------------------------------------
 * Per ray slot (pixel, sample): the lens quaternion o = vec3(0, -lens_x, +lens_y).quaternion() of trace()
 * (init.py:41-43; lib.py:322-338) and the ray's life (dist_max - dist_min) * ray_detail (init.py:56, 139).  Both are
 * functions of the pixel, its draws, the settings and cam->lens only -- not of the camera's position or rotation --
 * so with static seeds they are frame-invariant like the draw table: build once, pass to every vrt_render_tile
 * (which then only multiplies by the camera rotation, lib.py:353-358, 372-376, when a lane picks the ray up), or
 * pass NULL: a table that would be written for one frame and read once is not written at all -- each lane of the march
 * works out the record of the ray it picks up from the draw row (d_stats[VRT_S_RAYGEN_GROUPS] counts the workgroups
 * that did; one record per pixel -- below -- is still built into the workspace, and so is the per-ray table for scenes
 * with resolutions > 2, whose march has no such variant).
 *   layout: one 64-byte record per ray slot (n_px * max_samples of them): doubles ox, oy, oz, ow, life (life < 0:
 *   unused sample slot) and the three draws of the ray's first rough hit (lib.py:457), copied from the draw table so
 *   that they arrive with the ray.
 *   With st->dof == 0, lod_random == 0 and lod_samples == 0 neither the lens quaternion nor the life depends on the
 *   sample (no lens jitter; detail / (1 + s * 0) * (1 - 0 * draw) is the pixel's detail exactly): the table then holds one
 *   record per PIXEL (n_px of them: ox, oy, oz, ow, life, the pixel's sample count as a double, 0, 0) and the march
 *   reads a ray's first-hit draws from the draw table -- 16 x less memory at BASELINE config 5 (1.1 GB instead of
 *   17.2 GB).  vrt_ray_table_bytes / _build and vrt_render_tile choose the layout from the settings alone. */
int vrt_ray_table_bytes(const vrt_settings* st, int64_t n_px, int64_t* bytes);
int vrt_ray_table_build(const vrt_settings* st, double lens, const int32_t* d_pixels_xy, int64_t n_px,
                        const void* d_plan, const double* d_draw_table, int32_t fast_draws, double* d_ray_table,
                        int64_t table_bytes, void* stream);

/* Camera.tile (init.py:126-150) for the pixel list d_pixels_xy ([n_px][2] int32, order = settings.pixels[t]).
 * d_plan / n_distinct: the plan built for this pixel list and the distinct-seed count read from its header.
 * d_draw_table: table built by vrt_draw_table_build for this plan, fast_draws and st->seed_nonce, or NULL.
 * d_ray_table: table built by vrt_ray_table_build from that draw table for these settings and cam->lens, or NULL
 *   (needs d_draw_table when given).
 * With st->seed_nonce != 0 every ray slot has its own seed: n_distinct must be n_px * max_samples.
 * Outputs (each may be NULL):
 *   d_rgba_f32   [n_px][4] float   per-pixel mean of the samples' [r,g,b,alpha] (lib.average, before set_at)
 *   d_image_u8   [height][width][4] RGBA8 full-window image; only the listed pixels are written (others keep
 *                what the caller put there -- zero it to get tile()'s transparent background)
 *   d_ray_rgba   [n_px * max_samples] uint32 r|g<<8|b<<16|alpha<<24 per sample (0 for unused sample slots)
 *   d_rays       [n_px * max_samples] vrt_ray debug records (slower path; unused slots have s = -1)
 *   d_stats      [VRT_NSTATS] uint64
 *   trav         traversed box (or NULL) */
int vrt_render_tile(const vrt_scene* scene, const vrt_settings* st, const vrt_camera* cam,
                    const int32_t* d_pixels_xy, int64_t n_px, const void* d_plan, int64_t n_distinct,
                    int32_t fast_draws, const double* d_draw_table, const double* d_ray_table, void* d_workspace,
                    int64_t workspace_bytes, float* d_rgba_f32, uint8_t* d_image_u8, uint32_t* d_ray_rgba, vrt_ray* d_rays,
                    uint64_t* d_stats, const vrt_traversed* trav, void* stream);

/* vrt_render_tile for n_views cameras that share the scene, the settings, the lens, the pixel list, the plan, the draw
 * table and the ray table (ABI 9): one march launch over n_views times the ray slots (plus its two re-trace launches, a
 * clear, one set-up launch per 64 views and one resolve) per BATCH instead of per view -- what a small window needs,
 * whose own march launch leaves the GPU nearly empty (stereo pairs, cube faces, a camera path, many agents'
 * viewpoints of one world).  Every view's outputs are exactly those of vrt_render_tile with that camera.
 *   d_cams       DEVICE array of n_views records (a frame stays capturable: nothing is copied or allocated here).  Their
 *                `lens` fields must all equal the lens the ray table was built for -- the march never reads them, so the
 *                caller checks this before the upload (Camera.render_views does); positions and rotations must satisfy
 *                vrt_render_tile's range rule (|pos| + reach < 2^28, |rot| <= 1e3; Camera._check_pose_range restates it
 *                for the Python layer), which the library cannot test on
 *                device memory without synchronising (a camera out of range gives a wrong image, never a wild access).
 *   traversed    HOST array of n_views boxes, or NULL.  Equal `dims`, an `origin` each (checked per view like
 *                vrt_render_tile's, before any HIP call), and the keys view after view in ONE allocation:
 *                traversed[v].d_keys == traversed[0].d_keys + v * cells (or all NULL: do not record).  View v's keys are
 *                (ray slot inside the view) << 12 | resnap_index, so each view's list is the single frame's.
 *                traversed[0].reset applies to all of them.
 *   Static seeds and cached tables only -- a batch exists to reuse them: st->seed_nonce != 0, a NULL d_draw_table or
 *   d_ray_table, or a non-NULL d_rays (no debug records of a batch) returns VRT_ERR_ARG.
 *   n_views * n_px * max_samples must stay below 2^32; a batch of more than 2^28 ray slots is split into launches at view
 *   boundaries.
 * Outputs (each may be NULL), view-major:
 *   d_rgba_f32   [n_views][n_px][4] float
 *   d_image_u8   [n_views][height][width][4]
 *   d_ray_rgba   [n_views][n_px * max_samples] uint32
 *   d_stats      [VRT_NSTATS] uint64 for the batch as a whole (lanes count events for whatever rays they run; per-view
 *                counters are not to be had cheaply): words 0..11 equal the SUM of the words the n_views single frames
 *                report; words 12..15 are 0 (batched launches run neither the ray pool nor the look-ahead).
 * d_workspace: vrt_views_workspace_bytes() bytes -- the per-sample results of all views, the re-trace tables and the
 * view records. */
int vrt_views_workspace_bytes(const vrt_settings* st, int32_t n_views, int64_t n_px, int64_t* bytes);
int vrt_render_views(const vrt_scene* scene, const vrt_settings* st, const vrt_camera* d_cams, int32_t n_views,
                     const int32_t* d_pixels_xy, int64_t n_px, const void* d_plan, int64_t n_distinct, int32_t fast_draws,
                     const double* d_draw_table, const double* d_ray_table, void* d_workspace, int64_t workspace_bytes,
                     float* d_rgba_f32, uint8_t* d_image_u8, uint32_t* d_ray_rgba, vrt_ray* d_rays, uint64_t* d_stats,
                     const vrt_traversed* traversed, void* stream);

/* ---- first hit ----------------------------------------------------------------------------------------
 * What a pixel SEES: every primary ray of vrt_render_tile followed up to the moment `mat` is first non-empty (init.py:78)
 * and no further -- depth maps, the voxel under the cursor, material-id images, line-of-sight queries.  The pass needs
 * the cached ray table (lens quaternion and life per ray slot: the same jitter and the same life as the colour frame's
 * ray), the camera, the chunk table and the voxel bytes; no draws, no materials, no workspace, no traversed list.
 * One 48-byte record per ray. */
typedef struct vrt_hit {
    double  step;      /* ray.step when the loop of init.py:66 was left: at the first voxel, or >= life for a miss */
    double  pos[3];    /* ray.pos at that moment */
    int32_t cell[3];   /* floor(pos): the voxel asked for (init.py:76) */
    int32_t material;  /* material id of the first voxel found (1..255), 0 = none within the ray's life, -1 = unused sample
                          slot, -2 = rejected ray of vrt_cast_rays (every other field of a -1 or -2 record is 0) */
} vrt_hit;

/* d_hits[k], k = p * max_samples + s, describes ray slot k of vrt_render_tile for the same pixel list, settings and camera.
 *   first_sample_only  nonzero: d_hits has n_px records, equal to records p * max_samples of the full call, and only those
 *                      rays are marched.
 *   d_ray_table        required (vrt_ray_table_build for these settings and cam->lens).
 *   d_plan, n_distinct the plan of the pixel list, as vrt_render_tile takes them (checked, never read on the device).
 *   d_stats            [VRT_NSTATS] uint64, zeroed by the callee: word 8 (VRT_S_RAYS) = rays traced, word 4 (VRT_C_HIT) =
 *                      rays that found a voxel, every other word 0 (while the call runs the library keeps its launch-wide
 *                      ray counter in the last word).
 * The range rule is vrt_render_tile's and is checked before any HIP call; nothing is allocated or synchronised, so a call
 * may be captured into a hipGraph. */
int vrt_first_hit(const vrt_scene* scene, const vrt_settings* st, const vrt_camera* cam, const int32_t* d_pixels_xy,
                  int64_t n_px, const void* d_plan, int64_t n_distinct, const double* d_ray_table,
                  int32_t first_sample_only, vrt_hit* d_hits, uint64_t* d_stats, void* stream);

/* vrt_first_hit for n_views cameras in one launch: d_cams as vrt_render_views takes them (a DEVICE array; equal lenses and
 * the range rule are the caller's to check).  Records are view-major, [n_views][n_px * max_samples] (or [n_views][n_px]
 * with first_sample_only); n_views * n_px * max_samples must stay below 2^32, and a batch of more than 2^28 ray slots is
 * split into launches at view boundaries.  d_stats holds the batch's totals.  d_workspace: vrt_first_hit_views_workspace_bytes()
 * bytes, for the view records only. */
int vrt_first_hit_views_workspace_bytes(int32_t n_views, int64_t* bytes);
int vrt_first_hit_views(const vrt_scene* scene, const vrt_settings* st, const vrt_camera* d_cams, int32_t n_views,
                        const int32_t* d_pixels_xy, int64_t n_px, const void* d_plan, int64_t n_distinct,
                        const double* d_ray_table, int32_t first_sample_only, void* d_workspace, int64_t workspace_bytes,
                        vrt_hit* d_hits, uint64_t* d_stats, void* stream);

/* ---- explicit rays ------------------------------------------------------------------------------------
 * The first voxel along rays that come from no camera: range sensors, line of sight between two points, a projectile's
 * path, audio occlusion, a probe ahead of a moving box.  One launch marches n_rays rays, each from its own origin along its
 * own velocity for its own life: the reference's loop (init.py:66-116) from exactly that state up to the first non-empty
 * voxel, so every record is bit for bit what the renderer's ray would give from there.  The library does no arithmetic on
 * origin and vel.  No camera, plan, ray table, draws, materials or workspace; no traversed list, no bounces, no material
 * filter. */
typedef struct vrt_cast_ray {   /* 64 bytes, 64-byte aligned array */
    double origin[3];           /* ray.pos at step 0 */
    double vel[3];              /* ray.vel: pos advances by vel * stepsize per step (init.py:114-116); any length */
    double life;                /* the loop runs while step < life (init.py:66) */
    double reserved;            /* ignored */
} vrt_cast_ray;

/* d_hits[k] describes d_rays[k] (both DEVICE arrays of n_rays records).
 *   st        supplies chunk_size and chunk_radius (and is checked like every settings block); dist_min, dist_max and the
 *             rest are not read.
 *   max_life  in (0, 2^28]: the caller's bound on how long a lane may march.
 *   d_stats   [VRT_NSTATS] uint64, zeroed by the callee: word 8 (VRT_S_RAYS) = rays marched, word 4 (VRT_C_HIT) = rays that
 *             found a voxel, word 9 (VRT_S_CAST_REJECTED) = rays rejected, every other word 0 (while the call runs the
 *             library keeps its launch-wide ray counter in the last word).
 * The rays are device data and the call does not synchronise, so each ray is validated on the device.  A ray is REJECTED --
 * not marched, material -2, every other field 0, counted -- when one of its seven doubles is not finite, when
 * life > max_life, when |vel[a]| > 2^25 for an axis, or when it could leave the range the march's cell arithmetic covers:
 *     |origin[a]| + (max(life, 0) + 2 * chunk_size + 2) * max(1, |vel|_inf) < 2^28    must hold for every axis a
 * (vrt_render_tile's range rule, per ray).  A ray with life <= 0 is marched for no step: step 0, pos = origin, material 0.
 * n_rays = 0 only zeroes the statistics; n_rays >= 2^32 is VRT_ERR_ARG; more than 2^28 rays are split into launches.
 * Every argument is checked before any HIP call; nothing is allocated or synchronised, so a call may be captured into a
 * hipGraph. */
int vrt_cast_rays(const vrt_scene* scene, const vrt_settings* st, const vrt_cast_ray* d_rays, int64_t n_rays,
                  double max_life, vrt_hit* d_hits, uint64_t* d_stats, void* stream);

/* ---- shaded explicit rays -------------------------------------------------------------------------------
 * What colour and energy arrive along rays that come from no camera pixel: an orthographic or top-down map view, light
 * probes, a mirror or portal pass that starts at first-hit records, a fisheye or cube-map lens, a range sensor that wants
 * the shaded return.  vrt_cast_rays's rays (the same 64-byte vrt_cast_ray records, the same validation, the same max_life)
 * through the whole of Camera.trace's loop.
 *   Start state.  Ray i starts in the state of init.py:50-59 with the caller's doubles: pos = origin, vel = vel, life = life;
 *             step = bounces = energy = 0, colour (0, 0, 0), no current chunk.  The library does no arithmetic on origin,
 *             vel or life.
 *   What runs.  init.py:66-116 -- re-snap, lookup, lib.material, the termination tests, the per-axis reflection from three
 *             neighbours, the step -- then lib.material_background if st->has_background and
 *             alpha = round(min(1, energy + shutter) * 255) (init.py:119-120, 141).  Every output is bit for bit what the
 *             renderer's ray gives from that state.
 *   Draws.    The k-th random.random() ray i consumes is d_draws[i * n_draws + k], from k = 0: there are no lens or
 *             lod_random draws, they belong to Camera.tile.  n_draws = 0 with d_draws = NULL is legal (a ray that meets a
 *             rough material then runs out at once).
 *   st        supplies chunk_size, chunk_radius, has_background, shutter, falloff, max_light, max_bounces and lod_bounces
 *             (and is checked like every settings block); dist_min, dist_max, dof, lod_samples, lod_random, lod_edge, samples,
 *             width, height and proportions are not read.
 *   Rejection.  Exactly vrt_cast_rays's rule (see vrt_cast_ray), per ray on the device.  A rejected ray is never marched:
 *             d_rgba[i] = 0, d_records[i].s = -2 and every other field of the record 0, counted in
 *             d_stats[VRT_S_CAST_REJECTED].
 *   Exhaustion.  A ray that needs more draws than n_draws is not completed: d_rgba[i] = 0, d_records[i].s = -3 and every
 *             other field 0, counted in d_stats[VRT_S_RNG_EXHAUSTED] and not in d_stats[VRT_S_RAYS] -- the records alone
 *             tell which rays to repeat with a longer row.
 *   d_rgba    [n_rays] uint32 r | g << 8 | b << 16 | alpha << 24, or NULL.
 *   d_records [n_rays] vrt_ray, or NULL (not both): a completed ray has x = y = s = 0 and detail = 1.0; colour, alpha, energy,
 *             step, life, bounces, pos and vel are its end state; ntrav counts its distinct chunks; the counters are those
 *             vrt_trace_rays writes, counters[VRT_C_DRAW] the draws consumed.  (Records cost speed, as in vrt_render_tile.)
 *   d_stats   [VRT_NSTATS] uint64, zeroed by the callee: [0..7] event sums over completed rays, [8] completed rays,
 *             [9] rejected, [10] exhausted, [11] chunk visits outside the traversed box, [12..15] 0.
 *   trav      NULL, or a box with vrt_render_tile's key rule: ray index << 12 | resnap index; `reset` is honoured.  With
 *             culling on, a chunk that only a map view or a mirror sees would otherwise be dropped by the next selection.
 *   d_workspace: vrt_shade_workspace_bytes() bytes -- the launch-wide ray counter and a pow memo for frames whose falloff has
 *             no table of vrt_pow_memo_create's (which is used when present, as in vrt_trace_rays); nothing per ray.
 * n_rays = 0 only zeroes the statistics; n_rays >= 2^32 - 1 is VRT_ERR_ARG; more than 2^28 rays are split into launches.
 * Every argument is checked before any HIP call; nothing is allocated or synchronised, so a call may be captured into a
 * hipGraph.  Not offered: averaging several samples per ray, the ray pool (one ray per lane: march_kernel's schedule). */
int vrt_shade_workspace_bytes(int64_t n_rays, int64_t* bytes);
int vrt_shade_rays(const vrt_scene* scene, const vrt_settings* st, const vrt_cast_ray* d_rays, int64_t n_rays,
                   double max_life, const double* d_draws, int32_t n_draws, void* d_workspace, int64_t workspace_bytes,
                   uint32_t* d_rgba, vrt_ray* d_records, uint64_t* d_stats, const vrt_traversed* trav, void* stream);

/* ---- hit paths of explicit rays -----------------------------------------------------------------------------
 * Every voxel a ray SHADES, not only the first: picking through glass, the object a mirror shows, multi-return range
 * sensors, audio paths with their reflections, "which voxels lit this probe".  vrt_shade_rays's rays, start state, loop,
 * draws, validation and max_life; in front of every lib.material (init.py:78-79) the ray's state is stored as one vrt_hit
 * -- step, pos, cell = floor(pos), the material found -- which is exactly what vrt_cast_rays stores for the first one.
 *   d_hits    [n_rays][max_hits] vrt_hit: record j of ray i is its j-th hit (from 0) for j < min(count, max_hits); the
 *             other slots of the row hold the unused record (material -1, every other field 0, as vrt_first_hit marks an
 *             unused sample slot).  The records of a row are in the order the ray met them: step never decreases.
 *   d_counts  [n_rays] int32: all hits of the ray (its counters[VRT_C_HIT] in vrt_shade_rays), which may exceed max_hits
 *             -- the row then holds the first max_hits; -2 a rejected ray, -3 a ray whose draws ran out.
 *   d_rgba    [n_rays] uint32 as in vrt_shade_rays, or NULL.
 *   max_hits  1..64, and n_rays * max_hits < 2^31.
 *   Rejection.  vrt_cast_rays's rule (see vrt_cast_ray), per ray on the device: d_counts[i] = -2, every slot of the row unused,
 *             d_rgba[i] = 0, counted in d_stats[VRT_S_CAST_REJECTED]; the ray is never marched.
 *   Exhaustion.  A ray that needs more draws than n_draws is not completed and reports nothing: d_counts[i] = -3, every slot
 *             of the row unused (what the ray had stored is overwritten), d_rgba[i] = 0, counted in
 *             d_stats[VRT_S_RNG_EXHAUSTED] and not in d_stats[VRT_S_RAYS].
 *   d_stats   [VRT_NSTATS] uint64, zeroed by the callee: [0..10] as in vrt_shade_rays, [11] 0 (there is no traversed box),
 *             [12] (VRT_S_PATH_TRUNCATED) completed rays with more hits than max_hits, [13] (VRT_S_PATH_RECORDS) hit records
 *             written for completed rays = sum of min(count, max_hits), [14..15] 0.
 *   d_workspace: vrt_path_workspace_bytes() bytes, as for vrt_shade_rays; nothing per ray.
 * Every byte of d_hits, d_counts and d_rgba is defined when the call has run.  d_rgba and d_stats[0..10] are bit for bit
 * what vrt_shade_rays gives for the same rays and draws; run that call on the same rays for vrt_ray records or a traversed
 * box, which this one does not write.  d_hits rows are what vrt_hit_owners takes.
 * n_rays = 0 only zeroes the statistics; n_rays >= 2^32 - 1, max_hits outside 1..64, n_rays * max_hits >= 2^31, a NULL or
 * misaligned d_hits (8 bytes) or d_counts (4 bytes) with n_rays > 0 are VRT_ERR_ARG; more than 2^28 rays are split into
 * launches.  Every argument is checked before any HIP call; nothing is allocated or synchronised, so a call may be captured
 * into a hipGraph.  Not offered: the mix weight of each hit, the ray pool, paths inside vrt_render_tile. */
int vrt_path_workspace_bytes(int64_t n_rays, int64_t* bytes);
int vrt_path_rays(const vrt_scene* scene, const vrt_settings* st, const vrt_cast_ray* d_rays, int64_t n_rays,
                  double max_life, const double* d_draws, int32_t n_draws, int32_t max_hits, void* d_workspace,
                  int64_t workspace_bytes, vrt_hit* d_hits, int32_t* d_counts, uint32_t* d_rgba, uint64_t* d_stats,
                  void* stream);

/* The primary rays of a frame as vrt_cast_ray records: what turns "pixel (x, y), sample s of this camera" into a ray that
 * vrt_cast_rays, vrt_shade_rays and vrt_path_rays take.  The arguments are vrt_first_hit's; d_rays[k] (64-byte aligned,
 * n_px * max_samples records, or n_px with first_sample_only) is the start state vrt_first_hit and vrt_render_tile give ray
 * slot k -- vel from the ray table's lens quaternion and cam->rot, origin = cam->pos + vel * dist_min, life from the ray
 * table, reserved 0 -- computed by the same device code, so the doubles are bit for bit the frame's.  An unused sample slot
 * gets eight NaNs, which every explicit-ray call rejects.  No voxel is read.
 *   d_stats   [VRT_NSTATS] uint64, zeroed by the callee: word 8 (VRT_S_RAYS) = records that hold a ray, every other word 0.
 * The colour frame's ray (x, y, s) consumed first_draw draws of its row before its loop began (1: lod_random; 3 with
 * dof != 0: the lens jitter too), so vrt_shade_rays or vrt_path_rays with d_draws row k = that row from column first_draw
 * on reproduces the frame's per-ray colour.
 * The range rule is vrt_render_tile's and is checked before any HIP call; nothing is allocated or synchronised, so a call
 * may be captured into a hipGraph. */
int vrt_pixel_rays(const vrt_scene* scene, const vrt_settings* st, const vrt_camera* cam, const int32_t* d_pixels_xy,
                   int64_t n_px, const void* d_plan, int64_t n_distinct, const double* d_ray_table,
                   int32_t first_sample_only, vrt_cast_ray* d_rays, uint64_t* d_stats, void* stream);

/* Camera.trace (init.py:37-121) for explicit rays: direction (dir_x, dir_y), detail and the random draws the
 * ray may consume (d_draws[i * n_draws + k] = k-th random.random() of ray i).  d_rays[i].counters[VRT_C_DRAW]
 * tells how many were consumed.  Rays that would need more draws are counted in d_stats[VRT_S_RNG_EXHAUSTED].
 * d_workspace: vrt_trace_workspace_bytes(n_rays) bytes. */
int vrt_trace_workspace_bytes(int64_t n_rays, int64_t* bytes);
int vrt_trace_rays(const vrt_scene* scene, const vrt_settings* st, const vrt_camera* cam,
                   const double* d_dir_x, const double* d_dir_y, const double* d_detail,
                   const double* d_draws, int32_t n_draws, int64_t n_rays,
                   void* d_workspace, int64_t workspace_bytes,
                   vrt_ray* d_rays, uint64_t* d_stats, const vrt_traversed* trav, void* stream);

/* MT19937 exactly as CPython random.seed(seed); [random.random() for _ in range(n_draws)]
 * (init.py:137, 139; lib.py:434): d_out[i * n_draws + k] = k-th draw of seed d_seeds[i]. 2 <= n_draws <= 4096
 * (up to 113 draws come from the register-only seeding kernel, more from a slower full-state generator). */
int vrt_rng_draws(const uint64_t* d_seeds, int64_t n_seeds, int32_t n_draws, double* d_out, void* stream);

/* One visible object of the world (data.Object, data.py:430-494, 589-600): the world box it occupies and the model
 * its sprite holds.  64 bytes. */
typedef struct vrt_object {
    int32_t mins[3];   /* world box [mins, maxs): ceil(pos) - size/2 .. floor(pos) + size/2 (data.py:591-599) */
    int32_t maxs[3];
    int32_t size[3];   /* sprite size = shape of the model array */
    int32_t turns[3];  /* quarter turns about x, y, z: round(rot / 90) % 4 (data.py:338-371) */
    int64_t model;     /* offset in d_models of this sprite frame's u8 ids [size.x][size.y][size.z], 0 = empty */
    int32_t remap;     /* offset in d_remap of its table: model id -> world material id (entry 0 unused) */
    int32_t pad;
} vrt_object;

/* The object loop of Window.chunk_update (init.py:398-444) on the device: every world voxel of the chunk box
 * [origin, origin + dims * chunk_size) takes the voxel of the LAST object (in array order, the dict union of
 * init.py:437-439) that has one at that position, read through the object's quarter-turn rotation
 * (Sprite.get_voxel, data.py:417-419).
 *   d_voxels      out: dims.x * dims.y * dims.z blocks of chunk_size^3 bytes in vrt_voxel_offset order, block index =
 *                 (cx * dims.y + cy) * dims.z + cz
 *   d_world_table out: [dims] block index + 1 | 1 << 24 where the chunk holds a voxel, else 0 -- the world table
 *                 vrt_select_chunks reads; with it and d_voxels a vrt_scene is complete.
 *   d_chunk_list  NULL: every chunk of the box is rebuilt.  Else n_list chunk indices ((cx * dims.y + cy) * dims.z +
 *                 cz): only these chunks are rebuilt (from ALL objects, in array order) and the rest of d_voxels /
 *                 d_world_table stays as it is -- the reference's per-object invalidation (init.py:398-429: an object
 *                 that moved, turned, appeared or vanished marks the chunks its old and new boxes touch, and only
 *                 those are recombined), for a large world in which one object moves. */
int vrt_voxelize(const vrt_object* d_objects, int32_t n_objects, const uint8_t* d_models, const uint8_t* d_remap,
                 const int64_t* origin, const int32_t* dims, int32_t chunk_size, const uint32_t* d_chunk_list,
                 int64_t n_list, uint32_t* d_world_table, uint8_t* d_voxels, void* stream);

/* ---- sprite edits on the resident models ----------------------------------------------------------------
 * Sprite.set_voxel / set_voxels_area / clear (data.py:382-427) as operation records applied to d_models in place, so that
 * an edit costs a few bytes of upload and a vrt_voxelize of the chunks it can change, not a re-upload of the model. */
typedef struct vrt_edit {      /* 64 bytes, 16-byte aligned */
    int64_t model;             /* offset of the target model in d_models */
    int32_t size[3];           /* its shape [size.x][size.y][size.z] */
    int32_t lo[3], hi[3];      /* inclusive box, 0 <= lo <= hi < size (a point is a box of one voxel) */
    int32_t value;             /* local material id 1..255, 0 clears */
    int32_t force;             /* 0: only where the model byte is 0 */
    int32_t pad[3];
} vrt_edit;
/* The word vrt_edit_models writes into d_stats (every other word 0). */
enum { VRT_S_EDIT_INVALID = 9   /* records the device refused: none of their voxels was written */ };

/* After the call d_models equals the result of applying the n_edits records of d_edits (a DEVICE array, 16-byte aligned)
 * one after another in array order: a later record wins, and a record with force = 0 sees what the earlier ones left.
 * One launch serves all records (up to 65535; more are split), without atomics on the models: a thread owns one voxel of the
 * bounding box of the records that target its model, replays in order the records that cover it and writes once, and only
 * if the byte changed.  Records target the same model when `model` and `size` agree; records of DIFFERENT models whose
 * byte ranges overlap are applied in no defined order (every write still lies inside a validated model).
 * The device validates every record: size >= 1, lo <= hi inside size, model >= 0, model + size.x * size.y * size.z <=
 * models_bytes, 0 <= value <= 255.  An invalid record is skipped as a whole, never partly applied, and counted in
 * d_stats[VRT_S_EDIT_INVALID]; no byte outside [d_models, d_models + models_bytes) is ever read or written.
 *   d_stats   [VRT_NSTATS] uint64, zeroed by the callee.
 * n_edits = 0 only zeroes the statistics.  Every host-visible argument is checked before any HIP call; nothing is allocated
 * or synchronised, so a call may be captured into a hipGraph. */
int vrt_edit_models(uint8_t* d_models, int64_t models_bytes, const vrt_edit* d_edits, int32_t n_edits,
                    uint64_t* d_stats, void* stream);

/* Sprite.mix (data.py:311-321) for one frame pair: with i over the size.x * size.y * size.z bytes of two models of the same
 * shape at offsets dst and src of d_models,  dst[i] = d_idmap[src[i]]  where src[i] != 0 and (force or dst[i] == 0).
 *   d_idmap   256 bytes on the device: the source model's local material ids -> the target's (entry 0 unused).
 * VRT_ERR_ARG: a model that leaves [0, models_bytes), or dst and src ranges that overlap.  Checked before any HIP call;
 * nothing is allocated or synchronised. */
int vrt_stamp_model(uint8_t* d_models, int64_t models_bytes, int64_t dst, int64_t src, const int32_t* size,
                    const uint8_t* d_idmap, int32_t force, void* stream);

/* ---- owners of hit records -----------------------------------------------------------------------------
 * Which OBJECT a hit belongs to, and which voxel of that object's model: what picking, instance images and sprite edits
 * act on.  vrt_voxelize keeps only the material byte ("the later object wins"); the owner pass asks voxelize's question
 * again for the hit voxels only -- the objects from LAST to FIRST, the first that has a voxel there owns it -- so it needs
 * no owner volume, and the two cannot disagree about overlaps, quarter turns or sprite LOD.  One 32-byte record per hit
 * record. */
typedef struct vrt_owner {     /* 32 bytes */
    int32_t object;            /* index into d_objects (merge order); -1: the record is no hit (material <= 0);
                                  -2: a hit that no object accounts for (orphan) */
    int32_t resolution;        /* Frame.resolution of the chunk the voxel was read from; 0 when object < 0 */
    int32_t voxel[3];          /* the world voxel that supplied the material: (cell // r) * r, inside that chunk */
    int32_t local[3];          /* index into the object's model array [size.x][size.y][size.z], i.e. after the
                                  quarter-turn addressing -- the voxel a sprite edit would change */
} vrt_owner;
/* The words vrt_hit_owners writes into d_stats (every other word 0). */
enum { VRT_S_OWNER_EXAMINED = 8,   /* records with material > 0 */
       VRT_S_OWNER_RESOLVED = 4,   /* ... of them resolved to an object */
       VRT_S_OWNER_ORPHANS = 9,    /* ... of them that no chunk of the scene, or no object, accounts for: the hits came from
                                      another scene or another object list (examined = resolved + orphans) */
       VRT_S_OWNER_AMBIGUOUS = 10  /* records that TWO chunks explain; the first was taken (below) */ };

/* d_owners[k] describes d_hits[k] (records of vrt_first_hit, vrt_first_hit_views or vrt_cast_rays; DEVICE arrays of n_hits
 * records, d_hits 8-byte and d_owners 16-byte aligned).  Every field but `object` of a record with object < 0 is 0.
 *   scene     the scene the hits were produced against: its camera table with the LOD bytes, its voxels.
 *   d_objects, n_objects, d_models, d_remap   exactly what the last vrt_voxelize call of that world was given (d_objects
 *             16-byte aligned).  n_objects = 0 makes every hit an orphan.
 *   d_stats   [VRT_NSTATS] uint64, zeroed by the callee: the VRT_S_OWNER_* words.
 * Which voxel a record means.  The march reads the voxel c = (floor(pos) // r) * r of the ray's CURRENT chunk (r: that
 * chunk's resolution) and finds nothing if c lies outside the chunk.  The record holds floor(pos) and pos, not c, r or the
 * chunk, and a ray may stand exactly on its chunk's inclusive upper face (init.py:67): floor(pos) is then in the next chunk
 * while an r that does not divide chunk_size (r = 3) snaps c back into the ray's own.  So the CANDIDATE chunks of a record
 * are the chunk containing floor(pos) and, for every axis a on which pos[a] is a whole multiple of chunk_size, the chunk
 * one below on that axis: up to 8, tried in the order (x, y, z lowered) 000, 100, 010, 110, 001, 101, 011, 111 -- the
 * containing chunk first.  A candidate COUNTS if the table lists it, its c (with its own r) lies inside it and the voxel
 * byte at c equals the record's material.  The first that counts is taken; if a later one counts too and resolves to
 * another (object, local), the record is counted in VRT_S_OWNER_AMBIGUOUS: "two chunks explain this record; the first was
 * taken" -- the result may then name the wrong one of two real voxels of that material, and the count says so.  If none
 * counts the record is an orphan.
 * The owner of c is the last object of d_objects with mins <= c < maxs whose model byte at the quarter-turned c - mins is
 * not 0 (voxelize's loop, backwards); if its remapped material is not the record's, the record is an orphan.
 * n_hits = 0 only zeroes the statistics; n_hits >= 2^32 is VRT_ERR_ARG; more than 2^28 records are split into launches.
 * Every argument is checked before any HIP call; nothing is allocated or synchronised, so a call may be captured into a
 * hipGraph. */
int vrt_hit_owners(const vrt_scene* scene, const vrt_hit* d_hits, int64_t n_hits,
                   const vrt_object* d_objects, int32_t n_objects, const uint8_t* d_models, const uint8_t* d_remap,
                   vrt_owner* d_owners, uint64_t* d_stats, void* stream);

/* ---- per-chunk object lists ----------------------------------------------------------------------------
 * vrt_voxelize asks every object about every voxel of every chunk it rebuilds, and vrt_hit_owners walks every object for every
 * record.  The reference keeps, per chunk, the objects that have it (Window.chunks_objects, init.py:398-444) and merges only
 * those.  These lists are that structure on the device, and the two passes below read them instead of the whole array.
 *
 * The list of chunk c holds every object k of d_objects whose box [mins, maxs) -- half-open on all axes -- meets the chunk's box
 * [origin + c * chunk_size, origin + (c + 1) * chunk_size), in ASCENDING k, and nothing else.  Ascending k is the merge order:
 * the voxelisation walks a list forwards (the later object wins), the owner pass backwards.  An object with an empty box
 * (mins >= maxs on some axis) is in no list; a box that leaves the chunk box is listed only where it lies inside.  The lists
 * are a SUPERSET of the reference's dict, which names only chunks in which the object has a voxel: whether a model holds
 * anything there is still asked per voxel.
 * Why the list-driven passes give the scans' results: an object can only supply a voxel c with mins <= c < maxs; such a box
 * meets the chunk that contains c, so the object is in that chunk's list, and the list keeps the array's relative order. */
typedef struct vrt_chunk_lists {
    int64_t origin[3]; int32_t dims[3]; int32_t chunk_size;   /* the world chunk box the lists index: what vrt_voxelize takes */
    int64_t n_items_cap;       /* capacity of d_items in items, < 2^31 */
    uint32_t* d_offsets;       /* [n_chunks + 1], chunk index (cx * dims.y + cy) * dims.z + cz as in vrt_voxelize; 4-byte aligned */
    int32_t*  d_items;         /* object indices; the list of chunk c is d_items[d_offsets[c] .. d_offsets[c + 1]) */
} vrt_chunk_lists;
/* The words vrt_chunk_lists_build writes into d_stats (every other word 0). */
enum { VRT_S_LISTS_ITEMS = 8,     /* items the lists need: the sum of the list lengths, whether they fit or not */
       VRT_S_LISTS_OVERFLOW = 9   /* 1: that is more than n_items_cap; no item was written and the sentinel is set (below) */ };

/* Fills lists->d_offsets and lists->d_items for the n_objects records of d_objects (a DEVICE array, 16-byte aligned).
 *   d_stats   [VRT_NSTATS] uint64, zeroed by the callee: the VRT_S_LISTS_* words.
 * Deterministic: the same input gives the same bytes.  One wave per chunk takes the objects 64 at a time; a ballot marks the
 * boxes that meet the chunk and the population count below a lane is its slot, so the order needs neither atomics nor a sort.
 * The pass runs once to count, one workgroup sums the counts in place into d_offsets, and the pass runs again to fill: three
 * launches, n_chunks * ceil(n_objects / 64) wave iterations per pass.
 * OVERFLOW is never a wrong answer.  If the lists need more than n_items_cap items, VRT_S_LISTS_ITEMS says how many,
 * VRT_S_LISTS_OVERFLOW is 1, d_items is left alone and d_offsets[n_chunks] holds the sentinel 0xFFFFFFFF.  The two consumers
 * recognise the sentinel and walk the whole range 0 .. n_objects for every chunk: the scans' work, the scans' results.
 * MEMORY SAFETY of the consumers.  A consumer clamps every offset it reads to n_items_cap, treats an inverted pair as an
 * empty list and skips an item outside [0, n_objects), so lists that were built for another object array cannot make it read
 * outside its arguments.  What it then computes is the scan over the listed objects that exist: for lists built for a LONGER
 * array whose first n_objects records are the ones given, exactly the scan's result over those n_objects records.
 * VRT_ERR_ARG, before any HIP call: NULL lists, d_offsets or d_stats; a chunk_size that is no power of two in 8..256; dims < 1
 * or 2^24 - 2 chunks and more; an origin that is no multiple of chunk_size or a box outside +-2^30; n_items_cap < 0 or >= 2^31;
 * NULL d_items with n_items_cap > 0; n_objects < 0; NULL or misaligned d_objects with n_objects > 0.  Nothing is allocated or
 * synchronised: the call can sit on a stream next to vrt_voxelize and be captured into a hipGraph.  (A translation unit of its
 * own: a launch failure returns VRT_ERR_HIP without updating vrt_last_hip_error().) */
int vrt_chunk_lists_build(const vrt_object* d_objects, int32_t n_objects, const vrt_chunk_lists* lists,
                          uint64_t* d_stats, void* stream);

/* vrt_voxelize with the object loop of a chunk over that chunk's list only: d_voxels and d_world_table are byte for byte
 * vrt_voxelize's, for the whole box and for a d_chunk_list.  One workgroup per chunk; the list's records are staged in LDS,
 * 128 at a time; a chunk with an empty list is zeroed without touching an object.  `lists` are those of the LAST
 * vrt_chunk_lists_build over these d_objects; their origin, dims and chunk_size must equal the call's, else VRT_ERR_ARG.
 * Besides vrt_voxelize's own refusals and the lists' (above): d_objects and d_voxels must be 16-byte aligned.  A chunk index
 * of d_chunk_list outside the box is skipped.  Nothing is allocated or synchronised. */
int vrt_voxelize_lists(const vrt_object* d_objects, int32_t n_objects, const uint8_t* d_models, const uint8_t* d_remap,
                       const int64_t* origin, const int32_t* dims, int32_t chunk_size, const uint32_t* d_chunk_list,
                       int64_t n_list, uint32_t* d_world_table, uint8_t* d_voxels, const vrt_chunk_lists* lists, void* stream);

/* vrt_hit_owners with the walk over the objects replaced by a walk over ONE list: d_owners and the four VRT_S_OWNER_* words
 * are byte for byte vrt_hit_owners'.  The candidate rule is unchanged.  A candidate that counts yields the voxel c; the pass
 * searches the list of the chunk OF THE LISTS' OWN BOX that contains c, from its last item to its first.  The scene's box may
 * differ from the lists' box: if c lies outside the lists' box no listed object can hold it and the record is an orphan, as
 * it is for vrt_hit_owners with a foreign scene.  Later candidates of an ambiguous record use their own chunk's list.  One
 * lane per record; each lane walks on its own.
 * Besides vrt_hit_owners' own refusals: the lists' (above).  Nothing is allocated or synchronised, so a call may be captured
 * into a hipGraph. */
int vrt_hit_owners_lists(const vrt_scene* scene, const vrt_hit* d_hits, int64_t n_hits,
                         const vrt_object* d_objects, int32_t n_objects, const uint8_t* d_models, const uint8_t* d_remap,
                         vrt_owner* d_owners, const vrt_chunk_lists* lists, uint64_t* d_stats, void* stream);

/* ---- surfaces of hit records ---------------------------------------------------------------------------
 * HOW THE SURFACE LIES at a hit: the ray's velocity after the reference's reflection, the position one step on, what the
 * three neighbour lookups of that reflection asked and found, and a geometric normal -- what mirror, portal and
 * deferred-reflection passes that start at hit records need, and the normal image a G-buffer lacks.  The records say where
 * a ray met a voxel (vrt_hit) and whose voxel it is (vrt_owner); the reflection also depends on the chunk the ray stood in,
 * on chunk_get for a neighbour in another chunk and on that chunk's own LOD snap (init.py:92-111), which only the device
 * scene can answer.  One 64-byte record per hit record. */
typedef struct vrt_surface {   /* 64 bytes, 64-byte aligned array */
    double  vel[3];        /* the ray's velocity after the hit: normalised, reflected axes scaled (below) */
    double  next[3];       /* pos + vel * resolution: where the renderer's ray stands one step after the hit */
    int8_t  normal[3];     /* geometric normal: one component -1 or +1, or all 0 (enclosed) */
    int8_t  status;        /* 0 a surface; -1 the record is no hit (material <= 0); -2 orphan; -3 invalid input */
    uint8_t neighbour[3];  /* material id the reflection test found per axis, 0 = none (or not asked: ior == 0) */
    uint8_t resolution;    /* Frame.resolution of the chunk the ray stood in */
    uint8_t reflect;       /* bit a: init.py:106-111 reflects axis a */
    uint8_t side;          /* bit a: the neighbour asked on axis a lies at +1 (clear: -1) */
    uint8_t fetched;       /* bit a: that neighbour was outside the current chunk (chunk_get, init.py:100-102) */
    uint8_t open;          /* bit a: the incoming-side neighbour of the normal rule is empty */
    uint8_t pad[4];
} vrt_surface;
enum { VRT_SURFACE_NONE = -1, VRT_SURFACE_ORPHAN = -2, VRT_SURFACE_INVALID = -3 };   /* vrt_surface.status */
/* The words vrt_hit_surfaces writes into d_stats (every other word 0). */
enum { VRT_S_SURFACE_EXAMINED = 8,    /* records with material > 0 */
       VRT_S_SURFACE_RESOLVED = 4,    /* ... of them resolved (status 0) */
       VRT_S_SURFACE_ORPHANS = 9,     /* ... of them that no chunk of the scene accounts for: the hits came from another scene */
       VRT_S_SURFACE_AMBIGUOUS = 10,  /* records that TWO chunks explain differently; the first was taken (below) */
       VRT_S_SURFACE_INVALID = 11,    /* ... of the examined that the device refused (examined = resolved + orphans + invalid) */
       VRT_S_SURFACE_ENCLOSED = 12    /* resolved records with no open incoming side: normal (0, 0, 0) */ };

/* d_surfaces[k] describes d_hits[k], reached by d_rays[k] (DEVICE arrays of n records: d_hits 8-byte, d_rays and d_surfaces
 * 64-byte aligned).  Only `vel` of a ray record is read: the rays are what vrt_cast_rays was given, or what vrt_pixel_rays
 * writes for the frame of a vrt_first_hit (for row 0 of vrt_path_rays likewise; the incoming velocities of a row's later
 * hits are not recorded, so those are not offered).  Every field but `status` of a record with status < 0 is 0, and every
 * byte of d_surfaces is defined after the call.
 *   scene     the scene the hits were produced against: its camera table with the LOD bytes, as vrt_hit_owners takes it;
 *             d_materials is read for `ior` only.
 *   d_stats   [VRT_NSTATS] uint64, zeroed by the callee: the VRT_S_SURFACE_* words.
 * Which chunk the ray stood in: vrt_hit_owners's rule.  The candidates are the chunk containing `cell` and, for every axis on
 * which pos is a whole multiple of chunk_size, the chunk one below, in the order 000, 100, 010, 110, 001, 101, 011, 111; the
 * first that is listed, contains (cell // r) * r and holds `material` there is the CURRENT chunk: cmin its origin,
 * cmax = cmin + chunk_size (inclusive), r its resolution.  If none counts the record is an orphan (-2).  If a later candidate
 * counts too and gives another vel, reflect or neighbour, the first is taken and the record is counted in
 * VRT_S_SURFACE_AMBIGUOUS: "two chunks explain this record; the first was taken".
 * The reflection (init.py:84, 92-111), in binary64 without contraction, in this order:  v = ray.vel;  ref = max |v[a]|, and
 * v[a] /= ref if ref is neither 0 nor 1 (lib.py:310-314).  With ior of the hit's material: ior == 0 asks nothing
 * (reflect = side = fetched = 0, neighbour 0).  Otherwise direction = (ior - 0.5) * 2 and, per axis a:  p = pos with
 * p[a] = pos[a] + 1 if v[a] < direction, else pos[a] - 1;  the neighbour is read from the current chunk if cmin <= p <= cmax
 * on all three axes, otherwise (fetched bit a) from the chunk the table lists for p snapped to chunk_size, and is absent if
 * none is listed;  in either chunk it is read at (floor(p) // r') * r' with that chunk's own r', and is empty if that voxel
 * lies outside the chunk;  axis a is reflected unless a neighbour was found and its material's ior equals the hit's:
 * vel[a] = v[a] - v[a] * ior * 2.  Then next[a] = pos[a] + vel[a] * (double)r (init.py:114-116).
 * For a material of roughness 0 this is, bit for bit, the renderer's ray one step after the hit (vrt_shade_rays's end state
 * for a life that ends there).  For a ROUGH material lib.material jitters the velocity with three draws before the
 * normalisation; vel and next are then the answer for the UNJITTERED velocity.
 * The normal is this library's own definition, not the reference's (which has no normal: its reflection asks a side that
 * depends on ior).  f = cell; for every axis with v[a] != 0 the cell q = f - sgn(v[a]) * e_a is OPEN if the chunk containing
 * q is not listed, or its voxel at (q // r') * r' lies outside it, or is 0.  The normal is -sgn(v[a]) on the open axis with
 * the largest |v[a]| (ties: the lowest axis), 0 on the other two; if no axis is open the hit is ENCLOSED: normal (0, 0, 0),
 * counted in VRT_S_SURFACE_ENCLOSED.
 * The records are device data and the call does not synchronise, so each record is validated on the device.  A record with
 * material > 0 is INVALID -- status -3, counted, nothing further read for it -- when a pos or vel component is not finite,
 * when |pos[a]| >= 2^28, when cell != floor(pos), or when material > n_materials.  Every table and voxel index is checked
 * before it is used: no input makes the kernel read outside the scene's arrays.
 * n = 0 only zeroes the statistics; n >= 2^32 is VRT_ERR_ARG, as is a NULL or misaligned array; more than 2^28 records are
 * split into launches.  Every argument is checked before any HIP call; nothing is allocated or synchronised, so a call may
 * be captured into a hipGraph.  (This entry point lives in a translation unit of its own: a launch failure returns
 * VRT_ERR_HIP without updating vrt_last_hip_error().) */
int vrt_hit_surfaces(const vrt_scene* scene, const vrt_hit* d_hits, const vrt_cast_ray* d_rays, int64_t n,
                     vrt_surface* d_surfaces, uint64_t* d_stats, void* stream);

/* ---- object physics ------------------------------------------------------------------------------------
 * One physics tick of the reference, `for obj in objects: obj.update(cam_pos)` (init.py:469-470; Object.update_physics,
 * data.py:495-560), on the resident models: voxel-against-voxel collision between objects read through their quarter
 * turns, velocity transfer between physical objects, friction, elasticity, gravity and the velocity bounds.
 * One body per object of the world, in the world's order -- the physics order.  192 bytes, 8-byte aligned.  The embedded
 * vrt_object is what vrt_voxelize would be given for the object (model, shape, turns, remap); its mins and maxs are the
 * body's box and the kernel keeps them current: after the call they are ceil(pos) - half and floor(pos) + half of a body
 * that moved.  Unlike vrt_voxelize the physics reads the box INCLUSIVE of maxs (data.py:463-464, 532-534). */
typedef struct vrt_body {
    double  pos[3];          /* in, out: the centre */
    double  vel[3];          /* in, out */
    double  weight;          /* in: Object.weight */
    vrt_object object;       /* in; mins and maxs in, out */
    int32_t half[3];         /* in: trunc(sprite size / 2), Object.size */
    int32_t visible_before;  /* in: Object.visible as the last tick left it */
    int32_t visible_now;     /* in: what Object.update makes of it this tick, from the position at the start of the tick */
    int32_t awake;           /* in: that distance <= dist_move */
    int32_t physics;         /* in: Object.physics */
    int32_t has_sprite;      /* in: 0: no model; such a body neither moves nor is met */
    int32_t steps;           /* out: moves tried (iterations of data.py:500) */
    int32_t blocked_steps;   /* out: ... of them blocked */
    int32_t contacts;        /* out: pairs of solid voxels that met, over all steps */
    int32_t transfers;       /* out: velocity transfers to physical neighbours */
    int32_t moved;           /* out: 1 if the position changed (Object.move set redraw) */
    int32_t status;          /* out: 0 stepped; -1 skipped (not visible, asleep, not physical); -3 refused */
    int64_t rim;             /* in: offset in d_models of the plane [size.y][size.z] of model bytes at x = size.x, -1: empty (below) */
    int32_t pad[2];          /* vrt_physics_run ORs into pad[0]: 1 = some tick moved the body, 2 = some tick changed its visibility; vrt_physics_run_anim also 4 = some tick's anim_update changed the frame at its turn */
} vrt_body;
enum { VRT_BODY_SKIPPED = -1, VRT_BODY_REFUSED = -3 };   /* vrt_body.status */
typedef struct vrt_physics_params {
    double gravity, friction, friction_air, min_velocity, max_velocity;   /* settings of the [PHYSICS] section */
} vrt_physics_params;
/* The words vrt_physics_tick writes into d_stats (every other word 0). */
enum { VRT_S_PHYSICS_BODIES = 8,      /* bodies stepped (status 0) */
       VRT_S_PHYSICS_REFUSED = 9,     /* bodies the device refused (status -3) */
       VRT_S_PHYSICS_STEPS = 10,      /* steps of all bodies */
       VRT_S_PHYSICS_BLOCKED = 11,    /* ... of them blocked */
       VRT_S_PHYSICS_CONTACTS = 12,
       VRT_S_PHYSICS_TRANSFERS = 13,
       VRT_S_PHYSICS_CAPPED = 14      /* bodies whose step loop was ended by the iteration cap (below) */ };
/* ... and the two more that vrt_physics_tick_draws writes. */
enum { VRT_S_PHYSICS_RNG_INVALID = 7, /* 1 if the index word of d_rng was above 624: the tick did nothing */
       VRT_S_PHYSICS_DRAWS = 15       /* random.random() calls of the tick */ };
#define VRT_PHYSICS_MAX_VEL 1024       /* |vel|_inf above this: refused */
#define VRT_PHYSICS_MAX_HALF 1024      /* half or a box extent beyond 2 * this + 1: refused */
#define VRT_PHYSICS_STEP_CAP (3 * (VRT_PHYSICS_MAX_VEL + 2))

/* The tick is a sequential chain by the reference's semantics: body k meets the positions bodies 0..k-1 have just taken and
 * the velocity they have just handed it, and the steps of one body follow each other.  So the call is ONE launch of ONE
 * workgroup of 1024 threads that walks the bodies in array order and synchronises with workgroup barriers only; the width
 * goes to the work inside a step -- the slab of world voxels the body would enter, times the bodies whose boxes meet it.
 * Another body j is met by body k if it is visible -- visible_now for j < k, visible_before for j > k: Object.update refreshes
 * an object's flag immediately before its own physics -- has a sprite, was not refused, and its inclusive box meets the slab.
 * A physical one first takes vel_apply * max(0, min(1, max|vel_apply| * weight_k - weight_j)) (data.py:523-527), contact or
 * not.  Then every slab voxel asks j's model for its byte at `voxel - mins_j` through j's turns (vrt_voxelize's question;
 * positions outside the model hold nothing -- except the plane at model x = size.x, `rim`: the reference's import mirrors x as
 * size.x - x (data.py:287), so a file's x = 0 column lands there, outside the model vrt_voxelize reads, and the inclusive box
 * test above reaches it; the default mod's cubes rest on such voxels); if that material is solid, body k's own model is asked at `voxel - mins_k -
 * vel_dir` through k's turns; two solid voxels are a contact: the step is blocked and
 * friction += f_j * f_k * params.friction, elasticity += e_j * e_k * params.friction, evaluated left to right in binary64
 * without contraction and ADDED IN THE REFERENCE'S ORDER, bodies -> x -> y -> z (contacts are compacted in that order and one
 * lane adds them: a tree reduction gives other low bits).
 *   d_matphys   [n_materials + 1][4] doubles by world material id: solidity, friction, elasticity, 0 (row 0 unused);
 *               d_remap[object.remap + model byte] is the id.  A material is SOLID iff solidity >= 1: `solidity >
 *               random.random()` is then always true, and for solidity <= 0 always false.  Fractional solidities need the
 *               draws in the reference's order: vrt_physics_tick_draws (below) makes them; this call makes none and treats
 *               such a material as not solid.
 *   d_stats     [VRT_NSTATS] uint64, zeroed by the callee: the VRT_S_PHYSICS_* words.
 * The bodies are device data, so each is validated on the device.  A body is REFUSED -- status -3, counted, neither moved nor
 * met, its velocity untouched -- when a pos or vel component or the weight is not finite, |pos[a]| >= 2^28, |vel[a]| > VRT_PHYSICS_MAX_VEL,
 * half[a] < 0 or > VRT_PHYSICS_MAX_HALF, its box is not 0 <= maxs - mins <= 2 * VRT_PHYSICS_MAX_HALF + 1 inside +-2^29, or
 * (with has_sprite) its model shape is not 0 <= size[a] <= 32768, its model leaves [0, models_bytes), as its rim plane if rim is not -1, or its remap
 * offset leaves [0, remap_bytes).  A remap index or material id out of range reads as "no voxel".  No input makes the kernel read
 * outside d_models, d_remap or d_matphys.  The step loop of a body ends after VRT_PHYSICS_STEP_CAP iterations at the latest,
 * which a valid body cannot reach (each step takes 1 off the largest component or clears it); a hit is counted in
 * VRT_S_PHYSICS_CAPPED.  The kernel terminates on any input.
 * n_bodies = 0 only zeroes the statistics.  VRT_ERR_ARG, before any HIP call: NULL d_stats or params, n_bodies < 0 or
 * > 2^20, NULL or misaligned (8 bytes) d_bodies or d_matphys with n_bodies > 0, negative sizes, NULL d_models with
 * models_bytes > 0 or d_remap with remap_bytes > 0, n_materials > 255, params that are not finite.  Nothing is allocated or
 * synchronised.  (A translation unit of its own: a launch failure returns VRT_ERR_HIP without updating vrt_last_hip_error().) */
int vrt_physics_tick(vrt_body* d_bodies, int32_t n_bodies, const uint8_t* d_models, int64_t models_bytes,
                     const uint8_t* d_remap, int32_t remap_bytes, const double* d_matphys, int32_t n_materials,
                     const vrt_physics_params* params, uint64_t* d_stats, void* stream);

/* The same tick with the reference's random draws: every `solidity > random.random()` of data.py:537 (once for each slab voxel
 * that holds a voxel of the neighbour) and data.py:539 (once more if that passed and the mover has a voxel there) is made from
 * the caller's MT19937 state, in the reference's order -- bodies -> x -> y -> z, across passes, bodies, steps and ticks -- so a
 * material of 0 < solidity < 1 is solid exactly where it is for the reference.  Materials of solidity >= 1 and <= 0 draw as well
 * (their draws decide nothing and move the generator on); `solidity > draw` is a binary64 comparison, so a NaN solidity fails
 * it after consuming its one draw.  A contact is (solidity_j > d1) && voxel of k && (solidity_k > d2).
 *   d_rng       625 uint32 in device memory, 4-byte aligned: random.Random.getstate()[1] -- the 624 state words, then the index
 *               of the next output in them, 0..624 (624: the state is twisted before the next output; odd values are legal: a
 *               draw takes two outputs, which may lie in two successive states).  Read at the start of the call and written
 *               back at its end: afterwards it is the state of a generator that has made the reference's draws -- CPython's
 *               lazy regeneration, so a tick that ends on a state's last word hands that state back with index 624.
 * The index is device data and is checked on the device before it is used: above 624 the tick does nothing -- every body gets
 * status -3 and zeroed `out` words, nothing moves, d_rng is left as it is -- VRT_S_PHYSICS_RNG_INVALID is 1 and
 * VRT_S_PHYSICS_REFUSED is n_bodies.  VRT_S_PHYSICS_DRAWS counts the draws.  Everything else -- records, refusals, limits,
 * statistics, VRT_ERR_ARG -- is vrt_physics_tick's; VRT_ERR_ARG also for a NULL or misaligned (4 bytes) d_rng.  One launch of one
 * workgroup, a kernel of its own (vrt_physics_tick's is unchanged); nothing is allocated or synchronised. */
int vrt_physics_tick_draws(vrt_body* d_bodies, int32_t n_bodies, const uint8_t* d_models, int64_t models_bytes,
                           const uint8_t* d_remap, int32_t remap_bytes, const double* d_matphys, int32_t n_materials,
                           const vrt_physics_params* params, uint64_t* d_stats, uint32_t* d_rng, void* stream);

/* Many ticks in one launch, the bodies resident throughout: `n_ticks` times `for obj in objects: obj.update(cam_pos)`, every tick
 * bit for bit what vrt_physics_tick gives for the flags the host would have worked out for it, with the camera optionally
 * re-attached to one body before every tick (init.py:464: cam.pos = data.player.cam_pos; data.py:614-618).
 * What the host does around vrt_physics_tick happens on the device, at the START of every tick, from the positions as they
 * are then (during a tick only a body's own physics moves it, and its flags are refreshed before its own physics runs):
 *   camera      follow >= 0 and body `follow` is not refused at this tick: cam = pos[follow] + offset, componentwise, one
 *               binary64 add each (offset: what Object.set_camera_pos adds for the body's rotation, which physics never
 *               changes).  Otherwise the camera is `cam` as passed, at every such tick.
 *   flags       for every body, refused ones included: visible_before = visible_now (what the tick before left; ON INPUT
 *               visible_now holds Object.visible and visible_before and awake are ignored), dist = math.dist(pos, cam)
 *               (vrt_dist3 of vrt_math.h), visible_now = has_sprite && dist <= dist_max + max(half), awake = dist <= dist_move.
 *   validation  every body is validated anew against vrt_physics_tick's refusal rules: what can change between ticks -- pos,
 *               vel, the box -- is judged as it is at this tick, so a body is refused (status -3, counted, neither moved nor
 *               met, its velocity untouched) exactly at the ticks at which a fresh vrt_physics_tick would refuse it.
 * Then the tick runs as vrt_physics_tick's: bodies in order, candidates compacted in order, transfers by one lane, slab voxel x
 * candidate 1024 wide, contacts added serially in the reference's order, the step cap.  It makes no random draws: a material
 * of fractional solidity is not solid, as for vrt_physics_tick.  After the call the `out` words of a body are its last tick's,
 * the three flags are as the last tick set them, and pad[0] has been OR-ed with 1 if any tick moved the body and with 2 if any
 * tick changed its visibility (the caller clears it before the first launch; vrt_physics_tick never touches it).
 * ONE launch of ONE workgroup of 1024 threads with workgroup barriers only, as vrt_physics_tick: no grid barrier, no
 * cooperative launch, nothing that waits on memory.  The launch ends in bounded time on any input: it counts WORK -- one unit
 * per body turn, per step, and per pass of 1024 tests (flag refresh, box tests, voxel tests) -- and at the first tick boundary
 * at or past run->budget it stops; VRT_S_PHYSICS_TICKS says how many ticks it did, at least one.  The caller continues with
 * another launch on the same records (n_ticks less what was done, d_trace advanced by ticks done * n_bodies): chained launches
 * leave every byte of the bodies and of the trace as one launch does, and the statistics add up.
 *   d_trace     NULL, or [n_ticks][n_bodies] vrt_body_sample, 8-byte aligned: every body after every tick.
 *   d_stats     [VRT_NSTATS] uint64, zeroed by the callee: the VRT_S_PHYSICS_* words of vrt_physics_tick as totals over the
 *               ticks done (REFUSED counts a body once for each tick that refused it), VRT_S_PHYSICS_TICKS and _WORK.
 * n_bodies = 0: nothing to do, VRT_S_PHYSICS_TICKS = n_ticks.  VRT_ERR_ARG, before any HIP call: whatever vrt_physics_tick
 * refuses, NULL run, n_ticks < 1, budget < 1, follow outside [-1, n_bodies), cam, offset, dist_max or dist_move not finite,
 * misaligned (8 bytes) d_trace.  Nothing is allocated or synchronised.  A kernel and a translation unit of its own
 * (vrt_physics_tick's and vrt_physics_tick_draws's are unchanged). */
typedef struct vrt_physics_run_params {
    double  cam[3];          /* the camera where no body is followed (or the followed one is refused) */
    double  offset[3];       /* camera = pos[follow] + offset */
    double  dist_max;        /* settings.dist_max */
    double  dist_move;       /* settings.dist_move: bodies further from the camera are asleep */
    int64_t budget;          /* work units after which the launch stops at the next tick boundary (VRT_PHYSICS_RUN_BUDGET) */
    int32_t n_ticks;
    int32_t follow;          /* index of the body that carries the camera, -1: none */
} vrt_physics_run_params;
typedef struct vrt_body_sample {   /* 104 bytes: one body after one tick */
    double  pos[3], vel[3];
    int32_t mins[3], maxs[3];
    int32_t visible;         /* visible_now of the tick */
    int32_t awake;
    int32_t out[6];          /* steps, blocked_steps, contacts, transfers, moved, status */
} vrt_body_sample;
enum { VRT_S_PHYSICS_WORK = 5,        /* work units counted (vrt_physics_run only) */
       VRT_S_PHYSICS_TICKS = 6        /* ticks done by this launch (vrt_physics_run only) */ };
/* The default budget.  A work unit costs 1.8 to 2.8 us on the MI355X (tools/bench_physics_run.py, profiles/physics_run_bench.json);
 * 25 ms -- 50 ms with a factor of two to spare -- are 9028 units at the dearest, rounded down to a power of two: a launch lasts
 * about 23 ms at the most, plus the rest of the tick in which the budget ran out. */
#define VRT_PHYSICS_RUN_BUDGET 8192
int vrt_physics_run(vrt_body* d_bodies, int32_t n_bodies, const uint8_t* d_models, int64_t models_bytes,
                    const uint8_t* d_remap, int32_t remap_bytes, const double* d_matphys, int32_t n_materials,
                    const vrt_physics_params* params, const vrt_physics_run_params* run, vrt_body_sample* d_trace,
                    uint64_t* d_stats, void* stream);

/* vrt_physics_run with the sprites animated (Sprite.anim_update, data.py:304-306, as Object.update calls it: data.py:575-582):
 * the same launch, the same tick, and at body k's turn -- after its flags are known, before its physics -- the switch of its
 * sprite's frame.  The frame is state of the SPRITE: the first body of a tick that is not refused, visible_now and awake and
 * shows sprite s switches s for every body that shows it; bodies earlier in the order have met the old frame in that tick, the
 * later ones meet the new one.  Only the switching body gets the new frame's weight; the others keep theirs.
 *   d_body_sprite  [n_bodies] index into d_sprites; negative or >= n_sprites: the body shows no animated sprite.
 *   d_sprites      [n_sprites] in, out: `frame` is the sprite's current frame, and is where the run left it afterwards.
 *   d_frames       [n_frame_rows]: frame f of sprite s is row d_sprites[s].first_row + f -- where its model and its rim plane lie
 *                  in d_models, its base in d_remap and Object.set_weight's sum for it.
 *   d_schedule     [n_ticks][n_sprites]: the frame anim_update sets at that tick (worked out by the host: CPython's float //
 *                  and % stay off the device); a value outside [0, n_frames), -1 for one, changes nothing.  A chained launch
 *                  passes the pointer advanced by ticks done * n_sprites, as it does d_trace.
 *   d_anim_trace   NULL, or [n_ticks][n_bodies] vrt_anim_sample, 8-byte aligned, advanced like d_trace.
 * The switch, when schedule[t][s] is a frame of s other than the current one: d_sprites[s].frame is set, body k takes the row's
 * weight and 4 is OR-ed into its pad[0], and all 1024 threads walk the bodies: every body that shows s gets object.model,
 * object.remap and rim from the row and is validated at once as at the start of a tick -- a row whose model, rim or remap base
 * leaves the buffers gets those bodies refused (status -3, counted) from that moment of the tick on, and nothing is read out of
 * bounds.  One work unit per 1024 bodies of such a walk.  A sprite whose rows leave [0, n_frame_rows) is never switched (the
 * tables are device memory: the kernel checks this, the entry point cannot).
 * n_sprites = 0: every byte as vrt_physics_run leaves it.  VRT_ERR_ARG, before any HIP call: whatever vrt_physics_run refuses,
 * n_sprites or n_frame_rows negative, and while n_sprites > 0: NULL d_sprites or d_schedule, NULL d_body_sprite with bodies,
 * NULL d_frames with rows, a misaligned array (4 bytes; d_frames and d_anim_trace 8).  A kernel and a translation unit of its
 * own; the three other physics kernels are unchanged. */
typedef struct vrt_anim_sprite {   /* 16 bytes */
    int32_t frame;           /* in, out: Sprite.frame */
    int32_t n_frames;
    int32_t first_row;       /* row of frame 0 in d_frames */
    int32_t pad;
} vrt_anim_sprite;
typedef struct vrt_anim_frame {    /* 32 bytes */
    int64_t model;           /* vrt_object.model of a body that shows the frame */
    int64_t rim;             /* vrt_body.rim */
    int32_t remap;           /* vrt_object.remap */
    int32_t pad;
    double  weight;          /* Object.set_weight's sum over the frame */
} vrt_anim_frame;
typedef struct vrt_anim_sample {   /* 16 bytes: one body after one tick */
    double  weight;
    int32_t frame;           /* its sprite's frame, -1 if it shows no animated sprite */
    int32_t switched;        /* 1 if this body made the switch at this tick */
} vrt_anim_sample;
int vrt_physics_run_anim(vrt_body* d_bodies, int32_t n_bodies, const uint8_t* d_models, int64_t models_bytes,
                         const uint8_t* d_remap, int32_t remap_bytes, const double* d_matphys, int32_t n_materials,
                         const vrt_physics_params* params, const vrt_physics_run_params* run, vrt_body_sample* d_trace,
                         uint64_t* d_stats, void* stream, const int32_t* d_body_sprite, vrt_anim_sprite* d_sprites,
                         int32_t n_sprites, const vrt_anim_frame* d_frames, int32_t n_frame_rows, const int32_t* d_schedule,
                         vrt_anim_sample* d_anim_trace);

/* vrt_physics_run_anim with the reference's random draws (vrt_physics_tick_draws's, made tick after tick): everything
 * Object.update does per tick -- flags, the animation switch, the physics with every `solidity > random.random()` of
 * data.py:537 and :539 in the reference's order -- for many ticks in one launch, the generator's state resident on the device
 * throughout.  vrt_physics_run_anim's arguments in its order, then:
 *   d_rng         [625] uint32, 4-byte aligned, as vrt_physics_tick_draws takes it: read when the launch starts, written back
 *                 when it ends.  A chained launch passes the same pointer: the next launch goes on where this one stopped.
 *   d_tick_draws  NULL, or [n_ticks] uint64, 8-byte aligned: the random.random() calls of each tick done; a chained launch
 *                 passes the pointer advanced by the ticks done, as it does d_trace.
 * Every draw the reference makes is made, for solidities >= 1 and <= 0 too, where the draws decide nothing and still move the
 * generator on.  A body that is refused, asleep, invisible or not physical makes none; the animation switch makes none.
 * VRT_S_PHYSICS_DRAWS is the launch's total.  An index word above 624: the launch ends before its first tick and leaves
 * bodies, trace, sprites, d_rng and d_tick_draws untouched; VRT_S_PHYSICS_RNG_INVALID is 1 and VRT_S_PHYSICS_TICKS is 0 -- the
 * one case in which a launch reports 0 ticks.  Work units: vrt_physics_run_anim's, one more per MT19937 state regenerated and
 * one more per pass of 1024 tests that walks undecided tests.
 * n_sprites = 0 and no d_anim_trace: the bodies move as vrt_physics_run's plus draws (an instance of the kernel without the
 * sprite tables).  No material of fractional solidity: the bodies move as vrt_physics_run_anim's, and the generator advances
 * by exactly the draws that decide nothing.  A chain of launches leaves every byte as one launch does: bodies, trace, per-tick
 * draw counts, sprites and d_rng.
 * VRT_ERR_ARG, before any HIP call: whatever vrt_physics_run_anim refuses, a NULL d_rng, a d_rng that is not 4-byte aligned, a
 * d_tick_draws that is not 8-byte aligned.  ONE launch of ONE workgroup of 1024 threads with workgroup barriers only; a
 * translation unit and kernels of its own: the four other physics kernels are unchanged. */
/* The default budget of a run with draws.  A work unit costs 2.0 to 3.75 us on the MI355X when the passes draw
 * (tools/bench_physics_run_draws.py, profiles/physics_run_draws_bench.json: `fluid`, whose passes regenerate four or five
 * MT19937 states each, is the dearest); 25 ms -- 50 ms with a factor of two to spare, as for VRT_PHYSICS_RUN_BUDGET -- are 6658
 * units at the dearest, rounded down to a power of two: a launch lasts about 15 ms at the most, plus the rest of the tick in
 * which the budget ran out. */
#define VRT_PHYSICS_RUN_DRAWS_BUDGET 4096
int vrt_physics_run_draws(vrt_body* d_bodies, int32_t n_bodies, const uint8_t* d_models, int64_t models_bytes,
                          const uint8_t* d_remap, int32_t remap_bytes, const double* d_matphys, int32_t n_materials,
                          const vrt_physics_params* params, const vrt_physics_run_params* run, vrt_body_sample* d_trace,
                          uint64_t* d_stats, void* stream, const int32_t* d_body_sprite, vrt_anim_sprite* d_sprites,
                          int32_t n_sprites, const vrt_anim_frame* d_frames, int32_t n_frame_rows, const int32_t* d_schedule,
                          vrt_anim_sample* d_anim_trace, uint32_t* d_rng, uint64_t* d_tick_draws);

/* Many runs in one launch: n_runs what-if copies of one world's bodies -- the same models, other positions and velocities --
 * each stepped as vrt_physics_run steps its own, bit for bit: the camera from the followed body, the flags and the validation at
 * the start of every tick, the body walk, the ordered compaction and the serial sums, the step cap, the pad[0] bits.  A run is a
 * sequential chain and takes one workgroup; runs are independent, so the call is ONE launch of n_runs workgroups of 1024 threads
 * that never communicate: no grid barrier, no cooperative launch, no atomics on memory another workgroup reads, nothing that
 * waits on memory.  d_models, d_remap and d_matphys are read-only and shared by all runs.
 *   d_bodies      [n_runs][n_bodies] in, out: run r's records as vrt_physics_run takes them.
 *   run           shared by all runs: camera, offset, follow (an index into each run's own bodies), distances, budget -- and
 *                 n_ticks, here the TOTAL of the run, not what is left of it.
 *   d_ticks_done  [n_runs] int32, 4-byte aligned, in, out: the ticks run r has behind it; 0 before the first launch.
 *   d_trace       NULL, or [n_runs][run->n_ticks][n_bodies] vrt_body_sample, 8-byte aligned, indexed by ABSOLUTE tick:
 *                 d_trace[(r * n_ticks + tick) * n_bodies + k] is body k of run r after tick `tick`.
 *   d_stats       [n_runs][VRT_NSTATS] uint64, zeroed by the callee: vrt_physics_run's words for run r's share of this launch.
 * Each workgroup counts work as vrt_physics_run does and stops at the first tick boundary at or past run->budget, or when its
 * run has n_ticks behind it; before it returns it adds the ticks it did (VRT_S_PHYSICS_TICKS, at least one) to d_ticks_done[r].
 * The caller launches again with the SAME pointers while any d_ticks_done[r] < n_ticks: a run that is already done writes zeroed
 * statistics (TICKS = 0) and touches neither its bodies nor its trace.  Chained launches leave every byte of the bodies and of
 * the trace as one launch does, and the per-run statistics add up.  Every launch ends in bounded time on any input.
 * An entry of d_ticks_done outside [0, n_ticks] is device data: the kernel treats that run as done, touches nothing of it and
 * sets VRT_S_PHYSICS_BATCH_BADTICK in its statistics; the other runs are not affected.
 * It makes no random draws and animates nothing: a material of fractional solidity is not solid, as for vrt_physics_run
 * (vrt_physics_run_batch_draws, below, is the batch with draws; a batch with a clock would need sprite tables per run).
 * n_bodies = 0: nothing to do, every run reports n_ticks done (TICKS = what was left).  VRT_ERR_ARG, before any HIP call:
 * whatever vrt_physics_run refuses, n_runs outside [1, VRT_PHYSICS_BATCH_MAX_RUNS], n_runs * n_bodies > 2^20, NULL or
 * misaligned (4 bytes) d_ticks_done, NULL d_stats, misaligned (8 bytes) d_trace.  Nothing is allocated or synchronised.  A kernel
 * and a translation unit of its own: the other physics kernels are unchanged. */
#define VRT_PHYSICS_BATCH_MAX_RUNS 4096
enum { VRT_S_PHYSICS_BATCH_BADTICK = 4 /* 1 if d_ticks_done[r] was outside [0, n_ticks]: the run was left alone (vrt_physics_run_batch only) */ };
int vrt_physics_run_batch(vrt_body* d_bodies, int32_t n_runs, int32_t n_bodies, const uint8_t* d_models, int64_t models_bytes,
                          const uint8_t* d_remap, int32_t remap_bytes, const double* d_matphys, int32_t n_materials,
                          const vrt_physics_params* params, const vrt_physics_run_params* run, int32_t* d_ticks_done,
                          vrt_body_sample* d_trace, uint64_t* d_stats, void* stream);

/* vrt_physics_run_batch with the reference's random draws: n_runs what-if copies of one world's bodies, each with a generator
 * of its own, each stepped as vrt_physics_run_draws without sprite tables (n_sprites = 0, no d_anim_trace) steps its own, bit
 * for bit -- every `solidity > random.random()` of data.py:537 and :539 made from that run's MT19937 state in the reference's
 * order.  ONE launch of n_runs workgroups of 1024 threads that never communicate: workgroup barriers only, no grid barrier, no
 * cooperative launch, no atomics on memory another workgroup reads, nothing that waits on memory.  vrt_physics_run_batch's
 * arguments in its order, with its meaning (n_ticks is the TOTAL of a run, d_trace is indexed by absolute tick), then:
 *   d_rng         [n_runs][625] uint32, 4-byte aligned: run r's generator as vrt_physics_tick_draws takes it, read when a launch
 *                 starts on run r and written back when that launch ends its share of run r.  A chained launch passes the same
 *                 pointer and goes on where the last one stopped.
 *   d_tick_draws  NULL, or [n_runs][run->n_ticks] uint64, 8-byte aligned, indexed by ABSOLUTE tick: the random.random() calls of
 *                 tick `tick` of run r.  A launch writes only the ticks it does.
 *   d_stats       [n_runs][VRT_NSTATS] uint64, zeroed by the callee: vrt_physics_run_draws's words for run r's share of this
 *                 launch -- VRT_S_PHYSICS_DRAWS, _WORK, _TICKS and the rest; none of them is word VRT_S_PHYSICS_BATCH_BADTICK (4)
 *                 or VRT_S_PHYSICS_RNG_INVALID (7).
 * Each workgroup counts the work units of vrt_physics_run_draws and stops at the first tick boundary at or past run->budget, or
 * when its run has n_ticks behind it, and adds the ticks it did to d_ticks_done[r]; the caller launches again with the SAME
 * pointers while any d_ticks_done[r] < n_ticks.  Chained launches leave every byte of the bodies, the trace, d_tick_draws and
 * d_rng as one launch does, and the per-run statistics add up.  Every launch ends in bounded time on any input.  Per run:
 *   a run that is done (d_ticks_done[r] == n_ticks) touches nothing of its own but its zeroed statistics (TICKS = 0): not its
 *     bodies, not its trace, not its d_tick_draws, and in particular not its d_rng;
 *   an entry of d_ticks_done outside [0, n_ticks] is vrt_physics_run_batch's case: the run is left alone -- bodies, trace,
 *     d_rng, d_tick_draws and the entry itself -- and VRT_S_PHYSICS_BATCH_BADTICK is 1 in its statistics; it is checked before
 *     the generator is read;
 *   an index word (d_rng[r][624]) above 624: the run is left alone -- its bodies, trace, d_rng, d_tick_draws and
 *     d_ticks_done[r] are untouched -- and VRT_S_PHYSICS_RNG_INVALID is 1 in its statistics (TICKS = 0).  The caller must not
 *     launch again for such a run: it will never advance;
 *   n_bodies == 0: every tick is done (TICKS = what was left, d_ticks_done[r] = n_ticks), the ticks left get 0 in d_tick_draws,
 *     and d_rng is untouched.
 * In each of these cases the other runs are not affected.
 * VRT_ERR_ARG, before any HIP call: whatever vrt_physics_run_batch refuses, a NULL d_rng, a d_rng that is not 4-byte aligned, a
 * d_tick_draws that is not 8-byte aligned.  Nothing is allocated or synchronised.  The default budget of a run with draws is
 * VRT_PHYSICS_RUN_DRAWS_BUDGET.  A kernel and a translation unit of its own (vrt_physics_batch_draws.hip): the other physics
 * kernels are unchanged. */
int vrt_physics_run_batch_draws(vrt_body* d_bodies, int32_t n_runs, int32_t n_bodies, const uint8_t* d_models, int64_t models_bytes,
                                const uint8_t* d_remap, int32_t remap_bytes, const double* d_matphys, int32_t n_materials,
                                const vrt_physics_params* params, const vrt_physics_run_params* run, int32_t* d_ticks_done,
                                vrt_body_sample* d_trace, uint64_t* d_stats, void* stream, uint32_t* d_rng, uint64_t* d_tick_draws);

/* The CONTACT LOG of a batch of runs: who touched whom, where, along which direction and between which materials.  A contact is
 * one execution of the block under `if self_mat and self_mat.solidity > random.random():` of Object.update_physics
 * (data.py:532-542): one slab voxel at which a solid voxel of another object faces a solid voxel of the mover -- what
 * vrt_body.contacts and VRT_S_PHYSICS_CONTACTS count.  The order of a run's log is the reference's: ticks -> bodies in physics
 * order -> steps of the body's step loop -> met bodies in array order -> x -> y -> z.  A transfer of velocity without a contact
 * is no event. */
typedef struct vrt_contact {     /* 40 bytes */
    int32_t tick;                /* absolute tick of the run, from 0 */
    int32_t mover;               /* index of the body whose step it is */
    int32_t other;               /* index of the body it met */
    int32_t step;                /* iteration of the mover's step loop in this tick, from 0 */
    int32_t voxel[3];            /* world voxel of `other` that was met; the mover's voxel is voxel - dir */
    int8_t  dir[3];              /* vel_dir of the step */
    uint8_t mat_other;           /* world material id of the other's voxel (a row of d_matphys) */
    uint8_t mat_mover;           /* world material id of the mover's voxel */
    uint8_t reserved[7];         /* 0 */
} vrt_contact;
enum { VRT_CONTACTS_VOXELS = 0, /* every contact */
       VRT_CONTACTS_PAIRS = 1   /* the first record, in the order above, of every (tick, mover, step, other): one event per touch */ };
typedef struct vrt_contact_log {
    vrt_contact*   d_records;    /* [n_runs][capacity], 8-byte aligned; may be NULL iff capacity == 0 */
    uint64_t*      d_counts;     /* [n_runs] in, out, 8-byte aligned */
    const uint8_t* d_mask;       /* [n_bodies], or NULL: every contact */
    int32_t        capacity;     /* per run, >= 0 */
    int32_t        mode;         /* VRT_CONTACTS_VOXELS or VRT_CONTACTS_PAIRS */
} vrt_contact_log;

/* vrt_physics_run_batch with a contact log per run: vrt_physics_run_batch's arguments in its order, with its meaning, then
 *   d_rng         NULL: the batch without draws, vrt_physics_run_batch's tick, in which fractional solidity is not solid;
 *                 d_tick_draws is then not looked at.  Otherwise vrt_physics_run_batch_draws's tick with its d_rng and
 *                 d_tick_draws, generator handling included: every rule stated there holds here.
 *   log           the log, read before the call returns; its arrays are device memory that stays with the caller:
 *     d_mask      one byte per body, shared by all runs: bit 0 = log contacts in which this body is the mover, bit 1 = in which it
 *                 is the other; a contact is logged iff (mask[mover] & 1) || (mask[other] & 2).  Only bits 0 and 1 are read.
 *     d_counts    run r's count: the records run r would have logged after the filters.  It is read when a launch starts on run r
 *                 and written back when that launch ends its share, so chained launches continue the log where it stood, as
 *                 d_ticks_done continues the ticks; it keeps counting past capacity.  0 before the first launch of a fresh log.
 *     d_records   record p of run r goes to d_records[r * capacity + p] iff p < capacity; later ones are counted, not stored.  A
 *                 count at or past capacity on entry stores nothing and goes on counting.
 * ONE launch of n_runs workgroups of 1024 threads that never communicate: workgroup barriers only, no grid barrier, no atomics
 * on memory another workgroup reads, nothing that waits on memory.  The tick is the restated entry point's statement for
 * statement, and the work units are counted exactly as there: a run with a log stops at the same tick boundaries and reports
 * the same statistics and d_ticks_done as the same run without one, and leaves the same bytes in its bodies, its trace, its
 * d_tick_draws and its d_rng.  After a pass's
 * contacts are compacted in order the logging lanes are ranked by the same ordered compaction and each writes its own record.
 * A run that is left alone (an entry of d_ticks_done outside [0, n_ticks], an index word of its generator above 624, or
 * already done) leaves its count and records alone; so does n_bodies == 0.
 * VRT_ERR_ARG, before any HIP call: whatever the restated entry point refuses (of d_rng: misalignment), a NULL log, capacity < 0, a
 * mode other than the two, NULL or misaligned (8 bytes) d_counts, d_records NULL with capacity > 0 or misaligned (8 bytes),
 * n_runs * capacity > 2^31 - 1.  Nothing is allocated or synchronised.  Two kernels and a translation unit of their own
 * (vrt_physics_contacts.hip): the other physics kernels are unchanged, and so is VRT_ABI_VERSION -- the change only adds. */
int vrt_physics_run_batch_contacts(vrt_body* d_bodies, int32_t n_runs, int32_t n_bodies, const uint8_t* d_models, int64_t models_bytes,
                                   const uint8_t* d_remap, int32_t remap_bytes, const double* d_matphys, int32_t n_materials,
                                   const vrt_physics_params* params, const vrt_physics_run_params* run, int32_t* d_ticks_done,
                                   vrt_body_sample* d_trace, uint64_t* d_stats, void* stream, uint32_t* d_rng, uint64_t* d_tick_draws,
                                   const vrt_contact_log* log);

/* SCRIPTED ACCELERATIONS of a batch of runs: Object.accelerate(vel) (data.py:491-492) executed between two ticks of a run, as
 * the reference's window does for its player after every object's update and mods do for jumps, thrusters, wind and kicks.  An
 * impulse (tick, body, vel) is `vel = vel + impulse` per component in binary64, done BEFORE tick `tick` begins: after every
 * body's turn of tick - 1 and before tick `tick` computes its camera, flags and validation; tick 0's come before the first tick.
 * It is unconditional: a sleeping, invisible or non-physical body, or one without a sprite, takes the velocity and keeps it
 * until something uses it up.  Several impulses on one body before one tick add in list order (the sum is not associative);
 * impulses on different bodies commute.  No rule of validation is added: a sum that leaves the limits (|vel| > 1024, not
 * finite) is refused by the tick's own check, from that tick on, in that run. */
typedef struct vrt_impulse {     /* 32 bytes */
    int32_t tick;                /* absolute tick of the run, in [0, n_ticks) */
    int32_t body;                /* index of the body, in [0, n_bodies) */
    double  vel[3];              /* what is added to its velocity */
} vrt_impulse;
typedef struct vrt_impulse_list {
    const vrt_impulse* d_impulses;  /* run r's are [d_first[r], d_first[r + 1]), 8-byte aligned; NULL iff none */
    const int32_t*     d_first;     /* [n_runs + 1], non-decreasing from 0 */
    int32_t            total;       /* d_first[n_runs] as the host knows it, <= VRT_PHYSICS_MAX_IMPULSES */
} vrt_impulse_list;
#define VRT_PHYSICS_MAX_IMPULSES (1 << 20)
enum { VRT_S_PHYSICS_IMPULSES = 0,     /* entries applied by this launch's share of the run (vrt_physics_run_batch_impulses only) */
       VRT_S_PHYSICS_IMPULSES_BAD = 1  /* entries skipped, and a bad row of d_first once (likewise) */ };

/* vrt_physics_run_batch_contacts with a list of impulses per run: its arguments in its order, with their meaning -- but `log`
 * may be NULL: no contact log, and none of its code runs -- then
 *   impulses      the list, read before the call returns; its arrays are device memory that stays with the caller and that no
 *                 launch writes.  The host is expected to sort a run's entries by tick, within a tick by body, and to keep the
 *                 call order of one body's entries at one tick (a stable sort).
 * The arrays are DEVICE DATA and the kernel trusts none of it.  Entry i of a run belongs to the largest tick in [0, n_ticks)
 * found among entries 0..i of that run (tick 0 if there is none), so every entry belongs to one tick, whatever it holds.  An
 * entry is APPLIED at the beginning of the tick it belongs to iff its tick is that tick (so: in range, and not lower than any
 * in-range tick before it), its body is in [0, n_bodies) and not lower than the body of an earlier entry of that tick that
 * passed these tests, and its three components are finite.  Every other entry is never applied and is counted in
 * VRT_S_PHYSICS_IMPULSES_BAD when its tick begins; applied ones are counted in VRT_S_PHYSICS_IMPULSES.  A row of d_first that
 * decreases, is negative or passes `total` empties that run's list and counts once in VRT_S_PHYSICS_IMPULSES_BAD, in the
 * launch that starts the run at tick 0.  Nothing outside [0, total) is read, and the kernel terminates on any input.
 * CHAINING: ticks are absolute.  A launch that starts run r at d_ticks_done[r] = s applies exactly the entries of the ticks >= s
 * that it reaches; a launch that stopped at the boundary before tick s has not applied tick s's entries.  The next launch
 * finds its place from s and the list alone -- the first entry whose tick lies in [s, n_ticks) -- and no cursor is kept in
 * memory.  Both counts are per run and per launch like the other words: their sums over a chain are those of one launch.
 * WORK grows by one unit per 1024 entries taken in a tick and by nothing in a tick without entries: a run with an empty list
 * stops at the tick boundaries of vrt_physics_run_batch_contacts (without a log: of vrt_physics_run_batch or
 * vrt_physics_run_batch_draws), reports its words and leaves its bytes.  A run that is left alone (see there) and n_bodies == 0
 * look at no entry and count none.
 * ONE launch of n_runs workgroups of 1024 threads that never communicate; the lane whose entry is the first of its body among
 * the 1024 taken together adds it and goes on alone through the following entries of that body, so equal bodies add in order
 * and different bodies in parallel, with plain vector stores and no atomics.
 * VRT_ERR_ARG, before any HIP call: whatever vrt_physics_run_batch_contacts refuses, but for a NULL log; a NULL `impulses`, a
 * NULL or misaligned (4 bytes) d_first, total < 0 or > VRT_PHYSICS_MAX_IMPULSES, d_impulses NULL with total > 0 or misaligned
 * (8 bytes).  Nothing is allocated or synchronised.  A translation unit of its own (vrt_physics_impulses.hip): the other
 * physics kernels are unchanged, and so is VRT_ABI_VERSION -- the change only adds. */
int vrt_physics_run_batch_impulses(vrt_body* d_bodies, int32_t n_runs, int32_t n_bodies, const uint8_t* d_models, int64_t models_bytes,
                                   const uint8_t* d_remap, int32_t remap_bytes, const double* d_matphys, int32_t n_materials,
                                   const vrt_physics_params* params, const vrt_physics_run_params* run, int32_t* d_ticks_done,
                                   vrt_body_sample* d_trace, uint64_t* d_stats, void* stream, uint32_t* d_rng, uint64_t* d_tick_draws,
                                   const vrt_contact_log* log, const vrt_impulse_list* impulses);

/* Window.chunk_update's selection loop (init.py:447-452) on the device: which world chunks the camera renders this
 * frame and at which LOD.  The voxel blocks stay resident at full resolution; a chunk's LOD is only the resolution
 * byte of its table entry (a Frame of resolution r holds the voxels at coordinates divisible by r, which is what the
 * kernel's lookup snaps to), so re-selecting costs one tiny kernel and no voxel traffic.
 *   d_world_table  [dims] entries slot+1 (resolution bits ignored), 0 = no voxel data in this chunk
 *   d_camera_table [dims] out: slot+1 | (lod+1)<<24 where the chunk is kept, else 0
 *   kept iff (!culling || chunk position was traversed in `prev`) (init.py:447); prev = the vrt_traversed box a
 *   previous vrt_render_tile filled (NULL or NULL keys: nothing traversed)
 *   lod = min(trunc(dist(chunk centre, cam_pos) / (dist_max / (1 + chunk_lod))), chunk_lod) (init.py:448-449),
 *   chunk centre = position + round(chunk_size / 2); dist is the value CPython's math.dist returns for the two points
 *   (the reference's vec3.distance; vrt_dist3 of vrt_math.h), bit for bit -- not sqrt(dx^2 + dy^2 + dz^2), which is an
 *   ulp off on about one input in six and a whole LOD off where dist / step lands on an integer. */
int vrt_select_chunks(const uint32_t* d_world_table, const int64_t* origin, const int32_t* dims, int32_t chunk_size,
                      const double* cam_pos, double dist_max, int32_t chunk_lod, int32_t culling,
                      const vrt_traversed* prev, uint32_t* d_camera_table, void* stream);

/* Window.draw_tile (init.py:185-190): alpha-over blit of a tile's RGBA8 window image (vrt_render_tile's d_image_u8)
 * onto the persistent RGBA8 canvas, [height][width][4] both.  d_pixels_xy: the tile's own pixels ([n_px][2]), or NULL
 * for every pixel of the window -- the same result, since a tile's other pixels are transparent.  The blend restates
 * pygame 2's ALPHA_BLEND (dst alpha 0: copy; else dC = ((dC << 8) + (sC - dC) * sA + sC) >> 8, dA = sA + dA -
 * sA * dA / 255); pygame cannot be run in the build environment, so this entry point is PARITY UNPINNED. */
int vrt_canvas_blit(uint8_t* d_canvas_rgba8, const uint8_t* d_tile_rgba8, int32_t width, int32_t height,
                    const int32_t* d_pixels_xy, int64_t n_px, void* stream);

/* Optional per-kernel timing for bench.py.  Between vrt_profile_begin() and vrt_profile_end() every kernel
 * launched by vrt_render_tile is bracketed by HIP events on its launch stream.  vrt_profile_end() waits for
 * those events (the only call in this header that blocks on the device) and returns, per kind, the summed
 * milliseconds and the launch count.  An event pair costs a frame ~12 us (measured: 37 us for the three pairs of a
 * BASELINE config 2 frame of 0.56 ms); vrt_profile_begin_kinds(1 << VRT_PROF_MARCH) times the march alone. */
enum { VRT_PROF_RNG = 0, VRT_PROF_MARCH = 1, VRT_PROF_RETRACE = 2, VRT_PROF_RESOLVE = 3, VRT_PROF_RAYGEN = 4,
       VRT_NPROF = 8 };
int vrt_profile_begin(void);
int vrt_profile_begin_kinds(uint32_t kinds);   /* bit k: time kind k */
int vrt_profile_end(double* ms, int64_t* launches);

/* Fill a packed voxel buffer with the synthetic dense volume of BASELINE config 5: edge n voxels (multiple of
 * chunk_size), centred on the world origin, all chunks present at resolution 1, slot = linear chunk index.
 * d_chunk_table: [(n/cs)^3] uint32, d_voxels: [n^3] bytes. */
int vrt_synth_volume(int32_t n, int32_t chunk_size, uint32_t* d_chunk_table, uint8_t* d_voxels, void* stream);

#ifdef __cplusplus
}
#endif
#endif
