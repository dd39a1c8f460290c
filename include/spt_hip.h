/*
 * spt_hip.h -- C ABI of the MI355X (gfx950) render loop of SimplePathTracer.
 *
 * This is the drop-in boundary.  The reference's hot path is reached through
 * two void free functions that read mutable globals and write bytes into the
 * caller-owned framebuffer g_data:
 *
 *   void RenderSegment(RenderSegmentData)       SingleThreadPathTracer.hpp:114-137
 *   void RenderSegmentTask(RenderSegmentData)   TaskBasedPathTracer.hpp:54-206
 *
 * called from RenderJob (Renderer.hpp:242-255) on up to threadCount concurrent
 * threads and from RenderImage (Renderer.hpp:304-308).  Their implicit inputs
 * are the globals of Globals.hpp:8-37 (scene SoA, viewMatrix, eyePos,
 * initColor, g_width/g_height/g_samples/g_bounces).  The functions below make
 * each of those inputs explicit; include/spt/RenderSegmentShim.hpp rebuilds the
 * two reference entry points on top of them so Renderer.hpp / Main.cpp and the
 * GL preview keep compiling unchanged.
 *
 * Plain C types only.  Every function returns an spt_status; on failure
 * spt_last_error() describes why.  A context is safe to use from several host
 * threads: its state is guarded by a lock, and concurrent render calls (the
 * reference's RenderJob threads) are rendered together: the calls that arrive while
 * one batch renders form the next (one render + one fold launch over their tiles).
 */
#ifndef SPT_HIP_H
#define SPT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPT_ABI_VERSION 11

/* Only the functions below are exported from libspt_hip.so (built with
 * -fvisibility=hidden), so several builds can be loaded side by side. */
#if defined(__GNUC__)
#define SPT_API __attribute__((visibility("default")))
#else
#define SPT_API
#endif

typedef enum spt_status {
    SPT_OK = 0,
    SPT_ERR_ARG = 1,      /* invalid argument (null pointer, bad range, ...) */
    SPT_ERR_STATE = 2,    /* scene / camera / params not set */
    SPT_ERR_HIP = 3,      /* HIP runtime error */
    SPT_ERR_NOMEM = 4,    /* allocation failed */
    SPT_ERR_NODEVICE = 5, /* no gfx950 device / bad ordinal */
    SPT_ERR_TIMEOUT = 6   /* a render-service session did not end within SPT_SVC_TIMEOUT_MS
                             (default 30 s); the message counts its unpublished jobs */
} spt_status;

/* Material ids, Definitions.hpp:7-13 (enum class Material : uint8_t). */
enum { SPT_SKYBOX = 0, SPT_REFLECTIVE = 1, SPT_REFRACTIVE = 2, SPT_DIFFUSE = 3 };

/* Render modes: which reference entry point's semantics a launch follows. */
enum {
    SPT_MODE_SEGMENT = 0,  /* RenderSegment: every sample counts, acc *= 1/spp  */
    SPT_MODE_TASK = 1      /* RenderSegmentTask: paths needing > 10 passes are
                              dropped (TaskBasedPathTracer.hpp:81) and the pixel
                              is averaged over the samples that finished (196-205) */
};

typedef struct spt_ctx spt_ctx;

#define SPT_DIAG_WORDS 26

typedef struct spt_stats {
    uint64_t samples;      /* (pixel, sample) paths completed */
    uint64_t casts;        /* FindClosestIntersectionSphere calls (rays) */
    uint64_t dropped;      /* task mode: samples dropped by the pass cap */
    uint64_t launches;     /* render-kernel launches */
    double render_ms;      /* summed device time of render-kernel launches */
    double fold_ms;        /* summed device time of resolve (fold) launches */
    double last_render_ms; /* device time of the most recent render launch */
    uint32_t grid_blocks;  /* grid of the most recent render launch (the persistent grid
                              before any launch) */
    uint32_t block_threads; /* its block size (256; 1024 for the LDS tree kernel) */
    double render_busy_ms; /* length of the union of the render launches' intervals: with
                              frames in flight on several streams launches overlap, and
                              this is the device time during which some render launch ran */
    uint64_t diag[SPT_DIAG_WORDS]; /* diagnostic build only (-DSPT_DIAG=1): wave iterations,
                              clusters entered, tree nodes tested, s_memtime cycles in
                              cast / shading / refill, (lane, cluster) pairs that may
                              pass, live lanes of entered clusters, spheres tested per
                              wave, their update branches taken (some lane passes),
                              lanes passing in those branches, branches that
                              improve some lane's winner, RaySphereIntersection
                              evaluations for live lanes (lane-tests), member pretests
                              for live lanes (lane-pretests); then, of the primary
                              batches (64 new paths of one 8x8 tile cast together):
                              iterations, tree nodes tested, spheres tested, update
                              branches taken, s_memtime cycles of their casts; the
                              cube-minus-ball sampler's calls and its cooperative rounds
                              after round 0; tree leaves entered by at most 8 and at
                              most 16 lanes; s_memtime cycles in the sampler; wave
                              iterations after the launch's items ran out (the drain)
                              and their live lanes */
    uint64_t batches;       /* batched launches of concurrent spt_render_segment[_task] calls */
    uint64_t batched_calls; /* calls rendered in them */
    /* render service (spt_service_start); the device counters above include a session's
       waves once the session has ended (spt_service_stop, spt_synchronize) */
    uint64_t svc_sessions;       /* service sessions (resident launches) started */
    uint64_t svc_jobs;           /* jobs published to them */
    uint64_t svc_watchdog_exits; /* sessions whose waves left after 0.5 s without work */
    double svc_kernel_ms;        /* summed device time of the ended sessions' launches */
    uint32_t svc_running;        /* a session is resident now */
    uint32_t svc_grid_blocks;    /* the service's grid (one block slot per CU left free) */
    uint64_t svc_flow_restarts;  /* sessions ended because a publication would have waited for
                                    an unfinished fold (ring words or counter still in use) */
    uint64_t svc_closing_restarts; /* sessions ended because a wave had raised its closing flag */
    uint32_t prim_list_blocks;   /* 8x8 pixel blocks with a primary-ray candidate list (0: lists off) */
    uint32_t prim_list_entries;  /* candidate slots over all blocks' lists (8x8 and 8x4) */
    double prim_list_build_ms;   /* host time of their last build (device time where spt_update_scene built them) */
    uint64_t prim_list_builds;   /* builds so far (a setter rebuilds the lists only when the
                                    accel tables, the camera or the frame size changed) */
    double accel_build_ms;       /* host time of the last traversal-table build + upload
                                    (spt_set_scene / cluster setters) */
    /* Added at the end of the struct with SPT_ABI_VERSION still 11: a caller compiled against
       a header without this field must be recompiled before it calls spt_get_stats, which
       writes all of this struct (8 bytes past the older one). */
    uint64_t fold_table_entries; /* entries of the fold's colour table, one per diffuse sample code of
                                    the scene at the context's depth ((jmax + 1) * slots, at most 32 MiB
                                    of 16-byte entries), built by the first launched render after the
                                    scene or the depth changed; 0: no table (it would be larger, or
                                    none built yet) and the fold decodes every sample word
                                    arithmetically, as the folds of the batched host calls and of
                                    spt_render_frame always do; member 0's on a multi-device
                                    context */
} spt_stats;

SPT_API int spt_abi_version(void);
/* Number of visible HIP devices. */
SPT_API int spt_device_count(int *count);

/* Context on one device.  Replaces nothing in the reference (its state is global);
 * it owns the device copies of Globals.hpp's scene/camera and a workspace. */
SPT_API int spt_ctx_create(int device, spt_ctx **out);
/* Context over several devices (one process driving the node's
 * GPUs).  devices[0] is member 0; a device may be listed more than once (members on
 * one device render concurrently on their own streams).  Every setter applies to all
 * members (each keeps its own copy of the scene); spt_render_frame splits the frame
 * over the members; spt_render_segment[_task] / spt_render_progressive send each
 * call (a RenderJob tile) to the member with the fewest calls in flight; the other
 * entry points (rows/assemble/samples/selftest) use member 0. */
SPT_API int spt_ctx_create_multi(const int *devices, uint32_t n, spt_ctx **out);
/* Members of ctx: on entry *n = capacity of devices (nullable), on return *n = count. */
SPT_API int spt_ctx_devices(spt_ctx *ctx, uint32_t *n, int *devices);
SPT_API void spt_ctx_destroy(spt_ctx *ctx);
/* Last error of ctx, or of the calling thread when ctx is NULL. Never NULL. */
SPT_API const char *spt_last_error(const spt_ctx *ctx);

/* Scene SoA, Globals.hpp:31-37: g_spheres (float4 per sphere, w ignored),
 * g_radii, g_colors (float4, w ignored), g_materials, g_diffuses (fuzz),
 * g_sphereNumber.  Data is copied.  The reference's uint8_t sphere index
 * (Collision.hpp:87-92) limits it to n <= 255; this build uses a 32-bit index,
 * identical for n <= 255, and accepts larger scenes as an extension. */
SPT_API int spt_set_scene(spt_ctx *ctx, const float *centers4, const float *radii, const float *colors4,
                  const uint8_t *materials, const float *fuzz, uint32_t n);
/* viewMatrix (row-major, already transposed, Renderer.hpp:321; its fourth row
 * must be zero as CreateCameraBasisMatrix makes it), eyePos and initColor
 * (Globals.hpp:21-29).  w lanes of eye/sky are ignored (0 in the reference). */
SPT_API int spt_set_camera(spt_ctx *ctx, const float view[16], const float eye[4], const float sky[4]);
/* g_width, g_height, g_samples, g_bounces (Globals.hpp:12-15) + RNG seed.
 * bounces == 0 is rejected: `while (--bounceCount && ...)` would never count
 * down (SingleThreadPathTracer.hpp:28). */
SPT_API int spt_set_params(spt_ctx *ctx, uint32_t width, uint32_t height, uint32_t spp, uint32_t bounces, uint64_t seed);
/* Hot-loop culling: small spheres are grouped into clusters of k <= 8
 * (SPT_CLUSTER_AUTO, the default: 4 for a flat cluster list, 8 for a tree)
 * whose conservative bounding test skips them exactly when no ray of a wave can
 * pass RaySphereIntersection for any member; k = 0 tests every sphere for every
 * ray (the reference's brute force).  Results are identical either way. */
#define SPT_CLUSTER_AUTO 0xFFFFFFFFu
SPT_API int spt_set_cluster_size(spt_ctx *ctx, uint32_t k);
/* Clusters are the leaves of a tree of expanded boxes (built top down by the
 * surface-area heuristic); `branching` children per inner node at most, 0 = flat list
 * of clusters under bounding spheres, SPT_TREE_AUTO (default) = a tree with 4 (scenes
 * of <= 512 spheres) or 3 children.  Trees of 64..2431 nodes are walked lane by lane
 * from LDS, up to 9000 nodes lane by lane from global memory, others by the whole
 * wave.  Results are identical for any value. */
#define SPT_TREE_AUTO 0xFFFFFFFFu
SPT_API int spt_set_cluster_tree(spt_ctx *ctx, uint32_t branching);
/* Keep `n` CUs free of render launches (0, the default: none).  A launched render then
 * runs on a stream of ctx's own whose CU mask leaves out the mask's last n bits
 * (hipExtStreamCreateWithCUMask; the driver deals mask bits out XCC first, then shader
 * engine, so n = 8 is one CU per XCC and n = 32 one per shader engine on MI355X), ordered
 * after the caller's stream and before its later work, with a persistent grid sized to
 * the CUs it may use.  For co-scheduling other work beside a render: a block that needs
 * a whole CU (RCCL's gfx950 collective kernels: 248-256 VGPRs per wave) waits for room in
 * the shader engine it is dispatched to, so it starts at once only with one free CU per
 * engine (DESIGN.md §5 "Reserved CUs": 3.1 ms vs 18.5 ms into a 19 ms render at n = 32;
 * not bench.py's default -- the multi-rank bench is faster with the render service).
 * Results are identical for any n; the render service ignores it.  n < the CU count. */
/* The drop-in's warm-up (the C++ shim calls it once, right after creating its
 * context): creates the streams of the second batch set and of the tiling read-ahead
 * now, so that the first frame does not pay for them (a HIP stream costs ~9.5 ms to
 * create on MI355X and stalls the device's other queues meanwhile), runs one small
 * device-to-host 2D copy and one host-to-device upload (the process's first of each waits
 * ~8.5 ms for the runtime's copy setup: the first frame's tile copies, the setup's list
 * upload), and lets the tiling
 * read-ahead arm at a tiling's first call (RenderImageParallelMain's first tile to arrive)
 * rather than after one whole tiling, so that the reference app's one frame per process
 * (Renderer.hpp:335-344) is rendered whole at its first tile (SPT_READAHEAD_FIRST=0: not).
 * Results unchanged; optional. */
SPT_API int spt_prepare_dropin(spt_ctx *ctx);
SPT_API int spt_set_reserved_cus(spt_ctx *ctx, uint32_t n);
/* Host-only check (no device needed): build the traversal tables for a scene and
 * verify the properties exactness rests on (every sphere once, preorder/skip
 * structure of all 8 octant layouts, each node's bounding sphere contains every
 * member below it).  *out_nodes (nullable) = tree nodes per layout. */
SPT_API int spt_accel_check(const float *centers4, const float *radii, uint32_t n, uint32_t cluster_k,
                            uint32_t branching, uint32_t *out_nodes);
/* Host-only check (no device needed): the primary-ray candidate lists (DESIGN.md §4.2
 * item 6) a context builds for this scene (default traversal shape), camera (view as
 * spt_set_camera) and frame size.  counts[4] = {list entries, slots, blocks per row,
 * lists on}.  blocks8 (2 * ceil(width/8) * ceil(height/8) words) and blocks4
 * (2 * ceil(width/8) * ceil(height/4)) receive {first entry, count} per block (count
 * 0xFFFFFFFF: the block walks the tree), slot_ids the entries and slot_orig the sphere
 * index of every slot (0xFFFFFFFF: dummy); each nullable, the last two of capacity cap.
 * max_count: longer lists walk (the contexts use 24, SPT_PRIM_MAX). */
SPT_API int spt_prim_lists_check(const float *centers4, const float *radii, uint32_t n, const float view[16],
                                 const float eye[4], uint32_t width, uint32_t height, uint32_t max_count,
                                 uint32_t *blocks8, uint32_t *blocks4, uint32_t *slot_ids, uint32_t *slot_orig,
                                 uint32_t cap, uint32_t *counts);

/* ---- scene updates ------------------------------------------------------
 * An animation frame moves spheres and the camera by a little.  spt_update_scene applies the
 * new centres and / or the new camera without the setters' host work: the traversal tables
 * are refit -- their shape (slot order, leaves, tree topology, sibling order) stays, every
 * bound and pretest constant is recomputed with the builder's arithmetic -- and the
 * primary-ray candidate lists are built by a kernel on the device. */
typedef struct spt_update_info {
    double refit_ms;           /* host: refit + upload (0 when no centres were given) */
    double lists_ms;           /* device time of the list build (events), 0 if none */
    uint32_t list_blocks, list_entries;  /* as spt_stats' prim_list_blocks / prim_list_entries */
    uint32_t lists_on_device;  /* 1: built by the kernel; 0: the host builder was used, or lists are off */
    uint32_t refit;            /* 1: centres were applied */
    /* why lists_on_device is 0 (SPT_UPDATE_LISTS_*; 0 when it is 1) */
    uint32_t lists_reason;
} spt_update_info;
#define SPT_UPDATE_LISTS_DEVICE 0u     /* built on the device */
#define SPT_UPDATE_LISTS_OFF 1u        /* no lists for this state: camera or params not set, a tree walked
                                          lane by lane, SPT_PRIM_LISTS=0 */
#define SPT_UPDATE_LISTS_CAMERA 2u     /* host builder's call: non-finite camera or a frame beyond 65 535 */
#define SPT_UPDATE_LISTS_SLOTS 3u      /* more slots than the kernel's list holds (2 048, or
                                          SPT_PRIM_DEVICE_SLOTS if lower): host builder */
#define SPT_UPDATE_LISTS_UNCHANGED 4u  /* nothing the lists depend on changed: kept */
/* centers4 (nullable: the spheres stay): n float4 in the order of spt_set_scene (w ignored);
 * radii, colours, materials and fuzz are unchanged.  view / eye (nullable together: the camera
 * stays; the sky stays either way) as spt_set_camera.  Needs a scene (SPT_ERR_STATE before
 * spt_set_scene); the lists are built once camera and params are set.  A centre that is not
 * finite is SPT_ERR_ARG with the context unchanged (build puts such spheres in the always-
 * list, which a refit cannot); finite centres of any size are accepted.  Afterwards every
 * entry point behaves, bit for bit, as after spt_set_scene with the moved centres and
 * spt_set_camera with the new camera; only the culling (the tree's shape is the old scene's)
 * and so the speed may differ.  Like the setters: not from a progress callback, ends a
 * render-service session, applies to every member of a multi-device context (info: member
 * 0's), waits for the device before it writes a table. */
SPT_API int spt_update_scene(spt_ctx *ctx, const float *centers4, const float view[16], const float eye[4],
                             spt_update_info *info /* nullable */);
/* Host-only check (no device needed): build the traversal tables for (centers_a, radii) as
 * spt_accel_check does; with refit != 0 refit them to centers_b (spt_update_scene's refit)
 * and verify the result against centers_b as spt_accel_check verifies a build, with refit
 * == 0 return the build for centers_a itself (centers_b unused).  counts[4] = {slots, node
 * records of all 8 layouts (pads included), nodes per layout, leaves}.  The tables, each
 * nullable: slots4 (4 floats per slot), orig and kpre (one word per slot), nodes (8 words
 * per record: the 32-byte record as stored) of capacities cap_slots slots / cap_nodes
 * records; *pre_cm the scene bound of the member pretest. */
SPT_API int spt_accel_refit_check(const float *centers_a, const float *centers_b, const float *radii, uint32_t n,
                                  uint32_t cluster_k, uint32_t branching, int refit, uint32_t *counts, float *slots4,
                                  uint32_t *orig, float *kpre, uint32_t *nodes, float *pre_cm, uint32_t cap_slots,
                                  uint32_t cap_nodes);
/* The context's candidate lists in spt_prim_lists_check's output format: which = 0 the lists
 * its device holds now (read back; runs are at fixed strides when the device built them,
 * packed when the host did), which = 1 the host builder's lists for the context's current
 * tables, camera and frame (built now, on the host; the context's own lists stay).  counts[3]
 * = 0: lists off.  Member 0 of a multi-device context. */
SPT_API int spt_prim_lists_read(spt_ctx *ctx, int which, uint32_t *blocks8, uint32_t *blocks4, uint32_t *slot_ids,
                                uint32_t *slot_orig, uint32_t cap, uint32_t *counts);

/* Engine of the render loop (results are bit-identical either way):
 * SPT_ENGINE_MEGAKERNEL (default) -- one persistent kernel, per-lane state machines;
 * SPT_ENGINE_WAVEFRONT -- RenderSegmentTask's material-queue design
 *   (TaskBasedPathTracer.hpp:54-193): one launch per sample batch whose blocks are
 *   queue workers -- each block casts its ray queue, sorts the rays by material in LDS
 *   (ballot/prefix), shades them and compacts the survivors in place, pass after pass.
 *   Queue lengths never leave the device: the host issues the launch and reads nothing
 *   back. */
enum { SPT_ENGINE_MEGAKERNEL = 0, SPT_ENGINE_WAVEFRONT = 1 };
SPT_API int spt_set_engine(spt_ctx *ctx, int engine);
/* Upper bound of the per-sample workspace (default 16 GiB).  Larger frames are
 * rendered in sample batches folded in order. */
SPT_API int spt_set_workspace(spt_ctx *ctx, uint64_t bytes);

/* ---- drop-in entry points (host memory, blocking) ----------------------------
 * Render pixels [yBegin,yEnd) x [xBegin,xEnd).  Concurrent calls on one context run
 * on the GPU together (up to 8 in flight per device; SPT_HOST_SLOTS lowers it).
 * rgba_out (nullable): region-local row-major float4 per pixel = the reference's
 *   pixelColor after `*= 1/g_samples` (the value WritePixel receives).
 * g_data (nullable): full-frame width*height*3 bytes; the region's pixels are
 *   written at g_size - ((g_width - x)*3 + y*g_width*3) exactly as
 *   io::WritePixel does (IOHelpers.hpp:17-22), other bytes untouched. */
SPT_API int spt_render_segment(spt_ctx *ctx, uint32_t yBegin, uint32_t yEnd, uint32_t xBegin, uint32_t xEnd,
                       float *rgba_out, uint8_t *g_data);
/* The whole frame (RenderImage, Renderer.hpp:304-308, over every device of the
 * context): member r of n renders the interleaved row strips r, r+n, ... (strip =
 * the largest of 8/4/2/1 rows that deals the strips evenly) into a compact tile;
 * member 0 pulls the tiles over xGMI (peer copies), scatters them into the frame and
 * writes rgba_out (nullable, width*height float4, row-major) and g_data (nullable,
 * the reference layout).  Pixels are keyed per (pixel, sample), so the frame is
 * bit-identical for any member count.  In task mode a non-square frame
 * (RenderImage's RenderSegmentTask({0, H, 0, W}) aliases pixels across rows,
 * TaskBasedPathTracer.hpp:103,186) is split by ranges of its colorIndex instead: member
 * r folds outputs [r L, (r + 1) L) from the rows holding their sources.  Blocking. */
SPT_API int spt_render_frame(spt_ctx *ctx, int mode, float *rgba_out, uint8_t *g_data);
/* Progressive RenderSegment / RenderSegmentTask (the preview of RenderImageParallelMain,
 * Renderer.hpp:257-302): the region is rendered in passes of pass_spp samples; after
 * each pass rgba_out / g_data (either nullable) hold the render at the samples done so
 * far -- bit-identical to a render with g_samples = samples_done, since samples are
 * keyed per (pixel, sample) -- and cb(user, samples_done) runs on the calling thread
 * (nullable; a nonzero return stops the render there).  The last pass is the full
 * render.  cb runs with the context unlocked: it may read stats, pin buffers or render
 * elsewhere, but setters of the same context called from it fail with SPT_ERR_STATE. */
/* Page-lock a caller-owned host buffer -- typically g_data (Globals.hpp:19, malloc'd)
 * -- so the per-call device-to-host copy of the render is a direct DMA and the GL
 * thread's UpdateTexture (Renderer.hpp:157-164) reads the same pinned bytes.
 * Idempotent per pointer; spt_unpin_host releases it (spt_ctx_destroy releases all). */
SPT_API int spt_pin_host(spt_ctx *ctx, void *ptr, size_t bytes);
SPT_API int spt_unpin_host(spt_ctx *ctx, void *ptr);
typedef int (*spt_progress_fn)(void *user, uint32_t samples_done);
SPT_API int spt_render_progressive(spt_ctx *ctx, int mode, uint32_t yBegin, uint32_t yEnd, uint32_t xBegin,
                                   uint32_t xEnd, uint32_t pass_spp, float *rgba_out, uint8_t *g_data,
                                   spt_progress_fn cb, void *user);
SPT_API int spt_render_segment_task(spt_ctx *ctx, uint32_t yBegin, uint32_t yEnd, uint32_t xBegin, uint32_t xEnd,
                            float *rgba_out, uint8_t *g_data);

/* ---- device-resident entry point (asynchronous) -------------------------------
 * Rows y in [yBegin,yEnd) with ((y - yBegin) / strip) % parts == part, columns
 * [xBegin,xEnd) -- the interleaved row-strip tiling used to split a frame over
 * GPUs (parts = world size, part = rank; parts = 1 for a plain rectangle).
 * d_rgba (nullable): device float4 per local pixel, local order (row k of the
 *   owned rows, then x).  d_rgb8 (nullable): device full frame in g_data layout.
 * stream: a hipStream_t; NULL is HIP's default (null) stream, as for any HIP
 * call.  Launches are ordered on that stream only.  Returns after enqueueing;
 * pair with spt_synchronize or the caller's stream sync.  Each distinct stream
 * (up to 4 per context) gets its own workspace, so renders enqueued on different
 * streams may be in flight together: the next frame's blocks then fill the GPU
 * while the previous frame's last paths drain. */
SPT_API int spt_render_rows_async(spt_ctx *ctx, int mode, uint32_t yBegin, uint32_t yEnd, uint32_t strip, uint32_t parts,
                          uint32_t part, uint32_t xBegin, uint32_t xEnd, void *d_rgba, void *d_rgb8, void *stream);
/* ---- render service ----------------------------------------------------------------
 * spt_service_start: from now on the renders of spt_render_rows_async, spt_render_frame
 * and the unbatched host calls are jobs of a resident render service instead of launches
 * of their own.  One launch of the service kernel (a "session") stays on the device and
 * renders the jobs in the order they are published: claims of the next job fill the CUs
 * while the last paths of the previous one drain, so consecutive frames, rank shares and
 * sample batches pay no launch ramp and tail each.  A job's fold waits for its completion
 * counter on the caller's stream (hipStreamWaitValue32); results are bit-identical to the
 * launched renders.  Sessions start on the first job and end on spt_service_stop,
 * spt_synchronize, a setter, a render the service does not take (lane-walk trees,
 * spt_render_samples, the wavefront engine, jobs over half the slot ring: 1/16 of device
 * memory within [4, 16] GiB), when a
 * publication would have to wait for an unfinished fold (the ring wrapped onto words a
 * fold still reads; the next session's launch waits for it instead), or when its waves
 * have gone idle: a session's waves may leave after 0.5 s without work -- only through
 * a handshake with the host, so no job is ever published to a session that left -- and a
 * device-wide synchronisation (hipDeviceSynchronize, torch.cuda.synchronize) therefore
 * waits at most that long.  spt_service_stop drains and ends the session and turns the
 * service off.  Every host wait for a session is bounded (SPT_SVC_TIMEOUT_MS, default
 * 30 s: SPT_ERR_TIMEOUT). */
SPT_API int spt_service_start(spt_ctx *ctx);
/* full != 0: sessions take every block slot (SPT_SVC_FULL_GRID's setting, for callers that
 * end their sessions themselves and need no kernel of their own beside one); 0: one slot
 * per CU left free (the default).  SPT_ERR_STATE while a session runs. */
SPT_API int spt_service_set_full_grid(spt_ctx *ctx, uint32_t full);
SPT_API int spt_service_stop(spt_ctx *ctx);

/* Number of rows the (yBegin, yEnd, strip, parts, part) map owns. */
SPT_API int spt_rows_count(uint32_t yBegin, uint32_t yEnd, uint32_t strip, uint32_t parts, uint32_t part, uint32_t *rows);
/* Scatter a gathered, rank-major stack of local float4 tiles (parts tiles of
 * max_rows*(xEnd-xBegin) pixels each, on device) into a full-frame float4
 * buffer and/or a g_data RGB8 frame.  Used by rank 0 after the RCCL gather. */
SPT_API int spt_assemble_rows_async(spt_ctx *ctx, const void *d_tiles, uint32_t max_rows, uint32_t yBegin, uint32_t yEnd,
                            uint32_t strip, uint32_t parts, uint32_t xBegin, uint32_t xEnd, void *d_frame_rgba,
                            void *d_rgb8, void *stream);
SPT_API int spt_synchronize(spt_ctx *ctx);
/* The rank-share form of RenderImage's RenderSegmentTask({0, H, 0, W}) on a NON-SQUARE
 * frame (mode TASK, W != H).  There the reference strides its colour accumulator by the
 * tile height (TaskBasedPathTracer.hpp:103,186,196-205), so pixels alias across rows and a
 * row-strip split cannot resolve them locally; the frame is split by output index instead.
 * spt_task_range: part `part` of `parts`'s outputs [i0, i1) of the frame's row-major order
 * (outputs with sources dealt evenly; the last part also takes the source-less tail,
 * which resolves to NaN / bytes 0).  spt_render_task_range_async: renders the rows
 * holding those outputs' sources and writes outputs [i0, i1) to d_rgba[0, i1 - i0)
 * (float4, device) on `stream`.  The parts' outputs end to end are the frame, which
 * spt_assemble_rows_async turns into RGBA / g_data with max_rows = H, strip 1, parts 1.
 * (spt_render_frame does the same over a multi-device context.) */
SPT_API int spt_task_range(uint32_t width, uint32_t height, uint32_t parts, uint32_t part, uint32_t *i0, uint32_t *i1);
SPT_API int spt_render_task_range_async(spt_ctx *ctx, uint32_t i0, uint32_t i1, void *d_rgba, void *stream);

/* ---- copy-engine tile transport (one process per GPU, ranks of one node) -------------
 * The alternative to distributed.py's RCCL gather of the rank tiles (Renderer.hpp:257-302's
 * tile split; DESIGN.md §5 "Round 6"): rank 0 holds nbuf gathered buffers of world tiles
 * (tile_bytes each, rank-major, the layout spt_assemble_rows_async reads) in one device
 * allocation it exports by IPC handle; rank r > 0 copies its tile into slot r of the
 * frame's buffer with an asynchronous device-to-device copy on its own stream (peer
 * memory over xGMI) and then raises its ready word; rank 0's stream waits for every ready
 * word before its assemble and raises the buffer's consumed word after it, which a
 * rank's copy into the same buffer nbuf frames later waits for.  The words live in a
 * POSIX shared-memory segment (/dev/shm) page-locked in every process: stream
 * wait/write-value packets, no host thread and no collective kernel on the path.
 * Frames are numbered 0, 1, ... identically on every rank; frame f uses buffer f % nbuf.
 * Setup: rank 0 calls spt_tiles_create(name) first; after a barrier every other rank
 * calls it with the same name, then spt_tiles_attach with rank 0's spt_tiles_handle;
 * after another barrier rank 0 may spt_tiles_unlink the name (the mappings stay).
 * Rank 0 renders its own tile into slot 0 of spt_tiles_buffer(frame) on a stream ordered
 * after its spt_tiles_release_async(frame - nbuf).  spt_tiles_destroy synchronizes the
 * device (stop the render service first: a resident session would hold it up to its idle
 * exit).  Errors: SPT_ERR_ARG (bad sizes, a segment name in use), SPT_ERR_STATE (a call for
 * the other side), SPT_ERR_HIP. */
typedef struct spt_tiles spt_tiles;
SPT_API int spt_tiles_create(spt_ctx *ctx, const char *name, uint32_t rank, uint32_t world, uint64_t tile_bytes,
                             uint32_t nbuf, spt_tiles **out);
SPT_API int spt_tiles_handle(spt_tiles *t, uint8_t handle[64]);
SPT_API int spt_tiles_attach(spt_tiles *t, const uint8_t handle[64]);
SPT_API int spt_tiles_unlink(spt_tiles *t);
SPT_API int spt_tiles_buffer(spt_tiles *t, uint64_t frame, void **d_buffer);
SPT_API int spt_tiles_send_async(spt_tiles *t, uint64_t frame, const void *d_tile, void *stream);
/* The same for `bytes` at byte `offset` of the frame's buffer instead of slot `rank` (the
 * task-range split, spt_task_range: each part's outputs at their place in the frame) */
SPT_API int spt_tiles_send_range_async(spt_tiles *t, uint64_t frame, const void *d_src, uint64_t offset,
                                       uint64_t bytes, void *stream);
SPT_API int spt_tiles_recv_async(spt_tiles *t, uint64_t frame, void *stream);
SPT_API int spt_tiles_release_async(spt_tiles *t, uint64_t frame, void *stream);
/* Give the transport up: every ready / consumed word of the shared segment set to the
 * largest value from the host, so that no rank's stream stays blocked on a wait packet
 * (then destroy it).  Used when the setup check (distributed.TileTransport.verify) fails. */
SPT_API int spt_tiles_abort(spt_tiles *t);
SPT_API void spt_tiles_destroy(spt_tiles *t);

/* Per-(pixel, sample) colors of a rectangle, host memory: out[(p*spp + s)*4 + c]
 * with p the region-local pixel.  w = 1 if the sample counts, 0 if dropped
 * (task mode).  Debug/parity aid; same kernel as the render path. */
SPT_API int spt_render_samples(spt_ctx *ctx, int mode, uint32_t yBegin, uint32_t yEnd, uint32_t xBegin, uint32_t xEnd,
                       float *out);

/* ---- ray queries: batched FindClosestIntersectionSphere (Collision.hpp:87-109) ---------
 * The closest sphere of rays the caller chooses, cast with the render's own traversals
 * of the current culling shape (spt_set_cluster_size / spt_set_cluster_tree; results are
 * identical for any): picking, object-id / depth / normal buffers.  ("Is anything between
 * these two points?" is spt_occluded_rays, below.)
 * Rays are float4 {ox, oy, oz, -} and {dx, dy, dz, -}; the w lanes are ignored.
 * idx[i] = the ORIGINAL index of ray i's closest sphere, or the scene's sphere count on a
 *   miss (what the reference returns: g_sphereNumber).
 * hit (nullable): two float4 per ray, {Px, Py, Pz, t} with P = o + d t the closest contact
 *   point (Collision.hpp:49-56) and {nx, ny, nz, ds} with n = Normalize(P - C) the contact
 *   normal (67-71) and ds the squared distance the winner was chosen by; eight +0 on a miss.
 * They need a scene only (spt_primary_hits: camera and params too), use member 0 of a
 * multi-device context, end a resident render-service session first, and leave spt_stats
 * untouched.  n == 0 is SPT_OK and touches nothing. */
/* device pointers, asynchronous on `stream` (NULL = default stream) */
SPT_API int spt_cast_rays_async(spt_ctx *ctx, const void *d_origins4, const void *d_dirs4, uint32_t n, void *d_idx,
                                void *d_hit /*nullable*/, void *stream);
/* host pointers, blocking; staged in chunks (at most 256 MiB of staging, as spt_render_samples) */
SPT_API int spt_cast_rays(spt_ctx *ctx, const float *origins4, const float *dirs4, uint32_t n, uint32_t *idx,
                          float *hit /*nullable*/);
/* (x, y, s) triples -> closest sphere of that sample's primary ray; needs camera and params.
 * The ray is the render's own: stream keyed by (seed, y * width + x, s), the u draw first,
 * viewMatrix * (-1 + 2v, -1 + 2u, 1, 0) normalized, from the eye; dirs4 (nullable) receives
 * the directions (float4, w = 0).  SPT_ERR_ARG for x >= width, y >= height or s >= spp. */
SPT_API int spt_primary_hits(spt_ctx *ctx, const uint32_t *xys, uint32_t n, uint32_t *idx, float *hit /*nullable*/,
                             float *dirs4 /*nullable*/);

/* ---- occlusion queries: any-hit with a per-ray distance limit --------------------------
 * Line of sight, shadow rays for a caller's own lighting, ambient occlusion, picking
 * through a range.  For ray i with origin o, direction d and limit L (an fp32 SQUARED
 * distance, as the reference's distanceSq):
 *   occ[i] = 1  iff  idx_i < sphere count  and  ds_i < L   (fp32 compare)
 *   occ[i] = 0  otherwise
 * with (idx_i, ds_i) exactly what spt_cast_rays returns for (o, d) (ds: the second float4's
 * w).  FindClosestIntersectionSphere returns the passing sphere of least distanceSq, so this
 * is "some sphere passes with distanceSq < L": an any-hit query, answered by a walk that is
 * bounded by L from its first node and ends at the first blocker.  Hence:
 *   - L that is NaN or <= 0 gives 0;
 *   - L >= FLT_MAX (+inf included) gives "hits anything": the reference never accepts
 *     ds == FLT_MAX as a hit;
 *   - L == ds gives 0: the compare is strict;
 *   - the answer depends on neither the culling shape nor the walk;
 *   - RaySphereIntersection's 1e-3 thresholds apply as to a cast: a ray leaving a sphere's
 *     surface outward is not blocked by that sphere.
 * flags == 0: a4 and b4 are origins and directions (float4, w ignored), L_i = limits[i],
 *   or +inf where limits is null; scale is not read.
 * SPT_OCCLUDE_SEGMENTS: a4 and b4 are end points a and b; limits must be null
 *   (SPT_ERR_ARG otherwise).  v = b - a per component in fp32, o = a, d = Normalize(v) (the
 *   shading path's), L = ((vx vx + vy vy) + vz vz) * scale without contraction;
 *   scale = 1.0f leaves it unchanged.  a == b gives L = 0 and the answer 0.  A target point
 *   b ON a sphere has ds ~ L for that sphere, either side of it by rounding: callers who mean
 *   "up to but not including the target" pass a scale slightly below 1.
 * Any other flag bit is SPT_ERR_ARG.  occ is n bytes, each 0 or 1.  As spt_cast_rays they
 * need a scene only, use member 0 of a multi-device context, end a resident render-service
 * session first, and leave spt_stats untouched.  n == 0 is SPT_OK and touches nothing. */
#define SPT_OCCLUDE_SEGMENTS 1u
/* device pointers, asynchronous on `stream` (NULL = default stream) */
SPT_API int spt_occluded_rays_async(spt_ctx *ctx, const void *d_a4, const void *d_b4, const void *d_limits /*nullable*/,
                                    uint32_t n, uint32_t flags, float scale, void *d_occ /* n bytes */, void *stream);
/* host pointers, blocking; staged in chunks (at most 256 MiB of staging, as spt_cast_rays) */
SPT_API int spt_occluded_rays(spt_ctx *ctx, const float *a4, const float *b4, const float *limits /*nullable*/,
                              uint32_t n, uint32_t flags, float scale, uint8_t *occ);

/* ---- path queries: batched TraceAndSampleColor (SingleThreadPathTracer.hpp:94-112) -----
 * The colour along rays the caller chooses: other camera models, light and irradiance
 * probes, re-shading a G-buffer's secondary rays, radiance along a picked ray.  Ray i is
 * TraceAndSampleColor(d[i], o[i], bounces) in SPT_MODE_SEGMENT semantics, through the
 * render's own casts and shading steps; the w lanes of o and d are ignored.
 * states[i] is the raw splitmix state of ray i: its draw k mixes states[i] + (k + 1) gamma
 * (Random.hpp:30-36).  The reference's own stream start is seed << 31 | seed
 * (Random.hpp:19); the render's stream of a sample after its two jitter draws is
 * spt_sample_state(seed, y * width + x, s, 2).
 * rgba[i] = the colour, w = +0; 0 for a path cut at the 1024-event specular cap, as in a
 *   render.  The sky is the initColor of spt_set_camera.
 * info (nullable): two words per ray, {casts, specular events | cut at the cap << 31}.
 * They need scene and camera (not params: the depth is `bounces`, and the scene's sample
 * codes must fit at that depth as spt_set_params demands for its own, else SPT_ERR_ARG),
 * use member 0 of a multi-device context, end a resident render-service session first, and
 * leave spt_stats untouched.  bounces == 0 is SPT_ERR_ARG (spt_set_params); n == 0 is
 * SPT_OK and touches nothing. */
/* device pointers, asynchronous on `stream` (NULL = default stream) */
SPT_API int spt_trace_rays_async(spt_ctx *ctx, const void *d_origins4, const void *d_dirs4, const void *d_states,
                                 uint32_t n, uint32_t bounces, void *d_rgba, void *d_info /*nullable*/, void *stream);
/* host pointers, blocking; staged in chunks (at most 256 MiB of staging, as spt_cast_rays) */
SPT_API int spt_trace_rays(spt_ctx *ctx, const float *origins4, const float *dirs4, const uint64_t *states, uint32_t n,
                           uint32_t bounces, float *rgba, uint32_t *info /*nullable*/);
/* host only, no device: the state of the render's keyed stream of (seed, pixel, sample)
 * after `draws` draws, fmix64(fmix64(seed) ^ (pixel << 32 | sample)) + draws * gamma */
SPT_API int spt_sample_state(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t draws, uint64_t *state);

/* ---- feature buffers: first-hit albedo, coverage, normal, depth and ids of the frame ----
 * What a denoiser or a compositor takes beside the colour, computed on the device from the
 * frame's own jittered primary rays.  For pixel (x, y) of the frame of spt_set_params, over
 * samples s = 0 .. spp - 1 in this order: the ray is the render's own (as spt_primary_hits:
 * stream keyed by (seed, y * width + x, s), from the eye), its closest sphere and hit record
 * {t, P, n} are those of spt_cast_rays, and per sample, in fp32 without contraction,
 *   cov = 1 on a hit, else 0;  nrm = n on a hit, else 0;  dep = t on a hit, else 0;
 *   alb = colors[i].xyz (raw, without the 0.5 of shading) on a DIFFUSE sphere, (1, 1, 1) on
 *     a REFLECTIVE or REFRACTIVE one, else -- a miss, or a sphere of any other material
 *     byte, which the reference's switch sends to the skybox -- the sky term
 *     (sky_c * (d.y + 1.0f)) * 0.5f per channel.  (cov, nrm and dep are geometric: such a
 *     sphere still counts as hit.)
 * Each of the eight sums starts at +0, adds its samples in order and is multiplied by
 * 1.0f / (float)spp (RenderSegment's pixelColor *= 1 / g_samples).
 * feat: 8 floats per region-local pixel p (row-major), {alb.r, alb.g, alb.b, cov} then
 *   {nrm.x, nrm.y, nrm.z, dep}.  The mean hit depth is dep / cov; the mean normal is not
 *   renormalised.
 * ids: sample 0's sphere per pixel, as idx of spt_primary_hits (the sphere count on a miss).
 * They need scene, camera and params (SPT_ERR_STATE otherwise), use member 0 of a
 * multi-device context, end a resident render-service session first, ignore the engine
 * setting and leave spt_stats and the sample workspaces untouched.  SPT_ERR_ARG for
 * yEnd > height, xEnd > width, an inverted range, strip == 0, parts == 0, part >= parts, or
 * both outputs null; an empty rectangle is SPT_OK and touches nothing.  A call is cut into
 * launches of at most 2^31 - 1 samples, each whole periods of the row map (strip x parts
 * rows); SPT_ERR_ARG where strip x (xEnd - xBegin) x spp alone exceeds that.
 * The kernels read the context's primary-ray candidate lists while they run, as renders
 * do: the setters that rewrite the lists (spt_set_camera, spt_set_params, spt_set_scene and
 * the culling setters) wait for every features call in flight on any stream, as they wait
 * for the context's renders, so the async form may be followed by a setter at once. */
/* host pointers, blocking; rectangle [yBegin,yEnd) x [xBegin,xEnd); staged in chunks of whole
 * 8-row bands (at most 256 MiB of staging, as spt_cast_rays) */
SPT_API int spt_render_features(spt_ctx *ctx, uint32_t yBegin, uint32_t yEnd, uint32_t xBegin, uint32_t xEnd,
                                float *feat /*nullable*/, uint32_t *ids /*nullable*/);
/* device pointers, asynchronous on `stream` (NULL = default stream); the row map of
 * spt_render_rows_async, outputs in local pixel order (spt_rows_count rows) */
SPT_API int spt_render_features_async(spt_ctx *ctx, uint32_t yBegin, uint32_t yEnd, uint32_t strip, uint32_t parts,
                                      uint32_t part, uint32_t xBegin, uint32_t xEnd, void *d_feat /*nullable*/,
                                      void *d_ids /*nullable*/, void *stream);

/* ---- denoiser: edge-avoiding a-trous filter guided by the feature buffers ---------------
 * An image-space filter for previews at a few samples per pixel (Dammertz et al. 2010, with
 * the Lorentzian edge-stopping weight 1 / (1 + x) in place of exp(-x): one division, no
 * transcendental, so every bit is defined).  It needs no scene, camera or params.
 * The image is width x height pixels, row-major, p = y * width + x; its borders are the
 * image's borders, whether it is a frame or a region rendered on its own.
 *   rgba  float4 per pixel, colours on the 0..255 scale of the renders; w passes through.
 *   feat  8 floats per pixel as spt_render_features writes them: {alb.r, alb.g, alb.b, cov},
 *         {nrm.x, nrm.y, nrm.z, dep}.
 * Everything is fp32, one rounding per operation written, no contraction, IEEE division.
 * Once: k_t = 1.0f / (sigma_t * sigma_t) for t in {color, albedo, normal, depth}.
 * Per pixel: z = dep / cov if cov > 0, else +0;  a = alb.rgb and n = nrm.xyz as given.
 * Level k = 0 .. levels - 1: step s = 2^k, kc_k = k_color * 4^k (exact); the level reads u
 * (rgba.rgb for k = 0, then the previous level's output) and writes u'.  For pixel p =
 * (x, y): acc = (+0, +0, +0), ws = +0; then for j = -2 .. 2 (outer), i = -2 .. 2 (inner), the
 * tap q = (x + i * s, y + j * s), skipped if outside [0, width) x [0, height), else
 *   du = u_q - u_p;  dc  = (du.r*du.r + du.g*du.g) + du.b*du.b
 *   da = a_q - a_p;  d_a = (da.r*da.r + da.g*da.g) + da.b*da.b
 *   dn = n_q - n_p;  d_n = (dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z
 *   dz = z_q - z_p;  d_z = dz*dz
 *   X  = (dc*kc_k + d_a*k_albedo) + (d_n*k_normal + d_z*k_depth)
 *   w  = (h[|i|] * h[|j|]) / (1.0f + X),  h = {0.375f, 0.25f, 0.0625f}
 *   if !(w > 0) skip the tap (NaN and 0 both skip)
 *   acc.c = acc.c + w * u_q.c (c = r, g, b);  ws = ws + w
 * u'_p.c = acc.c / ws if ws > 0, else u'_p = u_p.  The output is the last level's u' and
 * rgba_p.w.  A pixel with a non-finite colour or feature passes through unchanged and is
 * skipped by its neighbours, so non-finite values never spread.
 * out_rgb8 (nullable): the output as a g_data frame of its own width x height, pixel (x, y)
 * at 3 * ((height - 1 - y) * width + x), each channel io::WritePixel's byte of the output.
 * Each sigma must be > 0; +inf switches its term off.  levels is 1..8.
 * Scratch: the caller's, so calls on different streams share no state:
 * spt_denoise_scratch_bytes gives min(levels - 1, 2) float4 planes of width x height (the
 * ping-pong between levels; 0 for one level), host only, no device.
 * They use member 0 of a multi-device context, end a resident render-service session first
 * and leave spt_stats and the sample workspaces untouched.  SPT_ERR_ARG, before anything is
 * launched and with the outputs untouched, for a null context or input, both outputs null,
 * levels outside 1..8, a sigma that is NaN or <= 0, width x height >= 2^31, a null scratch
 * where spt_denoise_scratch_bytes is not 0, or an output that overlaps rgba, feat or the
 * scratch.  width == 0 or height == 0 is SPT_OK and touches nothing. */
SPT_API int spt_denoise_scratch_bytes(uint32_t width, uint32_t height, uint32_t levels, uint64_t *bytes);
/* device pointers, asynchronous on `stream` (NULL = default stream) */
SPT_API int spt_denoise_async(spt_ctx *ctx, uint32_t width, uint32_t height, const void *d_rgba, const void *d_feat,
                              float sigma_color, float sigma_albedo, float sigma_normal, float sigma_depth,
                              uint32_t levels, void *d_out_rgba /*nullable*/, void *d_out_rgb8 /*nullable*/,
                              void *d_scratch, void *stream);
/* host pointers, blocking; allocates and frees its own device buffers */
SPT_API int spt_denoise(spt_ctx *ctx, uint32_t width, uint32_t height, const float *rgba, const float *feat,
                        float sigma_color, float sigma_albedo, float sigma_normal, float sigma_depth,
                        uint32_t levels, float *out_rgba /*nullable*/, uint8_t *out_rgb8 /*nullable*/);

/* ---- sample moments: per-pixel mean, second moment and variance of the samples' luminance
 * Where a frame is still noisy, from the sample words every render leaves on the device.
 * The call is a SPT_MODE_SEGMENT render of the region: rgba_out and g_data receive exactly
 * what spt_render_segment writes, bit for bit, and spt_stats counts it as the render it is.
 * For pixel p, c_s is the colour of sample s as the fold decodes it (the value
 * spt_render_samples returns).  Everything is fp32, one rounding per operation written, no
 * contraction; the sums start at +0 and run over s = 0 .. spp - 1 in that order:
 *   L_s = (c_s.r * 0.2126f + c_s.g * 0.7152f) + c_s.b * 0.0722f
 *   s1 = s1 + L_s;  s2 = s2 + L_s * L_s
 *   inv = 1.0f / (float)spp;  m1 = s1 * inv;  m2 = s2 * inv
 *   d = m2 - m1 * m1;  var = d < 0 ? +0 : d                  (NaN stays NaN)
 *   mom[p] = {m1, m2, var, (float)spp}                        float4, local pixel order
 * var is the population variance of the samples' luminance; var / spp is the variance of
 * the pixel mean, which spt_denoise_var uses.  The sum-of-squares form loses bits where all
 * samples are nearly equal (m2 and m1 * m1 cancel: var is then 0 or a few ulps of m2, not
 * the true small variance); spt_denoise_var's var_floor is there for that.
 * The region has to fit in one sample batch of the workspace (spt_set_workspace), as for
 * spt_render_samples: SPT_ERR_ARG otherwise, and nothing is rendered.  They need scene,
 * camera and params (SPT_ERR_STATE otherwise) and use member 0 of a multi-device context.
 * SPT_ERR_ARG for a null mom, yEnd > height, xEnd > width, an inverted range, strip == 0,
 * parts == 0 or part >= parts; an empty rectangle is SPT_OK and touches nothing. */
/* host pointers, blocking; rectangle [yBegin,yEnd) x [xBegin,xEnd) */
SPT_API int spt_render_moments(spt_ctx *ctx, uint32_t yBegin, uint32_t yEnd, uint32_t xBegin, uint32_t xEnd,
                               float *rgba_out /*nullable*/, uint8_t *g_data /*nullable*/, float *mom);
/* device pointers, asynchronous on `stream` (NULL = default stream); the row map and local
 * pixel order of spt_render_rows_async (d_rgb8: the full frame, g_data layout) */
SPT_API int spt_render_moments_async(spt_ctx *ctx, uint32_t yBegin, uint32_t yEnd, uint32_t strip, uint32_t parts,
                                     uint32_t part, uint32_t xBegin, uint32_t xEnd, void *d_rgba /*nullable*/,
                                     void *d_rgb8 /*nullable*/, void *d_mom, void *stream);

/* ---- variance-guided denoiser: the a-trous filter with its colour term normalised by the
 * variance of the pixel means (after Schied et al. 2017, SVGF, without the temporal part).
 * Everything in "denoiser" above holds, with these changes.
 *   mom  float4 per pixel as spt_render_moments writes it; z = var and w = spp are read.
 * k_color = 1.0f / (sigma_color * sigma_color) at every level (not scaled by 4^k):
 * sigma_color counts standard deviations, and the variance shrinks from level to level.
 * Per pixel once: g_p = mom_p.z / mom_p.w, one IEEE division; a quotient that is not finite
 * is taken as NaN (an infinite g would leave X finite).  Each level reads (u, g) and
 * writes (u', g').  For each tap, dc, d_a, d_n and d_z as above, then
 *   vn = var_floor + (g_p + g_q)
 *   X  = ((dc * k_color) / vn + d_a * k_albedo) + (d_n * k_normal + d_z * k_depth)
 *   w  = (h[|i|] * h[|j|]) / (1.0f + X);  if !(w > 0) skip the tap
 *   acc.c = acc.c + w * u_q.c;  ws = ws + w;  gacc = gacc + (w * w) * g_q
 * u'_p.c = acc.c / ws and g'_p = gacc / (ws * ws) if ws > 0, else both pass through.
 * Output: the last level's u' with rgba_p.w in the w lane; out_var (nullable), one float per
 * pixel: the last level's g'; out_rgb8 as above.  A non-finite colour, feature or g at the
 * centre makes X NaN: the pixel passes through and its neighbours skip it.
 * var_floor must be finite and > 0.  Scratch is what spt_denoise_scratch_bytes gives (g
 * rides in the w lane of the planes).  Argument errors as for spt_denoise, and: a null mom,
 * a var_floor that is not finite or <= 0, an out_var that overlaps an input, the scratch or
 * another output, an output that overlaps mom. */
/* device pointers, asynchronous on `stream` (NULL = default stream) */
SPT_API int spt_denoise_var_async(spt_ctx *ctx, uint32_t width, uint32_t height, const void *d_rgba, const void *d_feat,
                                  const void *d_mom, float sigma_color, float sigma_albedo, float sigma_normal,
                                  float sigma_depth, float var_floor, uint32_t levels, void *d_out_rgba /*nullable*/,
                                  void *d_out_rgb8 /*nullable*/, void *d_out_var /*nullable*/, void *d_scratch,
                                  void *stream);
/* host pointers, blocking; allocates and frees its own device buffers */
SPT_API int spt_denoise_var(spt_ctx *ctx, uint32_t width, uint32_t height, const float *rgba, const float *feat,
                            const float *mom, float sigma_color, float sigma_albedo, float sigma_normal,
                            float sigma_depth, float var_floor, uint32_t levels, float *out_rgba /*nullable*/,
                            uint8_t *out_rgb8 /*nullable*/, float *out_var /*nullable*/);

/* ---- adaptive sampling: stop converged 8x8 tiles, keep sampling the rest
 * A render whose sample count varies over the image.  The keyed stream per (pixel, sample)
 * makes it well defined: a pixel that stops after n samples equals that pixel of a plain
 * render at spp = n, bit for bit, as spt_render_progressive's passes do.
 * Parameters.  base_spp >= 1, step_spp >= 1, max_spp >= base_spp; tol >= 0, or +inf;
 * lum_floor finite and >= 0.
 * Scope.  SPT_MODE_SEGMENT only; one rectangle [yBegin, yEnd) x [xBegin, xEnd) of the frame
 * of spt_set_params, with no row map.  The context's own spp is not read; its width, height,
 * bounces and seed are.
 * Tiles.  The tiles are the region's 8x8 tiles anchored at (xBegin, yBegin), row-major,
 * ragged at the right and bottom edges.  All pixels of a tile always have the same sample
 * count n.
 * State per pixel.  acc (3 floats), s1, s2, all starting at +0.  c_s is the colour of sample
 * s as the fold decodes it, L_s as in "sample moments".  Sample s of a pixel is added as
 *   acc.c = acc.c + c_s.c;  s1 = s1 + L_s;  s2 = s2 + L_s * L_s
 * in sample order; fp32, one rounding per operation written, no contraction.
 * Passes.  Pass 0 gives every tile samples [0, base_spp).  After a pass in which the active
 * tiles reached n samples, for each pixel of an active tile:
 *   inv = 1.0f / (float)n;  m1 = s1 * inv;  m2 = s2 * inv
 *   d = m2 - m1 * m1;  var = d < 0 ? +0 : d           (NaN stays NaN)
 *   e = var * inv                                      (variance of the pixel mean)
 *   r = (m1 + lum_floor) * tol;  thr = r * r
 *   unconverged = e > thr                              (NaN compares false: such a pixel counts as converged)
 * A tile stays active iff n < max_spp and any of its pixels is unconverged.  The next pass
 * gives every active tile samples [n, n + min(step_spp, max_spp - n)); n is therefore
 * launch-uniform over the active tiles.  A tile that has gone inactive never returns.  The
 * loop ends when no tile is active.  With tol = +inf every tile stops at base_spp; with
 * tol = 0 exactly the tiles with some var > 0 run to max_spp.
 * Outputs.  Each pixel's outputs are written when its tile goes inactive, with that n:
 *   rgba_out  {acc.r * inv, acc.g * inv, acc.b * inv, +0}: what spt_render_segment writes at
 *             spp = n, on bits
 *   g_data    io::WritePixel's bytes of that colour, in the reference layout; other bytes are
 *             left untouched
 *   mom       {m1, m2, var, (float)n}, float4 in local pixel order: the layout
 *             spt_denoise_var reads; mom.w is the spp map
 *   info      (nullable, 2 x uint64) total samples rendered, and passes run
 * Limits and errors.  A pass's sample words must fit one sample batch of the workspace: at
 * most 2^31 - 1 items, within spt_set_workspace; the calls check the largest pass their
 * parameters allow (every tile, the longest pass) before anything is launched: SPT_ERR_ARG
 * otherwise, and nothing is rendered.  SPT_ERR_STATE without scene, camera or params.
 * SPT_ERR_ARG, with every output untouched, for a null mom together with null rgba_out and
 * g_data, a bad rectangle, and parameters outside the ranges above, NaN included.  An empty
 * rectangle is SPT_OK and touches nothing.
 * Behaviour.  The calls use member 0 of a multi-device context, end a resident service
 * session first (as the moments do) and ignore the engine setting: the passes are batched
 * launches of the megakernel.  spt_stats counts them as the renders they are: samples, casts,
 * one launch per pass.
 * Known limit.  A tile whose first base_spp samples all agree stops there, even if a later
 * sample would have differed (a small bright feature every early sample missed): base_spp is
 * the guard.  Activity does not spread to neighbouring tiles. */
/* host pointers, blocking */
SPT_API int spt_render_adaptive(spt_ctx *ctx, uint32_t yBegin, uint32_t yEnd, uint32_t xBegin, uint32_t xEnd,
                                uint32_t base_spp, uint32_t step_spp, uint32_t max_spp, float tol, float lum_floor,
                                float *rgba_out /*nullable*/, uint8_t *g_data /*nullable*/, float *mom /*nullable*/,
                                uint64_t *info /*nullable*/);
/* device pointers (d_rgb8: the full frame, g_data layout; info: host memory), on `stream`
 * (NULL = default stream).  Not fully asynchronous, hence the name: which tiles a pass
 * renders decides its launch's grid and item count, so the host waits on `stream` once per
 * pass for the plan's counts -- and with it for whatever was queued on `stream` before the
 * call.  It returns with the last pass's fold enqueued and info written. */
SPT_API int spt_render_adaptive_dev(spt_ctx *ctx, uint32_t yBegin, uint32_t yEnd, uint32_t xBegin, uint32_t xEnd,
                                    uint32_t base_spp, uint32_t step_spp, uint32_t max_spp, float tol, float lum_floor,
                                    void *d_rgba /*nullable*/, void *d_rgb8 /*nullable*/, void *d_mom /*nullable*/,
                                    uint64_t *info /*nullable*/, void *stream);

/* ---- temporal accumulation: reproject the last frame's colour and moments ---------------
 * The temporal part of Schied et al. 2017 (SVGF): each pixel's first hit is reprojected into
 * the previous frame, the history found there is blended with this frame by sample counts,
 * and the result is the next frame's history.  It needs no scene, camera or params; the
 * cameras are arguments.  The library holds no state: the caller keeps (out_rgba, out_mom,
 * feat, ids) and the camera as the next frame's history.
 * The image is width x height pixels, row-major, p = y * width + x.
 *   rgba  float4 per pixel, as the renders write it; w passes through.
 *   mom   float4 per pixel as spt_render_moments and spt_render_adaptive write it: {m1, m2,
 *         var, n}; n is the sample count.
 *   feat  8 floats per pixel as spt_render_features writes them: {alb.rgb, cov}, {nrm.xyz, dep}.
 *   ids   one uint32 per pixel as spt_render_features writes it: sample 0's sphere.
 *   hist_rgba, hist_mom, hist_feat, hist_ids  the same four of the previous frame (hist_rgba
 *         and hist_mom: a previous call's outputs, or a first frame's own rgba and mom); all
 *         four, or all NULL (no history: prev_view and prev_eye are then not read).
 *   out_mom has mom's layout, the one spt_denoise_var reads: {m1, m2, var, n'}; n' is the
 *         accumulated sample count and may be fractional.
 * Everything is fp32, one rounding per operation written, no contraction, IEEE division and
 * square root.  M is view, E is eye, Ep is prev_eye, Minv = spt_temporal_inverse(prev_view).
 * Per pixel p = (x, y):
 *   z   = dep / cov if cov > 0, else +0                   (the same for history pixels: zq)
 *   vx  = -1.0f + 2.0f * ((float)x / (float)height)       (the render's own: x over the height,
 *   vy  = -1.0f + 2.0f * ((float)y / (float)width)         y over the width; the jitter is
 *                                                          uniform(-1, 1), so the pixel's centre
 *                                                          is at integer x, y)
 *   r_i = (M[4i] * vx + M[4i+1] * vy) + M[4i+2]           i = 0, 1, 2
 *   d   = Normalize(r)                                    (the render's: r / sqrt(|r|^2), lane-wise)
 *   cov > 0:  P = E + d * z;  w = P - Ep;  L = sqrtf((w.x*w.x + w.y*w.y) + w.z*w.z)
 *   else:     w = d                                       (the sky: a point at infinity, it
 *                                                          follows the rotation only)
 *   q_i = (Minv[3i] * w.x + Minv[3i+1] * w.y) + Minv[3i+2] * w.z
 *   a = q.x / q.z;  b = q.y / q.z
 *   fx = ((a + 1.0f) * 0.5f) * (float)height;  fy = ((b + 1.0f) * 0.5f) * (float)width
 *   static rule: if the nine used entries of view and prev_view (rows 0..2 x columns 0..2) and
 *     the xyz of eye and prev_eye all compare equal (==), then fx = (float)x, fy = (float)y and
 *     q.z counts as positive (the arithmetic above returns the pixel's own place only to
 *     within a few 1e-6).
 *   history is sought iff q.z > 0 && fx > -1 && fx < width && fy > -1 && fy < height   (NaN fails)
 *   x0 = floorf(fx);  tx = fx - x0;  y0 = floorf(fy);  ty = fy - y0
 *   taps, j outer, i inner, i, j in {0, 1}: the tap pixel t = (x0 + i, y0 + j),
 *     wt = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty)
 *   a tap is taken iff: t lies inside the image;  wt > 0;  hist_mom_t.w > 0;  hist_rgba_t.rgb
 *     and hist_mom_t.x, .y, .w are finite;  hist_ids_t == ids_p;
 *     tol_normal == +inf, or with dn = hist_nrm_t - nrm_p:
 *       (dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z <= tol_normal;
 *     cov_p > 0 is false, or tol_depth == +inf, or with dz = zq_t - L, lim = tol_depth * L:
 *       dz*dz <= lim*lim
 *   a taken tap adds, all sums starting at +0 and written acc = acc + wt * v:
 *     ws += wt;  hc.c += wt * hist_rgba_t.c;  h1 += wt * hist_mom_t.x;  h2 += wt * hist_mom_t.y;
 *     hn += wt * hist_mom_t.w
 *   ws > 0:  hc.c /= ws;  h1 /= ws;  h2 /= ws;  nh = fminf(hn / ws, max_history);  nc = mom_p.w
 *            n' = nh + nc;  alpha = nc / n'
 *            out.c = hc.c + (rgba_p.c - hc.c) * alpha;  m1 = h1 + (mom_p.x - h1) * alpha;
 *            m2 = h2 + (mom_p.y - h2) * alpha;  dd = m2 - m1 * m1;  var = dd < 0 ? +0 : dd
 *            out_rgba_p = {out.rgb, rgba_p.w};  out_mom_p = {m1, m2, var, n'}
 *   else:    out_rgba_p = rgba_p;  out_mom_p = mom_p      (bits and all)
 * The outputs are the inputs, bit for bit, where no history is given, where any of the
 * pixel's rgba.rgb, its four mom lanes or its eight feat lanes is not finite, and where
 * mom_p.w > 0 is false.
 * tol_normal and tol_depth must be >= 0 (+inf switches the test off); max_history must be
 * > 0 (+inf: no cap).  They use member 0 of a multi-device context, end a resident
 * render-service session first and leave spt_stats and the sample workspaces untouched.
 * SPT_ERR_ARG, before anything is launched and with the outputs untouched, for a null
 * context, input (view and eye too) or output, some but not all history pointers null, a
 * tolerance that is NaN or negative, a max_history that is NaN or not > 0, with a history a
 * null prev_view or prev_eye or a prev_view that spt_temporal_inverse rejects, width x
 * height >= 2^31, or an output that overlaps any input or the other output.  width == 0 or
 * height == 0 is SPT_OK and touches nothing. */
/* host only, no device: the fp32 inverse of view's upper-left 3x3 (rows 0..2, columns 0..2;
 * row 3 and column 3 are not read), computed in double and rounded once per entry, row-major;
 * SPT_ERR_ARG for a non-finite entry or a determinant that is not finite and != 0 */
SPT_API int spt_temporal_inverse(const float view[16], float inv9[9]);
/* device pointers, asynchronous on `stream` (NULL = default stream); the cameras are read
 * before the call returns */
SPT_API int spt_temporal_async(spt_ctx *ctx, uint32_t width, uint32_t height, const void *d_rgba, const void *d_mom,
                               const void *d_feat, const void *d_ids, const float view[16], const float eye[4],
                               const void *d_hist_rgba /*nullable*/, const void *d_hist_mom /*nullable*/,
                               const void *d_hist_feat /*nullable*/, const void *d_hist_ids /*nullable*/,
                               const float prev_view[16] /*nullable*/, const float prev_eye[4] /*nullable*/,
                               float tol_normal, float tol_depth, float max_history, void *d_out_rgba, void *d_out_mom,
                               void *stream);
/* host pointers, blocking; allocates and frees its own device buffers, as spt_denoise does */
SPT_API int spt_temporal(spt_ctx *ctx, uint32_t width, uint32_t height, const float *rgba, const float *mom,
                         const float *feat, const uint32_t *ids, const float view[16], const float eye[4],
                         const float *hist_rgba /*nullable*/, const float *hist_mom /*nullable*/,
                         const float *hist_feat /*nullable*/, const uint32_t *hist_ids /*nullable*/,
                         const float prev_view[16] /*nullable*/, const float prev_eye[4] /*nullable*/, float tol_normal,
                         float tol_depth, float max_history, float *out_rgba, float *out_mom);
/* ---- temporal accumulation under moving spheres -------------------------------------------
 * The same call with a motion table: the spheres are uniformly coloured, so a rigid motion is
 * a translation of the centre and a change of radius (a rotation is invisible).
 *   motion  n_spheres records of 8 floats, 32 bytes each, {C.x, C.y, C.z, r, Cp.x, Cp.y, Cp.z,
 *           rp}: this frame's centre and radius, then the previous frame's; indexed by the
 *           sphere index that ids carries.  The caller keeps the spheres' count and order the
 *           same across the two frames; the call cannot check that.  A device table is 16-byte
 *           aligned, as every other device array of the call.
 * Everything under "temporal accumulation" above stands, but for the lines that form w, L and
 * the static rule.  With hit = cov > 0, id = ids_p and P = E + d * z as there, and
 * {C, r, Cp, rp} = motion[id]:
 *   mv = hit && id < n_spheres && !(C.x == Cp.x && C.y == Cp.y && C.z == Cp.z && r == rp)
 *   mv:   s = rp / r                                       (IEEE division)
 *         u = P - C;  Pp_i = Cp_i + u_i * s                (the product rounded, then the sum)
 *         history is not sought unless Pp.x, Pp.y, Pp.z are all finite
 *         w = Pp - Ep;  L = sqrtf((w.x*w.x + w.y*w.y) + w.z*w.z)
 *   !mv:  w, L as above (P - Ep on a hit, d on the sky)
 *   static rule: it applies to a pixel iff the cameras compare equal as above and !mv for
 *     that pixel (Cp + (P - C) does not return P in fp32, hence "unmoved" is a rule too).
 * A pixel with !mv -- the sky, an id >= n_spheres (the miss sentinel, or any other value), a
 * sphere whose record did not change -- gets spt_temporal's output, bit for bit; so does every
 * pixel of a table in which nothing moved, and of n_spheres == 0 (the table is then not read
 * and may be NULL).  No record is read for id >= n_spheres.  A record with r == 0, a
 * non-finite entry or radii of opposite sign has no case of its own: s or Pp is not finite and
 * the pixel passes through, or the taps fail their tests.  The id, normal and depth tests are
 * the same: the normal does not change under a translation and a positive scale, and the depth
 * test compares zq with the new L.
 * Errors, service, statistics, workspaces and member 0 as for spt_temporal; SPT_ERR_ARG as
 * well for n_spheres > 0 with a null table and for an output that overlaps the table. */
SPT_API int spt_temporal_motion_async(spt_ctx *ctx, uint32_t width, uint32_t height, const void *d_rgba,
                                      const void *d_mom, const void *d_feat, const void *d_ids, const float view[16],
                                      const float eye[4], const void *d_hist_rgba /*nullable*/,
                                      const void *d_hist_mom /*nullable*/, const void *d_hist_feat /*nullable*/,
                                      const void *d_hist_ids /*nullable*/, const float prev_view[16] /*nullable*/,
                                      const float prev_eye[4] /*nullable*/, const void *d_motion /*nullable*/,
                                      uint32_t n_spheres, float tol_normal, float tol_depth, float max_history,
                                      void *d_out_rgba, void *d_out_mom, void *stream);
/* host pointers, blocking; the table is staged with the images */
SPT_API int spt_temporal_motion(spt_ctx *ctx, uint32_t width, uint32_t height, const float *rgba, const float *mom,
                                const float *feat, const uint32_t *ids, const float view[16], const float eye[4],
                                const float *hist_rgba /*nullable*/, const float *hist_mom /*nullable*/,
                                const float *hist_feat /*nullable*/, const uint32_t *hist_ids /*nullable*/,
                                const float prev_view[16] /*nullable*/, const float prev_eye[4] /*nullable*/,
                                const float *motion /*nullable*/, uint32_t n_spheres, float tol_normal, float tol_depth,
                                float max_history, float *out_rgba, float *out_mom);

SPT_API int spt_get_stats(spt_ctx *ctx, spt_stats *out);
SPT_API int spt_reset_stats(spt_ctx *ctx);

/* ---- input producers (SceneGenerators.hpp, Math.hpp) -------------------------
 * GenerateSpheres (SceneGenerators.hpp:6-66) and InitSpheres (68-133) driven by
 * splitmix(seed) (Random.hpp:19) instead of the clock; capacity in spheres. */
SPT_API int spt_scene_generate_random(uint32_t seed, uint32_t capacity, float *centers4, float *radii, float *colors4,
                              uint8_t *materials, float *fuzz, uint32_t *n_out);
/* GenerateSpheres with its row loop (SceneGenerators.hpp:32) run to z < z_end instead of
 * 20 (z_end = 20 is spt_scene_generate_random): BASELINE.json's "~500-sphere" RTIOW scene
 * with the reference's placement rule and draw order (z_end 37.5: 488 spheres, seed 1). */
SPT_API int spt_scene_generate_random_rows(uint32_t seed, float z_end, uint32_t capacity, float *centers4, float *radii,
                                           float *colors4, uint8_t *materials, float *fuzz, uint32_t *n_out);
SPT_API int spt_scene_init_reference(uint32_t seed, float *centers4, float *radii, float *colors4, uint8_t *materials,
                             float *fuzz, uint32_t *n_out);
/* Stress scene for the >255-sphere extension (BASELINE config 5): the four big
 * spheres of GenerateSpheres plus n-4 small spheres on a jittered grid. */
SPT_API int spt_scene_generate_stress(uint32_t seed, uint32_t n, float *centers4, float *radii, float *colors4,
                              uint8_t *materials, float *fuzz);
/* Transpose(CreateCameraBasisMatrix(eye, lookAt, up)), Math.hpp:198-231. */
SPT_API int spt_camera_basis(const float eye[4], const float look_at[4], const float up[4], float view_out[16]);

/* io::SaveImage (IOHelpers.hpp:24-27) without stb: writes g_data (width x height,
 * comp = g_stride = 3 bytes per pixel, row 0 first) as the 24-bit BMP that
 * stbi_write_bmp(path, width, height, 3, g_data) writes: 54-byte header, rows
 * from the last to the first, BGR, each row zero-padded to 4 bytes. */
SPT_API int spt_save_bmp(const char *path, uint32_t width, uint32_t height, uint32_t comp, const uint8_t *data);

/* ---- numerics self-test ------------------------------------------------------
 * Runs the device primitives the render path relies on over n inputs and
 * writes SPT_SELFTEST_COLS floats per input: a/b, sqrtf(a),
 * glibc's powf(a, 5) and powf(c, 5) restated, powf(a, 2), the refraction scalar
 * r*a - sqrt(1 - r*r*(1 - a*a)) (r = 1/1.5; -1e30 under total reflection), uniform(-1,1)
 * of bits, u8 of a, Normalize({a, b, c}) (3 floats), c/a, uniform(-0.5,0.5) and
 * uniform(0,1) of bits, with c the float whose bit pattern is bits; then c and a
 * halved j times as the fold rebuilds a diffuse sample (j = (bits * 2654435761) >> 23
 * mod 301; spt_kernels.hip halve_n). */
#define SPT_SELFTEST_COLS 16
SPT_API int spt_selftest_numerics(spt_ctx *ctx, const float *a, const float *b, const uint32_t *bits, uint32_t n,
                          float *out);

#ifdef __cplusplus
}
#endif
#endif
