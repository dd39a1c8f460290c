// spt_internal.h -- kernel launch interface shared by spt_kernels.hip and the host side (spt_host.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spt_hip.h"
#include "spt_codes.h"

namespace spt {

// Row map of a launch: rows y in [y0, y1) with ((y - y0) / strip) % parts == part.
struct RowMap {
    uint32_t y0, y1, strip, parts, part;
    uint32_t x0, width;  // columns [x0, x0 + width)
};

__host__ __device__ inline uint32_t row_of(const RowMap &m, uint32_t lr)
{
    uint32_t blk = lr / m.strip;
    return m.y0 + (blk * m.parts + m.part) * m.strip + (lr - blk * m.strip);
}

__host__ __device__ inline uint32_t rows_owned(const RowMap &m)
{
    if (m.y1 <= m.y0) return 0;
    uint32_t h = m.y1 - m.y0;
    uint32_t period = m.strip * m.parts;
    uint32_t full = h / period, rem = h % period;
    uint32_t r = full * m.strip;
    uint32_t start = m.part * m.strip;
    if (rem > start) r += (rem - start < m.strip) ? rem - start : m.strip;
    return r;
}

// Pixel of the q-th item of one sample in a region of `rows` x `width` pixels
// whose items run through 8x8 tiles (row-major tiles, row-major inside a tile;
// ragged tiles at the right and bottom edges).  A wave's consecutive items then
// cover a compact patch instead of a 64-pixel row strip, so its rays start close
// together and cull together.  Bijective on [0, rows*width).
__host__ __device__ inline void tile_pixel(uint32_t q, uint32_t width, uint32_t rows, uint32_t &lr, uint32_t &col)
{
    const uint32_t band = (q / width) >> 3;
    const uint32_t h = rows - (band << 3) < 8u ? rows - (band << 3) : 8u;
    const uint32_t qb = q - band * 8u * width;
    const uint32_t ft = width >> 3, wr = width & 7u;
    uint32_t row, c;
    if (h == 8u) {
        const uint32_t t = qb >> 6;
        if (t < ft) {
            row = (qb >> 3) & 7u;
            c = (t << 3) | (qb & 7u);
        } else {
            const uint32_t e = qb - (ft << 6);
            row = e / wr;
            c = (ft << 3) + (e - row * wr);
        }
    } else {
        const uint32_t th = h << 3;
        const uint32_t t = qb / th;
        if (t < ft) {
            const uint32_t e = qb - t * th;
            row = e >> 3;
            c = (t << 3) | (e & 7u);
        } else {
            const uint32_t e = qb - ft * th;
            row = e / wr;
            c = (ft << 3) + (e - row * wr);
        }
    }
    lr = (band << 3) + row;
    col = c;
}

// FastDiv / fast_div (division by a launch constant): spt_codes.h

// row_of with the strip division by multiply-shift (div_strip = FastDiv(m.strip))
__host__ __device__ inline uint32_t row_of_fast(const RowMap &m, uint32_t lr, const FastDiv &div_strip)
{
    const uint32_t blk = fast_div(lr, div_strip);
    return m.y0 + (blk * m.parts + m.part) * m.strip + (lr - blk * m.strip);
}

// The sampler's dealing of a wave's 64 lanes to its np (1..64) pending lanes
// (coop_ball_vector, spt_path.h): with q = 64 / np and rem = 64 - q * np, pending ranks
// below rem get q + 1 consecutive lanes and the others q, so every lane works and the
// trial counts differ by at most one.  A rank's lanes are contiguous: its segment of the
// acceptance ballot is one shift of the 64-bit mask.  np is wave-uniform, so its rule
// is one scalar load from a 65-entry constant table (no division anywhere): `below`
// has bit p set when lane p + 1 starts a rank's segment, so the rank a lane helps is
// the count of set bits below the lane.
struct DealRule {
    uint64_t below;
    uint32_t q, rem;
};
constexpr DealRule make_deal_rule(uint32_t np)
{
    DealRule r{0ull, 0u, 0u};
    if (np == 0u || np > 64u) return r;
    r.q = 64u / np;
    r.rem = 64u - r.q * np;
    uint32_t start = 0;
    for (uint32_t k = 0; k < np; ++k) {
        if (start > 0u) r.below |= 1ull << (start - 1u);
        start += r.q + (k < r.rem ? 1u : 0u);
    }
    return r;
}
struct DealTable {
    DealRule e[65];
    constexpr DealTable() : e{}
    {
        for (uint32_t np = 0; np <= 64u; ++np) e[np] = make_deal_rule(np);
    }
};
alignas(16) static constexpr DealTable kDealTable{};  // a rule is one 16-byte scalar load
// first lane and lane count of pending rank `rank` (< np)
__host__ __device__ inline uint32_t deal_start(const DealRule &r, uint32_t rank)
{
    return rank * r.q + (rank < r.rem ? rank : r.rem);
}
__host__ __device__ inline uint32_t deal_count(const DealRule &r, uint32_t rank)
{
    return r.q + (rank < r.rem ? 1u : 0u);
}
// the pending rank `lane` helps and its trial offset within that rank's lanes
__host__ __device__ inline void deal_lane(const DealRule &r, uint32_t lane, uint32_t &rank, uint32_t &tt)
{
#ifdef __HIP_DEVICE_COMPILE__
    rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(r.below >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)r.below, 0u));
#else
    rank = (uint32_t)__builtin_popcountll(r.below & ((1ull << lane) - 1ull));
#endif
    tt = lane - deal_start(r, rank);
}

// (sample, pixel) of the q-th item of a batch of S samples over a region of
// `rows` x `width` pixels, items ordered [8-row band][8-column tile][sample]
// [pixel in tile] (ragged tiles at the right and bottom edges).  A claim of
// consecutive items then stays inside one 8x8 tile across several samples, so a
// wave's rays start close together whatever the claim size.  Full tiles use
// shifts; only edge tiles divide.  Bijective on [0, rows*width*S) (host test).
// div_band = FastDiv(8*width*S) (unused when rows < 8), div_tile = FastDiv(64*S).
__host__ __device__ inline void ts_item(uint32_t q, uint32_t width, uint32_t rows, uint32_t S, const FastDiv &div_band,
                                        const FastDiv &div_tile, uint32_t &sl, uint32_t &lr, uint32_t &col)
{
    // 8*width*S <= rows*width*S < 2^31 whenever rows >= 8; a single band otherwise
    const uint32_t band = rows >= 8u ? fast_div(q, div_band) : 0u;
    const uint32_t h = rows - (band << 3) < 8u ? rows - (band << 3) : 8u;
    const uint32_t qb = q - band * 8u * width * S;
    const uint32_t ft = width >> 3, wr = width & 7u;
    const uint32_t ti = h * 8u * S;  // items of a full-width tile of this band
    uint32_t e, wt, c0;
    if (h == 8u) {
        const uint32_t t = fast_div(qb, div_tile);
        if (t < ft) {
            e = qb - t * 64u * S;
            sl = e >> 6;
            const uint32_t pix = e & 63u;
            lr = (band << 3) + (pix >> 3);
            col = (t << 3) + (pix & 7u);
            return;
        }
        e = qb - ft * ti;
        wt = wr;
        c0 = ft << 3;
    } else {
        const uint32_t t = qb / ti;
        wt = t < ft ? 8u : wr;
        e = qb - (t < ft ? t : ft) * ti;
        c0 = (t < ft ? t : ft) << 3;
    }
    sl = e / (h * wt);
    const uint32_t pix = e - sl * h * wt;
    const uint32_t row = pix / wt;
    lr = (band << 3) + row;
    col = c0 + (pix - row * wt);
}

// Inverse of ts_item for one pixel: the item index (= slot) of sample 0 of local pixel
// (lr, col) and the step between its consecutive samples.  Slots are stored in item
// order, so a claim's paths write one contiguous run of slots; the fold reads sample s
// of a pixel at q0 + s * step (64 consecutive slots for the 64 pixels of a full 8x8 tile).
__host__ __device__ inline void ts_slot_base(uint32_t lr, uint32_t col, uint32_t width, uint32_t rows, uint32_t S,
                                             uint32_t &q0, uint32_t &step)
{
    const uint32_t band = lr >> 3;
    const uint32_t h = rows - (band << 3) < 8u ? rows - (band << 3) : 8u;
    const uint32_t ft = width >> 3, wr = width & 7u;
    const uint32_t t = col >> 3;
    const uint32_t tc = t < ft ? t : ft;  // full-width tile, or the ragged right one
    const uint32_t wt = t < ft ? 8u : wr;
    q0 = band * 8u * width * S + tc * h * 8u * S + (lr - (band << 3)) * wt + (col - (tc << 3));
    step = h * wt;
}

// Sample codes (code_word, word_code, diffuse_code, ...) and the colour table's indexing:
// spt_codes.h

constexpr uint32_t kMaxGroup = 16;     // sphere-table padding granule (>= SPT_GROUP)
constexpr uint32_t kClusterSlots = 8;  // max members per cluster = slots of a tree leaf
constexpr uint32_t kFlatLeafSlots = 4; // slots of a flat-list leaf holding <= 4 members
// Flat-list line test (spt_path.h find_closest): the 1e-4 |Cb-o|^2 margin is folded
// in by scaling the expanded |Cb-o|^2 by kFlatScale = 1 - 1e-4; nodes store
// kFlatScale |Cb|^2.
constexpr double kFlatScale = 1.0 - 1e-4;
// Tree nodes are boxes expanded by kBoxS (|o| + Bm) on every side (Bm >= max |C| + r
// over the node's members): a ray whose member test passes comes within
// sqrt(r^2 + 2.6e-6 X^2) <= r + 1.6125e-3 X of the member's centre, X = |C - o|
// <= |o| + Bm; the rest of the margin covers the slab arithmetic.
// The node stores kBoxS Bm in its box, the lane adds kBoxS |o|.
constexpr double kBoxS = 1.63e-3;
// Reciprocal of a direction component: |d_i| is raised to at least 2^-20 first (no
// inf/NaN in the slab arithmetic; sound by the margin argument of DESIGN.md §4.4).
constexpr float kBoxMinDir = 0x1p-20f;
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;  // AccelNode::slot of inner nodes
constexpr uint32_t kMiss = 0xFFFFFFFFu;    // Hit::idx when no sphere was hit

// Hot-loop traversal tables (spt_accel.cpp).
struct AccelView {
    const float4 *slots;    // {cx, cy, cz, r*r} in traversal order (always groups, then clusters)
    const uint32_t *orig;   // original sphere index per slot
    const void *nodes;      // AccelNode[8][n_nodes + 1]: per-octant preorder layouts (spt_accel.h)
    uint32_t always_groups, n_nodes;
    uint32_t tree;        // 0: flat cluster list (every node a leaf), 1: tree with inner nodes
    uint32_t leaf_slots;  // slots per leaf: kFlatLeafSlots or kClusterSlots
    const float *kpre;    // member pretest constant K' per slot (spt_accel.h)
    float pre_cm;         // >= max |C| + r over the cluster members
};

// Primary-ray candidate lists (round 5): for every 8x8 and 8x4
// pixel block of the frame, the slots a primary ray of the block -- from the eye, through
// any pixel of the block with any jitter -- can pass RaySphereIntersection for (a
// conservative cone test with the member test's fp reach, spt_accel.cpp
// build_prim_lists).  The closest hit of such a ray is in its block's list, so a
// primary batch (64 rays of one 8x8 tile) tests that list instead of walking the tree,
// with the same (distance, original index) winner.
struct PrimLists {
    const uint2 *b8, *b4;       // {first entry, count} per block, row-major; count kPrimWalk: walk
    const uint32_t *slots;      // candidate slots (each block's run ascending)
    uint32_t bw;                // blocks per row: ceil(width / 8)
    uint32_t on;                // lists built for this scene, camera and frame size
};
constexpr uint32_t kPrimWalk = 0xFFFFFFFFu;

struct DeviceScene {
    const float4 *shade;    // {red, green, blue, fuzz} per slot (hit geometry: accel.slots)
    const uint32_t *mat;    // material id per slot
    uint32_t n;
    uint32_t code_stride, code_jmax;  // diffuse sample codes (diffuse_code)
    AccelView accel;
};

struct Camera {
    float view[12];  // rows 0..2 of viewMatrix (row 3 is zero)
    float eye[3];
    float sky[3];
};

// One rectangle of a batched launch (several concurrent RenderSegment calls rendered
// by one render + one fold launch, spt_batch.cpp render_batched).  Its items are
// [item_off, item_end) of the launch, in the order of a single-rectangle launch
// (ts_item over w x rows pixels and all spp samples); item_off is a multiple of the
// launch's claim size, so a claim never spans two rectangles, and items in
// [item_end, next item_off) are padding (no path).  Its per-sample slots are
// [slot_off, slot_off + npix * spp), in its own item order; its fold output sits at
// pixels [pix_off, pix_off + npix) of the batch's staging.
struct BatchRect {
    uint32_t item_off, item_end, slot_off, pix_off;
    uint32_t x0, y0, w, rows;
    uint32_t npix, alias;  // alias: task mode on a non-square tile (fold_kernel)
    uint8_t *rgb8;         // the call's g_data as the device sees it (its page-locked host buffer,
                           // written in place, or the context's device frame), or null
    FastDiv div_band, div_tile;  // ts_item divisors 8*w*spp and 64*spp
};
static_assert(sizeof(BatchRect) == 72, "BatchRect layout");
constexpr uint32_t kInlineRects = 4;  // rectangles carried in the kernel arguments

struct RenderArgs {
    DeviceScene scene;
    Camera cam;
    uint32_t width, height, bounces, mode;
    uint64_t seed_key;  // fmix64(seed)
    RowMap map;
    uint32_t npix;       // pixels of the launch (rows_owned * width)
    uint32_t spp_batch;  // samples per pixel in this batch
    uint32_t s0;         // first sample index of the batch
    uint32_t n_items;    // npix * spp_batch
    uint32_t claim;      // items per queue claim
    FastDiv div_band, div_tile;  // ts_item divisors 8*width*spp_batch and 64*spp_batch
    FastDiv div_strip;           // row_of_fast divisor map.strip
    uint32_t *samples;   // [n_items] per-sample slots in item order: the sample word (segment mode) or
                         // {word, key} (task mode; key 0 = dropped path)
    uint32_t slot_words;  // 1 or 2
    uint32_t *head;      // queue head (zeroed before launch)
    unsigned long long *counters;  // [0] casts, [1] samples, [2] dropped
    const BatchRect *rects;  // batched launch: n_rects rectangles (map/npix/div_* unused); else null
    uint32_t n_rects;
    // claims come from n_queues counters head[k * kQueueStride], queue k
    // handing out items [k * queue_items, (k + 1) * queue_items) (claim multiples)
    uint32_t n_queues, queue_items;
    // batched launches of at most kInlineRects rectangles may carry them here, in the
    // kernel arguments (inline_rects = 1: no table upload before the launch)
    uint32_t inline_rects;
    BatchRect rects_inline[kInlineRects];
    // render service (render_kernel_svc): the session's device control words
    // (SvcCtl), its job table and first claim of every job (device copies, written by the
    // forwarder wave) and completion counters; the fields above then hold the session's constants only (scene,
    // camera, frame, mode, ring of sample slots in `samples`, claim size, n_queues)
    uint32_t *svc_ctl;
    const struct SvcJob *svc_jobs;
    const uint32_t *svc_job_claim;
    uint32_t *svc_done;
    // SPT_SVC_TRACE (diagnostics, null otherwise): per completion counter, the
    // s_memrealtime of the first and last claim taken and of the last count added
    unsigned long long *svc_trace;
    // the session's SvcHost words and host job tables in page-locked host memory (committed
    // jobs, closing flag, published pair, stop flag; records and first claims the forwarder
    // copies into svc_jobs / svc_job_claim), as the device sees them
    uint32_t *svc_host;
    const struct SvcJob *svc_host_jobs;
    const uint32_t *svc_host_job_claim;
    // primary-ray candidate lists (PrimLists; on = 0: every primary batch walks the tree)
    PrimLists prim;
};

// claim counters: at most one per XCD, 256 bytes apart (separate cache lines)
constexpr uint32_t kMaxQueues = 8, kQueueStride = 64;

// ---- render service (DESIGN.md §4.7 "Render service") --------------------------------
// One resident launch of render_kernel_svc renders a stream of jobs (a frame, a rank's
// strips, a sample batch, a drop-in tile), published while it runs.  A session's claims
// form one sequence: job j owns claims [job_claim[j], job_claim[j] + n) of `claim` items,
// its items [item_off, item_end) (item_off = its first claim * claim, the rest of its last
// claim is padding).  Queue q of n_queues reserves claims q, q + n_queues, ... from its
// counter; a wave keeps one reserved claim and takes it once the host has published it.
// Finished samples are counted per completion counter (several jobs may share one);
// hipStreamWaitValue32 on the counter gates the job's fold.
//
// Publication needs no GPU queue: the host writes the job records, their first claims and
// the published pair {claims, jobs} into fine-grained page-locked host memory (the SvcHost
// block and tables); one wave of the session kernel -- the forwarder, wave 0 of block 0,
// which renders nothing -- polls that pair with system-scope loads and copies new records
// into the device job table, then stores the device pair the render waves poll (the R1
// hand-off of MI355X_MICROARCH.md, as round 4's publish kernel did).  Round 4 published from
// a one-wave kernel on a stream of its own; a dispatch waiting for CU resources the session
// holds (an RCCL gather, the liveness test's blocker) held that kernel back, and with it
// the session (tests/test_gpu_service.py).
struct SvcJob {
    uint32_t item_off, item_end;  // session items of the job
    uint32_t slot_off;            // slot of its item 0 in the ring (samples, item order)
    uint32_t done_idx;            // its completion counter
    uint32_t rows, spp_batch, s0; // region rows; samples of the batch and the first one
    uint32_t claim_end;           // first claim after the job
    RowMap map;                   // region (rows or interleaved strips, columns)
    FastDiv div_band, div_tile, div_strip;  // ts_item / row_of_fast divisors
    uint32_t claim_first;         // its first claim (item_off / claim)
    uint32_t pad[7];
};
static_assert(sizeof(SvcJob) == 128, "SvcJob: 32 words, one per lane of the loading wave");
constexpr uint32_t kSvcJobWords = 32;
static_assert(offsetof(SvcJob, claim_first) == 24 * 4 && offsetof(SvcJob, map) == 8 * 4 &&
                  offsetof(SvcJob, div_strip) == 21 * 4,
              "SvcJob word offsets (the service kernel reads the record by word)");
// SvcCtl words (device memory, svc_ctl): claim counters head[q * kQueueStride]
// (q < kMaxQueues), then on lines of their own the device copy of the published pair
// {claims, jobs} (one 64-bit word, stored and loaded as one), the stop flag, and the
// render waves still in the session (the forwarder leaves at 0).
constexpr uint32_t kSvcPub = kMaxQueues * kQueueStride;  // uint64_t: claims | jobs << 32
constexpr uint32_t kSvcStop = kSvcPub + 64;
constexpr uint32_t kSvcLive = kSvcStop + 64;
constexpr uint32_t kSvcCtlWords = kSvcLive + 64;
// A wave with no work for 0.5 s (s_memrealtime, 100 MHz) may leave, but only through the
// closing handshake with the host (SvcHost words):
//   wave:  closing = 1; fence; c = committed; read the published pair; leave iff every one
//          of the c committed jobs is published and its reserved claim is not among them
//   host:  committed = jobs of the session after this publication; fence; if closing is
//          set, end the session and publish to a new one instead
// Store-then-load on both sides (system scope on the device, seq_cst on the host): at
// least one side sees the other's store, so a wave never leaves a session that is still
// owed a publication.  "Published" is the device pair (forwarded).
constexpr unsigned long long kSvcIdleTicks = 50000000ull;
// SvcHost words (page-locked host memory), each on a 128-byte line of its own: the
// committed job count, the closing flag, the host's published pair (uint64: claims |
// jobs << 32), the stop flag (stored after the session's last publication) and the
// watchdog flag (a wave left the session through the closing handshake)
constexpr uint32_t kSvcHostCommitted = 0, kSvcHostClosing = 32, kSvcHostPub = 64, kSvcHostStop = 96,
                   kSvcHostWatchdog = 128, kSvcHostWords = 160;
constexpr uint32_t kSvcTraceClaims = 1u << 21;  // SPT_SVC_TRACE: claims with a take time
// grid: blocks of the session kernel's shape (svc_grid: 256-thread blocks, or the LDS-tree
// kernel's 1 024-thread blocks when the scene's tree takes the LDS lane walk)
hipError_t launch_render_svc(const RenderArgs &a, uint32_t grid, hipStream_t s);
// (svc_supported, svc_lds: which scenes the service takes, below with the walk rule)
// the LDS-tree session's grid: every block slot (full) or one per CU fewer, at least one
// per CU; 0 when the LDS-tree kernel cannot run on this device
uint32_t svc_lds_grid(bool full);
// threads per block of the session kernel for this scene
uint32_t svc_block(const AccelView &ac);

struct FoldArgs {
    const uint32_t *samples;  // slot_words per slot, in item order (ts_slot_base)
    uint32_t slot_words;
    const float4 *shade;      // the scene's shading table (diffuse codes name its slots)
    float sky[3];             // initColor (sky words)
    FastDiv code_div;         // FastDiv(code stride): diffuse_decode
    const float4 *ctab;       // the scene's colour table (spt_codes.h): entry c - 2 = the colour of diffuse
    uint32_t ctab_n;          // code c, ctab_n >= 1 entries; null: every word is decoded arithmetically
    float4 *acc;         // persistent accumulator (w = sample count)
    float4 *out_rgba;    // nullable, local pixel order
    uint8_t *out_rgb8;   // nullable, full frame (g_data layout)
    RowMap map;
    uint32_t width, height, npix, spp_batch, spp_total;
    uint32_t s_done;     // samples folded after this batch (s0 + spp_batch)
    int first, last, mode;
    int preview;         // write the outputs after every batch (progressive rendering)
    int prio;            // fold_kernel raises its waves' priority (launched renders; not beside the service)
    int alias;           // task mode, one non-square rectangle: RenderSegmentTask's colorIndex
                         // (dx + dy * segmentHeight, TaskBasedPathTracer.hpp:103,186) aliases pixels
    const BatchRect *rects;  // batched fold: n_rects rectangles over npix = their total pixels
    uint32_t n_rects;        // (map and alias per rectangle; spp_batch = spp_total, first = last = 1)
    // range alias fold (spt_render_frame: RenderSegmentTask over a non-square frame split
    // over several devices by ranges of its colorIndex): the npix outputs are the alias
    // indices [out_i0, out_i0 + npix) of a call of map.width x alias_h pixels, whose source
    // pixels' slots are those of the launch's rows (map: rows [map.y0, map.y0 + src_rows))
    uint32_t range_alias, out_i0, alias_h, src_rows;
    // batched fold: the render's claim counters (head[k * kQueueStride], k < head_queues),
    // zeroed for the workspace's next launch (no memset before it); null = leave them
    uint32_t *head_reset;
    uint32_t head_queues;
    uint32_t inline_rects;                 // as RenderArgs::inline_rects / rects_inline
    BatchRect rects_inline[kInlineRects];
};

// Launch geometry of one render launch: the context's persistent grid for the
// 256-thread kernels (`grid`, `block`), a divisor of every kernel's full grid (several
// host calls in flight share the GPU side by side), and on return the grid and block
// the chosen kernel ran with (the LDS tree kernel sizes its own: 1024-thread blocks).
struct LaunchShape {
    uint32_t grid, block, div;
    uint32_t ran_grid, ran_block;
};
hipError_t launch_render(const RenderArgs &a, LaunchShape &sh, hipStream_t s);

// Wavefront variant (spt_wavefront.hip): per-block ray queues of qcap rays (three
// 16-byte records per ray; cap = blocks x qcap) and the batch's item counter.
constexpr uint32_t kWfCats = 5;  // sky/miss, diffuse first hit, mirror, glass, diffuse-loop step
constexpr uint32_t kWfStateWords = 4;
struct WavefrontBuffers {
    float4 *o, *d;
    uint4 *m;
    uint32_t *state;  // [kWfStateWords]
    uint32_t cap, qcap;
};
// Every pass of a sample batch's paths through the ray queues, in one launch: the
// host issues it and waits for nothing (queue lengths stay on the device).
hipError_t launch_wavefront(const WavefrontBuffers &b, const RenderArgs &a, hipStream_t s);
// Blocks of the engine resident at once on device dev (its launch's grid), 0 on error.
uint32_t wavefront_blocks(const AccelView &ac, int dev);
hipError_t launch_fold(const FoldArgs &a, hipStream_t s);
// spt_render_samples: pixels [p0, p0 + n) of the region, out[(p - p0) * spp + s]
hipError_t launch_expand(const FoldArgs &a, float4 *out, uint32_t p0, uint32_t n, hipStream_t s);
// ctab[i] = {decode_sample(code_word(i + 2)), +0} for i < n: the colour table of a's scene
// (a.shade, a.code_div; spt_codes.h), filled by the arithmetic decode itself
hipError_t launch_ctab_fill(const FoldArgs &a, float4 *ctab, uint32_t n, hipStream_t s);
hipError_t launch_assemble(const float4 *tiles, uint32_t max_rows, RowMap base, uint32_t width, uint32_t height,
                           float4 *frame, uint8_t *rgb8, hipStream_t s);
hipError_t launch_selftest(const float *a, const float *b, const uint32_t *bits, uint32_t n, float *out,
                           hipStream_t s);
hipError_t render_occupancy(uint32_t block, int *blocks_per_cu);
uint32_t render_group_size();  // spheres per group of the hot loop (SPT_GROUP)

constexpr uint32_t kSpecularCap = 1024;  // see spt_oracle.h SPO_SPECULAR_CAP
constexpr uint32_t kTaskPasses = 10;     // TaskBasedPathTracer.hpp:81
// threads per block of the 256-thread render kernels (the LDS tree kernel has its own)
#ifndef SPT_RENDER_BLOCK
#define SPT_RENDER_BLOCK 256
#endif
constexpr uint32_t kRenderBlock = SPT_RENDER_BLOCK;
uint32_t render_block_size();  // kRenderBlock of the kernel object (the launch uses it)

// Node counts that choose a tree's walk (cast_walk below).
// 32-byte node records (pad included) of the LDS copy per block: 2432 = 76 KiB, with the
// sampler's 4 KiB exactly half of the CU's 160 KiB
#ifndef SPT_LDS_NODES
#define SPT_LDS_NODES 2432
#endif
constexpr uint32_t kLdsNodeRecords = SPT_LDS_NODES;
// smallest tree walked from LDS: below it the 8 octant layouts (64 nodes: 16 KiB) fit
// the scalar cache
#ifndef SPT_LDS_MIN_NODES
#define SPT_LDS_MIN_NODES 64
#endif
constexpr uint32_t kLdsMinNodes = SPT_LDS_MIN_NODES;
// largest tree walked lane by lane from global memory; larger ones take the wave walk
// (stress scenes at 16 spp, lane / wave walk: 20 000 spheres, 4 083 nodes, 12.7 / 18.6
// ms; 30 000, 6 104: 15.6 / 20.1; 40 000, 8 115: 17.7 / 20.2; 50 000, 10 053: 23.8 /
// 21.2 -- the per-lane node reads outgrow the caches)
#ifndef SPT_GLANE_MAX_NODES
#define SPT_GLANE_MAX_NODES 9000
#endif
constexpr uint32_t kGlaneMaxNodes = SPT_GLANE_MAX_NODES;
// (cast_walk below relies on it; a build with -DSPT_GLANE_MAX_NODES below the LDS bound,
// which no variant of the Makefile makes, stops here instead of walking such trees from LDS)
static_assert(kLdsNodeRecords <= kGlaneMaxNodes + 1u, "the global lane walk takes over where the LDS copy ends");
// the LDS-tree session kernel (render_kernel_svc_lds) also holds its waves' job records
// (16 x kSvcRecWords words = 80 records' worth): its table is that much shorter, so that
// two blocks still fit a CU (at 81 920 B the compiler keeps 64 VGPRs, 8 waves per SIMD)
constexpr uint32_t kLdsSvcNodeRecords = kLdsNodeRecords - 80u;

// The walk of a traversal shape, the one rule every launcher follows (launch_render,
// launch_render_svc, the wavefront engine, the query kernels): flat cluster lists of 4 or 8
// leaf slots; trees of kLdsMinNodes nodes or more lane by lane, over the block's LDS copy
// of node layout 0 while it fits, then over global memory up to kGlaneMaxNodes; every
// other tree by the wave's octant walk.
enum : uint32_t { kCastWalkLds = 0, kCastWalkGlane = 1, kCastWalkWave = 2, kCastWalkFlat4 = 3, kCastWalkFlat8 = 4 };
inline uint32_t cast_walk(const AccelView &ac)
{
    if (!ac.tree) return ac.leaf_slots == kFlatLeafSlots ? kCastWalkFlat4 : kCastWalkFlat8;
    if (ac.n_nodes < kLdsMinNodes || ac.n_nodes > kGlaneMaxNodes) return kCastWalkWave;
    return ac.n_nodes + 1u <= kLdsNodeRecords ? kCastWalkLds : kCastWalkGlane;
}
// true when the tree is walked lane by lane (LDS or global-memory lane walk)
inline bool lane_walk_tree(const AccelView &ac) { return cast_walk(ac) == kCastWalkLds || cast_walk(ac) == kCastWalkGlane; }
// does the scene's service session run the LDS-tree kernel (1 024-thread blocks)?  Its own,
// shorter table bound
inline bool svc_lds(const AccelView &ac) { return cast_walk(ac) == kCastWalkLds && ac.n_nodes + 1u <= kLdsSvcNodeRecords; }
// the service covers the wave-walk kernels (render_kernel's shapes) and the LDS lane walk
// (render_kernel_lds's shape, round 6); trees walked from global memory, or from an LDS
// table longer than the session's, keep their launches
inline bool svc_supported(const AccelView &ac) { return !lane_walk_tree(ac) || svc_lds(ac); }

// ---- ray queries (spt_cast.hip; spt_cast_rays[_async], spt_primary_hits) ---------------
// n rays, one per lane, cast with the render kernels' traversals.  Ray mode: origins o and
// directions d (float4, w ignored).  Camera mode (xys non-null): (x, y, s) triples, each
// the primary ray of sample s of pixel (x, y) from the eye, its direction written to
// dirs (nullable).  idx[i] = the winner's original sphere index, n_spheres on a miss;
// hit (nullable) = two float4 per ray: {P, t} and {n, ds}, all +0 on a miss.
struct CastArgs {
    AccelView accel;
    uint32_t n_spheres, n;
    const float4 *o, *d;
    const uint32_t *xys;
    Camera cam;
    uint32_t width, height;
    uint64_t seed_key;  // fmix64(seed)
    uint32_t *idx;
    float4 *hit, *dirs;
};
hipError_t launch_cast(const CastArgs &a, hipStream_t s);

// ---- occlusion queries (spt_occlude.hip; spt_occluded_rays[_async]) --------------------
// n rays, one per lane: occ[i] = 1 iff the cast of ray i would hit with ds < L_i (DESIGN.md
// §4.17), else 0.  Ray form: origins a, directions b, L_i = limits[i] (+inf where limits is
// null).  Segment form: end points a and b; o = a, d = normalize(b - a), L = lensq(b - a) *
// scale.
struct OccludeArgs {
    AccelView accel;
    uint32_t n;
    uint32_t segments;
    float scale;
    const float4 *a, *b;
    const float *limits;
    uint8_t *occ;
};
hipError_t launch_occlude(const OccludeArgs &a, hipStream_t s);

// ---- path queries (spt_trace.hip; spt_trace_rays[_async]) ------------------------------
// n paths, one per lane: TraceAndSampleColor(d[i], o[i], bounces) in segment semantics,
// every draw of path i from the raw splitmix state st[i].  The trace kernel leaves path
// i's sample word in the first word of rgba[i] (shade_step's store); the decode pass that
// follows it on the stream rebuilds the colour there (decode_word), w = +0.
// info (nullable) = two words per path: {casts, specular events | cut at the cap << 31}.
struct TraceArgs {
    DeviceScene scene;  // code_jmax: the launch's own, from `bounces`
    uint32_t n, bounces;
    const float4 *o, *d;
    const uint64_t *st;
    float4 *rgba;
    uint32_t *info;
};
// `f`: the scene's shading table, sky and code divisor (fold_args)
hipError_t launch_trace(const TraceArgs &a, const FoldArgs &f, hipStream_t s);

// ---- feature buffers (spt_features.hip; spt_render_features[_async]) -------------------
// Per pixel of the region of RenderArgs::map, over the frame's own primary rays of samples
// 0 .. spp - 1 in order: feat (nullable) = two float4 per region-local pixel p (row-major),
// {albedo.rgb, coverage} and {normal.xyz, depth}, each the in-order sum of the per-sample
// values times 1.0f / (float)spp; ids (nullable) = sample 0's original sphere index, the
// sphere count on a miss.  The RenderArgs describes a render launch of all spp samples of
// the region at once; the kernels read of it what start_path_kernarg and prim_list_cast
// read (map, width, height, bounces, npix, n_items, spp_batch = spp, s0 = 0, seed_key,
// cam.view, cam.eye, div_band = FastDiv(8 * map.width * spp) where rows >= 8, div_tile =
// FastDiv(64 * spp), div_strip = FastDiv(map.strip), prim) and scene (accel, mat, shade,
// n), cam.sky.
struct FeatArgs {
    float4 *feat;
    uint32_t *ids;
    uint32_t rows;     // rows_owned(map)
    uint32_t tiles_x;  // 8x8 tiles per band: ceil(map.width / 8)
    uint32_t tiles;    // ceil(rows / 8) * tiles_x
    uint32_t spp;
};
hipError_t launch_features(const RenderArgs &k, const FeatArgs &f, hipStream_t s);

// ---- denoiser (spt_denoise.hip; spt_denoise[_async], spt_denoise_var[_async]) ----------
// One level of the a-trous filter over a width x height image: reads `in` (level 0: the
// caller's rgba, then the previous level's output) and feat, writes out (nullable) and / or
// the g_data bytes rgb8 (nullable, last level only).  The four factors are 1 / sigma^2; the
// plain form's kc is already times 4^level, the variance-guided form's is the same at every
// level.
//
// The fields after kz are the variance-guided form's (`var`): denoise_level_kernel reads
// none of them.  There `in` is the caller's rgba at level 0 (first: g is worked out from mom
// as the cell is staged), then the previous level's plane with g in its w lane.
// Intermediate levels write {u', g'} to out; the last level (rgba non-null: the caller's
// input, for its w lane) writes {u', rgba.w} to out and g' to out_var (nullable).
struct DenoiseArgs {
    const float4 *in, *feat;
    float4 *out;
    uint8_t *rgb8;
    uint32_t width, height;
    uint32_t step;              // 2^level
    uint32_t sx, sy;            // lattices with a pixel: min(step, width), min(step, height)
    uint32_t tiles_x, tiles_y;  // 16x16 tiles of the longest lattice: ceil(ceil(width / step) / 16), ...
    float kc, ka, kn, kz;
    float var_floor;
    uint32_t first;  // level 0
    const float4 *mom, *rgba;
    float *out_var;
};
hipError_t launch_denoise_level(const DenoiseArgs &a, bool var, hipStream_t s);

// ---- sample moments (spt_moments.hip; spt_render_moments[_async]) ----------------------
// Per pixel of a single-batch SPT_MODE_SEGMENT region whose sample words lie in f.samples
// (f.map, f.npix, f.spp_batch = spp; the decode tables of fold_args): mom[p] = {m1, m2, var,
// spp} of the samples' luminance in sample order, p the local row-major pixel.
hipError_t launch_moments(const FoldArgs &f, float4 *mom, hipStream_t s);

// ---- temporal accumulation (spt_temporal.hip; spt_temporal[_async]) --------------------
// One launch over a width x height image: this frame's rgba, mom, feat (two float4 per
// pixel) and ids, the history's four (all null: no history, the outputs are copies), and
// the two outputs.  m and e are this frame's camera (the nine used entries of view, rows
// 0..2 x columns 0..2, and the eye), minv and ep the previous one's (spt_temporal_inverse of
// its view, and its eye); fw and fh the width and height as floats; is_static: the two
// cameras compare equal, the static rule holds.  tiles_x is the launch's own.
// The motion variant (spt_temporal_motion[_async]) reads motion as well: n_spheres records
// of two float4, {C.xyz, r} of this frame and {Cp.xyz, rp} of the previous one, indexed by
// the pixel's id (null with n_spheres == 0); the plain kernel reads neither field.
struct TemporalArgs {
    const float4 *rgba, *mom, *feat;
    const uint32_t *ids;
    const float4 *h_rgba, *h_mom, *h_feat;
    const uint32_t *h_ids;
    float4 *out_rgba, *out_mom;
    uint32_t width, height, tiles_x;
    float fw, fh;
    float m[9], e[3], minv[9], ep[3];
    float tol_normal, tol_depth, max_history;
    uint32_t is_static;
    const float4 *motion;
    uint32_t n_spheres;
};
hipError_t launch_temporal(TemporalArgs a, bool motion, hipStream_t s);

// ---- candidate lists built on the device (spt_primlists.hip; spt_update_scene) ----------
// The PrimLists of the slot table `slots` (n_slots <= kPrimDevSlots, the kernel's LDS list)
// for a finite camera and a frame of at most 65 535 columns and rows, in fixed-stride
// storage: block b of level l (0: 8x8, 1: 8x4) owns entries [(l * nb8 + b) * stride, + stride)
// of `out`, stride = roundup4(prim_max) >= prim_max.  b8 / b4: nb8 / nb4 entries
// {first, count}, count kPrimWalk = walk; `pad` is a dummy slot of the table; totals[0] +=
// 8x8 blocks with a list, totals[1] += list entries (zeroed by the caller).
constexpr uint32_t kPrimDevSlots = 2048;
struct PrimBuildArgs {
    const float4 *slots;
    uint32_t n_slots, pad;
    Camera cam;
    uint32_t W, H, prim_max, stride;
    uint32_t bw, nb8;
    uint2 *b8, *b4;
    uint32_t *out;
    uint32_t *totals;
};
hipError_t launch_prim_lists(const PrimBuildArgs &a, hipStream_t s);

}  // namespace spt
