// spt_readahead.cpp -- the HIP half of the tiling read-ahead (SpecFrame in
// spt_host.h): the page-locked frame, the parts' streams and launches, the serve's copy.  What
// a call does is decided by spt_readahead.h (tile_of, ReadAhead); this file performs it, under
// three rules:
//   R1  spec_frame_bytes alone frees or reallocates SpecFrame::h8, once the gate is idle
//       (spec_destroy releases it with the context).
//   R2  after a step that may have released ctx->mu (a gate wait, spec_frame_bytes,
//       spec_prepare, spec_launch) everything is derived from the context again: spec_serve
//       goes round its loop, spec_prepare / spec_launch answer kSpecRetry for a stale tiling.
//   R3  a best-effort step (the setter's early allocation, spec_serve without a buffer) sets
//       no error: spec_frame_bytes never calls fail(), the callers that need the buffer do.
#include "spt_host.h"

namespace spt_api {

constexpr int kSpecRetry = -1;  // spec_prepare / spec_launch: the tiling is no longer the context's

// The priority of the read-ahead parts' streams: the least one (SPT_READAHEAD_PRIO
// overrides).  A priority the callers' streams do not use gives the parts hardware queues of
// their own, so a part's render does not queue behind another part's fold (tc = 4: 5.75-6.04
// -> 5.48-5.60 ms per frame in segment mode).
int readahead_prio()
{
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    const char *e = env_var("SPT_READAHEAD_PRIO");
    return e ? std::atoi(e) : lo;
}

// The stream and event of read-ahead part p (created on first use).
static int spec_stream(spt_ctx *ctx, int p)
{
    SpecFrame &sp = ctx->spec;
    BatchSet *bs = &sp.bs[p];
    if (!bs->stream) bs->stream = warm_take(ctx, 1 + p);
    if (!bs->stream) HIP_TRY(ctx, hipStreamCreateWithPriority(&bs->stream, hipStreamNonBlocking, readahead_prio()));
    if (!sp.ev[p]) HIP_TRY(ctx, hipEventCreateWithFlags(&sp.ev[p], hipEventDisableTiming));
    return SPT_OK;
}

// The read-ahead frame's page-locked bytes (SpecFrame::h8), at least `bytes` of them: the one
// place that frees or reallocates them (R1).  Called with lk (ctx->mu) held; before it grows
// the frame it waits (unlocked) until no serve copies out of the old bytes.  A failed
// allocation is the caller's to report or to drop (R3); only a service session that does not
// end (svc_end) leaves its own error.
int spec_frame_bytes(spt_ctx *ctx, std::unique_lock<std::mutex> &lk, size_t bytes)
{
    SpecFrame &sp = ctx->spec;
    if (sp.h8_cap >= bytes) return SPT_OK;
    sp.gate.wait_idle(lk);
    if (sp.h8_cap >= bytes) return SPT_OK;  // grown by another caller meanwhile
    // hipHostFree synchronises the device, which a resident service session would hold
    if (int rc = svc_end(ctx)) return rc;
    hipError_t e = sp.h8 ? hipHostFree(sp.h8) : hipSuccess;
    sp.h8 = sp.h8_dev = nullptr;
    sp.h8_cap = 0;
    void *dp = nullptr;
    if (e == hipSuccess) e = hipHostMalloc((void **)&sp.h8, bytes);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&dp, sp.h8, 0);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // dropped with the failure: the next launch's check starts clean
        if (sp.h8) (void)hipHostFree(sp.h8);
        sp.h8 = nullptr;
        return e == hipErrorOutOfMemory ? SPT_ERR_NOMEM : SPT_ERR_HIP;
    }
    sp.h8_dev = (uint8_t *)dp;
    sp.h8_cap = bytes;
    return SPT_OK;
}

// spec_frame_bytes for the steps that cannot go on without the frame: its failure is an error.
static int spec_need_frame(spt_ctx *ctx, std::unique_lock<std::mutex> &lk, const Tiling &t)
{
    const size_t bytes = (size_t)t.W * t.H * 3;
    const int rc = spec_frame_bytes(ctx, lk, bytes);
    return rc ? fail(ctx, rc, "read-ahead frame: %zu page-locked bytes not available", bytes) : SPT_OK;
}

// The buffers the read-ahead of tiling t will use (the frame's page-locked bytes, its parts'
// rectangle tables), allocated when the tiling arms: allocated by the first read-ahead itself,
// each part's first allocations held its launch until the previous part's render had ended
// (the four parts of the first read-ahead frame ran one after another, 15 ms apart,
// profiles/r05_dropin_trace.md).  The parts' streams and sample workspaces come with the first
// read-ahead (spec_launch): a one-frame caller (the reference's MainLoop renders one frame per
// process) never pays for them.  Called with lk (ctx->mu) held; may wait unlocked.
static int spec_prepare(spt_ctx *ctx, std::unique_lock<std::mutex> &lk, const Tiling &t)
{
    SpecFrame &sp = ctx->spec;
    host_trace("spec_prepare begin");
    int rc = spec_need_frame(ctx, lk, t);
    if (rc) return rc;
    if (t.W != ctx->W || t.H != ctx->H) return kSpecRetry;  // a setter ran during the wait (R2)
    host_trace("spec_prepare frame bytes");
    const uint32_t np = std::min(sp.parts, t.tc), rpp = (t.tc + np - 1) / np;
    for (uint32_t p = 0; p * rpp < t.tc; ++p) {
        BatchSet *bs = &sp.bs[p];
        const size_t tiles = (size_t)(std::min(t.tc, (p + 1) * rpp) - p * rpp) * t.tc;
        if ((rc = grow_host_rects(ctx, bs, tiles))) return rc;
        host_trace("spec_prepare host rects", (void *)(uintptr_t)p);
        if ((rc = ensure(ctx, &bs->d_rects, &bs->rects_cap, tiles))) return rc;
    }
    return SPT_OK;
}

// Render every tile of t (MakeRenderSegmentData order) into the read-ahead frame, in sp.parts
// batched launches of consecutive tile rows.  The previous frame's parts have been waited for.
static int spec_launch_parts(spt_ctx *ctx, const Tiling &t)
{
    SpecFrame &sp = ctx->spec;
    const uint32_t tc = t.tc, sw = t.sw(), sh = t.sh();
    std::vector<BatchReq> reqs(t.tiles());
    for (uint32_t j = 0; j < tc; ++j)
        for (uint32_t i = 0; i < tc; ++i)
            reqs[(size_t)j * tc + i] = BatchReq{t.mode,  sh * j, std::min(sh * j + sh, t.H), sw * i, std::min(sw * i + sw, t.W),
                                                nullptr, sp.h8,  SPT_OK,                     true,   false};
    const uint32_t np = std::min(sp.parts, tc), rpp = (tc + np - 1) / np;  // launches, tile rows each
    sp.rows_per_part = rpp;
    for (uint32_t p = 0; p * rpp < tc; ++p) {
        std::vector<BatchReq *> part;
        for (uint32_t j = p * rpp; j < std::min(tc, (p + 1) * rpp); ++j)
            for (uint32_t i = 0; i < tc; ++i) part.push_back(&reqs[(size_t)j * tc + i]);
        BatchSet *bs = &sp.bs[p];
        int rc = spec_stream(ctx, (int)p);
        if (rc || (rc = launch_batch(ctx, bs, part, sp.h8_dev))) return rc;
        HIP_TRY(ctx, hipEventRecord(sp.ev[p], bs->stream));
        sp.launched[p] = true;
        sp.finished[p] = false;
        ctx->batches++;
        ctx->batched_calls += part.size();
    }
    return SPT_OK;
}

// Begin a read-ahead frame of tiling t at generation gen.  Called with lk (ctx->mu) held;
// waits (unlocked) for the previous frame's serves still copying out of h8, which the new
// frame's folds rewrite.
static int spec_launch(spt_ctx *ctx, std::unique_lock<std::mutex> &lk, const Tiling &t, uint64_t gen)
{
    SpecFrame &sp = ctx->spec;
    sp.gate.wait_idle(lk);
    if (t.W != ctx->W || t.H != ctx->H || gen != ctx->gen) return kSpecRetry;  // a setter ran meanwhile (R2)
    // the gate is idle and the lock held from here on: spec_need_frame does not wait
    sp.st.begin_frame(t, gen);
    int rc = SPT_OK;
    for (int p = 0; p < SpecFrame::kParts && !rc; ++p)  // the previous frame's parts, before h8 is reused
        if (sp.launched[p]) {
            const hipError_t e = hipEventSynchronize(sp.ev[p]);
            if (e != hipSuccess) rc = fail(ctx, SPT_ERR_HIP, "read-ahead part wait failed: %s", hipGetErrorString(e));
            sp.launched[p] = false;
        }
    if (!rc) rc = spec_need_frame(ctx, lk, t);
    if (!rc) rc = spec_launch_parts(ctx, t);
    if (rc) sp.st.drop_frame();
    return rc;
}

// A RenderSegment call with only g_data: served from the read-ahead frame when it is one
// of its tiles not yet served (starting a read-ahead at any tile of an armed tiling: the
// reference's detached RenderJob threads call the tiles in no fixed order), else
// kSpecMiss.  Called with lk (ctx->mu) held; waits unlocked.  Each round of the loop derives
// the tile from the context as it is now and performs one step (R2).
int spec_serve(spt_ctx *ctx, std::unique_lock<std::mutex> &lk, int mode, uint32_t yB, uint32_t yE, uint32_t xB,
               uint32_t xE, uint8_t *g_data)
{
    SpecFrame &sp = ctx->spec;
    for (;;) {
        Tiling t;
        const int64_t k = tile_of(ctx->W, ctx->H, mode, xB, xE, yB, yE, &t);
        if (k < 0 || !tiling_fits(t, ctx->spp, batch_slot_bytes(ctx, mode, (uint64_t)t.sw() * t.sh() * t.tiles()),
                                  ctx->ws_bytes))
            return kSpecMiss;
        const size_t bytes = (size_t)t.W * t.H * 3;
        if (sp.h8_cap < bytes) {
            // the frame's page-locked bytes with the first tile-shaped call; without them the
            // call renders as usual (R3)
            if (spec_frame_bytes(ctx, lk, bytes) != SPT_OK) return kSpecMiss;
            continue;
        }
        int rc;
        switch (sp.st.next(t, (size_t)k, ctx->gen)) {
        case ReadAhead::Step::Miss:
        case ReadAhead::Step::NoteMiss:
            host_trace("spec_serve miss (not armed), tile", (void *)(uintptr_t)k);
            return kSpecMiss;
        case ReadAhead::Step::PrepareMiss:
            // the read-ahead's buffers now, while this frame's tiles render as usual
            if ((rc = spec_prepare(ctx, lk, t)) == kSpecRetry) continue;
            return rc ? rc : kSpecMiss;
        case ReadAhead::Step::PrepareLaunch:
            if ((rc = spec_prepare(ctx, lk, t)) != SPT_OK && rc != kSpecRetry) return rc;
            continue;
        case ReadAhead::Step::Launch:
            host_trace("spec_serve launch for tile", (void *)(uintptr_t)k);
            if ((rc = spec_launch(ctx, lk, t, ctx->gen)) != SPT_OK && rc != kSpecRetry) return rc;
            continue;
        case ReadAhead::Step::Serve:
        case ReadAhead::Step::ServeOwed:
            break;
        }
        // the copy keeps what it snapshots here, under the lock
        const uint32_t part = (uint32_t)k / t.tc / sp.rows_per_part;
        const hipEvent_t ev = sp.ev[part];
        const bool finished = sp.finished[part];
        const uint8_t *const src = sp.h8;
        sp.gate.enter();
        lk.unlock();
        // the part's fold wrote the tile's band into the page-locked frame (its event completes
        // after the kernel's writes; once one serve has seen it complete, the part's other
        // serves skip the sync: 1 024 serves per frame at tc = 32)
        const size_t pitch = (size_t)t.W * 3, off = band_offset(t.W, t.H, yE, xB);
        const hipError_t e = finished ? hipSuccess : hipEventSynchronize(ev);
        if (e == hipSuccess)
            for (uint32_t r = 0; r < yE - yB; ++r)
                std::memcpy(g_data + off + r * pitch, src + off + r * pitch, (size_t)(xE - xB) * 3);
        lk.lock();
        if (e == hipSuccess && sp.ev[part] == ev && sp.launched[part]) sp.finished[part] = true;
        sp.gate.leave();
        if (e != hipSuccess) return fail(ctx, SPT_ERR_HIP, "read-ahead tile copy failed: %s", hipGetErrorString(e));
        return SPT_OK;
    }
}

// The read-ahead's resources, at the context's end (no serve is in progress).
void spec_destroy(spt_ctx *ctx)
{
    SpecFrame &sp = ctx->spec;
    for (BatchSet &b : sp.bs) destroy_batch_set(&b);
    for (hipEvent_t e : sp.ev)
        if (e) (void)hipEventDestroy(e);
    if (sp.h8) (void)hipHostFree(sp.h8);
    sp.h8 = sp.h8_dev = nullptr;
    sp.h8_cap = 0;
}

}  // namespace spt_api
