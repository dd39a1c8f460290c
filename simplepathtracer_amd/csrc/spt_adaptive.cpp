// spt_adaptive.cpp -- adaptive sampling: spt_render_adaptive[_dev], the host half of
// spt_adaptive.hip (include/spt_hip.h "adaptive sampling").  A call is a
// sequence of passes on the caller's stream; each pass is
//   adaptive_plan_kernel   the flagged tiles -> the pass's BatchRect table and its counts
//   (the host waits for the counts: the one host synchronisation per pass -- the render's
//    grid, item count and queue split are launch arguments)
//   launch_render          the render kernels' batched launch over the table, s0 = n,
//                          spp_batch = take, as launch_batch builds it
//   adaptive_fold_kernel   sums, convergence test, flags or outputs
// Pass 0 takes the same path with every flag set.  The passes count in spt_stats as the
// renders they are and use member 0 of a multi-device context; like the batched host calls
// they are launches of the megakernel on every CU, whatever the engine setting.
#include "spt_host.h"

namespace spt_api {

namespace {

struct AdaptParams {
    uint32_t yB, yE, xB, xE, base, step, mx;
    float tol, lum_floor;
};

// the checks both forms share; *nothing: an empty rectangle, the call is over
int adaptive_check(spt_ctx *ctx, const AdaptParams &p, const void *rgba, const void *g, const void *mom, bool *nothing)
{
    *nothing = false;
    if (int rc = check_ready(ctx)) return rc;
    if (int rc = check_region(ctx, p.yB, p.yE, p.xB, p.xE)) return rc;
    if (p.yB > p.yE || p.xB > p.xE)
        return fail(ctx, SPT_ERR_ARG, "inverted region [%u,%u)x[%u,%u)", p.yB, p.yE, p.xB, p.xE);
    if (p.base < 1u || p.step < 1u || p.mx < p.base)
        return fail(ctx, SPT_ERR_ARG, "bad sample counts: base_spp %u, step_spp %u, max_spp %u (1 <= base <= max, step >= 1)",
                    p.base, p.step, p.mx);
    if (!(p.tol >= 0.0f)) return fail(ctx, SPT_ERR_ARG, "tol must be >= 0 or +inf");
    if (!(p.lum_floor >= 0.0f) || !std::isfinite(p.lum_floor)) return fail(ctx, SPT_ERR_ARG, "lum_floor must be finite and >= 0");
    if (p.yB == p.yE || p.xB == p.xE) {
        *nothing = true;
        return SPT_OK;
    }
    if (!rgba && !g && !mom) return fail(ctx, SPT_ERR_ARG, "null outputs: one of rgba, g_data and mom is needed");
    return SPT_OK;
}

// samples of the pass that starts at n samples
uint32_t take_at(const AdaptParams &p, uint32_t n) { return n == 0 ? p.base : std::min(p.step, p.mx - n); }

// The passes on stream s.  info (nullable): {samples rendered, passes run}.
int adaptive_run(spt_ctx *ctx, const AdaptParams &p, float4 *d_rgba, uint8_t *d_rgb8, float4 *d_mom, uint64_t *info,
                 hipStream_t s)
{
    const uint32_t w = p.xE - p.xB, h = p.yE - p.yB;
    const uint64_t npix64 = (uint64_t)w * h;
    // the largest pass any run of these parameters can have: every tile, the longest take
    const uint32_t take_max = p.mx > p.base ? std::max(p.base, std::min(p.step, p.mx - p.base)) : p.base;
    const uint64_t budget = std::min<uint64_t>(std::max<uint64_t>(ctx->ws_bytes / sizeof(uint32_t), 1), 0x7FFFFFFFull);
    if (npix64 * take_max > budget)
        return fail(ctx, SPT_ERR_ARG, "a pass of %ux%u pixels at %u samples exceeds one sample batch of the workspace", w, h,
                    take_max);
    const uint32_t npix = (uint32_t)npix64;
    {
        const spt::AdaptGeom g = spt::adaptive_geom(p.xB, p.yB, w, h, take_max, claim_size(ctx, npix64 * take_max));
        uint64_t items_pad, slots;
        spt::adaptive_totals(g, items_pad, slots);
        if (items_pad > 0x7FFFFFFFull)
            return fail(ctx, SPT_ERR_ARG, "a pass of %ux%u pixels at %u samples exceeds 2^31 - 1 items (workspace batch)", w, h,
                        take_max);
    }
    int rc = svc_end(ctx);
    if (rc || (rc = rebuild_ctab(ctx))) return rc;
    Workspace *ws = workspace_for(ctx, s);
    if (!ws) return SPT_ERR_STATE;
    const uint32_t n_tiles = ((w + 7u) >> 3) * ((h + 7u) >> 3);
    if ((rc = ensure(ctx, &ws->d_samples, &ws->samples_cap, (size_t)npix * take_max)) ||
        (rc = ensure(ctx, &ctx->ad_acc, &ctx->ad_acc_cap, npix)) || (rc = ensure(ctx, &ctx->ad_s12, &ctx->ad_s12_cap, npix)) ||
        (rc = ensure(ctx, &ctx->ad_flags, &ctx->ad_flags_cap, n_tiles)) ||
        (rc = ensure(ctx, &ctx->ad_rects, &ctx->ad_rects_cap, n_tiles)))
        return rc;
    if (!ctx->ad_count) {
        HIP_TRY(ctx, hipHostMalloc((void **)&ctx->ad_count, sizeof(spt::AdaptCount)));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ad_done, hipEventDisableTiming));
    } else {
        // the state is the context's: the last fold of an earlier call on another stream first
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ad_done, 0));
    }
    spt::AdaptCount *d_count = nullptr;
    HIP_TRY(ctx, hipHostGetDevicePointer((void **)&d_count, ctx->ad_count, 0));

    // pass 0: every flag set (any nonzero word)
    HIP_TRY(ctx, hipMemsetAsync(ctx->ad_flags, 1, (size_t)n_tiles * sizeof(uint32_t), s));

    spt::RenderArgs ra{};
    ra.scene = device_scene(ctx);
    ra.prim = ctx->prim;
    ra.cam = ctx->cam;
    ra.width = ctx->W;
    ra.height = ctx->H;
    ra.bounces = ctx->bounces;
    ra.mode = (uint32_t)SPT_MODE_SEGMENT;
    ra.seed_key = fmix64(ctx->seed);
    ra.map = spt::RowMap{0u, 1u, 1u, 1u, 0u, 0u, 1u};  // per rectangle (BatchRect)
    ra.div_strip = spt::make_fastdiv(1u);
    ra.div_band = ra.div_tile = spt::make_fastdiv(1u);
    ra.samples = ws->d_samples;
    ra.slot_words = 1u;
    ra.head = ws->d_head;
    ra.counters = ctx->d_counters;
    ra.rects = ctx->ad_rects;
    ra.inline_rects = 0u;
    ra.n_queues = ctx->queues;

    spt::FoldArgs fa = fold_args(ctx, ws->d_samples, 1u);
    fa.width = ctx->W;
    fa.height = ctx->H;
    const spt::AdaptState st{ctx->ad_acc, ctx->ad_s12, ctx->ad_flags};

    uint64_t samples = 0, passes = 0, active_pix = npix;
    for (uint32_t n = 0; n < p.mx;) {
        const uint32_t take = take_at(p, n);
        // the claim from the most the pass can hold: the pixels active in the pass before
        const uint32_t claim = claim_size(ctx, active_pix * take);
        const spt::AdaptGeom g = spt::adaptive_geom(p.xB, p.yB, w, h, take, claim);
        HIP_TRY(ctx, spt::launch_adaptive_plan(g, ctx->ad_flags, ctx->ad_rects, d_count, s));
        // the pass's counts are launch arguments of its render: the host waits for them here
        HIP_TRY(ctx, hipStreamSynchronize(s));
        const volatile spt::AdaptCount *hc = ctx->ad_count;
        const spt::AdaptCount c{hc->n_rects, hc->n_items, hc->n_slots, 0u};
        if (c.n_rects == 0) break;
        ra.npix = c.n_slots / take;
        ra.spp_batch = take;
        ra.s0 = n;
        ra.n_items = c.n_items;
        ra.claim = claim;
        ra.n_rects = c.n_rects;
        {
            const uint32_t per = (ra.n_items + ra.n_queues - 1u) / ra.n_queues;
            ra.queue_items = (per + claim - 1u) / claim * claim;
        }
        HIP_TRY(ctx, hipMemsetAsync(ws->d_head, 0, sizeof(uint32_t) * spt::kQueueStride * ra.n_queues, s));
        ws->head_clean = false;
        if (!ctx->ref_recorded) {
            HIP_TRY(ctx, hipEventRecord(ctx->ref_ev, s));
            ctx->ref_recorded = true;
        }
        EventPair ev = get_pair(ctx);
        HIP_TRY(ctx, hipEventRecord(ev.a, s));
        spt::LaunchShape sh{render_grid(ctx, ra.n_items, claim, 1u), ctx->block, 1u, 0, 0};
        HIP_TRY(ctx, spt::launch_render(ra, sh, s));
        ctx->last_grid = sh.ran_grid;
        ctx->last_block = sh.ran_block;
        HIP_TRY(ctx, hipEventRecord(ev.b, s));
        ctx->pending_render.push_back(ev);  // the setters wait for it (wait_own_renders)
        ctx->launches++;

        const spt::AdaptFoldArgs af{c.n_rects, n, p.mx, n == 0 ? 1u : 0u, p.tol, p.lum_floor, d_rgba, d_rgb8, d_mom};
        EventPair ef = get_pair(ctx);
        HIP_TRY(ctx, hipEventRecord(ef.a, s));
        HIP_TRY(ctx, spt::launch_adaptive_fold(fa, g, ctx->ad_rects, st, af, s));
        HIP_TRY(ctx, hipEventRecord(ef.b, s));
        ctx->pending_fold.push_back(ef);
        n += take;
        samples += c.n_slots;
        active_pix = ra.npix;
        ++passes;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ad_done, s));
    if (info) {
        info[0] = samples;
        info[1] = passes;
    }
    if (ctx->pending_render.size() > 256) return collect_timings(ctx);
    return SPT_OK;
}

}  // namespace

}  // namespace spt_api

extern "C" {

int spt_render_adaptive_dev(spt_ctx *ctx, uint32_t yB, uint32_t yE, uint32_t xB, uint32_t xE, uint32_t base_spp,
                            uint32_t step_spp, uint32_t max_spp, float tol, float lum_floor, void *d_rgba, void *d_rgb8,
                            void *d_mom, uint64_t *info, void *stream)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    const AdaptParams p{yB, yE, xB, xE, base_spp, step_spp, max_spp, tol, lum_floor};
    bool nothing;
    if (int rc = adaptive_check(ctx, p, d_rgba, d_rgb8, d_mom, &nothing)) return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return adaptive_run(ctx, p, (float4 *)d_rgba, (uint8_t *)d_rgb8, (float4 *)d_mom, info,
                        (hipStream_t)stream);  // NULL = the HIP default stream
}

int spt_render_adaptive(spt_ctx *ctx, uint32_t yB, uint32_t yE, uint32_t xB, uint32_t xE, uint32_t base_spp, uint32_t step_spp,
                        uint32_t max_spp, float tol, float lum_floor, float *rgba, uint8_t *g_data, float *mom, uint64_t *info)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    const AdaptParams p{yB, yE, xB, xE, base_spp, step_spp, max_spp, tol, lum_floor};
    bool nothing;
    if (int rc = adaptive_check(ctx, p, rgba, g_data, mom, &nothing)) return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t w = xE - xB, h = yE - yB, W = ctx->W, H = ctx->H;
    const size_t npix = (size_t)w * h;
    const hipStream_t s = ctx->stream;
    Staging st;
    if (!st.alloc(adaptive_staging_plan(npix, (size_t)W * H * 3, rgba != nullptr, mom != nullptr, g_data != nullptr), s))
        return fail(ctx, SPT_ERR_NOMEM, "spt_render_adaptive: %zu bytes of staging", st.plan.total);
    float4 *d_rgba = st.at<float4>(0), *d_mom = st.at<float4>(1);
    uint8_t *d8 = st.at<uint8_t>(2);
    uint64_t inf[2] = {0, 0};
    if (int rc = adaptive_run(ctx, p, d_rgba, d8, d_mom, inf, s)) return rc;
    if (rgba) HIP_TRY(ctx, hipMemcpyAsync(rgba, d_rgba, npix * sizeof(float4), hipMemcpyDeviceToHost, s));
    if (g_data) {
        // the region's band of the frame, as spt_render_segment copies it
        const size_t pitch = (size_t)W * 3, off = band_offset(W, H, yE, xB);
        HIP_TRY(ctx, hipMemcpy2DAsync(g_data + off, pitch, d8 + off, pitch, (size_t)w * 3, h, hipMemcpyDeviceToHost, s));
    }
    if (mom) HIP_TRY(ctx, hipMemcpyAsync(mom, d_mom, npix * sizeof(float4), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (info) {
        info[0] = inf[0];
        info[1] = inf[1];
    }
    return st.done(collect_timings(ctx));
}

}  // extern "C"
