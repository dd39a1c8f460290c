// spt_features.cpp -- feature buffers of the frame's own primary rays:
// spt_render_features[_async], the host half of spt_features.hip.  They read the scene,
// camera, params and primary-ray candidate lists of member 0, ignore the engine setting and
// touch neither the statistics nor the sample workspaces.
#include "spt_host.h"

namespace spt_api {

namespace {

// the checks both forms share, in the order the header gives them; *nothing: an empty
// rectangle, the call is over
int features_check(spt_ctx *ctx, uint32_t yB, uint32_t yE, uint32_t strip, uint32_t parts, uint32_t part, uint32_t xB,
                   uint32_t xE, bool outputs, bool *nothing)
{
    *nothing = false;
    if (!ctx->scene_set) return fail(ctx, SPT_ERR_STATE, "scene not set (spt_set_scene)");
    if (!ctx->cam_set) return fail(ctx, SPT_ERR_STATE, "camera not set (spt_set_camera)");
    if (!ctx->params_set) return fail(ctx, SPT_ERR_STATE, "params not set (spt_set_params)");
    if (strip == 0 || parts == 0 || part >= parts) return fail(ctx, SPT_ERR_ARG, "bad row map");
    if (int rc = check_region(ctx, yB, yE, xB, xE)) return rc;
    if (yB > yE || xB > xE) return fail(ctx, SPT_ERR_ARG, "inverted region [%u,%u)x[%u,%u)", yB, yE, xB, xE);
    if (yB == yE || xB == xE) {
        *nothing = true;
        return SPT_OK;
    }
    if (!outputs) return fail(ctx, SPT_ERR_ARG, "null feat and ids");
    return SPT_OK;
}

// one launch over the rows of `map`, whose rows x width x spp items fit ts_item's range
int features_launch_one(spt_ctx *ctx, const spt::RowMap &map, float4 *d_feat, uint32_t *d_ids, hipStream_t s)
{
    const uint32_t rows = spt::rows_owned(map);
    const uint64_t npix = (uint64_t)rows * map.width;
    if (npix == 0) return SPT_OK;
    spt::RenderArgs ra{};
    ra.scene = device_scene(ctx);
    ra.prim = ctx->prim;
    ra.cam = ctx->cam;
    ra.width = ctx->W;
    ra.height = ctx->H;
    ra.bounces = ctx->bounces;
    ra.seed_key = fmix64(ctx->seed);
    ra.map = map;
    // the items of a render launch of every sample at once: [band][tile][sample][pixel]
    ra.npix = (uint32_t)npix;
    ra.spp_batch = ctx->spp;
    ra.s0 = 0u;
    ra.n_items = (uint32_t)(npix * ctx->spp);
    ra.div_band = spt::make_fastdiv(rows >= 8 ? 8u * map.width * ctx->spp : 1u);  // (unused below 8 rows)
    ra.div_tile = spt::make_fastdiv(64u * ctx->spp);
    ra.div_strip = spt::make_fastdiv(map.strip);
    spt::FeatArgs fa{};
    fa.feat = d_feat;
    fa.ids = d_ids;
    fa.rows = rows;
    fa.tiles_x = (map.width + 7u) / 8u;
    fa.tiles = ((rows + 7u) / 8u) * fa.tiles_x;
    fa.spp = ctx->spp;
    HIP_TRY(ctx, spt::launch_features(ra, fa, s));
    return SPT_OK;
}

// The rows of `map`, in launches of whole periods (strip x parts rows of the frame, `strip`
// of them the part's own) whose items stay below 2^31, ts_item's range; the outputs are in
// local pixel order, so a launch's follow the rows before it.  Launches the service does
// not take: a resident session ends first.
int features_launch(spt_ctx *ctx, const spt::RowMap &map, float4 *d_feat, uint32_t *d_ids, hipStream_t s)
{
    const uint64_t per_period = (uint64_t)map.strip * map.width * ctx->spp;  // items
    if (per_period > 0x7FFFFFFFull)
        return fail(ctx, SPT_ERR_ARG, "%u rows of %u pixels at %u spp exceed 2^31 samples a launch", map.strip, map.width,
                    ctx->spp);
    if (int rc = svc_end(ctx)) return rc;
    const uint64_t periods = std::max<uint64_t>(1, 0x7FFFFFFFull / per_period);
    const uint64_t step = periods * map.strip * map.parts;  // frame rows a launch spans
    size_t pix = 0;
    int rc = SPT_OK;
    for (uint64_t y = map.y0; y < map.y1 && !rc; y += step) {
        spt::RowMap m = map;
        m.y0 = (uint32_t)y;
        m.y1 = (uint32_t)std::min<uint64_t>(map.y1, y + step);
        rc = features_launch_one(ctx, m, d_feat ? d_feat + 2 * pix : nullptr, d_ids ? d_ids + pix : nullptr, s);
        pix += (size_t)spt::rows_owned(m) * map.width;
    }
    // the kernels read the candidate lists from the caller's stream: the setters that
    // rewrite the lists wait for this event (wait_own_renders), as they wait for renders;
    // also after a failed launch, for the launches before it
    const std::string first = ctx->err;
    const int rc_mark = features_mark(ctx, s);
    if (rc) ctx->err = first;  // the launch's message, not the mark's
    return rc ? rc : rc_mark;
}

}  // namespace

}  // namespace spt_api

extern "C" {

int spt_render_features_async(spt_ctx *ctx, uint32_t yB, uint32_t yE, uint32_t strip, uint32_t parts, uint32_t part,
                              uint32_t xB, uint32_t xE, void *d_feat, void *d_ids, void *stream)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool nothing;
    if (int rc = features_check(ctx, yB, yE, strip, parts, part, xB, xE, d_feat || d_ids, &nothing)) return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const spt::RowMap map{yB, yE, strip, parts, part, xB, xE - xB};
    return features_launch(ctx, map, (float4 *)d_feat, (uint32_t *)d_ids, (hipStream_t)stream);  // NULL = the HIP default stream
}

int spt_render_features(spt_ctx *ctx, uint32_t yB, uint32_t yE, uint32_t xB, uint32_t xE, float *feat, uint32_t *ids)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool nothing;
    if (int rc = features_check(ctx, yB, yE, 1u, 1u, 0u, xB, xE, feat || ids, &nothing)) return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // per pixel: two float4 and one word out; chunks of whole 8-row bands, so a chunk's
    // tiles are the region's own
    const size_t w = xE - xB, h = yE - yB;
    const hipStream_t s = ctx->stream;
    Staging st;
    if (!st.alloc(features_plan(w, h, feat != nullptr, ids != nullptr), s))
        return fail(ctx, SPT_ERR_NOMEM, "spt_render_features: %zu bytes of staging", st.plan.total);
    float4 *d_feat = st.at<float4>(0);
    uint32_t *d_ids = st.at<uint32_t>(1);
    const size_t chunk = st.plan.chunk;
    for (size_t r0 = 0; r0 < h; r0 += chunk) {
        const size_t m = std::min(chunk, h - r0);
        const spt::RowMap map{yB + (uint32_t)r0, yB + (uint32_t)(r0 + m), 1u, 1u, 0u, xB, (uint32_t)w};
        if (int rc = features_launch(ctx, map, d_feat, d_ids, s)) return rc;
        if (feat) HIP_TRY(ctx, hipMemcpyAsync(feat + 8 * r0 * w, d_feat, m * w * 2 * sizeof(float4), hipMemcpyDeviceToHost, s));
        if (ids) HIP_TRY(ctx, hipMemcpyAsync(ids + r0 * w, d_ids, m * w * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    return st.done(SPT_OK);
}

}  // extern "C"
