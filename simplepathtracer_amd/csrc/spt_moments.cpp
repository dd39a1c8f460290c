// spt_moments.cpp -- per-pixel sample moments: spt_render_moments[_async], the host half of
// spt_moments.hip.  A call is a SPT_MODE_SEGMENT render of the region that keeps its one
// batch of sample words (render_impl with keep_samples, as spt_render_samples: launched on
// the caller's stream, never through the service or in double-buffered batches), folds them
// into the caller's outputs with the render's own fold, then reads the words a second time
// for the moments.  It counts in spt_stats as the render it is and uses member 0 of a
// multi-device context.
#include "spt_host.h"

namespace spt_api {

namespace {

// the checks both forms share; *nothing: an empty rectangle, the call is over
int moments_check(spt_ctx *ctx, uint32_t yB, uint32_t yE, uint32_t strip, uint32_t parts, uint32_t part, uint32_t xB,
                  uint32_t xE, const void *mom, bool *nothing)
{
    *nothing = false;
    if (int rc = check_ready(ctx)) return rc;
    if (strip == 0 || parts == 0 || part >= parts) return fail(ctx, SPT_ERR_ARG, "bad row map");
    if (int rc = check_region(ctx, yB, yE, xB, xE)) return rc;
    if (yB > yE || xB > xE) return fail(ctx, SPT_ERR_ARG, "inverted region [%u,%u)x[%u,%u)", yB, yE, xB, xE);
    if (yB == yE || xB == xE) {
        *nothing = true;
        return SPT_OK;
    }
    if (!mom) return fail(ctx, SPT_ERR_ARG, "null mom");
    return SPT_OK;
}

// render + fold + moments of the rows of `map` on `s`; a region over one sample batch fails
// in render_impl before anything is launched
int moments_launch(spt_ctx *ctx, const spt::RowMap &map, float4 *d_rgba, uint8_t *d_rgb8, float4 *d_mom, hipStream_t s)
{
    if (int rc = render_impl(ctx, SPT_MODE_SEGMENT, map, d_rgba, d_rgb8, s, true)) return rc;
    const Workspace *w = workspace_for(ctx, s);
    if (!w) return SPT_ERR_STATE;
    spt::FoldArgs fa = fold_args(ctx, w->d_samples, 1u);
    fa.map = map;
    fa.npix = spt::rows_owned(map) * map.width;
    fa.spp_batch = ctx->spp;
    HIP_TRY(ctx, spt::launch_moments(fa, d_mom, s));
    return SPT_OK;
}

}  // namespace

}  // namespace spt_api

extern "C" {

int spt_render_moments_async(spt_ctx *ctx, uint32_t yB, uint32_t yE, uint32_t strip, uint32_t parts, uint32_t part,
                             uint32_t xB, uint32_t xE, void *d_rgba, void *d_rgb8, void *d_mom, void *stream)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool nothing;
    if (int rc = moments_check(ctx, yB, yE, strip, parts, part, xB, xE, d_mom, &nothing)) return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const spt::RowMap map{yB, yE, strip, parts, part, xB, xE - xB};
    return moments_launch(ctx, map, (float4 *)d_rgba, (uint8_t *)d_rgb8, (float4 *)d_mom,
                          (hipStream_t)stream);  // NULL = the HIP default stream
}

int spt_render_moments(spt_ctx *ctx, uint32_t yB, uint32_t yE, uint32_t xB, uint32_t xE, float *rgba, uint8_t *g_data,
                       float *mom)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool nothing;
    if (int rc = moments_check(ctx, yB, yE, 1u, 1u, 0u, xB, xE, mom, &nothing)) return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t w = xE - xB, h = yE - yB, W = ctx->W, H = ctx->H;
    const size_t npix = (size_t)w * h;
    const hipStream_t s = ctx->stream;
    Staging st;
    if (!st.alloc(moments_plan(npix, (size_t)W * H * 3, rgba != nullptr, g_data != nullptr), s))
        return fail(ctx, SPT_ERR_NOMEM, "spt_render_moments: %zu bytes of staging", st.plan.total);
    float4 *d_rgba = st.at<float4>(0), *d_mom = st.at<float4>(1);
    uint8_t *d8 = st.at<uint8_t>(2);
    const spt::RowMap map{yB, yE, 1u, 1u, 0u, xB, w};
    if (int rc = moments_launch(ctx, map, d_rgba, d8, d_mom, s)) return rc;
    if (rgba) HIP_TRY(ctx, hipMemcpyAsync(rgba, d_rgba, npix * sizeof(float4), hipMemcpyDeviceToHost, s));
    if (g_data) {
        // the region's band of the frame, as spt_render_segment copies it
        const size_t pitch = (size_t)W * 3, off = band_offset(W, H, yE, xB);
        HIP_TRY(ctx, hipMemcpy2DAsync(g_data + off, pitch, d8 + off, pitch, (size_t)w * 3, h, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipMemcpyAsync(mom, d_mom, npix * sizeof(float4), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return st.done(collect_timings(ctx));
}

}  // extern "C"
