// spt_occlude.cpp -- bounded any-hit queries over the context's scene:
// spt_occluded_rays[_async], the host half of spt_occlude.hip.  As the ray queries
// (spt_cast.cpp) they read the scene of member 0 and touch neither the statistics nor the
// sample workspaces.
#include "spt_host.h"

namespace spt_api {

namespace {

// the checks both forms share, after the context's; SPT_OK: launch
int occlude_check(spt_ctx *ctx, const void *a4, const void *b4, const void *limits, uint32_t flags, const void *occ)
{
    if (flags & ~(uint32_t)SPT_OCCLUDE_SEGMENTS) return fail(ctx, SPT_ERR_ARG, "unknown flag bits 0x%x", flags);
    if (!a4 || !b4 || !occ) return fail(ctx, SPT_ERR_ARG, "null origins, directions (end points) or occ");
    if ((flags & SPT_OCCLUDE_SEGMENTS) && limits)
        return fail(ctx, SPT_ERR_ARG, "SPT_OCCLUDE_SEGMENTS takes no limits: a segment's is its own length (times scale)");
    return SPT_OK;
}

spt::OccludeArgs occlude_args(const spt_ctx *ctx, uint32_t flags, float scale)
{
    spt::OccludeArgs a{};
    a.accel = ctx->accel;
    a.segments = (flags & SPT_OCCLUDE_SEGMENTS) ? 1u : 0u;
    a.scale = scale;
    return a;
}

// a resident service session ends first, as for a cast
int occlude_launch(spt_ctx *ctx, const spt::OccludeArgs &a, hipStream_t s)
{
    if (int rc = svc_end(ctx)) return rc;
    HIP_TRY(ctx, spt::launch_occlude(a, s));
    return SPT_OK;
}

}  // namespace

}  // namespace spt_api

extern "C" {

int spt_occluded_rays_async(spt_ctx *ctx, const void *d_a4, const void *d_b4, const void *d_limits, uint32_t n,
                            uint32_t flags, float scale, void *d_occ, void *stream)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->scene_set) return fail(ctx, SPT_ERR_STATE, "scene not set (spt_set_scene)");
    if (n == 0) return SPT_OK;
    if (int rc = occlude_check(ctx, d_a4, d_b4, d_limits, flags, d_occ)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    spt::OccludeArgs a = occlude_args(ctx, flags, scale);
    a.n = n;
    a.a = (const float4 *)d_a4;
    a.b = (const float4 *)d_b4;
    a.limits = (const float *)d_limits;
    a.occ = (uint8_t *)d_occ;
    return occlude_launch(ctx, a, (hipStream_t)stream);  // NULL = the HIP default stream
}

int spt_occluded_rays(spt_ctx *ctx, const float *a4, const float *b4, const float *limits, uint32_t n, uint32_t flags,
                      float scale, uint8_t *occ)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->scene_set) return fail(ctx, SPT_ERR_STATE, "scene not set (spt_set_scene)");
    if (n == 0) return SPT_OK;
    if (int rc = occlude_check(ctx, a4, b4, limits, flags, occ)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t s = ctx->stream;
    Staging st;
    if (!st.alloc(occluded_rays_plan(n, limits != nullptr), s))
        return fail(ctx, SPT_ERR_NOMEM, "spt_occluded_rays: %zu bytes of staging", st.plan.total);
    float4 *d_a = st.at<float4>(0), *d_b = st.at<float4>(1);
    float *d_lim = st.at<float>(2);
    uint8_t *d_occ = st.at<uint8_t>(3);
    spt::OccludeArgs a = occlude_args(ctx, flags, scale);
    a.a = d_a;
    a.b = d_b;
    a.limits = d_lim;
    a.occ = d_occ;
    const size_t chunk = st.plan.chunk;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t m = std::min(chunk, (size_t)n - r0);
        HIP_TRY(ctx, hipMemcpyAsync(d_a, a4 + 4 * r0, m * sizeof(float4), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d_b, b4 + 4 * r0, m * sizeof(float4), hipMemcpyHostToDevice, s));
        if (limits) HIP_TRY(ctx, hipMemcpyAsync(d_lim, limits + r0, m * sizeof(float), hipMemcpyHostToDevice, s));
        a.n = (uint32_t)m;
        if (int rc = occlude_launch(ctx, a, s)) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(occ + r0, d_occ, m, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    return st.done(SPT_OK);
}

}  // extern "C"
