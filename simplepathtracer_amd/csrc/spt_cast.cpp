// spt_cast.cpp -- ray queries over the context's scene: spt_cast_rays[_async] (closest
// sphere of rays the caller chooses) and spt_primary_hits (of a sample's primary ray), the
// host half of spt_cast.hip.  They read the scene (and, for primary hits, camera and
// params) of member 0 and touch neither the statistics nor the sample workspaces.
#include "spt_host.h"

namespace spt_api {

namespace {

spt::CastArgs cast_args(const spt_ctx *ctx)
{
    spt::CastArgs a{};
    a.accel = ctx->accel;
    a.n_spheres = ctx->n;
    return a;
}

// a render the service does not take: a resident session ends first
int cast_launch(spt_ctx *ctx, const spt::CastArgs &a, hipStream_t s)
{
    if (int rc = svc_end(ctx)) return rc;
    HIP_TRY(ctx, spt::launch_cast(a, s));
    return SPT_OK;
}

}  // namespace

}  // namespace spt_api

extern "C" {

int spt_cast_rays_async(spt_ctx *ctx, const void *d_origins4, const void *d_dirs4, uint32_t n, void *d_idx, void *d_hit,
                        void *stream)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->scene_set) return fail(ctx, SPT_ERR_STATE, "scene not set (spt_set_scene)");
    if (n == 0) return SPT_OK;
    if (!d_origins4 || !d_dirs4 || !d_idx) return fail(ctx, SPT_ERR_ARG, "null origins, directions or idx");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    spt::CastArgs a = cast_args(ctx);
    a.n = n;
    a.o = (const float4 *)d_origins4;
    a.d = (const float4 *)d_dirs4;
    a.idx = (uint32_t *)d_idx;
    a.hit = (float4 *)d_hit;
    return cast_launch(ctx, a, (hipStream_t)stream);  // NULL = the HIP default stream
}

int spt_cast_rays(spt_ctx *ctx, const float *origins4, const float *dirs4, uint32_t n, uint32_t *idx, float *hit)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->scene_set) return fail(ctx, SPT_ERR_STATE, "scene not set (spt_set_scene)");
    if (n == 0) return SPT_OK;
    if (!origins4 || !dirs4 || !idx) return fail(ctx, SPT_ERR_ARG, "null origins, directions or idx");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t s = ctx->stream;
    Staging st;
    if (!st.alloc(cast_rays_plan(n, hit != nullptr), s))
        return fail(ctx, SPT_ERR_NOMEM, "spt_cast_rays: %zu bytes of staging", st.plan.total);
    float4 *d_o = st.at<float4>(0), *d_d = st.at<float4>(1), *d_hit = st.at<float4>(3);
    uint32_t *d_idx = st.at<uint32_t>(2);
    spt::CastArgs a = cast_args(ctx);
    a.o = d_o;
    a.d = d_d;
    a.idx = d_idx;
    a.hit = d_hit;
    const size_t chunk = st.plan.chunk;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t m = std::min(chunk, (size_t)n - r0);
        HIP_TRY(ctx, hipMemcpyAsync(d_o, origins4 + 4 * r0, m * sizeof(float4), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d_d, dirs4 + 4 * r0, m * sizeof(float4), hipMemcpyHostToDevice, s));
        a.n = (uint32_t)m;
        if (int rc = cast_launch(ctx, a, s)) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(idx + r0, d_idx, m * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (hit) HIP_TRY(ctx, hipMemcpyAsync(hit + 8 * r0, d_hit, m * 2 * sizeof(float4), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    return st.done(SPT_OK);
}

int spt_primary_hits(spt_ctx *ctx, const uint32_t *xys, uint32_t n, uint32_t *idx, float *hit, float *dirs4)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->scene_set) return fail(ctx, SPT_ERR_STATE, "scene not set (spt_set_scene)");
    if (!ctx->cam_set) return fail(ctx, SPT_ERR_STATE, "camera not set (spt_set_camera)");
    if (!ctx->params_set) return fail(ctx, SPT_ERR_STATE, "params not set (spt_set_params)");
    if (n == 0) return SPT_OK;
    if (!xys || !idx) return fail(ctx, SPT_ERR_ARG, "null xys or idx");
    for (size_t i = 0; i < n; ++i)
        if (xys[3 * i] >= ctx->W || xys[3 * i + 1] >= ctx->H || xys[3 * i + 2] >= ctx->spp)
            return fail(ctx, SPT_ERR_ARG, "triple %zu (x %u, y %u, s %u) outside the %u x %u frame at %u spp", i,
                        xys[3 * i], xys[3 * i + 1], xys[3 * i + 2], ctx->W, ctx->H, ctx->spp);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t s = ctx->stream;
    Staging st;
    if (!st.alloc(primary_hits_plan(n, hit != nullptr, dirs4 != nullptr), s))
        return fail(ctx, SPT_ERR_NOMEM, "spt_primary_hits: %zu bytes of staging", st.plan.total);
    uint32_t *d_xys = st.at<uint32_t>(0), *d_idx = st.at<uint32_t>(1);
    float4 *d_hit = st.at<float4>(2), *d_dirs = st.at<float4>(3);
    spt::CastArgs a = cast_args(ctx);
    a.xys = d_xys;
    a.cam = ctx->cam;
    a.width = ctx->W;
    a.height = ctx->H;
    a.seed_key = fmix64(ctx->seed);
    a.idx = d_idx;
    a.hit = d_hit;
    a.dirs = d_dirs;
    const size_t chunk = st.plan.chunk;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t m = std::min(chunk, (size_t)n - r0);
        HIP_TRY(ctx, hipMemcpyAsync(d_xys, xys + 3 * r0, m * 3 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        a.n = (uint32_t)m;
        if (int rc = cast_launch(ctx, a, s)) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(idx + r0, d_idx, m * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (hit) HIP_TRY(ctx, hipMemcpyAsync(hit + 8 * r0, d_hit, m * 2 * sizeof(float4), hipMemcpyDeviceToHost, s));
        if (dirs4) HIP_TRY(ctx, hipMemcpyAsync(dirs4 + 4 * r0, d_dirs, m * sizeof(float4), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    return st.done(SPT_OK);
}

}  // extern "C"
