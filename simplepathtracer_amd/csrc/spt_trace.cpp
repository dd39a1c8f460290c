// spt_trace.cpp -- path queries over the context's scene: spt_trace_rays[_async]
// (TraceAndSampleColor on rays the caller chooses, each on a raw splitmix stream of the
// caller's) and spt_sample_state (the render's keyed stream of a sample), the host half of
// spt_trace.hip.  They read the scene and the sky of member 0 and touch neither the
// statistics nor the sample workspaces.
#include "spt_host.h"

namespace spt_api {

namespace {

// the checks both forms share, in the order the header gives them; `arrays`: no required
// pointer is null; *nothing: n == 0, the call is over
int trace_check(spt_ctx *ctx, uint32_t n, uint32_t bounces, bool arrays, bool *nothing)
{
    *nothing = false;
    if (!ctx->scene_set) return fail(ctx, SPT_ERR_STATE, "scene not set (spt_set_scene)");
    if (!ctx->cam_set) return fail(ctx, SPT_ERR_STATE, "camera not set (spt_set_camera: the sky colour)");
    if (bounces == 0) return fail(ctx, SPT_ERR_ARG, "bounces must be >= 1 (--bounceCount never reaches 0)");
    if (n == 0) {
        *nothing = true;
        return SPT_OK;
    }
    if (!arrays) return fail(ctx, SPT_ERR_ARG, "null origins, directions, states or rgba");
    // the diffuse codes of this call's depth, not the context's (spt_set_params)
    const uint32_t jmax = std::min(bounces - 1u, ctx->code_jz);
    if (!spt::code_layout_fits(ctx->code_stride, jmax))
        return fail(ctx, SPT_ERR_ARG, "%u slots at %u bounces need more than %u sample codes (jmax %u)", ctx->code_stride,
                    bounces, spt::kCodeMax, jmax);
    return SPT_OK;
}

spt::TraceArgs trace_args(const spt_ctx *ctx, uint32_t bounces)
{
    spt::TraceArgs a{};
    a.scene = device_scene(ctx);
    a.scene.code_jmax = std::min(bounces - 1u, ctx->code_jz);
    a.bounces = bounces;
    return a;
}

// a launch the service does not take: a resident session ends first
int trace_launch(spt_ctx *ctx, const spt::TraceArgs &a, hipStream_t s)
{
    if (int rc = svc_end(ctx)) return rc;
    spt::FoldArgs f = fold_args(ctx, nullptr, 1);
    // the colour table holds the codes of the context's depth; a call deeper than that
    // writes codes past it and decodes them arithmetically
    if (f.ctab && a.scene.code_jmax > ctx->scene.ctab_jmax) {
        f.ctab = nullptr;
        f.ctab_n = 0;
    }
    HIP_TRY(ctx, spt::launch_trace(a, f, s));
    return SPT_OK;
}

}  // namespace

}  // namespace spt_api

extern "C" {

int spt_trace_rays_async(spt_ctx *ctx, const void *d_origins4, const void *d_dirs4, const void *d_states, uint32_t n,
                         uint32_t bounces, void *d_rgba, void *d_info, void *stream)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool nothing;
    if (int rc = trace_check(ctx, n, bounces, d_origins4 && d_dirs4 && d_states && d_rgba, &nothing)) return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    spt::TraceArgs a = trace_args(ctx, bounces);
    a.n = n;
    a.o = (const float4 *)d_origins4;
    a.d = (const float4 *)d_dirs4;
    a.st = (const uint64_t *)d_states;
    a.rgba = (float4 *)d_rgba;
    a.info = (uint32_t *)d_info;
    return trace_launch(ctx, a, (hipStream_t)stream);  // NULL = the HIP default stream
}

int spt_trace_rays(spt_ctx *ctx, const float *origins4, const float *dirs4, const uint64_t *states, uint32_t n,
                   uint32_t bounces, float *rgba, uint32_t *info)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool nothing;
    if (int rc = trace_check(ctx, n, bounces, origins4 && dirs4 && states && rgba, &nothing)) return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t s = ctx->stream;
    Staging st;
    if (!st.alloc(trace_rays_plan(n, info != nullptr), s))
        return fail(ctx, SPT_ERR_NOMEM, "spt_trace_rays: %zu bytes of staging", st.plan.total);
    float4 *d_o = st.at<float4>(0), *d_d = st.at<float4>(1), *d_rgba = st.at<float4>(2);
    uint64_t *d_st = st.at<uint64_t>(3);
    uint32_t *d_info = st.at<uint32_t>(4);
    spt::TraceArgs a = trace_args(ctx, bounces);
    a.o = d_o;
    a.d = d_d;
    a.st = d_st;
    a.rgba = d_rgba;
    a.info = d_info;
    const size_t chunk = st.plan.chunk;
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t m = std::min(chunk, (size_t)n - r0);
        HIP_TRY(ctx, hipMemcpyAsync(d_o, origins4 + 4 * r0, m * sizeof(float4), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d_d, dirs4 + 4 * r0, m * sizeof(float4), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d_st, states + r0, m * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        a.n = (uint32_t)m;
        if (int rc = trace_launch(ctx, a, s)) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(rgba + 4 * r0, d_rgba, m * sizeof(float4), hipMemcpyDeviceToHost, s));
        if (info) HIP_TRY(ctx, hipMemcpyAsync(info + 2 * r0, d_info, m * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    return st.done(SPT_OK);
}

int spt_sample_state(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t draws, uint64_t *state)
{
    if (!state) return fail(nullptr, SPT_ERR_ARG, "null state");
    // start_path's key (spt_path.h), then `draws` steps of the splitmix counter (Random.hpp:30-36)
    *state = fmix64(fmix64(seed) ^ (((uint64_t)pixel << 32) | (uint64_t)sample)) + (uint64_t)draws * 0x9E3779B97F4A7C15ull;
    return SPT_OK;
}

}  // extern "C"
