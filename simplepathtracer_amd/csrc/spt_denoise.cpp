// spt_denoise.cpp -- the edge-avoiding a-trous filter guided by the feature buffers:
// spt_denoise_scratch_bytes, spt_denoise[_async] and the variance-guided
// spt_denoise_var[_async], the host half of spt_denoise.hip.  They
// need no scene, camera or params, use member 0 of a multi-device context, end a resident
// service session first, touch neither the statistics nor the sample workspaces and read no
// candidate lists (no setter waits for them).
#include "spt_host.h"

namespace spt_api {

namespace {

constexpr uint32_t kMaxLevels = 8;

// float4 planes of the ping-pong between levels: level 0 reads the caller's rgba and the
// last level writes the caller's outputs, so levels - 1 intermediate images, two at most
inline uint64_t scratch_planes(uint32_t levels) { return std::min<uint32_t>(levels - 1u, 2u); }
inline uint64_t scratch_bytes(uint64_t npix, uint32_t levels) { return scratch_planes(levels) * npix * sizeof(float4); }

// One call of either form, as its entry point received it: host pointers for the blocking
// forms, device pointers for the async ones.
struct DenoiseCall {
    bool var;  // the variance-guided form: mom, var_floor and out_var count
    uint32_t W, H;
    const void *rgba, *feat, *mom;
    float sigma[4], var_floor;
    uint32_t levels;
    void *out, *rgb8, *out_var, *scratch;  // scratch: the async forms'
};

// the checks, the plain form's first and then the variance-guided form's own; *nothing: an
// empty image, the call is over
int denoise_check(spt_ctx *ctx, const DenoiseCall &c, bool need_scratch, bool *nothing)
{
    *nothing = false;
    if (!c.rgba || !c.feat) return fail(ctx, SPT_ERR_ARG, "null rgba or feat");
    if (!c.out && !c.rgb8) return fail(ctx, SPT_ERR_ARG, "null out_rgba and out_rgb8");
    if (c.levels < 1u || c.levels > kMaxLevels) return fail(ctx, SPT_ERR_ARG, "levels %u outside 1..%u", c.levels, kMaxLevels);
    for (int t = 0; t < 4; ++t)
        if (!(c.sigma[t] > 0.0f)) return fail(ctx, SPT_ERR_ARG, "sigma %d is %g: must be > 0 (+inf switches the term off)", t, (double)c.sigma[t]);
    const uint64_t npix = (uint64_t)c.W * c.H;
    if (npix >= 0x80000000ull) return fail(ctx, SPT_ERR_ARG, "%u x %u pixels exceed 2^31 - 1", c.W, c.H);
    if (npix == 0) {
        *nothing = true;
        return SPT_OK;
    }
    const uint64_t sb = scratch_bytes(npix, c.levels);
    if (need_scratch && sb && !c.scratch) return fail(ctx, SPT_ERR_ARG, "null scratch (spt_denoise_scratch_bytes: %llu)", (unsigned long long)sb);
    // every output against every input, then the outputs against each other; the rows of mom
    // and out_var take part with `var` only
    auto clash = [&](bool var) -> int {
        const struct {
            const void *p;
            uint64_t n;
            const char *name;
        } outs[3] = {{c.out, npix * 16u, "out_rgba"}, {c.rgb8, npix * 3u, "out_rgb8"}, {var ? c.out_var : nullptr, npix * 4u, "out_var"}},
          ins[4] = {{c.rgba, npix * 16u, "rgba"}, {c.feat, npix * 32u, "feat"}, {var ? c.mom : nullptr, npix * 16u, "mom"},
                    {c.scratch, sb, "scratch"}};
        for (const auto &o : outs)
            for (const auto &i : ins)
                if (overlaps(o.p, o.n, i.p, i.n)) return fail(ctx, SPT_ERR_ARG, "%s overlaps %s", o.name, i.name);
        if (overlaps(outs[0].p, outs[0].n, outs[1].p, outs[1].n)) return fail(ctx, SPT_ERR_ARG, "out_rgba overlaps out_rgb8");
        for (int t = 0; t < 2; ++t)
            if (overlaps(outs[2].p, outs[2].n, outs[t].p, outs[t].n)) return fail(ctx, SPT_ERR_ARG, "out_var overlaps %s", outs[t].name);
        return SPT_OK;
    };
    if (int rc = clash(false)) return rc;
    if (!c.var) return SPT_OK;
    if (!c.mom) return fail(ctx, SPT_ERR_ARG, "null mom");
    if (!(c.var_floor > 0.0f) || !std::isfinite(c.var_floor))
        return fail(ctx, SPT_ERR_ARG, "var_floor is %g: must be finite and > 0", (double)c.var_floor);
    return clash(true);  // the pairs of the first pass are clear: only the new rows can report
}

// the levels over device pointers, one launch each on `s`: level 0 reads rgba, level k > 0
// the plane level k - 1 wrote, the last writes the caller's outputs.  The variance-guided
// form's planes carry g in their w lane, and its last level takes the output's w lane from
// rgba
int denoise_launch(spt_ctx *ctx, const DenoiseCall &c, hipStream_t s)
{
    if (int rc = svc_end(ctx)) return rc;
    float k[4];
    for (int t = 0; t < 4; ++t) {
        const float s2 = c.sigma[t] * c.sigma[t];
        k[t] = 1.0f / s2;
    }
    const size_t npix = (size_t)c.W * c.H;
    const float4 *in = (const float4 *)c.rgba;
    for (uint32_t lv = 0; lv < c.levels; ++lv) {
        const bool last = lv + 1u == c.levels;
        spt::DenoiseArgs a{};
        a.in = in;
        a.feat = (const float4 *)c.feat;
        a.out = last ? (float4 *)c.out : (float4 *)c.scratch + (size_t)(lv & 1u) * npix;
        a.rgb8 = last ? (uint8_t *)c.rgb8 : nullptr;
        a.width = c.W;
        a.height = c.H;
        a.step = 1u << lv;
        a.sx = std::min(a.step, c.W);
        a.sy = std::min(a.step, c.H);
        a.tiles_x = ((c.W + a.step - 1u) / a.step + 15u) / 16u;
        a.tiles_y = ((c.H + a.step - 1u) / a.step + 15u) / 16u;
        a.ka = k[1];
        a.kn = k[2];
        a.kz = k[3];
        if (c.var) {
            a.kc = k[0];  // sigma_color counts standard deviations at every level
            a.var_floor = c.var_floor;
            a.first = lv == 0;
            a.mom = (const float4 *)c.mom;
            a.rgba = last ? (const float4 *)c.rgba : nullptr;
            a.out_var = last ? (float *)c.out_var : nullptr;
        } else {
            a.kc = k[0] * (float)(1u << (2u * lv));  // the colour sigma halves per level; exact
        }
        HIP_TRY(ctx, spt::launch_denoise_level(a, c.var, s));
        in = a.out;
    }
    return SPT_OK;
}

// what all four entry points do: the checks, then the levels on the caller's stream over the
// caller's device pointers (stream non-null; *stream NULL = the HIP default stream), or the
// blocking form over one allocation: rgba, feat, out, the scratch planes, mom, out_var, then
// the bytes
int denoise_run(spt_ctx *ctx, const DenoiseCall &c, const hipStream_t *stream)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool nothing;
    if (int rc = denoise_check(ctx, c, stream != nullptr, &nothing)) return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (stream) return denoise_launch(ctx, c, *stream);
    const size_t npix = (size_t)c.W * c.H, b_rgba = npix * sizeof(float4);
    const hipStream_t s = ctx->stream;
    Staging st;
    if (!st.alloc(denoise_plan(npix, (size_t)scratch_planes(c.levels), c.out != nullptr, c.rgb8 != nullptr, c.var,
                               c.var && c.out_var != nullptr), s))
        return fail(ctx, SPT_ERR_NOMEM, "%s: %zu bytes of device buffers", c.var ? "spt_denoise_var" : "spt_denoise", st.plan.total);
    DenoiseCall d = c;
    d.rgba = st.at<float4>(0);
    d.feat = st.at<float4>(1);
    d.out = st.at<float4>(2);
    d.scratch = st.at<float4>(3);
    d.mom = st.at<float4>(4);
    d.out_var = st.at<float>(5);
    d.rgb8 = st.at<uint8_t>(6);
    HIP_TRY(ctx, hipMemcpyAsync((void *)d.rgba, c.rgba, b_rgba, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync((void *)d.feat, c.feat, 2 * b_rgba, hipMemcpyHostToDevice, s));
    if (c.var) HIP_TRY(ctx, hipMemcpyAsync((void *)d.mom, c.mom, b_rgba, hipMemcpyHostToDevice, s));
    if (int rc = denoise_launch(ctx, d, s)) return rc;
    if (d.out) HIP_TRY(ctx, hipMemcpyAsync(c.out, d.out, b_rgba, hipMemcpyDeviceToHost, s));
    if (d.rgb8) HIP_TRY(ctx, hipMemcpyAsync(c.rgb8, d.rgb8, npix * 3, hipMemcpyDeviceToHost, s));
    if (d.out_var) HIP_TRY(ctx, hipMemcpyAsync(c.out_var, d.out_var, npix * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return st.done(SPT_OK);
}

}  // namespace

}  // namespace spt_api

extern "C" {

int spt_denoise_scratch_bytes(uint32_t width, uint32_t height, uint32_t levels, uint64_t *bytes)
{
    if (!bytes) return fail(nullptr, SPT_ERR_ARG, "null bytes");
    if (levels < 1u || levels > kMaxLevels) return fail(nullptr, SPT_ERR_ARG, "levels %u outside 1..%u", levels, kMaxLevels);
    const uint64_t npix = (uint64_t)width * height;
    if (npix >= 0x80000000ull) return fail(nullptr, SPT_ERR_ARG, "%u x %u pixels exceed 2^31 - 1", width, height);
    *bytes = scratch_bytes(npix, levels);
    return SPT_OK;
}

int spt_denoise_async(spt_ctx *ctx, uint32_t width, uint32_t height, const void *d_rgba, const void *d_feat,
                      float sigma_color, float sigma_albedo, float sigma_normal, float sigma_depth, uint32_t levels,
                      void *d_out_rgba, void *d_out_rgb8, void *d_scratch, void *stream)
{
    const hipStream_t s = (hipStream_t)stream;
    return denoise_run(ctx, {false, width, height, d_rgba, d_feat, nullptr,
                             {sigma_color, sigma_albedo, sigma_normal, sigma_depth}, 0.0f, levels, d_out_rgba, d_out_rgb8,
                             nullptr, d_scratch}, &s);
}

int spt_denoise(spt_ctx *ctx, uint32_t width, uint32_t height, const float *rgba, const float *feat, float sigma_color,
                float sigma_albedo, float sigma_normal, float sigma_depth, uint32_t levels, float *out_rgba, uint8_t *out_rgb8)
{
    return denoise_run(ctx, {false, width, height, rgba, feat, nullptr,
                             {sigma_color, sigma_albedo, sigma_normal, sigma_depth}, 0.0f, levels, out_rgba, out_rgb8,
                             nullptr, nullptr}, nullptr);
}

int spt_denoise_var_async(spt_ctx *ctx, uint32_t width, uint32_t height, const void *d_rgba, const void *d_feat,
                          const void *d_mom, float sigma_color, float sigma_albedo, float sigma_normal, float sigma_depth,
                          float var_floor, uint32_t levels, void *d_out_rgba, void *d_out_rgb8, void *d_out_var,
                          void *d_scratch, void *stream)
{
    const hipStream_t s = (hipStream_t)stream;
    return denoise_run(ctx, {true, width, height, d_rgba, d_feat, d_mom,
                             {sigma_color, sigma_albedo, sigma_normal, sigma_depth}, var_floor, levels, d_out_rgba, d_out_rgb8,
                             d_out_var, d_scratch}, &s);
}

int spt_denoise_var(spt_ctx *ctx, uint32_t width, uint32_t height, const float *rgba, const float *feat, const float *mom,
                    float sigma_color, float sigma_albedo, float sigma_normal, float sigma_depth, float var_floor,
                    uint32_t levels, float *out_rgba, uint8_t *out_rgb8, float *out_var)
{
    return denoise_run(ctx, {true, width, height, rgba, feat, mom,
                             {sigma_color, sigma_albedo, sigma_normal, sigma_depth}, var_floor, levels, out_rgba, out_rgb8,
                             out_var, nullptr}, nullptr);
}

}  // extern "C"
