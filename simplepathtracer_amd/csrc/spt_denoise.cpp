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

inline bool overlaps(const void *a, uint64_t na, const void *b, uint64_t nb)
{
    if (!a || !b || !na || !nb) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// the checks both forms share; *nothing: an empty image, the call is over
int denoise_check(spt_ctx *ctx, uint32_t W, uint32_t H, const void *rgba, const void *feat, const float sigma[4],
                  uint32_t levels, const void *out, const void *rgb8, const void *scratch, bool need_scratch,
                  bool *nothing)
{
    *nothing = false;
    if (!rgba || !feat) return fail(ctx, SPT_ERR_ARG, "null rgba or feat");
    if (!out && !rgb8) return fail(ctx, SPT_ERR_ARG, "null out_rgba and out_rgb8");
    if (levels < 1u || levels > kMaxLevels) return fail(ctx, SPT_ERR_ARG, "levels %u outside 1..%u", levels, kMaxLevels);
    for (int t = 0; t < 4; ++t)
        if (!(sigma[t] > 0.0f)) return fail(ctx, SPT_ERR_ARG, "sigma %d is %g: must be > 0 (+inf switches the term off)", t, (double)sigma[t]);
    const uint64_t npix = (uint64_t)W * H;
    if (npix >= 0x80000000ull) return fail(ctx, SPT_ERR_ARG, "%u x %u pixels exceed 2^31 - 1", W, H);
    if (npix == 0) {
        *nothing = true;
        return SPT_OK;
    }
    const uint64_t sb = scratch_bytes(npix, levels);
    if (need_scratch && sb && !scratch) return fail(ctx, SPT_ERR_ARG, "null scratch (spt_denoise_scratch_bytes: %llu)", (unsigned long long)sb);
    const struct {
        const void *p;
        uint64_t n;
        const char *name;
    } outs[2] = {{out, npix * 16u, "out_rgba"}, {rgb8, npix * 3u, "out_rgb8"}},
      ins[3] = {{rgba, npix * 16u, "rgba"}, {feat, npix * 32u, "feat"}, {need_scratch ? scratch : nullptr, sb, "scratch"}};
    for (const auto &o : outs)
        for (const auto &i : ins)
            if (overlaps(o.p, o.n, i.p, i.n)) return fail(ctx, SPT_ERR_ARG, "%s overlaps %s", o.name, i.name);
    if (overlaps(out, npix * 16u, rgb8, npix * 3u)) return fail(ctx, SPT_ERR_ARG, "out_rgba overlaps out_rgb8");
    return SPT_OK;
}

// the levels, one launch each on `s`: level 0 reads rgba, level k > 0 the plane level k - 1
// wrote, the last writes the caller's outputs
int denoise_launch(spt_ctx *ctx, uint32_t W, uint32_t H, const float4 *d_rgba, const float4 *d_feat, const float sigma[4],
                   uint32_t levels, float4 *d_out, uint8_t *d_rgb8, float4 *d_scratch, hipStream_t s)
{
    if (int rc = svc_end(ctx)) return rc;
    float k[4];
    for (int t = 0; t < 4; ++t) {
        const float s2 = sigma[t] * sigma[t];
        k[t] = 1.0f / s2;
    }
    const size_t npix = (size_t)W * H;
    const float4 *in = d_rgba;
    for (uint32_t lv = 0; lv < levels; ++lv) {
        const bool last = lv + 1u == levels;
        spt::DenoiseArgs a{};
        a.in = in;
        a.feat = d_feat;
        a.out = last ? d_out : d_scratch + (size_t)(lv & 1u) * npix;
        a.rgb8 = last ? d_rgb8 : nullptr;
        a.width = W;
        a.height = H;
        a.step = 1u << lv;
        a.sx = std::min(a.step, W);
        a.sy = std::min(a.step, H);
        a.tiles_x = ((W + a.step - 1u) / a.step + 15u) / 16u;
        a.tiles_y = ((H + a.step - 1u) / a.step + 15u) / 16u;
        a.kc = k[0] * (float)(1u << (2u * lv));  // the colour sigma halves per level; exact
        a.ka = k[1];
        a.kn = k[2];
        a.kz = k[3];
        HIP_TRY(ctx, spt::launch_denoise_level(a, s));
        in = a.out;
    }
    return SPT_OK;
}

// spt_denoise_var's checks: spt_denoise's, then mom, var_floor and out_var
int denoise_var_check(spt_ctx *ctx, uint32_t W, uint32_t H, const void *rgba, const void *feat, const void *mom,
                      const float sigma[4], float var_floor, uint32_t levels, const void *out, const void *rgb8,
                      const void *out_var, const void *scratch, bool need_scratch, bool *nothing)
{
    if (int rc = denoise_check(ctx, W, H, rgba, feat, sigma, levels, out, rgb8, scratch, need_scratch, nothing)) return rc;
    if (*nothing) return SPT_OK;
    if (!mom) return fail(ctx, SPT_ERR_ARG, "null mom");
    if (!(var_floor > 0.0f) || !std::isfinite(var_floor))
        return fail(ctx, SPT_ERR_ARG, "var_floor is %g: must be finite and > 0", (double)var_floor);
    const uint64_t npix = (uint64_t)W * H;
    const struct {
        const void *p;
        uint64_t n;
        const char *name;
    } outs[3] = {{out, npix * 16u, "out_rgba"}, {rgb8, npix * 3u, "out_rgb8"}, {out_var, npix * 4u, "out_var"}},
      ins[4] = {{rgba, npix * 16u, "rgba"}, {feat, npix * 32u, "feat"}, {mom, npix * 16u, "mom"},
                {need_scratch ? scratch : nullptr, scratch_bytes(npix, levels), "scratch"}};
    for (const auto &o : outs)
        for (const auto &i : ins)
            if (overlaps(o.p, o.n, i.p, i.n)) return fail(ctx, SPT_ERR_ARG, "%s overlaps %s", o.name, i.name);
    for (int t = 0; t < 2; ++t)
        if (overlaps(out_var, npix * 4u, outs[t].p, outs[t].n)) return fail(ctx, SPT_ERR_ARG, "out_var overlaps %s", outs[t].name);
    return SPT_OK;
}

// the variance-guided levels, as denoise_launch: the planes between levels carry g in
// their w lane, and the last level takes the output's w lane from d_rgba
int denoise_var_launch(spt_ctx *ctx, uint32_t W, uint32_t H, const float4 *d_rgba, const float4 *d_feat, const float4 *d_mom,
                       const float sigma[4], float var_floor, uint32_t levels, float4 *d_out, uint8_t *d_rgb8,
                       float *d_out_var, float4 *d_scratch, hipStream_t s)
{
    if (int rc = svc_end(ctx)) return rc;
    float k[4];
    for (int t = 0; t < 4; ++t) {
        const float s2 = sigma[t] * sigma[t];
        k[t] = 1.0f / s2;
    }
    const size_t npix = (size_t)W * H;
    const float4 *in = d_rgba;
    for (uint32_t lv = 0; lv < levels; ++lv) {
        const bool last = lv + 1u == levels;
        spt::DenoiseVarArgs a{};
        a.in = in;
        a.feat = d_feat;
        a.mom = d_mom;
        a.rgba = last ? d_rgba : nullptr;
        a.out = last ? d_out : d_scratch + (size_t)(lv & 1u) * npix;
        a.out_var = last ? d_out_var : nullptr;
        a.rgb8 = last ? d_rgb8 : nullptr;
        a.width = W;
        a.height = H;
        a.step = 1u << lv;
        a.sx = std::min(a.step, W);
        a.sy = std::min(a.step, H);
        a.tiles_x = ((W + a.step - 1u) / a.step + 15u) / 16u;
        a.tiles_y = ((H + a.step - 1u) / a.step + 15u) / 16u;
        a.first = lv == 0;
        a.kc = k[0];  // sigma_color counts standard deviations at every level
        a.ka = k[1];
        a.kn = k[2];
        a.kz = k[3];
        a.var_floor = var_floor;
        HIP_TRY(ctx, spt::launch_denoise_var_level(a, s));
        in = a.out;
    }
    return SPT_OK;
}

}  // namespace

}  // namespace spt_api

extern "C" {

int spt_denoise_var_async(spt_ctx *ctx, uint32_t width, uint32_t height, const void *d_rgba, const void *d_feat,
                          const void *d_mom, float sigma_color, float sigma_albedo, float sigma_normal, float sigma_depth,
                          float var_floor, uint32_t levels, void *d_out_rgba, void *d_out_rgb8, void *d_out_var,
                          void *d_scratch, void *stream)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    const float sigma[4] = {sigma_color, sigma_albedo, sigma_normal, sigma_depth};
    bool nothing;
    if (int rc = denoise_var_check(ctx, width, height, d_rgba, d_feat, d_mom, sigma, var_floor, levels, d_out_rgba, d_out_rgb8,
                                   d_out_var, d_scratch, true, &nothing))
        return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return denoise_var_launch(ctx, width, height, (const float4 *)d_rgba, (const float4 *)d_feat, (const float4 *)d_mom, sigma,
                              var_floor, levels, (float4 *)d_out_rgba, (uint8_t *)d_out_rgb8, (float *)d_out_var,
                              (float4 *)d_scratch, (hipStream_t)stream);  // NULL = the HIP default stream
}

int spt_denoise_var(spt_ctx *ctx, uint32_t width, uint32_t height, const float *rgba, const float *feat, const float *mom,
                    float sigma_color, float sigma_albedo, float sigma_normal, float sigma_depth, float var_floor,
                    uint32_t levels, float *out_rgba, uint8_t *out_rgb8, float *out_var)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    const float sigma[4] = {sigma_color, sigma_albedo, sigma_normal, sigma_depth};
    bool nothing;
    if (int rc = denoise_var_check(ctx, width, height, rgba, feat, mom, sigma, var_floor, levels, out_rgba, out_rgb8, out_var,
                                   nullptr, false, &nothing))
        return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // spt_denoise's allocation, and a second one for mom and out_var
    const size_t npix = (size_t)width * height, b_rgba = npix * sizeof(float4);
    const hipStream_t s = ctx->stream;
    Staging st, sv;
    if (!st.alloc(denoise_plan(npix, (size_t)scratch_planes(levels), out_rgba != nullptr, out_rgb8 != nullptr), s))
        return fail(ctx, SPT_ERR_NOMEM, "spt_denoise_var: %zu bytes of device buffers", st.plan.total);
    if (!sv.alloc(denoise_var_plan(npix, out_var != nullptr), s))
        return fail(ctx, SPT_ERR_NOMEM, "spt_denoise_var: %zu bytes of device buffers", sv.plan.total);
    float4 *d_rgba = st.at<float4>(0), *d_feat = st.at<float4>(1), *d_out = st.at<float4>(2), *d_scr = st.at<float4>(3);
    uint8_t *d_rgb8 = st.at<uint8_t>(4);
    float4 *d_mom = sv.at<float4>(0);
    float *d_var = sv.at<float>(1);
    HIP_TRY(ctx, hipMemcpyAsync(d_rgba, rgba, b_rgba, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d_feat, feat, 2 * b_rgba, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d_mom, mom, b_rgba, hipMemcpyHostToDevice, s));
    if (int rc = denoise_var_launch(ctx, width, height, d_rgba, d_feat, d_mom, sigma, var_floor, levels, d_out, d_rgb8, d_var,
                                    d_scr, s))
        return rc;
    if (out_rgba) HIP_TRY(ctx, hipMemcpyAsync(out_rgba, d_out, b_rgba, hipMemcpyDeviceToHost, s));
    if (out_rgb8) HIP_TRY(ctx, hipMemcpyAsync(out_rgb8, d_rgb8, npix * 3, hipMemcpyDeviceToHost, s));
    if (out_var) HIP_TRY(ctx, hipMemcpyAsync(out_var, d_var, npix * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    sv.done(SPT_OK);
    return st.done(SPT_OK);
}

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
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    const float sigma[4] = {sigma_color, sigma_albedo, sigma_normal, sigma_depth};
    bool nothing;
    if (int rc = denoise_check(ctx, width, height, d_rgba, d_feat, sigma, levels, d_out_rgba, d_out_rgb8, d_scratch, true, &nothing))
        return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return denoise_launch(ctx, width, height, (const float4 *)d_rgba, (const float4 *)d_feat, sigma, levels, (float4 *)d_out_rgba,
                          (uint8_t *)d_out_rgb8, (float4 *)d_scratch, (hipStream_t)stream);  // NULL = the HIP default stream
}

int spt_denoise(spt_ctx *ctx, uint32_t width, uint32_t height, const float *rgba, const float *feat, float sigma_color,
                float sigma_albedo, float sigma_normal, float sigma_depth, uint32_t levels, float *out_rgba, uint8_t *out_rgb8)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    const float sigma[4] = {sigma_color, sigma_albedo, sigma_normal, sigma_depth};
    bool nothing;
    if (int rc = denoise_check(ctx, width, height, rgba, feat, sigma, levels, out_rgba, out_rgb8, nullptr, false, &nothing)) return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // one allocation: rgba, feat, out, the scratch planes, then the bytes
    const size_t npix = (size_t)width * height, b_rgba = npix * sizeof(float4);
    const hipStream_t s = ctx->stream;
    Staging st;
    if (!st.alloc(denoise_plan(npix, (size_t)scratch_planes(levels), out_rgba != nullptr, out_rgb8 != nullptr), s))
        return fail(ctx, SPT_ERR_NOMEM, "spt_denoise: %zu bytes of device buffers", st.plan.total);
    float4 *d_rgba = st.at<float4>(0), *d_feat = st.at<float4>(1), *d_out = st.at<float4>(2), *d_scr = st.at<float4>(3);
    uint8_t *d_rgb8 = st.at<uint8_t>(4);
    HIP_TRY(ctx, hipMemcpyAsync(d_rgba, rgba, b_rgba, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d_feat, feat, 2 * b_rgba, hipMemcpyHostToDevice, s));
    if (int rc = denoise_launch(ctx, width, height, d_rgba, d_feat, sigma, levels, d_out, d_rgb8, d_scr, s)) return rc;
    if (out_rgba) HIP_TRY(ctx, hipMemcpyAsync(out_rgba, d_out, b_rgba, hipMemcpyDeviceToHost, s));
    if (out_rgb8) HIP_TRY(ctx, hipMemcpyAsync(out_rgb8, d_rgb8, npix * 3, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return st.done(SPT_OK);
}

}  // extern "C"
