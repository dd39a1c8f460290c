// spt_temporal.cpp -- temporal accumulation: spt_temporal_inverse and
// spt_temporal[_async] and spt_temporal_motion[_async] (§4.15: the same call with a table of
// the spheres' motion), the host half of spt_temporal.hip.  Like the denoiser they need no
// scene, camera or params, use member 0 of a multi-device context, end a resident service
// session first, touch neither the statistics nor the sample workspaces and read no candidate
// lists.  The library keeps no history: the caller passes the last frame's outputs back in.
#include "spt_host.h"

namespace spt_api {

namespace {

// the fp32 inverse of view's upper-left 3x3: adjugate over determinant in double, each entry
// rounded once; false for a non-finite entry or a determinant that is not finite and != 0
bool inverse3(const float view[16], float inv9[9])
{
    double m[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            m[i][j] = (double)view[4 * i + j];
            if (!std::isfinite(m[i][j])) return false;
        }
    double adj[3][3];  // adj[i][j] = cofactor of m[j][i]
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
            adj[i][j] = m[r0][c0] * m[r1][c1] - m[r0][c1] * m[r1][c0];
        }
    const double det = m[0][0] * adj[0][0] + m[0][1] * adj[1][0] + m[0][2] * adj[2][0];
    if (!std::isfinite(det) || det == 0.0) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) inv9[3 * i + j] = (float)(adj[i][j] / det);
    return true;
}

// One call of either form, as its entry point received it: host pointers for the blocking
// form, device pointers for the async one.
struct TemporalCall {
    uint32_t W, H;
    const void *rgba, *mom, *feat, *ids;
    const float *view, *eye;
    const void *h_rgba, *h_mom, *h_feat, *h_ids;
    const float *prev_view, *prev_eye;
    float tol_normal, tol_depth, max_history;
    void *out_rgba, *out_mom;
    bool with_motion = false;      // the motion entry points: the table below is an argument
    const void *motion = nullptr;  // n_spheres records of 8 floats (null with n_spheres == 0)
    uint32_t n_spheres = 0;
};

// the checks; on SPT_OK with *nothing clear, `a` holds the cameras and the parameters
int temporal_check(spt_ctx *ctx, const TemporalCall &c, spt::TemporalArgs *a, bool *nothing)
{
    *nothing = false;
    if (!c.rgba || !c.mom || !c.feat || !c.ids) return fail(ctx, SPT_ERR_ARG, "null rgba, mom, feat or ids");
    if (!c.view || !c.eye) return fail(ctx, SPT_ERR_ARG, "null view or eye");
    if (!c.out_rgba || !c.out_mom) return fail(ctx, SPT_ERR_ARG, "null out_rgba or out_mom");
    if (c.n_spheres > 0 && !c.motion) return fail(ctx, SPT_ERR_ARG, "null motion with n_spheres = %u", c.n_spheres);
    const int n_hist = (c.h_rgba != nullptr) + (c.h_mom != nullptr) + (c.h_feat != nullptr) + (c.h_ids != nullptr);
    if (n_hist != 0 && n_hist != 4) return fail(ctx, SPT_ERR_ARG, "%d of the four history pointers are null: all or none", 4 - n_hist);
    const bool hist = n_hist == 4;
    if (!(c.tol_normal >= 0.0f)) return fail(ctx, SPT_ERR_ARG, "tol_normal is %g: must be >= 0 (+inf switches the test off)", (double)c.tol_normal);
    if (!(c.tol_depth >= 0.0f)) return fail(ctx, SPT_ERR_ARG, "tol_depth is %g: must be >= 0 (+inf switches the test off)", (double)c.tol_depth);
    if (!(c.max_history > 0.0f)) return fail(ctx, SPT_ERR_ARG, "max_history is %g: must be > 0", (double)c.max_history);
    *a = spt::TemporalArgs{};
    if (hist) {
        if (!c.prev_view || !c.prev_eye) return fail(ctx, SPT_ERR_ARG, "null prev_view or prev_eye with a history");
        if (!inverse3(c.prev_view, a->minv)) return fail(ctx, SPT_ERR_ARG, "prev_view: its 3x3 block has a non-finite entry or no inverse");
    }
    const uint64_t npix = (uint64_t)c.W * c.H;
    if (npix >= 0x80000000ull) return fail(ctx, SPT_ERR_ARG, "%u x %u pixels exceed 2^31 - 1", c.W, c.H);
    if (npix == 0) {
        *nothing = true;
        return SPT_OK;
    }
    const struct {
        const void *p;
        uint64_t n;
        const char *name;
    } outs[2] = {{c.out_rgba, npix * 16u, "out_rgba"}, {c.out_mom, npix * 16u, "out_mom"}},
      ins[9] = {{c.rgba, npix * 16u, "rgba"}, {c.mom, npix * 16u, "mom"}, {c.feat, npix * 32u, "feat"}, {c.ids, npix * 4u, "ids"},
                {c.h_rgba, npix * 16u, "hist_rgba"}, {c.h_mom, npix * 16u, "hist_mom"}, {c.h_feat, npix * 32u, "hist_feat"},
                {c.h_ids, npix * 4u, "hist_ids"}, {c.n_spheres ? c.motion : nullptr, (uint64_t)c.n_spheres * 32u, "motion"}};
    // An output that overlaps one buffer usually runs on into whatever the allocator placed
    // beside it, so several overlaps can hold at once.  The one named must not depend on
    // those neighbours: first the motion table (the one input that is no image plane: an
    // output may reach it with its last bytes only), then the buffer an output BEGINS in --
    // an input before the other output --, then any other overlap in argument order.
    const auto begins_in = [](const void *o, const void *p, uint64_t n) { return overlaps(o, 1, p, n); };
    for (const auto &o : outs)
        if (overlaps(o.p, o.n, ins[8].p, ins[8].n)) return fail(ctx, SPT_ERR_ARG, "%s overlaps %s", o.name, ins[8].name);
    for (const auto &o : outs)
        for (const auto &i : ins)
            if (begins_in(o.p, i.p, i.n)) return fail(ctx, SPT_ERR_ARG, "%s overlaps %s", o.name, i.name);
    if (begins_in(outs[0].p, outs[1].p, outs[1].n) || begins_in(outs[1].p, outs[0].p, outs[0].n))
        return fail(ctx, SPT_ERR_ARG, "out_rgba overlaps out_mom");
    for (const auto &o : outs)
        for (const auto &i : ins)
            if (overlaps(o.p, o.n, i.p, i.n)) return fail(ctx, SPT_ERR_ARG, "%s overlaps %s", o.name, i.name);
    // (two overlapping outputs: the later one begins in the earlier, caught above)
    a->width = c.W;
    a->height = c.H;
    a->fw = (float)c.W;
    a->fh = (float)c.H;
    bool same = hist;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            a->m[3 * i + j] = c.view[4 * i + j];
            same = same && c.view[4 * i + j] == c.prev_view[4 * i + j];
        }
        a->e[i] = c.eye[i];
        if (hist) a->ep[i] = c.prev_eye[i];
        same = same && c.eye[i] == c.prev_eye[i];
    }
    a->is_static = same;
    a->tol_normal = c.tol_normal;
    a->tol_depth = c.tol_depth;
    a->max_history = c.max_history;
    return SPT_OK;
}

int temporal_launch(spt_ctx *ctx, const TemporalCall &c, spt::TemporalArgs a, hipStream_t s)
{
    if (int rc = svc_end(ctx)) return rc;
    a.rgba = (const float4 *)c.rgba;
    a.mom = (const float4 *)c.mom;
    a.feat = (const float4 *)c.feat;
    a.ids = (const uint32_t *)c.ids;
    a.h_rgba = (const float4 *)c.h_rgba;
    a.h_mom = (const float4 *)c.h_mom;
    a.h_feat = (const float4 *)c.h_feat;
    a.h_ids = (const uint32_t *)c.h_ids;
    a.out_rgba = (float4 *)c.out_rgba;
    a.out_mom = (float4 *)c.out_mom;
    a.motion = c.n_spheres ? (const float4 *)c.motion : nullptr;
    a.n_spheres = c.n_spheres;
    HIP_TRY(ctx, spt::launch_temporal(a, c.with_motion, s));
    return SPT_OK;
}

// what both entry points do: the checks, then the launch on the caller's stream over the
// caller's device pointers (stream non-null; *stream NULL = the HIP default stream), or the
// blocking form over one allocation (temporal_plan)
int temporal_run(spt_ctx *ctx, const TemporalCall &c, const hipStream_t *stream)
{
    if (!ctx) return fail(nullptr, SPT_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool nothing;
    spt::TemporalArgs a;
    if (int rc = temporal_check(ctx, c, &a, &nothing)) return rc;
    if (nothing) return SPT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (stream) return temporal_launch(ctx, c, a, *stream);
    const size_t npix = (size_t)c.W * c.H, b16 = npix * sizeof(float4);
    const bool hist = c.h_rgba != nullptr;
    const hipStream_t s = ctx->stream;
    Staging st;
    const size_t table = (size_t)c.n_spheres * 32;
    if (!st.alloc(temporal_plan(npix, hist, table), s)) return fail(ctx, SPT_ERR_NOMEM, "spt_temporal: %zu bytes of device buffers", st.plan.total);
    TemporalCall d = c;
    char *cur = st.at<char>(0), *old = st.at<char>(2), *out = st.at<char>(4);
    d.rgba = cur;
    d.mom = cur + b16;
    d.feat = cur + 2 * b16;
    d.ids = st.at<uint32_t>(1);
    d.h_rgba = hist ? old : nullptr;
    d.h_mom = hist ? old + b16 : nullptr;
    d.h_feat = hist ? old + 2 * b16 : nullptr;
    d.h_ids = st.at<uint32_t>(3);
    d.out_rgba = out;
    d.out_mom = out + b16;
    d.motion = st.at<char>(5);
    if (table) HIP_TRY(ctx, hipMemcpyAsync((void *)d.motion, c.motion, table, hipMemcpyHostToDevice, s));
    const struct {
        const void *dst, *src;
        size_t n;
    } in[8] = {{d.rgba, c.rgba, b16}, {d.mom, c.mom, b16}, {d.feat, c.feat, 2 * b16}, {d.ids, c.ids, npix * 4},
               {d.h_rgba, c.h_rgba, b16}, {d.h_mom, c.h_mom, b16}, {d.h_feat, c.h_feat, 2 * b16}, {d.h_ids, c.h_ids, npix * 4}};
    for (const auto &i : in)
        if (i.dst) HIP_TRY(ctx, hipMemcpyAsync((void *)i.dst, i.src, i.n, hipMemcpyHostToDevice, s));
    if (int rc = temporal_launch(ctx, d, a, s)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(c.out_rgba, d.out_rgba, b16, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(c.out_mom, d.out_mom, b16, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return st.done(SPT_OK);
}

}  // namespace

}  // namespace spt_api

extern "C" {

int spt_temporal_inverse(const float view[16], float inv9[9])
{
    if (!view || !inv9) return fail(nullptr, SPT_ERR_ARG, "null view or inv9");
    float r[9];
    if (!inverse3(view, r)) return fail(nullptr, SPT_ERR_ARG, "view: its 3x3 block has a non-finite entry or no inverse");
    std::memcpy(inv9, r, sizeof r);
    return SPT_OK;
}

int spt_temporal_async(spt_ctx *ctx, uint32_t width, uint32_t height, const void *d_rgba, const void *d_mom,
                       const void *d_feat, const void *d_ids, const float view[16], const float eye[4],
                       const void *d_hist_rgba, const void *d_hist_mom, const void *d_hist_feat, const void *d_hist_ids,
                       const float prev_view[16], const float prev_eye[4], float tol_normal, float tol_depth,
                       float max_history, void *d_out_rgba, void *d_out_mom, void *stream)
{
    const hipStream_t s = (hipStream_t)stream;
    return temporal_run(ctx, {width, height, d_rgba, d_mom, d_feat, d_ids, view, eye, d_hist_rgba, d_hist_mom, d_hist_feat,
                              d_hist_ids, prev_view, prev_eye, tol_normal, tol_depth, max_history, d_out_rgba, d_out_mom}, &s);
}

int spt_temporal_motion_async(spt_ctx *ctx, uint32_t width, uint32_t height, const void *d_rgba, const void *d_mom,
                              const void *d_feat, const void *d_ids, const float view[16], const float eye[4],
                              const void *d_hist_rgba, const void *d_hist_mom, const void *d_hist_feat,
                              const void *d_hist_ids, const float prev_view[16], const float prev_eye[4],
                              const void *d_motion, uint32_t n_spheres, float tol_normal, float tol_depth,
                              float max_history, void *d_out_rgba, void *d_out_mom, void *stream)
{
    const hipStream_t s = (hipStream_t)stream;
    return temporal_run(ctx, {width, height, d_rgba, d_mom, d_feat, d_ids, view, eye, d_hist_rgba, d_hist_mom, d_hist_feat,
                              d_hist_ids, prev_view, prev_eye, tol_normal, tol_depth, max_history, d_out_rgba, d_out_mom,
                              true, d_motion, n_spheres}, &s);
}

int spt_temporal_motion(spt_ctx *ctx, uint32_t width, uint32_t height, const float *rgba, const float *mom,
                        const float *feat, const uint32_t *ids, const float view[16], const float eye[4],
                        const float *hist_rgba, const float *hist_mom, const float *hist_feat, const uint32_t *hist_ids,
                        const float prev_view[16], const float prev_eye[4], const float *motion, uint32_t n_spheres,
                        float tol_normal, float tol_depth, float max_history, float *out_rgba, float *out_mom)
{
    return temporal_run(ctx, {width, height, rgba, mom, feat, ids, view, eye, hist_rgba, hist_mom, hist_feat, hist_ids,
                              prev_view, prev_eye, tol_normal, tol_depth, max_history, out_rgba, out_mom, true, motion,
                              n_spheres}, nullptr);
}

int spt_temporal(spt_ctx *ctx, uint32_t width, uint32_t height, const float *rgba, const float *mom, const float *feat,
                 const uint32_t *ids, const float view[16], const float eye[4], const float *hist_rgba,
                 const float *hist_mom, const float *hist_feat, const uint32_t *hist_ids, const float prev_view[16],
                 const float prev_eye[4], float tol_normal, float tol_depth, float max_history, float *out_rgba,
                 float *out_mom)
{
    return temporal_run(ctx, {width, height, rgba, mom, feat, ids, view, eye, hist_rgba, hist_mom, hist_feat, hist_ids,
                              prev_view, prev_eye, tol_normal, tol_depth, max_history, out_rgba, out_mom}, nullptr);
}

}  // extern "C"
