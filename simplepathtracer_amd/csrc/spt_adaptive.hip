// spt_adaptive.hip -- adaptive sampling's device code between render launches:
// spt_render_adaptive[_dev] (spt_adaptive.cpp; the definition is include/spt_hip.h "adaptive
// sampling").  The passes themselves are batched launches of the render
// kernels over the table adaptive_plan_kernel writes; nothing of spt_kernels.hip changes.
//
// adaptive_fold_kernel: one wave per rectangle (an 8x8 tile, ragged at the region's right and
// bottom edges) of the pass's table, lane i its i-th pixel in tile_pixel order.  A pass's
// words for a tile are [sample][pixel] (ts_slot_base over the tile alone), so each sample is
// one run of at most 256 bytes per wave.  A lane keeps kAdaptRun words' loads in flight
// before it decodes any (decode_word, the fold's own colour of a word), continues the
// pixel's in-order sums, evaluates the rule, and one ballot gives the tile's verdict: a tile
// still active raises its flag, a tile that is not writes its pixels' outputs.  Bound by
// memory: 4 B read per sample, 24 B of state read and written per pixel and pass.
//
// adaptive_plan_kernel: one block.  An ordered scan of the tile flags (each thread a run of
// consecutive tiles, the runs' sums scanned through LDS) gives every active tile the padded
// items and the words of the active tiles before it; adaptive_rect (spt_adaptive.h) turns
// them into its BatchRect.  The counts go to page-locked host words the host loop waits for.
#include "spt_adaptive.h"
#include "spt_decode.h"

namespace spt {

// words loaded ahead per lane (fold_pixel's SPT_FOLD_RUN, moments_kernel's SPT_MOM_RUN)
#ifndef SPT_ADAPT_RUN
#define SPT_ADAPT_RUN 8
#endif
constexpr int kAdaptRun = SPT_ADAPT_RUN;
constexpr uint32_t kPlanThreads = 1024;

__global__ __launch_bounds__(kPlanThreads) void adaptive_plan_kernel(AdaptGeom g, uint32_t *flags, BatchRect *rects,
                                                                     AdaptCount *count)
{
    __shared__ uint32_t sh[3][kPlanThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t n_tiles = g.tiles_x * g.tiles_y;
    const uint32_t per = (n_tiles + kPlanThreads - 1u) / kPlanThreads;
    const uint32_t t0 = min(t * per, n_tiles), t1 = min(t0 + per, n_tiles);
    AdaptSum own{0u, 0u, 0u};
    for (uint32_t i = t0; i < t1; ++i)
        if (flags[i] != 0u) adaptive_add(g, i, own);
    sh[0][t] = own.rects;
    sh[1][t] = own.items;
    sh[2][t] = own.slots;
    __syncthreads();
    for (uint32_t off = 1; off < kPlanThreads; off <<= 1) {
        uint32_t v[3] = {0u, 0u, 0u};
        if (t >= off)
            for (int k = 0; k < 3; ++k) v[k] = sh[k][t - off];
        __syncthreads();
        for (int k = 0; k < 3; ++k) sh[k][t] += v[k];
        __syncthreads();
    }
    const uint32_t n_rects = sh[0][kPlanThreads - 1u];
    // the sums over the active tiles before this thread's run
    AdaptSum at{sh[0][t] - own.rects, sh[1][t] - own.items, sh[2][t] - own.slots};
    for (uint32_t i = t0; i < t1; ++i) {
        if (flags[i] == 0u) continue;
        flags[i] = 0u;
        const BatchRect b = adaptive_rect(g, i, at.items, at.slots);
        rects[at.rects] = b;
        if (at.rects + 1u == n_rects) count->n_items = b.item_end;
        adaptive_add(g, i, at);
    }
    if (t == 0u) {
        count->n_rects = n_rects;
        count->n_slots = sh[2][kPlanThreads - 1u];
        if (n_rects == 0u) count->n_items = 0u;
    }
}

template <bool TAB>
__global__ __launch_bounds__(256) void adaptive_fold_kernel(FoldArgs f, AdaptGeom g, const BatchRect *rects, AdaptState st,
                                                            AdaptFoldArgs a)
{
    const uint32_t ri = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (ri >= a.n_rects) return;
    const uint32_t lane = threadIdx.x & 63u;
    const BatchRect &r = rects[ri];
    const uint32_t w = r.w, rows = r.rows, npix = r.npix, S = g.take;
    const bool live = lane < npix;  // ragged tiles leave lanes idle
    uint32_t lr = 0, col = 0, q0 = 0, step = 0;
    if (live) {
        tile_pixel(lane, w, rows, lr, col);
        ts_slot_base(lr, col, w, rows, S, q0, step);
    }
    // the pixel in the region (state, rgba, mom: local row-major) and in the frame (bytes)
    const uint32_t x = r.x0 + col, y = r.y0 + lr;
    const size_t p = (size_t)(y - g.y0) * g.w + (x - g.x0);
    const uint32_t n = a.n0 + S;
    bool unconverged = false;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float s1 = 0.f, s2 = 0.f;
    float inv = 0.f, m1 = 0.f, m2 = 0.f, var = 0.f;
    if (live) {
        if (!a.first) {
            acc = st.acc[p];
            const float2 s = st.s12[p];
            s1 = s.x;
            s2 = s.y;
        }
        const uint32_t *words = f.samples + r.slot_off;
        auto add = [&](uint32_t wd) {
            const f3 c = decode_word<TAB>(f, wd);
            acc.x = acc.x + c.x;
            acc.y = acc.y + c.y;
            acc.z = acc.z + c.z;
            const float L = (c.x * 0.2126f + c.y * 0.7152f) + c.z * 0.0722f;
            s1 = s1 + L;
            s2 = s2 + L * L;
        };
        uint32_t k = 0;
        for (; k + kAdaptRun <= S; k += kAdaptRun) {
            uint32_t wd[kAdaptRun];
#pragma unroll
            for (int t = 0; t < kAdaptRun; ++t) wd[t] = words[q0 + (k + t) * step];
#pragma unroll
            for (int t = 0; t < kAdaptRun; ++t) add(wd[t]);
        }
        for (; k < S; ++k) add(words[q0 + k * step]);
        inv = 1.0f / (float)n;
        m1 = s1 * inv;
        m2 = s2 * inv;
        const float d = m2 - m1 * m1;
        var = d < 0.0f ? 0.0f : d;  // NaN stays NaN
        const float e = var * inv;
        const float rr = (m1 + a.lum_floor) * a.tol;
        const float thr = rr * rr;
        unconverged = e > thr;  // NaN compares false: converged
    }
    const bool active = n < a.max_spp && __ballot(unconverged) != 0ull;
    if (active) {
        if (live) {
            st.acc[p] = acc;
            st.s12[p] = make_float2(s1, s2);
        }
        if (lane == 0u) st.flags[r.pix_off] = 1u;
        return;
    }
    if (!live) return;
    const float cr = acc.x * inv, cg = acc.y * inv, cb = acc.z * inv;
    if (a.out_rgba) a.out_rgba[p] = make_float4(cr, cg, cb, 0.f);
    if (a.out_rgb8) {
        const size_t gi = (size_t)3 * ((size_t)(f.height - 1u - y) * f.width + x);
        a.out_rgb8[gi + 0] = gamma_byte(cr);
        a.out_rgb8[gi + 1] = gamma_byte(cg);
        a.out_rgb8[gi + 2] = gamma_byte(cb);
    }
    if (a.mom) a.mom[p] = make_float4(m1, m2, var, (float)n);
}

hipError_t launch_adaptive_plan(const AdaptGeom &g, uint32_t *flags, BatchRect *rects, AdaptCount *count, hipStream_t s)
{
    hipLaunchKernelGGL(adaptive_plan_kernel, dim3(1), dim3(kPlanThreads), 0, s, g, flags, rects, count);
    return hipGetLastError();
}

hipError_t launch_adaptive_fold(const FoldArgs &f, const AdaptGeom &g, const BatchRect *rects, const AdaptState &st,
                                const AdaptFoldArgs &a, hipStream_t s)
{
    if (a.n_rects == 0) return hipSuccess;
    hipLaunchKernelGGL(fold_uses_table(f) ? adaptive_fold_kernel<true> : adaptive_fold_kernel<false>,
                       dim3((a.n_rects + 3u) / 4u), dim3(256), 0, s, f, g, rects, st, a);
    return hipGetLastError();
}

}  // namespace spt
