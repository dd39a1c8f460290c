// spt_moments.hip -- per-pixel luminance moments of a region's sample words:
// spt_render_moments[_async] (spt_moments.cpp; the definition is include/spt_hip.h "sample
// moments").
//
// One lane per pixel, in the fold's order: thread i takes the i-th pixel of the region's
// 8x8 tiles (tile_pixel), so the 64 lanes of a wave read 64 consecutive words per sample
// (ts_slot_base) -- one 256-byte run, as fold_kernel.  A lane keeps kMomRun words' loads in
// flight before it decodes any (decode_word, the fold's own colour of a word: through the
// scene's colour table where the context has one, TAB), then adds
// them in sample order; the remainder goes word by word.  One float4 store per pixel, in
// local row-major order (so a wave's stores are eight 128-byte rows of a tile).  The pass is
// bound by memory: 4 B read per sample, 16 B written per pixel.
#include "spt_decode.h"

namespace spt {

// words loaded ahead per lane (fold_pixel's SPT_FOLD_RUN)
#ifndef SPT_MOM_RUN
#define SPT_MOM_RUN 8
#endif
constexpr int kMomRun = SPT_MOM_RUN;

template <bool TAB>
__global__ __launch_bounds__(256) void moments_kernel(FoldArgs a, float4 *mom)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.npix) return;
    const uint32_t W = a.map.width, rows = a.npix / W, S = a.spp_batch;
    uint32_t lr, col, q0, step;
    tile_pixel(i, W, rows, lr, col);
    ts_slot_base(lr, col, W, rows, S, q0, step);
    float s1 = 0.0f, s2 = 0.0f;
    auto add = [&](uint32_t w) {
        const f3 c = decode_word<TAB>(a, w);
        const float L = (c.x * 0.2126f + c.y * 0.7152f) + c.z * 0.0722f;
        s1 = s1 + L;
        s2 = s2 + L * L;
    };
    uint32_t k = 0;
    for (; k + kMomRun <= S; k += kMomRun) {
        uint32_t w[kMomRun];
#pragma unroll
        for (int t = 0; t < kMomRun; ++t) w[t] = a.samples[q0 + (k + t) * step];
#pragma unroll
        for (int t = 0; t < kMomRun; ++t) add(w[t]);
    }
    for (; k < S; ++k) add(a.samples[q0 + k * step]);
    const float inv = 1.0f / (float)S;
    const float m1 = s1 * inv, m2 = s2 * inv;
    const float d = m2 - m1 * m1;
    mom[(size_t)lr * W + col] = make_float4(m1, m2, d < 0.0f ? 0.0f : d, (float)S);  // NaN stays NaN
}

hipError_t launch_moments(const FoldArgs &f, float4 *mom, hipStream_t s)
{
    if (f.npix == 0) return hipSuccess;
    hipLaunchKernelGGL(fold_uses_table(f) ? moments_kernel<true> : moments_kernel<false>, dim3((f.npix + 255u) / 256u), dim3(256), 0, s, f, mom);
    return hipGetLastError();
}

}  // namespace spt
