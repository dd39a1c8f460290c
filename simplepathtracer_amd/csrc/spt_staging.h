// spt_staging.h -- device staging of the blocking queries (spt_cast_rays, spt_primary_hits,
// spt_occluded_rays, spt_trace_rays, spt_render_features, spt_denoise, spt_denoise_var, spt_render_moments,
// spt_render_adaptive, spt_temporal): one
// device allocation cut into the arrays of a chunk of the call's items (rays, rows of
// pixels, or the whole image), which the call copies in, launches over and copies out chunk
// by chunk.  One plan per form (the two filters share denoise_plan: the variance-guided one
// has two more arrays present).  The plan -- chunk size, offsets, total -- is HIP-free
// (standard headers only: tests/cpp/staging_check.cpp drives it on the CPU); Staging, the
// allocation itself, is spt_staging.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace spt_api {

// at most 256 MiB on the device, as spt_render_samples
constexpr size_t kCastStagingBytes = (size_t)256 << 20;
inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
// rays per chunk at per_ray staging bytes each: whole waves, within the staging bound
inline size_t cast_chunk(size_t per_ray) { return std::max<size_t>(64, ((kCastStagingBytes - 64) / per_ray) & ~(size_t)63); }
// rows per chunk at per_row staging bytes each: whole 8-row bands, so a chunk's tiles are
// the region's own
inline size_t band_chunk(size_t per_row) { return std::max<size_t>(8, (kCastStagingBytes / per_row) & ~(size_t)7); }

// One array of a chunk: item_bytes per item, absent arrays (optional outputs the caller
// did not ask for) take no bytes.  Every array starts at a multiple of 16 bytes and takes
// a multiple of 16, but for one with `exact` (bytes that nothing follows).
struct StagingArray {
    size_t item_bytes;
    bool present = true, exact = false;
};
enum class StagingItems { kRays, kRows, kAll };  // chunks of cast_chunk, of band_chunk, or one chunk
constexpr int kStagingMaxArrays = 7;
struct StagingPlan {
    size_t chunk = 0;  // items per chunk, at most the call's
    size_t total = 0;  // bytes to allocate
    size_t off[kStagingMaxArrays] = {}, bytes[kStagingMaxArrays] = {};  // of present arrays: ascending, chunk * item_bytes
    bool present[kStagingMaxArrays] = {};
};
inline StagingPlan staging_plan(const StagingArray *arrays, int n_arrays, size_t items, StagingItems kind)
{
    StagingPlan p;
    size_t per_item = 0;
    for (int i = 0; i < n_arrays; ++i) per_item += arrays[i].present ? arrays[i].item_bytes : 0;
    p.chunk = kind == StagingItems::kAll ? items
                                         : std::min(items, kind == StagingItems::kRays ? cast_chunk(per_item) : band_chunk(per_item));
    for (int i = 0; i < n_arrays; ++i) {
        if (!(p.present[i] = arrays[i].present)) continue;
        p.off[i] = p.total;
        p.bytes[i] = p.chunk * arrays[i].item_bytes;
        p.total += arrays[i].exact ? p.bytes[i] : round16(p.bytes[i]);
    }
    return p;
}

// The blocking forms' arrays, in the order their Staging::at() indices name them.
// spt_cast_rays, per ray: origin, direction in; index (+ hit record: two float4) out
inline StagingPlan cast_rays_plan(size_t n, bool hit)
{
    const StagingArray a[4] = {{16}, {16}, {4}, {32, hit}};
    return staging_plan(a, 4, n, StagingItems::kRays);
}
// spt_occluded_rays, per ray: origin, direction or end point in (+ the limit in); one byte
// out, last (a chunk is whole waves, so but for the call's last chunk it is a multiple of 16)
inline StagingPlan occluded_rays_plan(size_t n, bool limits)
{
    const StagingArray a[4] = {{16}, {16}, {4, limits}, {1, true, true}};
    return staging_plan(a, 4, n, StagingItems::kRays);
}
// spt_primary_hits, per ray: the (x, y, s) triple in; index (+ hit record, + direction) out
inline StagingPlan primary_hits_plan(size_t n, bool hit, bool dirs)
{
    const StagingArray a[4] = {{12}, {4}, {32, hit}, {16, dirs}};
    return staging_plan(a, 4, n, StagingItems::kRays);
}
// spt_trace_rays, per ray: origin, direction in; colour out; state in (+ two words out)
inline StagingPlan trace_rays_plan(size_t n, bool info)
{
    const StagingArray a[5] = {{16}, {16}, {16}, {8}, {8, info}};
    return staging_plan(a, 5, n, StagingItems::kRays);
}
// spt_render_features, per row of w pixels: two float4 and / or one word per pixel out
inline StagingPlan features_plan(size_t w, size_t h, bool feat, bool ids)
{
    const StagingArray a[2] = {{w * 32, feat}, {w * 4, ids}};
    return staging_plan(a, 2, h, StagingItems::kRows);
}
// spt_denoise and spt_denoise_var, per pixel of the whole image: rgba, feat in; out_rgba,
// the ping-pong planes between levels; the variance-guided form's mom in and out_var out
// (both absent for spt_denoise); then the g_data bytes
inline StagingPlan denoise_plan(size_t npix, size_t planes, bool out, bool rgb8, bool mom = false, bool out_var = false)
{
    const StagingArray a[7] = {{16}, {32}, {16, out}, {planes * 16, planes != 0}, {16, mom}, {4, out_var}, {3, rgb8, true}};
    return staging_plan(a, 7, npix, StagingItems::kAll);
}
// spt_render_moments, the whole region as one item: rgba out, mom out, then the frame's
// g_data bytes (the fold writes the region's band of a full frame)
inline StagingPlan moments_plan(size_t npix, size_t frame_bytes, bool rgba, bool g_data)
{
    const StagingArray a[3] = {{npix * 16, rgba}, {npix * 16}, {frame_bytes, g_data, true}};
    return staging_plan(a, 3, 1, StagingItems::kAll);
}
// spt_render_adaptive, the whole region as one item: moments_plan with mom optional too
inline StagingPlan adaptive_staging_plan(size_t npix, size_t frame_bytes, bool rgba, bool mom, bool g_data)
{
    const StagingArray a[3] = {{npix * 16, rgba}, {npix * 16, mom}, {frame_bytes, g_data, true}};
    return staging_plan(a, 3, 1, StagingItems::kAll);
}
// spt_temporal, per pixel of the whole image: this frame's {rgba, mom, feat} (16 + 16 + 32
// bytes, three planes one after the other) and ids in, the history's same two arrays (absent
// without a history), then {out_rgba, out_mom} out (two planes); spt_temporal_motion's table
// of motion_bytes bytes (32 per sphere, not per pixel) follows them as array 5, absent at 0
inline StagingPlan temporal_plan(size_t npix, bool hist, size_t motion_bytes = 0)
{
    const StagingArray a[5] = {{64}, {4}, {64, hist}, {4, hist}, {32}};
    StagingPlan p = staging_plan(a, 5, npix, StagingItems::kAll);
    if ((p.present[5] = motion_bytes != 0)) {
        p.off[5] = p.total;
        p.bytes[5] = motion_bytes;
        p.total += round16(motion_bytes);
    }
    return p;
}

// The allocation of a plan, for one blocking call on one stream (spt_staging.cpp).  A call
// that leaves with an error leaves `ok` unset: the stream is then synchronised before the
// memory is freed, whatever is still queued on it.
struct Staging {
    StagingPlan plan;
    char *base = nullptr;
    void *stream = nullptr;  // hipStream_t
    bool ok = false;
    // false: the allocation of plan.total bytes failed
    bool alloc(const StagingPlan &p, void *stream_);
    template <class T>
    T *at(int i) const { return plan.present[i] ? (T *)(base + plan.off[i]) : nullptr; }
    int done(int rc) { return (ok = rc == 0), rc; }
    ~Staging();
    Staging() = default;
    Staging(const Staging &) = delete;
    Staging &operator=(const Staging &) = delete;
};

}  // namespace spt_api
