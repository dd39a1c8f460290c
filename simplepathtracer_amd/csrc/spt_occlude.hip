// spt_occlude.hip -- batched bounded any-hit queries for rays or segments the caller
// chooses: spt_occluded_rays[_async] (spt_occlude.cpp).
//
// The contract (include/spt_hip.h): occ[i] = 1 iff spt_cast_rays would
// report a hit for ray i with ds < L_i, an fp32 compare of squared distances; 0 otherwise.
// Since the cast's winner is the passing sphere of least ds, that is "some sphere passes
// RaySphereIntersection, lies ahead and has ds < L": an any-hit query, and the walk may stop
// at the first such sphere.
//
// One ray per lane, a wave per run of 64 rays, five kernels chosen by the one walk rule
// (cast_walk), as the other query families.  The traversal is the casts' own (spt_path.h)
// with two changes:
//   - the lane's bound starts at min(L, FLT_MAX) with no winner, so the near test culls
//     beyond the limit from the first node on and the strict member update (ds < best; a
//     tie needs a winner) can only take a sphere with ds < L;
//   - a lane that has taken one is decided: it leaves every node mask, and the wave ends
//     when no active lane is undecided.
// The wave casts do both inside find_closest<..., ANY = true>; the lane walks run lane_cast
// in slices of kSliceBudget iterations from a preset bound and retire decided lanes between
// slices.  Lanes past the batch's end and lanes whose L is NaN or <= 0 are inactive: they
// carry o = d = 0 and a bound of 0, open no node and answer 0.
//
// Segment form: o = a, d = normalize(b - a) (the shading path's), L = lensq(b - a) * scale,
// formed here per lane, without contraction (the build's -ffp-contract=off).
#include "spt_query.h"

namespace spt {

namespace {

// walk iterations and leaf passes of the lane walks between two looks at who is decided:
// each slice re-tests the always-list and re-forms the node test's terms, so it is not 1
#ifndef SPT_OCC_SLICE
#define SPT_OCC_SLICE 6
#endif
constexpr uint32_t kSliceBudget = SPT_OCC_SLICE;

template <bool TREE, int LEAF, int WALK, uint32_t BLOCK>
__device__ __forceinline__ void occlude_body(const OccludeArgs &a)
{
    __shared__ uint32_t s_lds[(TREE && WALK == kWalkWave) ? BLOCK : 1];
    const AccelView &ac = a.accel;
    const uint32_t *const nodes = lds_node_table<WALK, BLOCK>(ac);
    const uint32_t lane = __lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (BLOCK / 64u) + (threadIdx.x >> 6));
    const uint32_t n_waves = gridDim.x * (BLOCK / 64u);
    const uint32_t runs = (a.n + 63u) >> 6;
    for (uint32_t r = wave; r < runs; r += n_waves) {
        const uint32_t i = (r << 6) + lane;
        const bool in = i < a.n;
        f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
        float L = 0.f;
        if (in) {
            const float4 a4 = a.a[i], b4 = a.b[i];  // w lanes ignored
            o = mk(a4.x, a4.y, a4.z);
            if (a.segments) {
                const f3 v = sub(mk(b4.x, b4.y, b4.z), o);
                d = normalize(v);
                L = lensq(v) * a.scale;
            } else {
                d = mk(b4.x, b4.y, b4.z);
                L = a.limits ? a.limits[i] : INFINITY;
            }
        }
        // NaN and <= 0 limits answer 0 without a walk; the reference never accepts
        // ds == FLT_MAX, so the clamp is exact (and keeps inf - inf out of the near bound)
        const bool active = in && L > 0.f;
        const float lim = active ? __builtin_fminf(L, FLT_MAX) : 0.f;
        if (!active) o = d = mk(0.f, 0.f, 0.f);
        CastDiag dg;
        Hit h;
        if (WALK == kWalkWave) {
            h = find_closest<TREE, LEAF, false, true>(ac, o, d, active, dg, nullptr,
                                                      TREE ? s_lds + (threadIdx.x & ~63u) : nullptr, lim);
        } else {
            constexpr bool BYTES = WALK == kWalkLds;
            const uint32_t *const ln = BYTES ? nodes : (const uint32_t *)ac.nodes;
            const uint32_t end = BYTES ? ac.n_nodes << 5 : ac.n_nodes;
            h.idx = kMiss;
            h.best = lim;
            h.t = 0.f;
            uint32_t ni = active ? 0u : end, leaf = kNoSlot, leaf2 = kNoSlot;
            bool live = active;
            for (;;) {
                const bool done = lane_cast<LEAF, BYTES>(ac, o, d, live, dg, ln, false, kSliceBudget, h, ni, leaf, leaf2);
                // a decided lane stops walking and drops its parked leaves
                const bool dec = h.idx != kMiss;
                ni = dec ? end : ni;
                leaf = dec ? kNoSlot : leaf;
                leaf2 = dec ? kNoSlot : leaf2;
                live = live && !dec;
                if (__ballot(!done && !dec) == 0ull) break;
            }
        }
        if (in) a.occ[i] = (active && h.idx != kMiss) ? (uint8_t)1 : (uint8_t)0;
    }
}

constexpr uint32_t kOccBlock = 256, kOccLdsBlock = 1024;

}  // namespace

// flat cluster lists and the wave's octant walk of the tree
template <bool TREE, int LEAF>
__global__ __launch_bounds__(kOccBlock) void occlude_kernel(OccludeArgs a)
{
    occlude_body<TREE, LEAF, kWalkWave, kOccBlock>(a);
}
// lane walk over layout 0 in global memory
__global__ __launch_bounds__(kOccBlock) void occlude_kernel_glane(OccludeArgs a)
{
    occlude_body<true, (int)kClusterSlots, kWalkGlane, kOccBlock>(a);
}
// lane walk over the block's LDS copy of layout 0: two 1024-thread blocks per CU, as
// cast_kernel_lds
__global__ __launch_bounds__(kOccLdsBlock) __attribute__((amdgpu_waves_per_eu(2 * kOccLdsBlock / 256))) void occlude_kernel_lds(OccludeArgs a)
{
    occlude_body<true, (int)kClusterSlots, kWalkLds, kOccLdsBlock>(a);
}

hipError_t launch_occlude(const OccludeArgs &a, hipStream_t s)
{
    if (a.n == 0u) return hipSuccess;
    // (in the order of cast_walk's values)
    void (*const kernels[5])(OccludeArgs) = {occlude_kernel_lds, occlude_kernel_glane,
                                             occlude_kernel<true, (int)kClusterSlots>,
                                             occlude_kernel<false, (int)kFlatLeafSlots>,
                                             occlude_kernel<false, (int)kClusterSlots>};
    // a wave per run of 64 rays
    return launch_query(a.accel, kernels, kOccBlock, kOccLdsBlock, (a.n + 63u) / 64u, s, a);
}

}  // namespace spt
