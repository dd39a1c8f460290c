// spt_query.h -- what the query kernels share (spt_cast.hip, spt_occlude.hip, spt_trace.hip,
// spt_features.hip): each family is five kernels, one per walk of cast_walk
// (spt_internal.h), over a body of its own.  Here: the walk a body is compiled for, the
// block's LDS copy of node layout 0, the cast that goes with the walk, and the launcher
// that picks the family's kernel for a scene and sizes its grid.
#pragma once
#include "spt_path.h"

#include <algorithm>
#include <mutex>

namespace spt {

// the walk of a kernel body: the wave's casts (flat cluster lists and the octant walk of
// the tree, by TREE), or the lane walk over layout 0 in LDS or in global memory
enum : int { kWalkWave = 0, kWalkLds = 1, kWalkGlane = 2 };

// The block's LDS copy of node layout 0 for the LDS lane walk, made by all BLOCK threads
// at the top of the kernel; the other walks get a table of one record that nothing reads.
template <int WALK, uint32_t BLOCK>
__device__ __forceinline__ const uint32_t *lds_node_table(const AccelView &ac)
{
    __shared__ uint4 s_nodes[WALK == kWalkLds ? 2 * kLdsNodeRecords : 1];
    if (WALK == kWalkLds) {
        // the host launches this variant only when n_nodes + 1 <= kLdsNodeRecords; skip
        // links as byte offsets, as render_kernel_lds keeps them (lane_cast BYTES)
        const uint4 *src = (const uint4 *)ac.nodes;
        const uint32_t n4 = 2u * (ac.n_nodes + 1u);
        for (uint32_t k = threadIdx.x; k < n4; k += BLOCK) {
            uint4 v = src[k];
            if (k & 1u) v.x <<= 5;
            s_nodes[k] = v;
        }
        __syncthreads();
    }
    return (const uint32_t *)s_nodes;
}

// One cast of the wave's 64 rays with the render kernels' own per-wave casts (spt_path.h).
// nodes: lds_node_table's; lds: the wave's 64 words of scratch for the wave walk's dealt
// leaf tests (test_leaf_pairs), read only where TREE.
template <bool TREE, int LEAF, int WALK>
__device__ __forceinline__ Hit query_cast(const AccelView &ac, const f3 &o, const f3 &d, bool active, CastDiag &dg,
                                          const uint32_t *nodes, uint32_t *lds)
{
    Hit h;
    if (WALK == kWalkLds) {
        uint32_t ni, leaf, leaf2;
        (void)lane_cast<LEAF, true>(ac, o, d, active, dg, nodes, true, 0xFFFFFFFFu, h, ni, leaf, leaf2);
    } else if (WALK == kWalkGlane) {
        h = find_closest_lane<LEAF>(ac, o, d, active, dg, (const uint32_t *)ac.nodes);
    } else {
        h = find_closest<TREE, LEAF>(ac, o, d, active, dg, nullptr, TREE ? lds : nullptr);
    }
    return h;
}

// (internal linkage: each family's file has its own cache, keyed by its own kernels)
namespace {

// resident blocks of kernel `f` on the current device (cached per device and walk)
template <class F>
uint32_t resident_blocks(F f, uint32_t block, uint32_t walk)
{
    constexpr int kMaxDevices = 64, kWalks = 5;
    static std::mutex mu;
    static uint32_t cache[kMaxDevices][kWalks];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0u;
    std::lock_guard<std::mutex> lk(mu);
    if (cache[dev][walk] == 0u) {
        int per_cu = 0, num_cu = 0;
        if (hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, (int)block, 0) != hipSuccess || per_cu <= 0 ||
            num_cu <= 0)
            return 0u;
        cache[dev][walk] = (uint32_t)per_cu * (uint32_t)num_cu;
    }
    return cache[dev][walk];
}

// The family's kernel for the scene's walk (kernels[w]: that of cast_walk's value w;
// lds_block threads for the LDS walk, block for the others) over `units` wave-sized pieces
// of work (runs of 64 rays, tiles): a wave per unit until the device is full, then waves
// take several.
template <class F, class... Args>
hipError_t launch_query(const AccelView &ac, F const (&kernels)[5], uint32_t block, uint32_t lds_block, uint32_t units,
                        hipStream_t s, const Args &...args)
{
    const uint32_t walk = cast_walk(ac);
    const F f = kernels[walk];
    const uint32_t threads = walk == kCastWalkLds ? lds_block : block;
    const uint32_t resident = resident_blocks(f, threads, walk);
    if (resident == 0u) return hipErrorLaunchFailure;
    const uint32_t per_block = threads / 64u;
    const uint32_t grid = std::min((units + per_block - 1u) / per_block, resident);
    hipLaunchKernelGGL(f, dim3(grid), dim3(threads), 0, s, args...);
    return hipGetLastError();
}

}  // namespace

}  // namespace spt
