// spt_cast.hip -- batched FindClosestIntersectionSphere (Collision.hpp:87-109) for rays the
// caller chooses: spt_cast_rays[_async] and spt_primary_hits (spt_cast.cpp).
//
// One ray per lane.  A wave takes runs of 64 consecutive rays and casts each run with the
// render kernels' own per-wave casts (spt_path.h): find_closest over a flat cluster list
// or the wave's octant walk of the tree, lane_cast over the block's LDS copy of node
// layout 0, or find_closest_lane over layout 0 in global memory -- chosen per launch by
// the one walk rule (cast_walk, spt_internal.h).  Nothing of the traversal is restated here, so
// every culling proof of DESIGN.md §4.4 is exercised ray by ray on whatever rays the
// caller builds.  Primary-ray candidate lists are not used: they hold for camera rays only.
//
// Lanes past the batch's end are passed as inactive: they open no node, read no ray and
// write nothing.  Per ray the kernel writes the winner's ORIGINAL sphere index (the
// scene's sphere count on a miss, as the reference returns g_sphereNumber) and, when
// asked, two float4: {P, t} with P = contact(o, d, t) (ClosestContactPoint,
// Collision.hpp:49-56) and {n, ds} with n = Normalize(P - C) (ContactNormal, 67-71; the
// shading path's normalize) and ds the squared distance the winner was chosen by; eight
// +0 on a miss.
//
// Camera mode (CastArgs::xys): the ray is the primary ray of sample s of pixel (x, y),
// formed by the render's start_path itself, from the eye.
#include "spt_query.h"

namespace spt {

namespace {

template <bool TREE, int LEAF, int WALK, uint32_t BLOCK>
__device__ __forceinline__ void cast_body(const CastArgs &a)
{
    // wave-private scratch of the wave walk's dealt leaf tests (test_leaf_pairs)
    __shared__ uint32_t s_lds[(TREE && WALK == kWalkWave) ? BLOCK : 1];
    const AccelView &ac = a.accel;
    // lds_node_table's copy (spt_query.h), written out: with the loop inlined from there this
    // kernel alone gets another scalar register allocation (7 more s_mov in the lane walk's
    // member loop; sorted rays 1 % slower on the MI355X)
    __shared__ uint4 s_nodes[WALK == kWalkLds ? 2 * kLdsNodeRecords : 1];
    if (WALK == kWalkLds) {
        const uint4 *src = (const uint4 *)ac.nodes;
        const uint32_t n4 = 2u * (ac.n_nodes + 1u);
        for (uint32_t k = threadIdx.x; k < n4; k += BLOCK) {
            uint4 v = src[k];
            if (k & 1u) v.x <<= 5;
            s_nodes[k] = v;
        }
        __syncthreads();
    }
    const uint32_t *const nodes = (const uint32_t *)s_nodes;
    const uint32_t lane = __lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (BLOCK / 64u) + (threadIdx.x >> 6));
    const uint32_t n_waves = gridDim.x * (BLOCK / 64u);
    const uint32_t runs = (a.n + 63u) >> 6;
    const bool cam = a.xys != nullptr;
    for (uint32_t r = wave; r < runs; r += n_waves) {
        const uint32_t i = (r << 6) + lane;
        const bool active = i < a.n;
        f3 o = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 0.f);
        if (cam) {
            if (active) {
                // start_path itself, on the one-pixel, one-sample launch whose item 0 is
                // sample s of pixel (x, y): ts_item(0) of a 1 x 1 region is row 0, column 0,
                // sample 0, so the path is keyed (seed, y * width + x, s0 + 0)
                RenderArgs ra;
                ra.map = RowMap{a.xys[3u * i + 1u], a.xys[3u * i + 1u] + 1u, 1u, 1u, 0u, a.xys[3u * i], 1u};
                ra.width = a.width;
                ra.height = a.height;
                ra.bounces = 0u;
                ra.spp_batch = 1u;
                ra.s0 = a.xys[3u * i + 2u];
                ra.seed_key = a.seed_key;
                ra.div_band = ra.div_tile = ra.div_strip = FastDiv{1u, 0u, 0u};
#pragma unroll
                for (int q = 0; q < 12; ++q) ra.cam.view[q] = a.cam.view[q];
                Path ps;
                start_path(ra, 0u, 1u, recip((float)a.width), recip((float)a.height),
                           mk(a.cam.eye[0], a.cam.eye[1], a.cam.eye[2]), ps);
                o = ps.o;
                d = ps.d;
                if (a.dirs) a.dirs[i] = make_float4(d.x, d.y, d.z, 0.f);
            }
        } else if (active) {
            const float4 o4 = a.o[i], d4 = a.d[i];  // w lanes ignored, as the reference's Vec4
            o = mk(o4.x, o4.y, o4.z);
            d = mk(d4.x, d4.y, d4.z);
        }
        CastDiag dg;
        const Hit h = query_cast<TREE, LEAF, WALK>(ac, o, d, active, dg, nodes, s_lds + (threadIdx.x & ~63u));
        if (active) {
            const bool miss = h.idx == kMiss;
            a.idx[i] = miss ? a.n_spheres : ac.orig[h.idx];
            if (a.hit) {
                float4 pt = make_float4(0.f, 0.f, 0.f, 0.f), nd = pt;
                if (!miss) {
                    const float4 cs = ac.slots[h.idx];
                    const f3 p = contact(o, d, h.t);
                    const f3 nrm = normalize(sub(p, mk(cs.x, cs.y, cs.z)));
                    pt = make_float4(p.x, p.y, p.z, h.t);
                    nd = make_float4(nrm.x, nrm.y, nrm.z, h.best);
                }
                a.hit[2u * i] = pt;
                a.hit[2u * i + 1u] = nd;
            }
        }
    }
}

constexpr uint32_t kCastBlock = 256, kCastLdsBlock = 1024;

}  // namespace

// flat cluster lists (4 or 8 leaf slots; brute force is a list without nodes) and the
// wave's octant walk of the tree
template <bool TREE, int LEAF>
__global__ __launch_bounds__(kCastBlock) void cast_kernel(CastArgs a)
{
    cast_body<TREE, LEAF, kWalkWave, kCastBlock>(a);
}
// lane walk over layout 0 in global memory
__global__ __launch_bounds__(kCastBlock) void cast_kernel_glane(CastArgs a)
{
    cast_body<true, (int)kClusterSlots, kWalkGlane, kCastBlock>(a);
}
// lane walk over the block's LDS copy of layout 0: two 1024-thread blocks per CU, as
// render_kernel_lds (8 waves per SIMD)
__global__ __launch_bounds__(kCastLdsBlock) __attribute__((amdgpu_waves_per_eu(2 * kCastLdsBlock / 256))) void cast_kernel_lds(CastArgs a)
{
    cast_body<true, (int)kClusterSlots, kWalkLds, kCastLdsBlock>(a);
}

hipError_t launch_cast(const CastArgs &a, hipStream_t s)
{
    if (a.n == 0u) return hipSuccess;
    // (in the order of cast_walk's values)
    void (*const kernels[5])(CastArgs) = {cast_kernel_lds, cast_kernel_glane, cast_kernel<true, (int)kClusterSlots>,
                                          cast_kernel<false, (int)kFlatLeafSlots>, cast_kernel<false, (int)kClusterSlots>};
    // a wave per run of 64 rays
    return launch_query(a.accel, kernels, kCastBlock, kCastLdsBlock, (a.n + 63u) / 64u, s, a);
}

}  // namespace spt
