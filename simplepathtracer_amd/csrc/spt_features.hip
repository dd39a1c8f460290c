// spt_features.hip -- feature buffers of the frame's own primary rays: per pixel the
// first-hit albedo, coverage, normal and depth averaged over the spp samples, and sample
// 0's sphere: spt_render_features[_async] (spt_features.cpp).
//
// One wave per 8x8 tile of the region, lanes on pixels as ts_item lays out the items of a
// render launch of all spp samples ([band][tile][sample][pixel]: sample s of a tile is the
// run of items at base + s * count, lane L its item L), so every sample's 64 rays are the
// primary batch the render casts for that tile.  The wave loops over the samples s = 0 ..
// spp - 1: the ray is start_path's own, through start_path_kernarg (keyed (seed, y * width
// + x, s); the launch fields are read from the kernel arguments where they are used, not
// held in SGPRs across the loop), the cast is the render's primary-batch cast against the
// candidate lists (prim_list_cast), or where that declines (no list for the block, lists
// off, a lane that may not cull) the walk cast_walk picks for the context's shape -- the
// five variants of spt_cast.hip.  Nothing of the ray, the traversal or the hit record is
// restated here.
//
// The eight sums and the id stay in registers across the sample loop, added in sample
// order; the epilogue scales them by 1.0f / (float)spp (RenderSegment's pixelColor *=
// 1 / g_samples) and stores two float4 and one word per lane.  No per-sample workspace, no
// fold, no atomics.  Tiles are dealt statically (wave w of W takes tiles w, w + W, ...):
// no counter, so launches on any number of streams share no state.  Lanes past a ragged
// tile's pixels are inactive: they cast nothing and store nothing.
//
// prim_list_cast reads the kernel's first argument as a RenderArgs (kernarg_args), so the
// kernels take a RenderArgs first and FeatArgs second.
#include "spt_query.h"

namespace spt {

namespace {

template <bool TREE, int LEAF, int WALK, uint32_t BLOCK>
__device__ __forceinline__ void features_body(const RenderArgs &k, const FeatArgs &f)
{
    // wave-private scratch of the wave walk's dealt leaf tests (test_leaf_pairs)
    __shared__ uint32_t s_lds[(TREE && WALK == kWalkWave) ? BLOCK : 1];
    const AccelView &ac = k.scene.accel;
    const uint32_t *const nodes = lds_node_table<WALK, BLOCK>(ac);
    const uint32_t lane = __lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (BLOCK / 64u) + (threadIdx.x >> 6));
    const uint32_t n_waves = gridDim.x * (BLOCK / 64u);
    const uint32_t width = k.map.width, ft = width >> 3, wr = width & 7u;
    for (uint32_t tile = wave; tile < f.tiles; tile += n_waves) {
        // the tile's items in ts_item's order [band][tile][sample][pixel]: sample s of its
        // pixels is the run of `count` items at base + s * count, one primary batch
        const uint32_t band = tile / f.tiles_x, t = tile - band * f.tiles_x;
        const uint32_t h = min(f.rows - (band << 3), 8u);
        const uint32_t count = h * (t < ft ? 8u : wr);
        const uint32_t base = (band * 8u * width + t * h * 8u) * f.spp;
        const bool active = lane < count;
        float alb_r = 0.f, alb_g = 0.f, alb_b = 0.f, cov = 0.f;
        float nrm_x = 0.f, nrm_y = 0.f, nrm_z = 0.f, dep = 0.f;
        uint32_t id = 0;
        for (uint32_t s = 0; s < f.spp; ++s) {
            Path ps;
            ps.o = ps.d = mk(0.f, 0.f, 0.f);
            uint32_t pxy = 0;
            if (active) start_path_kernarg(base + s * count + lane, f.rows, ps, &pxy);
            CastDiag dg;
            Hit h1;
            bool listed = false;
            if (kernarg_args()->prim.on) listed = prim_list_cast(ac, ps.o, ps.d, active, pxy, h1, dg);
            if (!listed) h1 = query_cast<TREE, LEAF, WALK>(ac, ps.o, ps.d, active, dg, nodes, s_lds + (threadIdx.x & ~63u));
            if (active) {
                const bool miss = h1.idx == kMiss;
                // the sky term of SampleColorSkybox, as decode_sample rebuilds it
                kargs_t &kk = *kernarg_args();
                const float ky = ps.d.y + 1.0f;
                f3 alb = mul(mk(kk.cam.sky[0] * ky, kk.cam.sky[1] * ky, kk.cam.sky[2] * ky), 0.5f);
                f3 nrm = mk(0.f, 0.f, 0.f);
                float c = 0.f, tt = 0.f;
                if (!miss) {
                    // the hit record of spt_cast_rays: contact, normalize(P - C)
                    const float4 cs = ac.slots[h1.idx];
                    nrm = normalize(sub(contact(ps.o, ps.d, h1.t), mk(cs.x, cs.y, cs.z)));
                    c = 1.0f;
                    tt = h1.t;
                    // TraceAndSampleColor's switch: any other material byte goes to the skybox
                    const uint32_t m = kk.scene.mat[h1.idx];
                    if (m == SPT_DIFFUSE_ID) {
                        const float4 sh = kk.scene.shade[h1.idx];
                        alb = mk(sh.x, sh.y, sh.z);
                    } else if (m == SPT_REFLECTIVE_ID || m == SPT_REFRACTIVE_ID) {
                        alb = mk(1.f, 1.f, 1.f);
                    }
                }
                if (s == 0u) id = miss ? kk.scene.n : ac.orig[h1.idx];
                alb_r = alb_r + alb.x;
                alb_g = alb_g + alb.y;
                alb_b = alb_b + alb.z;
                cov = cov + c;
                nrm_x = nrm_x + nrm.x;
                nrm_y = nrm_y + nrm.y;
                nrm_z = nrm_z + nrm.z;
                dep = dep + tt;
            }
        }
        if (active) {
            // region-local pixel of the lane's items (row-major over rows x width)
            kargs_t &kk = *kernarg_args();
            uint32_t sl, lr, cx;
            ts_item(base + lane, width, f.rows, f.spp, FastDiv{kk.div_band.d, kk.div_band.m, kk.div_band.s},
                    FastDiv{kk.div_tile.d, kk.div_tile.m, kk.div_tile.s}, sl, lr, cx);
            const uint32_t p = lr * width + cx;
            const float inv = 1.0f / (float)f.spp;
            if (f.feat) {
                f.feat[2u * p] = make_float4(alb_r * inv, alb_g * inv, alb_b * inv, cov * inv);
                f.feat[2u * p + 1u] = make_float4(nrm_x * inv, nrm_y * inv, nrm_z * inv, dep * inv);
            }
            if (f.ids) f.ids[p] = id;
        }
    }
}

constexpr uint32_t kFeatBlock = 256, kFeatLdsBlock = 1024;

}  // namespace

// flat cluster lists (4 or 8 leaf slots; brute force is a list without nodes) and the
// wave's octant walk of the tree
template <bool TREE, int LEAF>
__global__ __launch_bounds__(kFeatBlock) void features_kernel(RenderArgs k, FeatArgs f)
{
    features_body<TREE, LEAF, kWalkWave, kFeatBlock>(k, f);
}
// lane walk over layout 0 in global memory
__global__ __launch_bounds__(kFeatBlock) void features_kernel_glane(RenderArgs k, FeatArgs f)
{
    features_body<true, (int)kClusterSlots, kWalkGlane, kFeatBlock>(k, f);
}
// lane walk over the block's LDS copy of layout 0: two 1024-thread blocks per CU, as
// render_kernel_lds (8 waves per SIMD)
__global__ __launch_bounds__(kFeatLdsBlock) __attribute__((amdgpu_waves_per_eu(2 * kFeatLdsBlock / 256))) void features_kernel_lds(RenderArgs k, FeatArgs f)
{
    features_body<true, (int)kClusterSlots, kWalkLds, kFeatLdsBlock>(k, f);
}

hipError_t launch_features(const RenderArgs &k, const FeatArgs &f, hipStream_t s)
{
    if (f.tiles == 0u) return hipSuccess;
    // (in the order of cast_walk's values)
    void (*const kernels[5])(RenderArgs, FeatArgs) = {features_kernel_lds, features_kernel_glane,
                                                      features_kernel<true, (int)kClusterSlots>,
                                                      features_kernel<false, (int)kFlatLeafSlots>,
                                                      features_kernel<false, (int)kClusterSlots>};
    // a wave per tile
    return launch_query(k.scene.accel, kernels, kFeatBlock, kFeatLdsBlock, f.tiles, s, k, f);
}

}  // namespace spt
