// spt_trace.hip -- batched TraceAndSampleColor (SingleThreadPathTracer.hpp:94-112) for rays
// the caller chooses: spt_trace_rays[_async] (spt_trace.cpp).
//
// One path per lane, in the render kernels' own per-path code (spt_path.h): every cast is
// find_closest / lane_cast / find_closest_lane, chosen per launch by launch_cast's rule
// (cast_walk), every shading step is shade_step in segment mode.  Nothing of the traversal
// or the shading is restated here.  Path i draws from the caller's raw splitmix state
// st[i] where a render's path draws from its keyed one.
//
// Lanes are state machines that refill: a lane whose path ends takes the wave's next ray
// while the other lanes go on (paths run from one cast to over a thousand).  Rays are
// partitioned statically: wave w of W owns the runs w, w + W, ... of 64 consecutive rays.
// The run a wave will hand out next sits in registers, one ray per lane, loaded (coalesced)
// when the run before it was used up, so its latency passes behind the casts in between;
// an idle lane takes its ray from the holding lane by ds_bpermute (the LDS-tree kernel has
// no registers to hold a run in: its lanes load their ray when they take it).  No counter,
// no atomic, nothing to zero on the stream: launches on any number of streams share no
// state.  Lanes past the batch's end hold no ray: they read nothing, open no node and write
// nothing, and the cooperative sampler still sees all 64 lanes in wave-uniform control flow.
//
// shade_step stores a finished path's sample word at samples[item]; with samples = the
// rgba output and item = 4 i the word lands in the first word of rgba[i].  A second, small
// kernel on the same stream turns each word into its colour in place with the fold's own
// decode_word (spt_decode.h).  (Decoding in the trace kernel would need the word back
// from memory: a store-to-load round trip in every iteration in which a path ends.)
#include "spt_query.h"
#include "spt_decode.h"

namespace spt {

namespace {

// rays per launch: item = 4 i stays below 2^32 (launch_trace cuts larger batches)
constexpr uint32_t kTraceLaunchRays = 1u << 28;

template <bool TREE, int LEAF, int WALK, uint32_t BLOCK>
__device__ __forceinline__ void trace_body(const TraceArgs &a)
{
    // the next run waits in registers (8 VGPRs).  Not in the LDS-tree kernel: its 8 waves
    // per SIMD leave 64 VGPRs, and with the run held the lane walk spilled 6 of them to
    // scratch; there a lane loads its ray when it takes it, and the SIMD's other seven
    // waves cover the latency
    constexpr bool AHEAD = WALK != kWalkLds;
    // wave-private scratch of the cooperative sampler and the wave walk's dealt leaf tests
    __shared__ uint32_t s_lds[BLOCK];
    const AccelView &ac = a.scene.accel;
    const uint32_t *const nodes = lds_node_table<WALK, BLOCK>(ac);
    // what shade_step reads of a render launch: the scene, the depth, segment mode, and
    // the sample slots (the rgba output as words, path i's slot at word 4 i)
    RenderArgs ra;
    ra.scene = a.scene;
    ra.bounces = a.bounces;
    ra.mode = 0u;
    ra.samples = (uint32_t *)a.rgba;
    uint32_t *const lds = s_lds + (threadIdx.x & ~63u);

    const uint32_t lane = __lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (BLOCK / 64u) + (threadIdx.x >> 6));
    const uint32_t n_waves = gridDim.x * (BLOCK / 64u);
    const uint32_t runs = (a.n + 63u) >> 6;
    // the run being handed out: lane L holds its ray L; rays [q_pos, q_n) are not taken yet
    uint32_t run = wave, q_n = 0, q_pos = 0;
    f3 qo = mk(0.f, 0.f, 0.f), qd = mk(0.f, 0.f, 0.f);
    uint32_t qs_lo = 0, qs_hi = 0;
    auto load_run = [&]() {
        q_n = run < runs ? min(64u, a.n - (run << 6)) : 0u;
        q_pos = 0;
        if (AHEAD && lane < q_n) {
            const uint32_t i = (run << 6) + lane;
            const float4 o4 = a.o[i], d4 = a.d[i];  // w lanes ignored, as the reference's Vec4
            const uint64_t st = a.st[i];
            qo = mk(o4.x, o4.y, o4.z);
            qd = mk(d4.x, d4.y, d4.z);
            qs_lo = (uint32_t)st;
            qs_hi = (uint32_t)(st >> 32);
        }
    };
    load_run();

    Path ps;
    ps.phase = PH_IDLE;
    ps.item = ps.bounce = ps.spec = 0;
    ps.st = 0;
    ps.o = ps.d = mk(0.f, 0.f, 0.f);
    ps.slot = 0;
    ps.job = 0;
    uint32_t casts = 0;                         // of the lane's current path
    uint32_t done = 0, dropped = 0;  // shade_step's launch counters: not reported
    CastDiag dg;

    for (;;) {
        // ---- refill: idle lanes take the next rays of the wave's run (ballot + prefix),
        // as soon as they are idle: a refill is eight ds_bpermute, and waiting until 2 / 4 /
        // 8 / 16 lanes can refill together (the render's rule, whose refill forms a primary
        // ray) measured 0 / 1.2 / 2 / 4% slower on config 2's paths
        const unsigned long long need = __ballot(ps.phase == PH_IDLE);
        if (need != 0ull && q_n != 0u) {
            // at most the rest of this run: lanes left over take from the next one next time
            const uint32_t take = min((uint32_t)__popcll(need), q_n - q_pos);
            const uint32_t rank = lane_rank(need);
            const bool get = __builtin_amdgcn_inverse_ballot_w64(need) && rank < take;
            const int from = (int)(get ? q_pos + rank : lane);  // q_pos + rank < q_n <= 64
            f3 o = mk(0.f, 0.f, 0.f), d = o;
            uint64_t st = 0;
            if (AHEAD) {
                o = mk(__shfl(qo.x, from), __shfl(qo.y, from), __shfl(qo.z, from));
                d = mk(__shfl(qd.x, from), __shfl(qd.y, from), __shfl(qd.z, from));
                st = ((uint64_t)(uint32_t)__shfl((int)qs_hi, from) << 32) | (uint32_t)__shfl((int)qs_lo, from);
            }
            if (get) {
                const uint32_t i = (run << 6) + (uint32_t)from;
                if (!AHEAD) {
                    const float4 o4 = a.o[i], d4 = a.d[i];
                    st = a.st[i];
                    o = mk(o4.x, o4.y, o4.z);
                    d = mk(d4.x, d4.y, d4.z);
                }
                ps.o = o;
                ps.d = d;
                ps.st = st;
                ps.item = 4u * i;
                ps.phase = PH_TRACE;
                ps.bounce = a.bounces;
                ps.spec = 0;
                casts = 0;
            }
            q_pos += take;
            if (q_pos == q_n) {
                run += n_waves;
                load_run();
            }
        }
        const unsigned long long live = __ballot(ps.phase != PH_IDLE);
        if (live == 0ull) {
            if (q_n == 0u) break;  // no path and no ray left
            continue;              // (every lane is idle: the next refill hands out a ray)
        }
        // ---- one cast + one shading step ----
        const bool act = ps.phase != PH_IDLE;
        const Hit h = query_cast<TREE, LEAF, WALK>(ac, ps.o, ps.d, act, dg, nodes, lds);
        casts += act ? 1u : 0u;
        shade_step(ra, ps, h, act, done, dropped, lds);
        if (act && ps.phase == PH_IDLE && a.info) {
            // the path ended in this step (its word is stored): spo_trace_ray's counts
            const uint32_t ev = ps.spec & 0xFFFFu;
            uint32_t *rec = a.info + (ps.item >> 1);
            rec[0] = casts;
            rec[1] = ev | (ev > kSpecularCap ? 0x80000000u : 0u);
        }
    }
}

constexpr uint32_t kTraceBlock = 256, kTraceLdsBlock = 1024;

}  // namespace

// flat cluster lists (4 or 8 leaf slots; brute force is a list without nodes) and the
// wave's octant walk of the tree.  6 waves per SIMD: the wave walk otherwise takes 81 VGPRs,
// one more than 6 waves allow (80, no spill; config 2's paths +4%)
template <bool TREE, int LEAF>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(6))) void trace_kernel(TraceArgs a)
{
    trace_body<TREE, LEAF, kWalkWave, kTraceBlock>(a);
}
// lane walk over layout 0 in global memory
__global__ __launch_bounds__(kTraceBlock) void trace_kernel_glane(TraceArgs a)
{
    trace_body<true, (int)kClusterSlots, kWalkGlane, kTraceBlock>(a);
}
// lane walk over the block's LDS copy of layout 0: two 1024-thread blocks per CU, as
// render_kernel_lds (8 waves per SIMD)
__global__ __launch_bounds__(kTraceLdsBlock) __attribute__((amdgpu_waves_per_eu(2 * kTraceLdsBlock / 256))) void trace_kernel_lds(TraceArgs a)
{
    trace_body<true, (int)kClusterSlots, kWalkLds, kTraceLdsBlock>(a);
}

// each path's sample word, in the first word of its rgba slot, to its colour (w = +0)
// (TAB: through the scene's colour table, spt_decode.h)
template <bool TAB>
__global__ __launch_bounds__(256) void trace_decode_kernel(FoldArgs f, float4 *rgba, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const f3 c = decode_word<TAB>(f, f.samples[4u * i]);
    rgba[i] = make_float4(c.x, c.y, c.z, 0.f);
}

hipError_t launch_trace(const TraceArgs &all, const FoldArgs &fa, hipStream_t s)
{
    // (in the order of cast_walk's values)
    void (*const kernels[5])(TraceArgs) = {trace_kernel_lds, trace_kernel_glane, trace_kernel<true, (int)kClusterSlots>,
                                           trace_kernel<false, (int)kFlatLeafSlots>, trace_kernel<false, (int)kClusterSlots>};
    for (uint64_t r0 = 0; r0 < all.n; r0 += kTraceLaunchRays) {
        TraceArgs a = all;
        a.n = (uint32_t)std::min<uint64_t>(kTraceLaunchRays, all.n - r0);
        a.o += r0;
        a.d += r0;
        a.st += r0;
        a.rgba += r0;
        if (a.info) a.info += 2u * r0;
        // a wave per run of 64 rays
        hipError_t e = launch_query(a.scene.accel, kernels, kTraceBlock, kTraceLdsBlock, (a.n + 63u) / 64u, s, a);
        if (e != hipSuccess) return e;
        FoldArgs f = fa;
        f.samples = (const uint32_t *)a.rgba;
        hipLaunchKernelGGL(fold_uses_table(f) ? trace_decode_kernel<true> : trace_decode_kernel<false>, dim3((a.n + 255u) / 256u), dim3(256), 0, s, f, a.rgba, a.n);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace spt
