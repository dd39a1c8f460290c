// spt_primlists.hip -- the primary-ray candidate lists (PrimLists, spt_internal.h) built on
// the device: spt_update_scene's list build (spt_scenestate.cpp update_lists).
//
// The lists are those of the host builder (spt_accel.cpp build_prim_lists): per 8x8 and 8x4
// pixel block the slots whose member test a primary ray of the block can pass, ascending,
// padded to groups of 4 with a dummy slot, or "walk" where the block's cone is unusable or the
// list longer than prim_max.  The cone and the candidate test are the host's own functions
// (spt_primcone.h, fp64, contraction off); only atan2 / asin / sqrt come from the device's
// library, whose error is orders of magnitude inside the 1e-6 rad the test adds (DESIGN.md
// §4.16), so the device's lists are sound wherever the host's are.
//
// Fixed-stride storage: block b of level l owns `stride` = roundup4(prim_max) entries at
// entry (l * nb8 + b) * stride (nb8 8x8 blocks precede the 8x4 blocks), so no scan and no
// atomics decide where a run lies: the tables are a function of the inputs alone.
//
// One 256-thread workgroup per 64 x 64-pixel super-block (config 2: 247 of them, one per CU).
//   phase 0  thread t < blocks computes the cone of the super-block's t-th block into LDS
//            (at most 64 + 128 blocks; the cones of a wave's blocks then cost no lane any
//            fp64 work), every thread the super-block's own cone;
//   phase 1  the threads stride over the slot table; the slots the super-block's cone keeps
//            go to LDS in ascending order (ballot + per-wave counts: a slot's place is the
//            number of kept slots before it);
//   phase 2  each wave takes the blocks in turn; the lanes stride over the LDS list and a
//            ballot compaction writes the kept slots straight into the block's run.
// LDS: 48 B x 192 cones + (4 + 16) B x kPrimDevSlots slots + counts = 50 KiB; the host falls
// back to its own builder for tables of more than kPrimDevSlots slots.
#include "spt_primcone.h"

namespace spt {

constexpr uint32_t kPrimSupBlocks = 64 + 128;  // 8x8 and 8x4 blocks of a 64 x 64 super-block

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(256) void prim_lists_kernel(PrimBuildArgs a)
{
    __shared__ PrimCone s_cone[kPrimSupBlocks];
    __shared__ float4 s_slot[kPrimDevSlots];
    __shared__ uint32_t s_id[kPrimDevSlots];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_tot[2];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t sbw = (a.W + 63u) / 64u;
    const uint32_t sx = (blockIdx.x % sbw) * 64u, sy = (blockIdx.x / sbw) * 64u;
    const uint32_t ex = min(a.W, sx + 64u), ey = min(a.H, sy + 64u);
    // the super-block's blocks: level 0 (8 rows) then level 1 (4 rows), each row-major
    const uint32_t bwid = (ex - sx + 7u) / 8u;
    const uint32_t n8 = bwid * ((ey - sy + 7u) / 8u), n4 = bwid * ((ey - sy + 3u) / 4u);
    const double e[3] = {(double)a.cam.eye[0], (double)a.cam.eye[1], (double)a.cam.eye[2]};

    auto block_rect = [&](uint32_t t, uint32_t &level, uint32_t &x, uint32_t &y, uint32_t &hgt) {
        level = t < n8 ? 0u : 1u;
        const uint32_t q = t < n8 ? t : t - n8;
        hgt = level == 0u ? 8u : 4u;
        x = sx + (q % bwid) * 8u;
        y = sy + (q / bwid) * hgt;
    };
    if (tid < n8 + n4) {
        uint32_t level, x, y, hgt;
        block_rect(tid, level, x, y, hgt);
        s_cone[tid] = prim_cone(a.cam, a.W, a.H, x, min(a.W, x + 8u), y, min(a.H, y + hgt));
    }
    if (tid < 2) s_tot[tid] = 0u;
    const PrimCone sc = prim_cone(a.cam, a.W, a.H, sx, ex, sy, ey);

    // phase 1: a.n_slots <= kPrimDevSlots (the host checks), so the list always fits
    uint32_t kept = 0;
    for (uint32_t base = 0; base < a.n_slots; base += 256u) {
        const uint32_t s = base + tid;
        float4 sl = make_float4(0.f, 0.f, 0.f, -INFINITY);
        bool keep = false;
        if (s < a.n_slots) {
            sl = a.slots[s];
            keep = !sc.ok || prim_candidate(sc, sl, e);
        }
        const unsigned long long m = __ballot(keep);
        __syncthreads();  // the previous round's counts are read
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            before += w < wave ? s_wave[w] : 0u;
            all += s_wave[w];
        }
        const uint32_t at = kept + before + lanes_below(m);
        if (keep && at < kPrimDevSlots) {
            s_id[at] = s;
            s_slot[at] = sl;
        }
        kept += all;
    }
    __syncthreads();
    kept = min(kept, kPrimDevSlots);

    // phase 2
    uint32_t lists8 = 0, entries = 0;  // lane 0 of each wave counts its blocks
    for (uint32_t t = wave; t < n8 + n4; t += 4u) {
        uint32_t level, x, y, hgt;
        block_rect(t, level, x, y, hgt);
        const uint32_t blk = (y / hgt) * a.bw + x / 8u;
        uint2 *entry = (level == 0u ? a.b8 : a.b4) + blk;
        const uint32_t first = ((level == 0u ? 0u : a.nb8) + blk) * a.stride;
        const PrimCone &pc = s_cone[t];
        uint32_t count = pc.ok ? 0u : kPrimWalk;
        for (uint32_t base = 0; count <= a.prim_max && base < kept; base += 64u) {
            const uint32_t j = base + lane;
            const bool keep = j < kept && prim_candidate(pc, s_slot[j], e);
            const unsigned long long m = __ballot(keep);
            const uint32_t at = count + lanes_below(m);
            if (keep && at < a.prim_max) a.out[first + at] = s_id[j];  // prim_max <= stride
            count += (uint32_t)__popcll(m);
        }
        if (count > a.prim_max) {  // the cone is unusable or the list too long: walk
            if (lane == 0) *entry = make_uint2(0u, kPrimWalk);
            continue;
        }
        // whole groups of 4 (the kernels load 4 entries at a time): pad with the dummy slot
        const uint32_t padded = (count + 3u) & ~3u;
        if (lane < padded - count) a.out[first + count + lane] = a.pad;
        if (lane == 0) {
            *entry = make_uint2(first, padded);
            lists8 += level == 0u ? 1u : 0u;
            entries += padded;
        }
    }
    if (lane == 0) {
        atomicAdd(&s_tot[0], lists8);
        atomicAdd(&s_tot[1], entries);
    }
    __syncthreads();
    if (tid < 2 && s_tot[tid] != 0u) atomicAdd(&a.totals[tid], s_tot[tid]);
}

hipError_t launch_prim_lists(const PrimBuildArgs &a, hipStream_t s)
{
    if (a.W == 0 || a.H == 0 || a.n_slots > kPrimDevSlots || a.prim_max > a.stride) return hipErrorInvalidValue;
    const uint32_t sups = ((a.W + 63u) / 64u) * ((a.H + 63u) / 64u);
    hipLaunchKernelGGL(prim_lists_kernel, dim3(sups), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace spt
