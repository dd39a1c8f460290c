// spt_primplan.h -- who builds the primary-ray candidate lists of a state (spt_scenestate.cpp
// update_lists), and the shape of the device's arrays: spt_primlists.hip writes one run of
// `stride` entries per 8x8 and per 8x4 block, the host builder packs its runs and sizes its own.
// A pure function, standard headers only (tests/cpp/primplan_check.cpp drives it on the CPU).
#pragma once
#include <cstddef>
#include <cstdint>

namespace spt_api {

// PrimPlan::reason: SPT_UPDATE_LISTS_DEVICE / _CAMERA / _SLOTS (spt_scenestate.cpp asserts it)
constexpr uint32_t kPrimPlanDevice = 0, kPrimPlanCamera = 2, kPrimPlanSlots = 3;

struct PrimPlan {
    bool device = false;  // the kernel builds; else the host builder, for `reason`
    uint32_t reason = kPrimPlanCamera;
    // 8x8 blocks per row, 8x8 and 8x4 blocks, entries per run, entries in all (0: reason camera)
    uint32_t bw = 0, nb8 = 0, nb4 = 0, stride = 0;
    uint64_t total = 0;
};

// n_slots: slots of the traversal tables; dev_slots: the most the kernel's LDS list holds;
// camera_usable, pad_slot: the host builder's two conditions (prim_camera_usable, prim_pad_slot
// != kPrimWalk) -- where it turns the lists off, it decides.
inline PrimPlan prim_plan(size_t n_slots, uint32_t W, uint32_t H, uint32_t prim_max, uint32_t dev_slots, bool camera_usable,
                          bool pad_slot)
{
    PrimPlan p;
    if (W > 0xFFFFu || H > 0xFFFFu || !camera_usable || !pad_slot) return p;
    p.bw = (W + 7) / 8;
    p.nb8 = p.bw * ((H + 7) / 8);
    p.nb4 = p.bw * ((H + 3) / 4);
    p.stride = (prim_max + 3u) & ~3u;
    p.total = ((uint64_t)p.nb8 + p.nb4) * p.stride;
    // a run's first entry is a uint32
    p.device = n_slots <= dev_slots && p.total <= 0xFFFFFFFFull;
    p.reason = p.device ? kPrimPlanDevice : kPrimPlanSlots;
    return p;
}

}  // namespace spt_api
