// Host check of the candidate-list plan (spt_primplan.h): who builds the lists of a state --
// the device, or the host builder with the reason spt_update_info reports -- and the shape
// of the device's fixed-stride arrays, against values written out below as literals.
// Standard headers only.  Exit 0 = pass.
#include <cstdio>

#include "spt_primplan.h"

using namespace spt_api;

namespace {

constexpr uint32_t kCap = 2048;  // the kernel's LDS list (kPrimDevSlots)

struct Case {
    const char *what;
    PrimPlan plan;
    bool device;
    uint32_t reason, bw, nb8, nb4, stride;
    uint64_t total;
};
#define P(call) #call, call
constexpr uint32_t DEV = kPrimPlanDevice, CAM = kPrimPlanCamera, SLOTS = kPrimPlanSlots;

const Case kCases[] = {
    // prim_plan(slots, W, H, prim_max, device slot cap, camera usable, pad slot)
    // the host builder's call: a frame beyond 65 535, an unusable camera, no pad slot
    {P(prim_plan(164, 0x10000, 37, 24, kCap, true, true)), false, CAM, 0, 0, 0, 0, 0},
    {P(prim_plan(164, 75, 0x10000, 24, kCap, true, true)), false, CAM, 0, 0, 0, 0, 0},
    {P(prim_plan(164, 75, 37, 24, kCap, false, true)), false, CAM, 0, 0, 0, 0, 0},
    {P(prim_plan(164, 75, 37, 24, kCap, true, false)), false, CAM, 0, 0, 0, 0, 0},
    // ... which comes before the slot count
    {P(prim_plan(kCap + 1, 75, 37, 24, kCap, false, true)), false, CAM, 0, 0, 0, 0, 0},
    // the largest frame the kernel takes
    {P(prim_plan(164, 0xFFFF, 0xFFFF, 4, kCap, true, true)), true, DEV, 8192, 67108864, 134217728, 4, 805306368ull},
    // more slots than the kernel's list holds: at the cap the device, one above the host
    {P(prim_plan(kCap, 75, 37, 24, kCap, true, true)), true, DEV, 10, 50, 100, 24, 3600},
    {P(prim_plan(kCap + 1, 75, 37, 24, kCap, true, true)), false, SLOTS, 10, 50, 100, 24, 3600},
    {P(prim_plan(64, 75, 37, 24, 64, true, true)), true, DEV, 10, 50, 100, 24, 3600},
    {P(prim_plan(164, 75, 37, 24, 64, true, true)), false, SLOTS, 10, 50, 100, 24, 3600},  // SPT_PRIM_DEVICE_SLOTS=64
    {P(prim_plan(1, 75, 37, 24, 0, true, true)), false, SLOTS, 10, 50, 100, 24, 3600},
    // a run's first entry is a uint32: 8192 * (5461 + 10922) * 32 = 2^32 - 262 144 entries
    // fit, 8192 * (5462 + 10923) * 32 = 2^32 + 262 144 do not
    {P(prim_plan(164, 0xFFFF, 43688, 32, kCap, true, true)), true, DEV, 8192, 44736512, 89473024, 32, 4294705152ull},
    {P(prim_plan(164, 0xFFFF, 43689, 32, kCap, true, true)), false, SLOTS, 8192, 44744704, 89481216, 32, 4295229440ull},
    // geometry: 75 x 37 has a 3-pixel last block, a 5-row last 8-block and a 1-row last 4-block
    {P(prim_plan(164, 75, 37, 24, kCap, true, true)), true, DEV, 10, 50, 100, 24, 3600},
    {P(prim_plan(164, 7, 3, 24, kCap, true, true)), true, DEV, 1, 1, 1, 24, 48},
    {P(prim_plan(164, 64, 64, 24, kCap, true, true)), true, DEV, 8, 64, 128, 24, 4608},
    {P(prim_plan(164, 1, 1, 24, kCap, true, true)), true, DEV, 1, 1, 1, 24, 48},
    // the stride: prim_max rounded up to whole groups of 4
    {P(prim_plan(164, 75, 37, 1, kCap, true, true)), true, DEV, 10, 50, 100, 4, 600},
    {P(prim_plan(164, 75, 37, 0, kCap, true, true)), true, DEV, 10, 50, 100, 0, 0},
    {P(prim_plan(164, 75, 37, 25, kCap, true, true)), true, DEV, 10, 50, 100, 28, 4200},
    {P(prim_plan(164, 75, 37, 28, kCap, true, true)), true, DEV, 10, 50, 100, 28, 4200},
};

}  // namespace

int main()
{
    int bad = 0;
    for (const Case &c : kCases) {
        const PrimPlan &p = c.plan;
        const bool ok = p.device == c.device && p.reason == c.reason && p.bw == c.bw && p.nb8 == c.nb8 && p.nb4 == c.nb4 &&
                        p.stride == c.stride && p.total == c.total;
        if (!ok) {
            ++bad;
            std::printf("%s: device %d reason %u bw %u nb8 %u nb4 %u stride %u total %llu, expected %d %u %u %u %u %u %llu\n",
                        c.what, (int)p.device, p.reason, p.bw, p.nb8, p.nb4, p.stride, (unsigned long long)p.total,
                        (int)c.device, c.reason, c.bw, c.nb8, c.nb4, c.stride, (unsigned long long)c.total);
        }
    }
    if (bad) return 1;
    std::printf("ok\n");
    return 0;
}
