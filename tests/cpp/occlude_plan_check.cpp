// Host check of the staging plan of spt_occluded_rays (spt_staging.h: occluded_rays_plan):
// per ray 16 bytes of origin, 16 of direction or end point, 4 of limit (optional) and the
// answer's 1 byte.  For batches below, at and far above a chunk, with and without limits: the
// chunk is whole waves (or the whole call), every offset is a multiple of 16, arrays neither
// overlap nor leave the allocation, the absent limits take no bytes, and the total stays
// within the 256 MiB bound.  Literal values pin the large plans.  Standard headers only.
// Exit 0 = pass.
#include <cstdio>

#include "spt_staging.h"

using namespace spt_api;

namespace {

int check(size_t n, bool limits, size_t want_chunk, size_t want_total)
{
    const StagingPlan p = occluded_rays_plan(n, limits);
    const size_t item[4] = {16, 16, 4, 1};
    bool ok = p.chunk >= 1 && p.chunk <= n && (p.chunk == n || p.chunk % 64 == 0) && p.total <= kCastStagingBytes;
    ok = ok && p.present[0] && p.present[1] && p.present[2] == limits && p.present[3];
    for (int i = 4; i < kStagingMaxArrays; ++i) ok = ok && !p.present[i];
    size_t end = 0;
    for (int i = 0; i < 4; ++i) {
        if (!p.present[i]) {
            ok = ok && p.bytes[i] == 0;
            continue;
        }
        ok = ok && p.off[i] % 16 == 0 && p.off[i] >= end && p.bytes[i] == p.chunk * item[i] &&
             p.off[i] + p.bytes[i] <= p.total;
        end = p.off[i] + p.bytes[i];
    }
    // the answer bytes come last and end the allocation exactly
    ok = ok && end == p.total;
    if (want_chunk) ok = ok && p.chunk == want_chunk && p.total == want_total;
    if (!ok) {
        std::printf("FAIL occluded_rays_plan(%zu, %d): chunk %zu total %zu offsets", n, (int)limits, p.chunk, p.total);
        for (int i = 0; i < 4; ++i) std::printf(p.present[i] ? " %zu" : " -", p.off[i]);
        std::printf("\n");
    }
    return ok ? 0 : 1;
}

}  // namespace

int main()
{
    int bad = 0;
    // per ray 33 / 37 bytes: (2^28 - 64) / 33 = 8134405 -> 8134400, / 37 = 7255010 -> 7254976
    bad += check(100000000, false, 8134400, (size_t)8134400 * 33);
    bad += check(100000000, true, 7254976, (size_t)7254976 * 37);
    bad += check(0xFFFFFFFFu, true, 7254976, (size_t)7254976 * 37);
    // small and ragged batches: one chunk, 16-byte offsets, the bytes exact
    bad += check(101, false, 101, 1616 + 1616 + 101);
    bad += check(101, true, 101, 1616 + 1616 + 416 + 101);
    bad += check(1, true, 1, 16 + 16 + 16 + 1);
    bad += check(1, false, 1, 16 + 16 + 1);
    for (size_t n : {(size_t)63, (size_t)64, (size_t)65, (size_t)4099, (size_t)8134399, (size_t)8134400, (size_t)8134401})
        for (bool l : {false, true}) bad += check(n, l, 0, 0);
    if (bad) return 1;
    std::printf("ok\n");
    return 0;
}
