// Host check of the staging plans of the five blocking queries (spt_staging.h): for each
// form and each combination of its optional outputs, the chunk, every array's offset and
// the total equal the numbers the forms computed inline before the plan existed (written
// out below as literals: 256 MiB of staging, whole waves of rays, whole 8-row bands, the
// denoiser's single chunk); offsets are multiples of 16, ascending and non-overlapping,
// and absent arrays take no bytes.  Standard headers only.  Exit 0 = pass.
#include <cstdio>

#include "spt_staging.h"

using namespace spt_api;

namespace {

constexpr size_t X = (size_t)-1;  // an absent array

struct Case {
    const char *what;
    StagingPlan plan;
    size_t chunk, off[kStagingMaxArrays], total;
};
#define P(call) #call, call

const Case kCases[] = {
    // spt_cast_rays(n, hit): per ray 36 / 68 bytes
    {P(cast_rays_plan(10000000, false)), 7456512, {0, 119304192, 238608384, X}, 268434432},
    {P(cast_rays_plan(10000000, true)), 3947520, {0, 63160320, 126320640, 142110720}, 268431360},
    {P(cast_rays_plan(101, false)), 101, {0, 1616, 3232, X}, 3648},
    {P(cast_rays_plan(101, true)), 101, {0, 1616, 3232, 3648}, 6880},
    // spt_primary_hits(n, hit, dirs)
    {P(primary_hits_plan(50000000, false, false)), 16777152, {0, 201325824, X, X}, 268434432},
    {P(primary_hits_plan(50000000, false, true)), 8388544, {0, 100662528, X, 134216704}, 268433408},
    {P(primary_hits_plan(50000000, true, false)), 5592384, {0, 67108608, 89478144, X}, 268434432},
    {P(primary_hits_plan(50000000, true, true)), 4194240, {0, 50330880, 67107840, 201323520}, 268431360},
    {P(primary_hits_plan(101, false, false)), 101, {0, 1216, X, X}, 1632},
    {P(primary_hits_plan(101, false, true)), 101, {0, 1216, X, 1632}, 3248},
    {P(primary_hits_plan(101, true, false)), 101, {0, 1216, 1632, X}, 4864},
    {P(primary_hits_plan(101, true, true)), 101, {0, 1216, 1632, 4864}, 6480},
    // spt_trace_rays(n, info)
    {P(trace_rays_plan(10000000, false)), 4793472, {0, 76695552, 153391104, 230086656, X}, 268434432},
    {P(trace_rays_plan(10000000, true)), 4194240, {0, 67107840, 134215680, 201323520, 234877440}, 268431360},
    {P(trace_rays_plan(101, false)), 101, {0, 1616, 3232, 4848, X}, 5664},
    {P(trace_rays_plan(101, true)), 101, {0, 1616, 3232, 4848, 5664}, 6480},
    // spt_render_features(w, h, feat, ids): more rows than a chunk, fewer, a ragged band
    {P(features_plan(8192, 8192, true, true)), 904, {0, 236978176}, 266600448},
    {P(features_plan(8192, 8192, true, false)), 1024, {0, X}, 268435456},
    {P(features_plan(8192, 8192, false, true)), 8192, {X, 0}, 268435456},
    {P(features_plan(1201, 13, true, true)), 13, {0, 499616}, 562080},
    {P(features_plan(1201, 13, true, false)), 13, {0, X}, 499616},
    {P(features_plan(1201, 13, false, true)), 13, {X, 0}, 62464},
    {P(features_plan(3, 5, true, true)), 5, {0, 480}, 544},
    {P(features_plan(3, 5, true, false)), 5, {0, X}, 480},
    {P(features_plan(3, 5, false, true)), 5, {X, 0}, 64},
    // spt_denoise(npix, planes = min(levels - 1, 2), out_rgba, out_rgb8): 1201 x 801, 5 x 3; mom and
    // out_var, the variance-guided form's arrays, are absent and the bytes stay last
    {P(denoise_plan(962001, 0, true, true)), 962001, {0, 15392016, 46176048, X, X, X, 61568064}, 64454067},
    {P(denoise_plan(962001, 0, true, false)), 962001, {0, 15392016, 46176048, X, X, X, X}, 61568064},
    {P(denoise_plan(962001, 0, false, true)), 962001, {0, 15392016, X, X, X, X, 46176048}, 49062051},
    {P(denoise_plan(962001, 1, true, true)), 962001, {0, 15392016, 46176048, 61568064, X, X, 76960080}, 79846083},
    {P(denoise_plan(962001, 1, true, false)), 962001, {0, 15392016, 46176048, 61568064, X, X, X}, 76960080},
    {P(denoise_plan(962001, 1, false, true)), 962001, {0, 15392016, X, 46176048, X, X, 61568064}, 64454067},
    {P(denoise_plan(962001, 2, true, true)), 962001, {0, 15392016, 46176048, 61568064, X, X, 92352096}, 95238099},
    {P(denoise_plan(962001, 2, true, false)), 962001, {0, 15392016, 46176048, 61568064, X, X, X}, 92352096},
    {P(denoise_plan(962001, 2, false, true)), 962001, {0, 15392016, X, 46176048, X, X, 76960080}, 79846083},
    {P(denoise_plan(15, 0, true, true)), 15, {0, 240, 720, X, X, X, 960}, 1005},
    {P(denoise_plan(15, 0, true, false)), 15, {0, 240, 720, X, X, X, X}, 960},
    {P(denoise_plan(15, 0, false, true)), 15, {0, 240, X, X, X, X, 720}, 765},
    {P(denoise_plan(15, 1, true, true)), 15, {0, 240, 720, 960, X, X, 1200}, 1245},
    {P(denoise_plan(15, 1, true, false)), 15, {0, 240, 720, 960, X, X, X}, 1200},
    {P(denoise_plan(15, 1, false, true)), 15, {0, 240, X, 720, X, X, 960}, 1005},
    {P(denoise_plan(15, 2, true, true)), 15, {0, 240, 720, 960, X, X, 1440}, 1485},
    {P(denoise_plan(15, 2, true, false)), 15, {0, 240, 720, 960, X, X, X}, 1440},
    {P(denoise_plan(15, 2, false, true)), 15, {0, 240, X, 720, X, X, 1200}, 1245},
    // spt_denoise_var(..., mom = true, out_var): 16 B of mom and 4 B of out_var per pixel (4 * 962001 =
    // 3848004 takes 3848016, 4 * 15 = 60 takes 64) after the planes, before the bytes
    {P(denoise_plan(962001, 2, true, true, true, true)), 962001, {0, 15392016, 46176048, 61568064, 92352096, 107744112, 111592128}, 114478131},
    {P(denoise_plan(962001, 2, true, true, true, false)), 962001, {0, 15392016, 46176048, 61568064, 92352096, X, 107744112}, 110630115},
    {P(denoise_plan(962001, 0, false, true, true, true)), 962001, {0, 15392016, X, X, 46176048, 61568064, 65416080}, 68302083},
    {P(denoise_plan(962001, 1, true, false, true, false)), 962001, {0, 15392016, 46176048, 61568064, 76960080, X, X}, 92352096},
    {P(denoise_plan(15, 2, true, true, true, true)), 15, {0, 240, 720, 960, 1440, 1680, 1744}, 1789},
    {P(denoise_plan(15, 2, true, true, true, false)), 15, {0, 240, 720, 960, 1440, X, 1680}, 1725},
    {P(denoise_plan(15, 0, false, true, true, true)), 15, {0, 240, X, X, 720, 960, 1024}, 1069},
    {P(denoise_plan(15, 1, true, false, true, false)), 15, {0, 240, 720, 960, 1200, X, X}, 1440},
};

}  // namespace

int main()
{
    for (const Case &c : kCases) {
        const StagingPlan &p = c.plan;
        bool ok = p.chunk == c.chunk && p.total == c.total;
        size_t end = 0;
        for (int i = 0; i < kStagingMaxArrays; ++i) {
            if (!p.present[i]) {
                ok = ok && (c.off[i] == X || c.off[i] == 0);  // (rows past the form's arrays are zero-filled)
                continue;
            }
            // at its literal, on a 16-byte boundary, after the last byte of everything before
            // it, and with all its own bytes inside the allocation
            ok = ok && p.off[i] == c.off[i] && p.off[i] % 16 == 0 && p.off[i] >= end && p.bytes[i] > 0 &&
                 p.off[i] + p.bytes[i] <= p.total;
            end = p.off[i] + p.bytes[i];
        }
        if (!ok) {
            std::printf("FAIL %s: chunk %zu total %zu offsets", c.what, p.chunk, p.total);
            for (int i = 0; i < kStagingMaxArrays; ++i) std::printf(p.present[i] ? " %zu" : " -", p.off[i]);
            std::printf("\n");
            return 1;
        }
    }
    // non-overlap, and no bytes for absent arrays: with every array's own size written out,
    // each present array ends where the next begins (rounded up to 16) and the last at the total
    {
        const StagingArray a[4] = {{12}, {4, false}, {32}, {3, true, true}};
        const StagingPlan p = staging_plan(a, 4, 101, StagingItems::kRays);
        if (p.chunk != 101 || p.off[0] != 0 || p.present[1] || p.off[2] != 1216 || p.off[3] != 1216 + 3232 ||
            p.total != 1216 + 3232 + 303) {
            std::printf("FAIL generic plan\n");
            return 1;
        }
    }
    // a chunk is whole waves / whole bands, and at least one, however large an item is
    if (cast_chunk(68) != 3947520 || cast_chunk((size_t)1 << 30) != 64 || band_chunk((size_t)1 << 30) != 8) {
        std::printf("FAIL chunk bounds\n");
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
