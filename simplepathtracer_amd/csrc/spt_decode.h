// spt_decode.h -- the colour of a sample word, shared by the fold (spt_kernels.hip) and
// the path queries' decode pass (spt_trace.hip), so both rebuild a colour with the same
// instructions.
#pragma once
#include "spt_device.h"
#include "spt_internal.h"

#pragma clang fp contract(off)

namespace spt {

// The colour of a sample word (code_word, spt_internal.h), with the render kernel's own
// operations: the sky as SampleColorSkybox computes it (SingleThreadPathTracer.hpp:11-14),
// a diffuse sample as the albedo * 0.5 (line 24) halved once more per further bounce
// (line 31), bit for bit.  Halving is exact while the value stays normal, so j halvings
// are one multiply by 2^-j when the result is normal (or 0 / inf / NaN); otherwise (a
// denormal result: each halving may round) they are done one at a time.
__device__ __forceinline__ float halve_n(float x, uint32_t j)
{
    if (j <= 126u) {
        const float r = x * __uint_as_float((127u - j) << 23);
        if (__builtin_fabsf(r) >= 0x1p-126f || x == 0.f || !__builtin_isfinite(x)) return r;
    }
    for (uint32_t i = 0; i < j; ++i) x = x * 0.5f;
    return x;
}
__device__ __forceinline__ f3 decode_sample(const FoldArgs &a, uint32_t w)
{
    const uint32_t c = word_code(w);
    if (c == 0u) {
        const float k = __uint_as_float(w);
        return mul(mk(a.sky[0] * k, a.sky[1] * k, a.sky[2] * k), 0.5f);
    }
    if (c == 1u) return mk(0.f, 0.f, 0.f);
    uint32_t j, slot;
    diffuse_decode(c, a.code_div, j, slot);
    const float4 sh = a.shade[slot];
    return mk(halve_n(sh.x * 0.5f, j), halve_n(sh.y * 0.5f, j), halve_n(sh.z * 0.5f, j));
}

}  // namespace spt
