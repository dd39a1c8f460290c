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

// The table forms.  A diffuse word's colour depends on the scene, its slot order and the
// depth only, so the context keeps decode_sample's answer for every diffuse code of the
// scene in a.ctab (spt_codes.h; filled by ctab_fill_kernel from decode_sample itself: the
// same bits, denormal halvings, inf and NaN albedos included) and a kernel reads it back:
// no division, no halving, no branch.  A kernel is compiled for one form (TAB) and launched
// by the one the context has (fold_uses_table): contexts whose table would pass
// kCtabMaxBytes have none and keep decode_sample.

// the table entry of word w (ctab_word_index: any entry for a sky word or the zero word,
// whose colours ctab_select takes elsewhere); the byte offset fits 32 bits (kCtabMaxBytes),
// so the load is the table's base plus one 32-bit lane offset
__device__ __forceinline__ float4 ctab_load(const FoldArgs &a, uint32_t w)
{
    const uint32_t off = ctab_word_index(w, a.ctab_n) << 4;
    return *(const float4 *)((const char *)a.ctab + off);
}
// the colour of word w given its table entry t: decode_sample's three cases, as selects
__device__ __forceinline__ f3 ctab_select(const FoldArgs &a, uint32_t w, const float4 &t)
{
    const float k = __uint_as_float(w);
    const f3 s = mul(mk(a.sky[0] * k, a.sky[1] * k, a.sky[2] * k), 0.5f);
    const bool coded = word_is_code(w), zero = w == kZeroWord;
    f3 r;
    r.x = coded ? (zero ? 0.f : t.x) : s.x;
    r.y = coded ? (zero ? 0.f : t.y) : s.y;
    r.z = coded ? (zero ? 0.f : t.z) : s.z;
    return r;
}
template <bool TAB>
__device__ __forceinline__ f3 decode_word(const FoldArgs &a, uint32_t w)
{
    if constexpr (TAB)
        return ctab_select(a, w, ctab_load(a, w));
    else
        return decode_sample(a, w);
}
inline bool fold_uses_table(const FoldArgs &a) { return a.ctab != nullptr && a.ctab_n != 0u; }

}  // namespace spt
