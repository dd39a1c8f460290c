// spt_codes.h -- the sample codes and the indexing of the fold's colour
// table: plain integer arithmetic shared by the kernels and the host, free of the HIP
// headers so that a host-only program can include it (tests/cpp/ctab_check.cpp).
// spt_internal.h includes it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SPT_HD __host__ __device__
#else
#define SPT_HD
#endif

namespace spt {

// Division of x < 2^31 by a divisor d >= 1 fixed for a launch (Granlund-Montgomery,
// N = 31 bits): l = ceil(log2 d), m = floor(2^(31+l) / d) + 1 < 2^32, and
// x / d == mulhi(x, m) >> (l - 1) for every x < 2^31; d == 1 passes x through.
struct FastDiv {
    uint32_t d, m, s;
};
inline FastDiv make_fastdiv(uint32_t d)
{
    FastDiv f{d, 0u, 0u};
    if (d <= 1u) return f;
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    f.m = (uint32_t)(((1ull << (31 + l)) / d) + 1ull);
    f.s = l - 1u;
    return f;
}
SPT_HD inline uint32_t fast_div(uint32_t x, const FastDiv &f)
{
#ifdef __HIP_DEVICE_COMPILE__
    const uint32_t hi = __umulhi(x, f.m);
#else
    const uint32_t hi = (uint32_t)(((uint64_t)x * f.m) >> 32);
#endif
    return f.d <= 1u ? x : hi >> f.s;
}

// Sample codes: one 32-bit word per sample instead of its colour.  A
// sample's colour is one of
//   * the sky, initColor * k * 0.5 with k = d.y + 1.f of the final ray
//     (SampleColorSkybox, SingleThreadPathTracer.hpp:11-14): the word is k's bits;
//   * a diffuse albedo halved 1 + j times (SampleColorDiffuse, lines 21-37: the first
//     diffuse hit's colour * 0.5, then * 0.5 per further bounce): a code naming the
//     first hit's slot and j;
//   * 0 (the specular-event cap; RenderSegmentTask's dropped paths).
// A finite k is 0 or at least 2^-24 in magnitude (fl(y + 1) for float y: only y = -1
// lies within 2^-24 of -1), so the words whose magnitude as a float is below 2^-24 and
// nonzero never hold a k: they carry the codes c in [1, kCodeMax], positive words
// first, then the same magnitudes with the sign bit.  c = 1 is the colour 0,
// c = 2 + j * stride + slot a diffuse sample (stride = the scene's slot count).  j is
// saturated at jmax = min(bounces - 1, jz): j <= bounces - 1 always, and after jz
// halvings every finite albedo of the scene is 0 (inf / NaN stay themselves; jz <=
// kCodeSat, since 2^-280 * FLT_MAX rounds to 0), so saturating there changes no colour.
// A scene fits when (jmax + 1) * stride + 1 <= kCodeMax: ~34 M slots at depth 50, ~11 M
// for deep paths over albedos up to 255 (jz = 157).  The fold rebuilds the colour with
// the render kernel's own operations: bit-identical.
constexpr uint32_t kCodeSmall = 0x33800000u;        // bits of 2^-24
constexpr uint32_t kCodeMax = 2u * (kCodeSmall - 1u);  // the largest code
constexpr uint32_t kCodeSat = 280;                  // 2^-280 * FLT_MAX rounds to 0
SPT_HD inline bool code_layout_fits(uint64_t stride, uint32_t jmax)
{
    return (jmax + 1ull) * stride + 1ull <= kCodeMax;
}
// diffuse code of (j, slot) and back (div = FastDiv(stride))
SPT_HD inline uint32_t diffuse_code(uint32_t j, uint32_t slot, uint32_t stride)
{
    return 2u + j * stride + slot;
}
SPT_HD inline void diffuse_decode(uint32_t c, const FastDiv &div, uint32_t &j, uint32_t &slot)
{
    const uint32_t v = c - 2u;  // < kCodeMax < 2^31 (fast_div's range)
    j = fast_div(v, div);
    slot = v - j * div.d;
}
SPT_HD inline uint32_t code_word(uint32_t c)
{
    return c < kCodeSmall ? c : 0x80000000u | (c - kCodeSmall + 1u);
}
// the code of a word, 0 for a sky word
SPT_HD inline uint32_t word_code(uint32_t w)
{
    const uint32_t a = w & 0x7FFFFFFFu;
    if (a == 0u || a >= kCodeSmall) return 0u;
    return (w >> 31) ? a + kCodeSmall - 1u : a;
}
constexpr uint32_t kZeroWord = 1u;  // code_word(1): the colour 0

// The fold's colour table (spt_decode.h): one float4 per diffuse code of
// the scene at the context's depth, entry c - 2 the colour of code c, (jmax + 1) * stride
// entries, filled on the device by the first launched render after the slot order, the
// shading table or jmax changed.
// A table above kCtabMaxBytes is not built (deep paths over a scene near the code
// capacity would want gigabytes): the kernels then decode every word arithmetically.
constexpr uint64_t kCtabMaxBytes = 32ull << 20;
constexpr uint64_t kCtabEntryBytes = 16;  // float4
SPT_HD inline uint64_t ctab_entries(uint64_t stride, uint32_t jmax) { return (jmax + 1ull) * stride; }
SPT_HD inline bool ctab_fits(uint64_t stride, uint32_t jmax)
{
    return ctab_entries(stride, jmax) * kCtabEntryBytes <= kCtabMaxBytes;
}
// The entry read for code c of a table of n >= 1 entries: c - 2, clamped into the table.
// The render writes diffuse codes below 2 + n only; any other word (codes 0 and 1 wrap to
// the top, a word the render never wrote) reads the last entry instead of memory outside.
SPT_HD inline uint32_t ctab_index(uint32_t c, uint32_t n)
{
    const uint32_t v = c - 2u, last = n - 1u;
    return v < last ? v : last;
}
// does word w carry a code (word_code(w) != 0)?  With a = w & 0x7FFFFFFF: 1 <= a < kCodeSmall,
// as one shift-add and one compare: (w << 1) drops the sign, 2 a - 2 wraps to the top for a = 0
SPT_HD inline bool word_is_code(uint32_t w) { return (w << 1) - 2u < 2u * kCodeSmall - 2u; }
// ctab_index(word_code(w), n) of a code word w, straight from the word: a table has at most
// kCtabMaxBytes / 16 = 2^21 entries, far fewer than the kCodeSmall - 1 codes of the
// positive words, so a positive code word is its own code (w - 2 = c - 2) and a word with
// the sign bit (c >= kCodeSmall) lies past the table either way: w - 2 >= 2^31 - 1 clamps to
// the last entry as c - 2 does.  (A sky word gets some entry in the table; its colour does
// not come from there.)
SPT_HD inline uint32_t ctab_word_index(uint32_t w, uint32_t n)
{
    const uint32_t v = w - 2u, last = n - 1u;
    return v < last ? v : last;
}

}  // namespace spt
