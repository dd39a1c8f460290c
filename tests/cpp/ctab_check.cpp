// Host check of the fold's colour table arithmetic (spt_codes.h), plain g++: for slot
// counts S and saturations jmax, every (j, slot) maps through diffuse_code to a distinct
// entry inside the table and back through diffuse_decode; the entry a kernel reads straight
// from a word (ctab_word_index) is the one of the word's code (ctab_index of word_code) and
// lies inside the table for every word, written by the render or not; word_is_code agrees
// with word_code; the size cap decides at its edge.  Exit 0 and "ok" = pass.
#include <cstdio>
#include <vector>

#include "spt_codes.h"

static int fail(const char *what, unsigned long long a, unsigned long long b, unsigned long long c)
{
    std::printf("FAIL %s: %llu %llu %llu\n", what, a, b, c);
    return 1;
}

int main()
{
    const uint32_t strides[] = {1u, 2u, 164u, 10240u}, jmaxes[] = {0u, 1u, 49u, 280u};
    for (uint32_t S : strides)
        for (uint32_t jmax : jmaxes) {
            const uint64_t n64 = spt::ctab_entries(S, jmax);
            if (n64 != (uint64_t)(jmax + 1u) * S) return fail("entries", S, jmax, n64);
            const bool fits = spt::ctab_fits(S, jmax);
            if (fits != (n64 * 16u <= (32ull << 20))) return fail("fits", S, jmax, n64);
            if (!spt::code_layout_fits(S, jmax)) return fail("codes", S, jmax, n64);
            const uint32_t n = (uint32_t)n64;
            const spt::FastDiv div = spt::make_fastdiv(S);
            std::vector<unsigned char> seen(n, 0);
            for (uint32_t j = 0; j <= jmax; ++j)
                for (uint32_t slot = 0; slot < S; ++slot) {
                    const uint32_t c = spt::diffuse_code(j, slot, S);
                    const uint32_t e = spt::ctab_index(c, n);
                    if (e != c - 2u || e >= n || seen[e]++) return fail("entry", j, slot, e);
                    uint32_t j2, s2;
                    spt::diffuse_decode(e + 2u, div, j2, s2);
                    if (j2 != j || s2 != slot) return fail("back", j, slot, e);
                    // (the fill kernel decodes code_word(e + 2); the fold reads a word's entry)
                    const uint32_t w = spt::code_word(c);
                    if (spt::word_code(w) != c || !spt::word_is_code(w)) return fail("word", j, slot, w);
                    if (fits && spt::ctab_word_index(w, n) != e) return fail("word entry", j, slot, w);
                }
            for (uint32_t e = 0; e < n; ++e)
                if (seen[e] != 1) return fail("cover", S, jmax, e);
            // words the render never wrote, codes 0 and 1, both signs, the range's ends: some
            // entry of the table, and for a code word the one ctab_index gives its code
            const uint32_t probes[] = {0u, 1u, 2u, 3u, n, n + 1u, n + 2u, n + 3u, spt::kCodeSmall - 2u, spt::kCodeSmall - 1u,
                                       spt::kCodeSmall, spt::kCodeSmall + 1u, 0x3F800000u, 0x7F800000u, 0x7FC00000u,
                                       0x7FFFFFFFu};
            for (uint32_t p : probes)
                for (uint32_t sign : {0u, 0x80000000u}) {
                    const uint32_t w = p | sign, c = spt::word_code(w);
                    if (spt::word_is_code(w) != (c != 0u)) return fail("is_code", S, jmax, w);
                    if (spt::ctab_index(c, n) >= n || spt::ctab_word_index(w, n) >= n) return fail("bounds", S, jmax, w);
                    if (fits && c != 0u && spt::ctab_word_index(w, n) != spt::ctab_index(c, n))
                        return fail("probe entry", S, jmax, w);
                }
        }
    // word_is_code against word_code around every boundary of the code range
    for (uint32_t base : {0u, spt::kCodeSmall, 0x7FFFFFF0u})
        for (uint32_t d = 0; d < 64u; ++d)
            for (uint32_t sign : {0u, 0x80000000u}) {
                const uint32_t w = ((base + d - 32u) & 0x7FFFFFFFu) | sign;
                if (spt::word_is_code(w) != (spt::word_code(w) != 0u)) return fail("is_code edge", base, d, w);
            }
    // the cap at its edge: 32 MiB / 16 B = 2^21 entries fit, one more does not
    const uint64_t edge = (32ull << 20) / 16u;
    if (spt::kCtabMaxBytes != (32ull << 20) || spt::kCtabEntryBytes != 16u) return fail("constants", 0, 0, 0);
    if (!spt::ctab_fits(edge, 0) || spt::ctab_fits(edge + 1u, 0)) return fail("cap, one row", edge, 0, 0);
    if (!spt::ctab_fits(edge / 64u, 63) || spt::ctab_fits(edge / 64u + 1u, 63)) return fail("cap, 64 rows", edge, 63, 0);
    if (!spt::ctab_fits(8192, 255) || spt::ctab_fits(8192, 256)) return fail("cap, by depth", 8192, 256, 0);
    // a table that fits has fewer entries than the positive code words: ctab_word_index's premise
    if (edge >= spt::kCodeSmall - 1u) return fail("premise", edge, spt::kCodeSmall, 0);
    std::printf("ok\n");
    return 0;
}
