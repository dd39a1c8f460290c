// Host check of adaptive sampling's tile plan (spt_adaptive.h): the rectangles adaptive_rect
// gives the flagged 8x8 tiles of a region, walked in ascending tile order with the running
// sums of adaptive_add as adaptive_plan_kernel walks them -- once in one run, once cut into
// the kernel's 1 024 runs with a prefix sum between them.  For every region, flag pattern,
// pass length and claim: rectangles ascending in item_off, every item_off a multiple of the
// claim, item ranges disjoint, slot_off compact and inside the total, each rectangle's
// pixels (through ts_item, as the render kernels start paths) inside the region and covering
// exactly the flagged tiles once per sample, and the totals.  Exit 0 = pass.
#include <cstdio>
#include <vector>

#include "spt_adaptive.h"

namespace {

struct Plan {
    std::vector<spt::BatchRect> rects;
    spt::AdaptCount count{};
};

// the kernel's walk, in one run
Plan plan_serial(const spt::AdaptGeom &g, const std::vector<uint32_t> &flags)
{
    Plan p;
    spt::AdaptSum at{0u, 0u, 0u};
    for (uint32_t i = 0; i < flags.size(); ++i) {
        if (!flags[i]) continue;
        p.rects.push_back(spt::adaptive_rect(g, i, at.items, at.slots));
        spt::adaptive_add(g, i, at);
    }
    p.count.n_rects = at.rects;
    p.count.n_slots = at.slots;
    p.count.n_items = p.rects.empty() ? 0u : p.rects.back().item_end;
    return p;
}

// the kernel's walk as its threads do it: `threads` runs of consecutive tiles, each run's
// sums first, an exclusive prefix over the runs, then the rectangles
Plan plan_runs(const spt::AdaptGeom &g, const std::vector<uint32_t> &flags, uint32_t threads)
{
    const uint32_t n = (uint32_t)flags.size(), per = (n + threads - 1u) / threads;
    std::vector<spt::AdaptSum> own(threads, spt::AdaptSum{0u, 0u, 0u});
    auto lo = [&](uint32_t t) { return std::min(t * per, n); };
    for (uint32_t t = 0; t < threads; ++t)
        for (uint32_t i = lo(t); i < std::min(lo(t) + per, n); ++i)
            if (flags[i]) spt::adaptive_add(g, i, own[t]);
    Plan p;
    spt::AdaptSum total{0u, 0u, 0u};
    for (const spt::AdaptSum &o : own) {
        total.rects += o.rects;
        total.items += o.items;
        total.slots += o.slots;
    }
    p.rects.resize(total.rects);
    spt::AdaptSum before{0u, 0u, 0u};
    for (uint32_t t = 0; t < threads; ++t) {
        spt::AdaptSum at = before;
        for (uint32_t i = lo(t); i < std::min(lo(t) + per, n); ++i) {
            if (!flags[i]) continue;
            p.rects[at.rects] = spt::adaptive_rect(g, i, at.items, at.slots);
            if (at.rects + 1u == total.rects) p.count.n_items = p.rects[at.rects].item_end;
            spt::adaptive_add(g, i, at);
        }
        before.rects += own[t].rects;
        before.items += own[t].items;
        before.slots += own[t].slots;
    }
    p.count.n_rects = total.rects;
    p.count.n_slots = total.slots;
    return p;
}

bool same_rect(const spt::BatchRect &a, const spt::BatchRect &b)
{
    return a.item_off == b.item_off && a.item_end == b.item_end && a.slot_off == b.slot_off && a.pix_off == b.pix_off &&
           a.x0 == b.x0 && a.y0 == b.y0 && a.w == b.w && a.rows == b.rows && a.npix == b.npix && a.alias == b.alias &&
           a.rgb8 == b.rgb8 && a.div_band.d == b.div_band.d && a.div_band.m == b.div_band.m && a.div_band.s == b.div_band.s &&
           a.div_tile.d == b.div_tile.d && a.div_tile.m == b.div_tile.m && a.div_tile.s == b.div_tile.s;
}

#define FAIL(...)                 \
    do {                          \
        std::printf("FAIL ");     \
        std::printf(__VA_ARGS__); \
        std::printf("\n");        \
        return false;             \
    } while (0)

bool check(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t take, uint32_t claim, const std::vector<uint32_t> &flags,
           const char *what)
{
    const spt::AdaptGeom g = spt::adaptive_geom(x0, y0, w, h, take, claim);
    if (g.tiles_x * g.tiles_y != flags.size()) FAIL("%s: %ux%u tiles", what, g.tiles_x, g.tiles_y);
    const Plan p = plan_serial(g, flags), q = plan_runs(g, flags, 1024u);
    if (p.rects.size() != q.rects.size() || p.count.n_rects != q.count.n_rects || p.count.n_items != q.count.n_items ||
        p.count.n_slots != q.count.n_slots)
        FAIL("%s %ux%u take %u claim %u: the runs' counts differ", what, w, h, take, claim);
    for (size_t i = 0; i < p.rects.size(); ++i)
        if (!same_rect(p.rects[i], q.rects[i])) FAIL("%s %ux%u: rect %zu differs between the walks", what, w, h, i);
    uint32_t flagged = 0;
    for (uint32_t f : flags) flagged += f ? 1u : 0u;
    if (p.count.n_rects != flagged || p.rects.size() != flagged) FAIL("%s %ux%u: %u rects for %u flags", what, w, h, p.count.n_rects, flagged);
    // seen[sample][pixel of the region]
    std::vector<unsigned char> seen((size_t)take * w * h, 0);
    uint64_t item = 0, slot = 0;
    uint32_t last_tile = 0;
    for (size_t i = 0; i < p.rects.size(); ++i) {
        const spt::BatchRect &r = p.rects[i];
        if (r.item_off % claim != 0u) FAIL("%s %ux%u: rect %zu item_off %u is no multiple of the claim %u", what, w, h, i, r.item_off, claim);
        if (r.item_off < item) FAIL("%s %ux%u: rect %zu item_off %u overlaps the one before (%llu)", what, w, h, i, r.item_off, (unsigned long long)item);
        if (r.item_off - item >= claim) FAIL("%s %ux%u: rect %zu leaves a whole claim empty", what, w, h, i);
        if (r.item_end != r.item_off + r.npix * take || r.npix != r.w * r.rows) FAIL("%s %ux%u: rect %zu item_end / npix", what, w, h, i);
        if (r.slot_off != slot) FAIL("%s %ux%u: rect %zu slot_off %u, compact %llu", what, w, h, i, r.slot_off, (unsigned long long)slot);
        if (i > 0 && r.pix_off <= last_tile) FAIL("%s %ux%u: rect %zu tile order", what, w, h, i);
        if (r.pix_off >= flags.size() || !flags[r.pix_off]) FAIL("%s %ux%u: rect %zu is tile %u, not flagged", what, w, h, i, r.pix_off);
        if (r.alias != 0u || r.rgb8 != nullptr) FAIL("%s %ux%u: rect %zu alias / rgb8", what, w, h, i);
        last_tile = r.pix_off;
        const uint32_t ty = r.pix_off / g.tiles_x, tx = r.pix_off % g.tiles_x;
        for (uint32_t k = 0; k < r.item_end - r.item_off; ++k) {
            uint32_t sl, lr, col;
            spt::ts_item(k, r.w, r.rows, take, r.div_band, r.div_tile, sl, lr, col);
            if (sl >= take || lr >= r.rows || col >= r.w) FAIL("%s %ux%u: rect %zu item %u -> (%u, %u, %u)", what, w, h, i, k, sl, lr, col);
            const uint32_t x = r.x0 + col, y = r.y0 + lr;
            if (x < x0 || x >= x0 + w || y < y0 || y >= y0 + h) FAIL("%s %ux%u: rect %zu item %u leaves the region: (%u, %u)", what, w, h, i, k, x, y);
            if ((x - x0) >> 3 != tx || (y - y0) >> 3 != ty) FAIL("%s %ux%u: rect %zu item %u leaves its tile", what, w, h, i, k);
            unsigned char &s = seen[((size_t)sl * h + (y - y0)) * w + (x - x0)];
            if (s++) FAIL("%s %ux%u: rect %zu item %u: sample %u of (%u, %u) twice", what, w, h, i, k, sl, x, y);
            // the fold's address of the word: ts_slot_base over the tile alone
            uint32_t q0, step;
            spt::ts_slot_base(lr, col, r.w, r.rows, take, q0, step);
            if (q0 + sl * step != k) FAIL("%s %ux%u: rect %zu item %u: slot %u + %u * %u", what, w, h, i, k, q0, sl, step);
        }
        item = r.item_end;
        slot += (uint64_t)r.npix * take;
    }
    if (p.count.n_items != (uint32_t)item || p.count.n_slots != slot) FAIL("%s %ux%u: totals", what, w, h);
    // covered exactly the flagged tiles, every sample
    for (uint32_t s = 0; s < take; ++s)
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const bool want = flags[(y >> 3) * g.tiles_x + (x >> 3)] != 0u;
                if ((seen[((size_t)s * h + y) * w + x] != 0) != want) FAIL("%s %ux%u: sample %u of local (%u, %u): covered %d, flagged %d", what, w, h, s, x, y, !want, want);
            }
    // the host's worst case is the all-set plan
    if (flagged == flags.size()) {
        uint64_t items_pad, slots;
        spt::adaptive_totals(g, items_pad, slots);
        const uint32_t last_pad = (p.rects.back().item_end + claim - 1u) / claim * claim;
        if (slots != slot || items_pad != last_pad) FAIL("%s %ux%u: adaptive_totals %llu / %llu against %u / %llu", what, w, h, (unsigned long long)items_pad, (unsigned long long)slots, last_pad, (unsigned long long)slot);
    }
    return true;
}

}  // namespace

int main()
{
    const uint32_t regions[][2] = {{1, 1}, {7, 5}, {8, 8}, {9, 17}, {45, 37}, {1200, 800}};
    uint64_t z = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return z; };
    for (auto &rg : regions) {
        const uint32_t w = rg[0], h = rg[1], tx = (w + 7) / 8, ty = (h + 7) / 8, n = tx * ty;
        const bool big = (uint64_t)w * h > 100000;
        const uint32_t takes[] = {1, 3, 8, 11}, claims[] = {64, 192, 448};
        for (uint32_t take : takes)
            for (uint32_t claim : claims) {
                if (big && !((take == 3 && claim == 192) || (take == 1 && claim == 448))) continue;
                const uint32_t x0 = take == 3 ? 5u : 0u, y0 = take == 3 ? 3u : 0u;  // a region off the frame's own grid
                std::vector<uint32_t> f(n, 1u);
                if (!check(x0, y0, w, h, take, claim, f, "all set")) return 1;
                f.assign(n, 0u);
                if (!check(x0, y0, w, h, take, claim, f, "none set")) return 1;
                const uint32_t corners[] = {0u, tx - 1u, (ty - 1u) * tx, n - 1u};
                for (uint32_t c : corners) {
                    f.assign(n, 0u);
                    f[c] = 0x01010101u;  // any nonzero word
                    if (!check(x0, y0, w, h, take, claim, f, "one corner")) return 1;
                }
                for (int rep = 0; rep < (big ? 2 : 6); ++rep) {
                    const uint32_t den = 2u + (uint32_t)rep * 3u;  // from half to one in 17
                    for (uint32_t i = 0; i < n; ++i) f[i] = rnd() % den == 0 ? 1u : 0u;
                    if (!check(x0, y0, w, h, take, claim, f, "random")) return 1;
                }
            }
    }
    std::printf("ok\n");
    return 0;
}
