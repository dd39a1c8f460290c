// spt_adaptive.h -- adaptive sampling's tile plan (spt_render_adaptive[_dev]; include/spt_hip.h
// "adaptive sampling"): the arithmetic that turns a region's 8x8 tiles into
// the BatchRect table of one pass, shared by adaptive_plan_kernel (spt_adaptive.hip), the host
// loop (spt_adaptive.cpp) and the host check (tests/cpp/adaptive_check.cpp), which therefore
// runs the very code the device runs.
//
// The region [y0, y0 + h) x [x0, x0 + w) is cut into 8x8 tiles anchored at (x0, y0),
// row-major, ragged at the right and bottom edges: tile_pixel's tiles.  A pass renders `take`
// samples of every active tile as one rectangle of a batched launch (spt_internal.h BatchRect):
// its items [item_off, item_end) in ts_item's order over the tile alone ([sample][pixel]),
// item_off a multiple of the launch's claim, its words compact at slot_off.  There are at
// most four tile shapes -- full, right edge, bottom edge, corner -- so everything a rectangle
// holds beside its position and offsets comes from a four-entry table the host fills once per
// pass (adaptive_geom).
#pragma once
#include "spt_internal.h"

namespace spt {

// One tile shape of a pass: w x rows pixels, its items rounded up to the claim, and
// launch_batch's ts_item divisors (rows >= 8 ? 8 * w * take : 1, and 64 * take).
struct AdaptShape {
    uint32_t w, rows, items, items_pad;
    FastDiv div_band, div_tile;
};
// A pass over a region: shape[(bottom edge ? 2 : 0) | (right edge ? 1 : 0)].
struct AdaptGeom {
    uint32_t x0, y0, w, h;       // the region
    uint32_t tiles_x, tiles_y;   // ceil(w / 8), ceil(h / 8)
    uint32_t take, claim;        // samples of the pass, items per claim of its launch
    AdaptShape shape[4];
};

inline AdaptGeom adaptive_geom(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t take, uint32_t claim)
{
    AdaptGeom g{};
    g.x0 = x0;
    g.y0 = y0;
    g.w = w;
    g.h = h;
    g.tiles_x = (w + 7u) >> 3;
    g.tiles_y = (h + 7u) >> 3;
    g.take = take;
    g.claim = claim;
    for (uint32_t k = 0; k < 4u; ++k) {
        AdaptShape &s = g.shape[k];
        s.w = (k & 1u) && (w & 7u) ? (w & 7u) : 8u;
        s.rows = (k & 2u) && (h & 7u) ? (h & 7u) : 8u;
        s.items = s.w * s.rows * take;
        s.items_pad = (s.items + claim - 1u) / claim * claim;
        s.div_band = make_fastdiv(s.rows >= 8u ? 8u * s.w * take : 1u);
        s.div_tile = make_fastdiv(64u * take);
    }
    return g;
}

// the shape of tile `tile` (row-major over tiles_x x tiles_y)
__host__ __device__ inline uint32_t adaptive_shape_of(const AdaptGeom &g, uint32_t tile)
{
    const uint32_t ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    return (ty + 1u == g.tiles_y ? 2u : 0u) | (tx + 1u == g.tiles_x ? 1u : 0u);
}

// Items (claim-padded) and sample words of the pass's worst case, every tile active:
// the host's size check, before anything is launched.
inline void adaptive_totals(const AdaptGeom &g, uint64_t &items_pad, uint64_t &slots)
{
    const uint64_t nx[2] = {g.tiles_x - 1u, 1u}, ny[2] = {g.tiles_y - 1u, 1u};
    items_pad = slots = 0;
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t n = nx[k & 1u] * ny[k >> 1];
        items_pad += n * g.shape[k].items_pad;
        slots += n * g.shape[k].items;
    }
}

// The rectangle of active tile `tile`, given the sums over the active tiles before it:
// item_off (of their padded items) and slot_off (of their npix * take).  pix_off, which no
// render kernel reads, holds the tile index (adaptive_fold_kernel reads it back).
__host__ __device__ inline BatchRect adaptive_rect(const AdaptGeom &g, uint32_t tile, uint32_t item_off, uint32_t slot_off)
{
    const uint32_t ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    const AdaptShape &s = g.shape[adaptive_shape_of(g, tile)];
    BatchRect b;
    b.item_off = item_off;
    b.item_end = item_off + s.items;
    b.slot_off = slot_off;
    b.pix_off = tile;
    b.x0 = g.x0 + (tx << 3);
    b.y0 = g.y0 + (ty << 3);
    b.w = s.w;
    b.rows = s.rows;
    b.npix = s.w * s.rows;
    b.alias = 0u;
    b.rgb8 = nullptr;
    b.div_band = s.div_band;
    b.div_tile = s.div_tile;
    return b;
}

// What the plan leaves in its page-locked host words for the host loop.
struct AdaptCount {
    uint32_t n_rects;  // active tiles
    uint32_t n_items;  // the launch's items: the last rectangle's item_end
    uint32_t n_slots;  // sample words of the pass: the sum of npix * take
    uint32_t pad;
};

// The running sums of the plan's ordered walk over the flagged tiles: rectangles, claim-padded
// items and sample words so far.  The walk visits a run of tiles twice, first for the run's
// sums alone, then -- from the sums of the runs before -- for the rectangles themselves.
struct AdaptSum {
    uint32_t rects, items, slots;
};
__host__ __device__ inline void adaptive_add(const AdaptGeom &g, uint32_t tile, AdaptSum &a)
{
    const AdaptShape &s = g.shape[adaptive_shape_of(g, tile)];
    a.rects += 1u;
    a.items += s.items_pad;
    a.slots += s.items;
}

// ---- launch interface (spt_adaptive.hip) ---------------------------------------------------
// State of a call, owned by the context: per region pixel (local row-major) the in-order
// colour sums {acc.rgb, -} and luminance sums {s1, s2}; per tile one flag word, nonzero = the
// tile is active (set by the fold, cleared by the plan that reads it).
struct AdaptState {
    float4 *acc;
    float2 *s12;
    uint32_t *flags;
};
// One block: rects[] and *count (device view of page-locked host words) of the pass over the
// flagged tiles, in ascending tile order; clears the flags it read.
hipError_t launch_adaptive_plan(const AdaptGeom &g, uint32_t *flags, BatchRect *rects, AdaptCount *count, hipStream_t s);
// One wave per rectangle of the pass: continues the sums with the pass's words (f.samples,
// f's decode tables; f.width / f.height the frame), tests convergence at n = n0 + g.take
// samples and either raises the tile's flag or writes its pixels' outputs (each nullable).
struct AdaptFoldArgs {
    uint32_t n_rects, n0, max_spp, first;
    float tol, lum_floor;
    float4 *out_rgba;
    uint8_t *out_rgb8;
    float4 *mom;
};
hipError_t launch_adaptive_fold(const FoldArgs &f, const AdaptGeom &g, const BatchRect *rects, const AdaptState &st,
                                const AdaptFoldArgs &a, hipStream_t s);

}  // namespace spt
