// spt_readahead.h -- the HIP-free half of the tiling read-ahead (the HIP half is
// spt_readahead.cpp): which rectangles are tiles of the reference's tc x tc tiling
// (Renderer.hpp:264-273, MakeRenderSegmentData), the bookkeeping that decides what a tile's
// call does, and the gate that keeps the read-ahead frame's bytes in place under the serves
// copying out of them.  Standard headers only: tests/cpp/readahead_check.cpp drives it on the
// CPU.  Everything here is called with the context's mutex held.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <vector>

namespace spt_api {

constexpr uint32_t kSpecMaxTiles = 64 * 64;

// The tc x tc tiling of a W x H frame in one mode: tiles of sw() x sh() pixels, numbered
// row-major over tile rows j, columns i.
struct Tiling {
    int mode = -1;
    uint32_t tc = 0, W = 0, H = 0;
    uint32_t sw() const { return W / tc; }
    uint32_t sh() const { return H / tc; }
    size_t tiles() const { return (size_t)tc * tc; }
    bool operator==(const Tiling &o) const { return mode == o.mode && tc == o.tc && W == o.W && H == o.H; }
};

// The tile of a tiling of the W x H frame that the rectangle [xB, xE) x [yB, yE) is (*out:
// the tiling), or -1: W / tc x H / tc pixels at a multiple of that, tc even.
inline int64_t tile_of(uint32_t W, uint32_t H, int mode, uint32_t xB, uint32_t xE, uint32_t yB, uint32_t yE,
                       Tiling *out)
{
    if (xE <= xB || yE <= yB) return -1;
    const uint32_t w = xE - xB, h = yE - yB, tc = W / w;
    if (!(tc >= 2 && tc % 2 == 0 && (uint64_t)tc * tc <= kSpecMaxTiles && W / tc == w && H / tc == h &&
          xB % w == 0 && yB % h == 0 && xB / w < tc && yB / h < tc))
        return -1;
    *out = Tiling{mode, tc, W, H};
    return (int64_t)(yB / h) * tc + xB / w;
}

// Whether a whole frame of the tiling renders in the read-ahead's launches: its per-sample
// slots (slot_bytes, batch_slot_bytes of all its pixels) within the workspace, its items
// (each tile's rounded up to a claim) below the kernels' 2^31 bound.
inline bool tiling_fits(const Tiling &t, uint32_t spp, uint64_t slot_bytes, uint64_t ws_bytes)
{
    return slot_bytes <= ws_bytes && (uint64_t)t.sw() * t.sh() * (t.tc * t.tc + t.tc) * spp < 0x7FFF0000ull;
}

// The read-ahead's bookkeeping: the current frame and which of its tiles have been served,
// and the tiling the caller's plain calls are arming.
class ReadAhead {
public:
    enum class Step {
        Miss,           // render the call as usual
        NoteMiss,       // the same; the tile now counts towards arming its tiling
        PrepareMiss,    // the same; this call armed the tiling: allocate the read-ahead's buffers
        PrepareLaunch,  // arm_first, a tiling's first call: allocate, then ask again (-> Launch)
        Launch,         // armed and no frame to serve from: render one, then ask again (-> Serve)
        Serve,          // copy the tile out of the current frame
        ServeOwed,      // the same, for a call an earlier frame of the tiling still owed
    };

    // arm at a tiling's first call instead of after a whole tiling (the drop-in,
    // spt_prepare_dropin: its caller is RenderImageParallelMain, which renders every tile
    // of every frame -- and MainLoop only one frame per process)
    void set_arm_first(bool on) { arm_first_ = on; }
    bool arm_first() const { return arm_first_; }

    // What the call of tile k of t must do, gen being the context's generation (spt_ctx::gen).
    Step next(const Tiling &t, size_t k, uint64_t gen)
    {
        if (active_ && frame_ == t && gen_ == gen) {
            if (!served_[k]) {
                served_[k] = 1;
                return Step::Serve;
            }
            if (owed_[k] > 0) {
                // a call an earlier frame still owed (late RenderJob thread): same bytes
                --owed_[k];
                return Step::ServeOwed;
            }
        }
        if (armed_ && arm_ == t) return Step::Launch;
        // not armed: note the tile; the tiling arms once all its tiles have been called
        if (!(arm_ == t)) {
            arm_ = t;
            arm_seen_.assign(t.tiles(), 0);
            arm_count_ = 0;
            armed_ = false;
        }
        if (arm_seen_[k]) return Step::Miss;
        // arm_first: the first call of a tiling (RenderImageParallelMain's detached threads
        // reach the library in no fixed order) arms it and starts the read-ahead at once --
        // the one frame of the reference's MainLoop is then rendered whole
        const bool now = arm_first_ && arm_count_ == 0;
        arm_seen_[k] = 1;
        armed_ = ++arm_count_ == t.tiles() || now;
        return now ? Step::PrepareLaunch : armed_ ? Step::PrepareMiss : Step::NoteMiss;
    }

    // A frame of t begins.  The unserved tiles of the frame it replaces, when that is one of
    // the same tiling and generation, are owed to late callers: a RenderJob thread that starts
    // only after its frame's final wait ended (Renderer.hpp:242-255, 282-292) is served from
    // this frame (same state, the same bytes) instead of starting another one.  At most 4 per
    // tile, so a caller that never asks for a tile does not accumulate them.
    void begin_frame(const Tiling &t, uint64_t gen)
    {
        if (active_ && frame_ == t && gen_ == gen) {
            for (size_t k = 0; k < owed_.size(); ++k)
                if (!served_[k] && owed_[k] < 4) owed_[k]++;
        } else {
            owed_.assign(t.tiles(), 0);
        }
        active_ = true;
        frame_ = t;
        gen_ = gen;
        served_.assign(t.tiles(), 0);
    }
    // The current frame is gone (its launches failed): nothing is served from it.
    void drop_frame() { active_ = false; }

    uint32_t owed(size_t k) const { return k < owed_.size() ? owed_[k] : 0; }

private:
    bool active_ = false;
    Tiling frame_;
    uint64_t gen_ = 0;                   // the context's generation when the frame began
    std::vector<uint8_t> served_, owed_;  // per tile of frame_ (both tiles() long once a frame began)
    Tiling arm_;                         // the tiling whose tiles plain calls have called so far
    std::vector<uint8_t> arm_seen_;
    uint32_t arm_count_ = 0;
    bool armed_ = false, arm_first_ = false;
};

// Serves copy out of the read-ahead frame with the context unlocked; whoever rewrites or
// reallocates it waits until none is inside.  enter() and leave() with the context's mutex
// held, wait_idle() with its unique_lock (released while waiting).
class ReaderGate {
public:
    void enter() { ++readers_; }
    void leave()
    {
        if (--readers_ == 0) idle_.notify_all();
    }
    void wait_idle(std::unique_lock<std::mutex> &lk)
    {
        idle_.wait(lk, [&] { return readers_ == 0; });
    }

private:
    uint32_t readers_ = 0;
    std::condition_variable idle_;
};

}  // namespace spt_api
