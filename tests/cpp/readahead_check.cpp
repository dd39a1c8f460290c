// readahead_check.cpp -- the HIP-free half of the tiling read-ahead (spt_readahead.h) on the
// CPU: tile recognition against the expression it replaced, arming, frames and owed tiles,
// staleness, and the reader gate under threads.  Built with plain g++ and a sanitizer by
// tests/test_readahead_state.py; prints "ok".
#include "spt_readahead.h"

#include <cstdio>
#include <cstdlib>
#include <thread>

using namespace spt_api;
using Step = ReadAhead::Step;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static Tiling tiling(uint32_t W, uint32_t H, uint32_t tc, int mode = 0) { return Tiling{mode, tc, W, H}; }

// tile (i, j) of t through tile_of
static int64_t find(const Tiling &t, uint32_t i, uint32_t j, Tiling *out)
{
    return tile_of(t.W, t.H, t.mode, t.sw() * i, t.sw() * (i + 1), t.sh() * j, t.sh() * (j + 1), out);
}

static void check_recognition()
{
    for (uint32_t W = 1; W <= 24; ++W)
        for (uint32_t H = 1; H <= 24; ++H)
            for (int mode = 0; mode < 2; ++mode)
                for (uint32_t xB = 0; xB < W; ++xB)
                    for (uint32_t xE = xB + 1; xE <= W; ++xE)
                        for (uint32_t yB = 0; yB < H; ++yB)
                            for (uint32_t yE = yB + 1; yE <= H; ++yE) {
                                // the predicate spec_serve had inline (its geometric part), verbatim
                                const uint32_t w = xE - xB, h = yE - yB, tc = W / w;
                                const bool want = tc >= 2 && tc % 2 == 0 && (uint64_t)tc * tc <= kSpecMaxTiles && W / tc == w && H / tc == h &&
                                                  xB % w == 0 && yB % h == 0 && xB / w < tc && yB / h < tc;
                                Tiling t;
                                const int64_t k = tile_of(W, H, mode, xB, xE, yB, yE, &t);
                                CHECK((k >= 0) == want);
                                if (want) {
                                    CHECK((t == Tiling{mode, tc, W, H}));
                                    CHECK(k == (int64_t)((yB / h) * tc + xB / w));
                                }
                            }
    Tiling t;
    const Tiling t4 = tiling(240, 160, 4, 1);
    for (uint32_t j = 0; j < 4; ++j)
        for (uint32_t i = 0; i < 4; ++i) {
            CHECK(find(t4, i, j, &t) == (int64_t)(j * 4 + i));
            CHECK(t == t4 && t.sw() == 60 && t.sh() == 40);
        }
    CHECK(tile_of(240, 160, 0, 0, 240, 0, 160, &t) < 0);  // the full frame, tc = 1
    CHECK(tile_of(240, 160, 0, 0, 80, 0, 53, &t) < 0);    // tc = 3
    CHECK(tile_of(240, 160, 0, 80, 160, 53, 106, &t) < 0);
    CHECK(tile_of(6600, 6600, 0, 0, 100, 0, 100, &t) < 0);  // tc = 66: 66^2 > 4096
    CHECK(tile_of(6400, 6400, 0, 100, 200, 6300, 6400, &t) == 63 * 64 + 1 && t.tc == 64);
    CHECK(tile_of(240, 160, 0, 30, 90, 0, 40, &t) < 0);  // not at a multiple of the tile
    CHECK(tile_of(240, 160, 0, 5, 5, 0, 40, &t) < 0);    // empty
    // the size limits: the frame's slots within the workspace, its items below the bound
    CHECK(tiling_fits(t4, 4, 1000, 1000) && !tiling_fits(t4, 4, 1001, 1000));
    const Tiling big = tiling(16384, 16384, 2);  // 8192^2 * 6 * spp items
    CHECK(tiling_fits(big, 5, 0, 0) && !tiling_fits(big, 6, 0, 0));
}

static void check_arming()
{
    const Tiling t2 = tiling(160, 96, 2);
    {
        ReadAhead ra;  // tile (0, 0) alone, twice: never arms
        CHECK(ra.next(t2, 0, 1) == Step::NoteMiss);
        CHECK(ra.next(t2, 0, 1) == Step::Miss);
        CHECK(ra.next(t2, 0, 1) == Step::Miss);
    }
    const size_t orders[][4] = {{0, 1, 2, 3}, {3, 2, 1, 0}, {2, 0, 3, 1}};
    for (const auto &o : orders)
        for (size_t after = 0; after < 4; ++after) {
            ReadAhead ra;
            for (int n = 0; n < 3; ++n) CHECK(ra.next(t2, o[n], 1) == Step::NoteMiss);
            CHECK(ra.next(t2, o[3], 1) == Step::PrepareMiss);  // the last one arms the tiling
            CHECK(ra.next(t2, after, 1) == Step::Launch);      // then any tile starts a frame
        }
    {
        ReadAhead ra;  // a call from another tiling resets the count
        const Tiling t4 = tiling(160, 96, 4), t2task = tiling(160, 96, 2, 1);
        for (size_t k = 0; k < 3; ++k) CHECK(ra.next(t2, k, 1) == Step::NoteMiss);
        CHECK(ra.next(t4, 5, 1) == Step::NoteMiss);
        for (size_t k = 0; k < 3; ++k) CHECK(ra.next(t2, k, 1) == Step::NoteMiss);
        CHECK(ra.next(t2task, 3, 1) == Step::NoteMiss);  // the other mode is another tiling
        CHECK(ra.next(t2, 3, 1) == Step::NoteMiss);
        for (size_t k = 0; k < 2; ++k) CHECK(ra.next(t2, k, 1) == Step::NoteMiss);
        CHECK(ra.next(t2, 2, 1) == Step::PrepareMiss);
        // armed for t2; another tiling's call disarms it
        CHECK(ra.next(t4, 0, 1) == Step::NoteMiss);
        CHECK(ra.next(t2, 0, 1) == Step::NoteMiss);
    }
    {
        ReadAhead ra;  // arm_first: the very first call prepares and launches
        ra.set_arm_first(true);
        CHECK(ra.arm_first());
        CHECK(ra.next(t2, 2, 1) == Step::PrepareLaunch);
        CHECK(ra.next(t2, 2, 1) == Step::Launch);  // asked again after the prepare
        ra.begin_frame(t2, 1);
        CHECK(ra.next(t2, 2, 1) == Step::Serve);
    }
}

// an armed tc = 2 tiling of generation gen
static void arm(ReadAhead &ra, const Tiling &t, uint64_t gen)
{
    for (size_t k = 0; k < t.tiles(); ++k) (void)ra.next(t, k, gen);
    CHECK(ra.next(t, 0, gen) == Step::Launch);
}

// one call as spec_serve makes it: a Launch begins a frame and asks again; returns launches
static int call(ReadAhead &ra, const Tiling &t, size_t k, uint64_t gen, Step want)
{
    Step s = ra.next(t, k, gen);
    int launches = 0;
    if (s == Step::Launch) {
        ra.begin_frame(t, gen);
        launches = 1;
        s = ra.next(t, k, gen);
    }
    CHECK(s == want);
    return launches;
}

static void check_frames()
{
    const Tiling t2 = tiling(160, 96, 2);
    const size_t a = 0, b = 1, c = 2, d = 3;
    {
        ReadAhead ra;
        arm(ra, t2, 7);
        int launches = 0;
        for (int frame = 0; frame < 3; ++frame)  // each tile served once per frame; a served tile starts the next
            for (size_t k : {c, a, d, b}) launches += call(ra, t2, k, 7, Step::Serve);
        CHECK(launches == 3);
        for (size_t k = 0; k < 4; ++k) CHECK(ra.owed(k) == 0);
    }
    {
        ReadAhead ra;  // test_late_call_is_served_without_another_frame's sequence
        arm(ra, t2, 7);
        int launches = 0;
        for (size_t k : {a, b, c}) launches += call(ra, t2, k, 7, Step::Serve);  // frame 1 without its late d
        CHECK(launches == 1 && ra.owed(d) == 0);
        launches += call(ra, t2, a, 7, Step::Serve);  // frame 2 begins
        CHECK(launches == 2 && ra.owed(d) == 1 && ra.owed(a) == 0 && ra.owed(b) == 0 && ra.owed(c) == 0);
        launches += call(ra, t2, d, 7, Step::Serve);  // frame 1's late call
        CHECK(ra.owed(d) == 1);
        for (size_t k : {b, c}) launches += call(ra, t2, k, 7, Step::Serve);
        launches += call(ra, t2, d, 7, Step::ServeOwed);
        CHECK(launches == 2 && ra.owed(d) == 0);
        launches += call(ra, t2, d, 7, Step::Serve);  // nothing owed any more: frame 3
        CHECK(launches == 3);
    }
    {
        ReadAhead ra;  // a tile that is never called: owed at most 4
        arm(ra, t2, 7);
        for (int frame = 0; frame < 10; ++frame) {
            for (size_t k : {a, b, c}) (void)call(ra, t2, k, 7, Step::Serve);
            CHECK(ra.owed(d) == (uint32_t)(frame < 4 ? frame : 4));
        }
        for (int n = 0; n < 5; ++n) (void)call(ra, t2, d, 7, n == 0 ? Step::Serve : Step::ServeOwed);
        CHECK(ra.owed(d) == 0);
    }
    {
        ReadAhead ra;  // staleness: after the generation changes no tile of the old frame is served
        arm(ra, t2, 7);
        CHECK(call(ra, t2, a, 7, Step::Serve) == 1);
        for (size_t k : {b, c, d, a}) CHECK(ra.next(t2, k, 8) == Step::Launch);
        CHECK(call(ra, t2, b, 8, Step::Serve) == 1);
        CHECK(ra.owed(c) == 0);  // the frame of generation 7 owes nothing to generation 8
        CHECK(ra.next(t2, a, 7) == Step::Launch);
        // a frame whose launches failed is not served from
        ra.drop_frame();
        CHECK(ra.next(t2, c, 8) == Step::Launch);
    }
}

// R1 in miniature: readers enter under the mutex and read the buffer unlocked; the writer
// waits for the gate to be idle, under the same mutex, before it frees the buffer.
static void check_gate()
{
    constexpr int kReaders = 8, kRounds = 2000, kGrow = 200;
    std::mutex mu;
    ReaderGate gate;
    std::vector<uint8_t> buf(4096, 1);
    unsigned long long sums[kReaders] = {};
    long reads = 0;  // under mu: paces the writer, so that its rounds fall among the reads
    std::vector<std::thread> th;
    for (int r = 0; r < kReaders; ++r)
        th.emplace_back([&, r] {
            for (int n = 0; n < kRounds; ++n) {
                std::unique_lock<std::mutex> lk(mu);
                const uint8_t *p = buf.data();
                const size_t len = buf.size();
                gate.enter();
                lk.unlock();
                unsigned long long s = 0;
                for (size_t i = 0; i < len; ++i) s += p[i];
                lk.lock();
                gate.leave();
                ++reads;
                CHECK(s == len);
                sums[r] += s;
            }
        });
    th.emplace_back([&] {
        for (int n = 0; n < kGrow; ++n) {
            std::unique_lock<std::mutex> lk(mu);
            while (reads < (long)n * (kReaders * kRounds / kGrow / 2)) {
                lk.unlock();
                std::this_thread::yield();
                lk.lock();
            }
            gate.wait_idle(lk);
            std::vector<uint8_t>(buf.size() + 64, 1).swap(buf);  // frees the old storage
        }
    });
    for (std::thread &t : th) t.join();
    CHECK(buf.size() == 4096 + 64 * kGrow);
    for (unsigned long long s : sums) CHECK(s >= 4096ull * kRounds);
}

int main()
{
    check_recognition();
    check_arming();
    check_frames();
    check_gate();
    std::printf("ok\n");
    return 0;
}
