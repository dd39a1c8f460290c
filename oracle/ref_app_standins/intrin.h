/*
 * <intrin.h> of the headless APPLICATION build: the first header the reference includes
 * (Math.hpp), so it is the first-seen header of oracle/ref_app_standins/, the directory
 * layered in front of oracle/ref_standins/ for the two binaries that run the reference's
 * Renderer.hpp and Main.cpp against the drop-in shim (make -C oracle ref:
 * _ref/ref_dropin_main, _ref/ref_dropin_driver).  oracle/ref_standins/ and ref_harness are
 * untouched; this file ends by handing over to that directory's <intrin.h>.
 *
 * TEST INFRASTRUCTURE ONLY, our own text: it holds no line of the reference.  Each piece
 * of this directory, and why it cannot change a byte of g_data:
 *
 *   std headers first   ref_standins/intrin.h ends with `#define typename` and `#define
 *                       random ...`.  The shim (spt/RenderSegmentShim.hpp) and Renderer.hpp
 *                       include <mutex>, <atomic>, <condition_variable>, <iostream>,
 *                       <fstream> and <thread> after that: they are included here, before
 *                       the macros exist, so the macros never reach into libstdc++ (the
 *                       later #include lines are then no-ops).
 *   condition_variable  renamed by macro to a polling stand-in, as ref_standins/intrin.h
 *                       renames steady_clock.  RenderJob (Renderer.hpp:242-255) returns its
 *                       slot with an unlocked fetch_add followed by notify_one: the wake-up
 *                       can fall between the waiter's predicate check and its sleep, and
 *                       the final wait of RenderImageParallelMain then sleeps for ever.
 *                       The stand-in's wait(lock, pred) sleeps a millisecond with the lock
 *                       released and then checks pred, until pred holds; notify_one is
 *                       empty, so a RenderJob thread that outlives RenderImageParallelMain
 *                       touches nothing of its dead locals through it.  It sleeps BEFORE
 *                       the first check as well: a RenderJob thread takes its slot only
 *                       when it starts to run, so a check made in the microsecond after
 *                       the spawn can find every slot free while the newest tile has not
 *                       begun, and SaveImage would then run on an unfinished frame; the
 *                       millisecond lets the spawned thread take its slot first.  Both are
 *                       races of the calling pattern (tools/dropin_harness.cpp spells them
 *                       out), not of the code under test.  Waiting decides only WHEN the
 *                       main thread goes on; what a tile's RenderSegment call writes
 *                       does not depend on it.
 *   the clock           spt_ref_app_seed_clock() sets the reading of ref_standins' clock
 *                       from SPT_REF_CLOCK_SEED (32 bits, default 0); the glfwInit stand-in
 *                       calls it, which is before MainLoop's first draw constructs the main
 *                       thread's thread_local generator.  Only InitSpheres/GenerateSpheres
 *                       draw from it: the shim samples from its own keyed streams.
 *   the deadline        a safety net (SPT_REF_DEADLINE_S, default 120): once it has passed,
 *                       glfwWindowShouldClose and the polling wait print what happened and
 *                       _exit(3), without a destructor or another GPU call.
 *   GL.hpp              Renderer.hpp:9 spells it GL.hpp, the file is Gl.hpp (one file on a
 *                       case-insensitive file system): forwards to <Gl.hpp>.
 *   glbinding, GLFW     null: no window, no GL; see the two headers.  g_data is only ever
 *                       read by them (glTexImage2D ignores it).
 *   stb_image_write.h   stbi_write_bmp records its arguments and writes the bytes it was
 *                       handed, raw, to SPT_REF_DUMP.<call>: it reads g_data, never writes.
 */
#ifndef SPT_REF_APP_STANDIN_INTRIN_H
#define SPT_REF_APP_STANDIN_INTRIN_H

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <unistd.h>

namespace spt_ref_app {

inline const std::chrono::steady_clock::time_point started = std::chrono::steady_clock::now();
inline std::atomic<int> saved{0};  /* stbi_write_bmp calls so far */

inline double deadline_seconds()
{
    const char *s = std::getenv("SPT_REF_DEADLINE_S");
    const double v = s ? std::atof(s) : 0.0;
    return v > 0.0 ? v : 120.0;
}

/* the safety net: never returns once the deadline has passed */
inline void check_deadline(const char *where)
{
    static const double limit = deadline_seconds();
    const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - started).count();
    if (t <= limit) return;
    std::fprintf(stderr, "spt_ref_app: deadline of %.0f s passed in %s after %d saved frame(s); giving up\n", limit,
                 where, saved.load());
    std::fflush(stderr);
    _exit(3);
}

inline void sleep_ms() { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }

}  // namespace spt_ref_app

namespace std {
struct spt_ref_polling_cv {
    template <class Lock, class Pred> void wait(Lock &lock, Pred pred)
    {
        do {
            lock.unlock();
            spt_ref_app::sleep_ms();
            spt_ref_app::check_deadline("condition_variable::wait");
            lock.lock();
        } while (!pred());
    }
    void notify_one() noexcept {}
    void notify_all() noexcept {}
};
}  // namespace std

#include_next <intrin.h>

#define condition_variable spt_ref_polling_cv

/* after ref_standins/intrin.h: its clock's reading, set from the environment */
inline void spt_ref_app_seed_clock()
{
    const char *s = std::getenv("SPT_REF_CLOCK_SEED");
    spt_ref_clock_reading = static_cast<long long>(s ? static_cast<uint32_t>(std::strtoull(s, nullptr, 0)) : 0u);
}

#endif
