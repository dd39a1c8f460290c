/*
 * <intrin.h> stand-in: lets the reference's MSVC-only headers compile with g++ so that
 * oracle/ref_harness.cpp can call the reference's own functions (make -C oracle ref).
 *
 * TEST INFRASTRUCTURE ONLY, our own text: it holds no line of the reference.  It is the
 * first header the reference includes (Math.hpp), so everything below is in place before
 * any of the reference's code is seen.  Each piece, and why it cannot change a result:
 *
 *   std headers first   every std header the reference or the harness uses is included
 *                       here, before the macros below exist: the macros never reach into
 *                       libstdc++ (the reference's own #include lines are then no-ops).
 *                       <math.h> is not among them: that pow/sqrt/abs on floats find the
 *                       float overloads in the tracers is the stb headers' doing
 *                       (stb_image*.h beside this file keep their <stdlib.h> and
 *                       <math.h>, tests/test_oracle_kat.py::test_overload_probe).
 *   union __m128        MSVC's __m128 is a 16-byte-aligned union with an m128_f32[4]
 *                       member, which Math.hpp reads (Mat4::operator*) and which the
 *                       reference's {x, y, z} initialisers fill (missing lanes zero);
 *                       gcc's is an opaque vector.  The union here has that float array
 *                       first and gcc's vector second (same 16 bytes, same alignment).
 *   _mm_* macros        each names a one-line wrapper that unwraps the union, executes
 *                       the real intrinsic of <smmintrin.h> / <pmmintrin.h> on the vector
 *                       and wraps the result: the instruction, its operand order and its
 *                       immediate are the reference's.
 *   __forceinline       an MSVC inlining hint; inlining does not change IEEE results
 *                       (the build uses -ffp-contract=off, no fast-math).
 *   std::sqrtf          MSVC's <cmath> declares it, libstdc++ 11 does not: a
 *                       using-declaration of the C library's sqrtf (correctly rounded).
 *   random              glibc's <stdlib.h> declares ::random(), which clashes with the
 *                       reference's `namespace random`: a rename of the identifier.
 *   typename            the reference writes `template <typename uint8_t D>`, which MSVC
 *                       reads as `template <uint8_t D>`; dropping the keyword gives g++
 *                       the same declaration.  The reference has no other use of it.
 *   steady_clock        the reference seeds each thread's generator from
 *                       steady_clock::now() (Random.hpp).  The rename points it at a
 *                       clock whose reading the harness sets, so that a fresh thread's
 *                       stream starts from a chosen 32-bit seed: the one seam of the
 *                       comparison (tests/test_reference_parity.py, the seam test).  The
 *                       reading goes through the reference's own static_cast and splitmix
 *                       constructor.
 */
#ifndef SPT_REF_STANDIN_INTRIN_H
#define SPT_REF_STANDIN_INTRIN_H

/* gcc's vector type under another name, before libstdc++ (whose <random> includes the SSE
 * headers) can define it as __m128 */
#define __m128 spt_ref_native_m128
#include <smmintrin.h>
#undef __m128

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

union __m128 {
    float m128_f32[4];
    spt_ref_native_m128 v;
};

#define SPT_REF_WRAP2(name)                                        \
    static inline __m128 spt_ref##name(__m128 a, __m128 b)         \
    {                                                              \
        __m128 r;                                                  \
        r.v = name(a.v, b.v);                                      \
        return r;                                                  \
    }
SPT_REF_WRAP2(_mm_add_ps)
SPT_REF_WRAP2(_mm_sub_ps)
SPT_REF_WRAP2(_mm_mul_ps)
SPT_REF_WRAP2(_mm_div_ps)
SPT_REF_WRAP2(_mm_xor_ps)
SPT_REF_WRAP2(_mm_hadd_ps)
#undef SPT_REF_WRAP2

static inline __m128 spt_ref_mm_sqrt_ps(__m128 a) { __m128 r; r.v = _mm_sqrt_ps(a.v); return r; }
static inline __m128 spt_ref_mm_set1_ps(float s) { __m128 r; r.v = _mm_set1_ps(s); return r; }
static inline __m128 spt_ref_mm_set_ps1(float s) { __m128 r; r.v = _mm_set_ps1(s); return r; }
static inline __m128 spt_ref_mm_load_ps(const float *p) { __m128 r; r.v = _mm_load_ps(p); return r; }
static inline void spt_ref_mm_store_ps(float *p, __m128 a) { _mm_store_ps(p, a.v); }
static inline void spt_ref_mm_store_ss(float *p, __m128 a) { _mm_store_ss(p, a.v); }
template <int M> static inline __m128 spt_ref_mm_dp_ps(__m128 a, __m128 b) { __m128 r; r.v = _mm_dp_ps(a.v, b.v, M); return r; }

#undef _mm_dp_ps
#define _mm_add_ps spt_ref_mm_add_ps
#define _mm_sub_ps spt_ref_mm_sub_ps
#define _mm_mul_ps spt_ref_mm_mul_ps
#define _mm_div_ps spt_ref_mm_div_ps
#define _mm_xor_ps spt_ref_mm_xor_ps
#define _mm_hadd_ps spt_ref_mm_hadd_ps
#define _mm_sqrt_ps spt_ref_mm_sqrt_ps
#define _mm_set1_ps spt_ref_mm_set1_ps
#define _mm_set_ps1 spt_ref_mm_set_ps1
#define _mm_load_ps spt_ref_mm_load_ps
#define _mm_store_ps spt_ref_mm_store_ps
#define _mm_store_ss spt_ref_mm_store_ss
#define _mm_dp_ps(a, b, m) spt_ref_mm_dp_ps<(m)>((a), (b))

#define __forceinline

namespace std { using ::sqrtf; }

/* the reading of the reference's clock: the harness sets it before it starts a thread */
inline long long spt_ref_clock_reading = 0;
namespace std { namespace chrono {
struct spt_ref_clock {
    struct duration { long long ticks; long long count() const { return ticks; } };
    struct time_point { duration since; duration time_since_epoch() const { return since; } };
    static time_point now() { return time_point{duration{spt_ref_clock_reading}}; }
};
} }

#define random spt_ref_random
#define steady_clock spt_ref_clock
#define typename

#endif
