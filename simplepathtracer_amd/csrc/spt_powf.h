// spt_powf.h -- powf(float, float) exactly as this image's glibc (2.35) computes it.
//
// Why: the reference's `pow(1.f - c, 5.f)` and `pow(-0.2f, 2.f)`
// (SingleThreadPathTracer.hpp:58-59,75-76; TaskBasedPathTracer.hpp:137-138,155-156)
// bind to std::pow(float, float) -- IOHelpers.hpp:5-9 pulls in the stb
// implementations, whose <math.h>/<stdlib.h> are libstdc++'s wrappers
// (`using std::pow; using std::sqrt; using std::abs;`), and they come before
// SingleThreadPathTracer.hpp in Renderer.hpp:4-8 (oracle/probe_overloads.cpp
// shows the resolution).  std::pow(float, float) is __builtin_powf, i.e. glibc's
// powf, which is NOT correctly rounded: its double-precision core is accurate to
// ~2^-34 only, so x^5 correctly rounded differs from it on 0.07% of inputs.
//
// This restates glibc's algorithm (sysdeps/ieee754/flt-32/e_powf.c, the ARM
// optimized-routines powf: 16-entry log2 table + order-5 polynomial, 32-entry
// exp2 table + order-3 polynomial, POWF_SCALE_BITS = 0, no toint intrinsics) as
// the x86-64 build selects it on AVX2+FMA hosts (the __powf_fma ifunc: every
// `a * b + c` of the C source contracted to one fma).  Pinned exhaustively: equal
// bit for bit to the host's powf(x, 5.f) for all 2^32 - 2^24 non-NaN floats x,
// and for (+-0.2f, 2.f) (tests/test_oracle_kat.py::test_powf_restatement_*).  On
// a host without FMA glibc takes the non-FMA variant, which differs on 6 of those
// inputs (x = +-0x1.14708ep-1, +-0x1.ef5ee8p-1, +-0x1.14708ep+0).
//
// exp2 table: tab[i] = bits(2^(i/32) rounded to double) - (i << 47), derived
// exactly (tools/derive_exp2_table.py); log2 table and the polynomials are the
// published constants of the algorithm.
//
// Provenance and license: the algorithm, its log2 table (powf_log2_data.c) and
// polynomial coefficients come from ARM's Optimized Routines
// (github.com/ARM-software/optimized-routines, math/powf.c, Szabolcs Nagy, 2017-2018),
// contributed to glibc 2.28 as sysdeps/ieee754/flt-32/e_powf.c and e_powf_data.c.
// Optimized Routines is released under "MIT OR Apache-2.0 WITH LLVM-exception"
// (SPDX), glibc under LGPL-2.1-or-later; this restatement follows the MIT-licensed
// upstream: Copyright (c) 2017-2018 Arm Limited.  Permission is hereby granted, free
// of charge, to any person obtaining a copy of this software to deal in it without
// restriction, subject to including this notice; the software is provided "as is",
// without warranty of any kind.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SPT_POWF_HD __host__ __device__
#else
#define SPT_POWF_HD
#endif

namespace spt_powf_detail {

struct Log2Entry {
    double invc, logc;
};

// __powf_log2_data.tab: invc ~ 1/c for the subinterval centre c, logc = log2(c)
static constexpr Log2Entry kLog2Tab[16] = {
    {0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2}, {0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2},
    {0x1.49539f0f010bp+0, -0x1.7418b0a1fb77bp-2},  {0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2},
    {0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2}, {0x1.25e227b0b8eap+0, -0x1.97c1d1b3b7afp-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3}, {0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4},
    {0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4},  {0x1.ca4b31f026aap-1, 0x1.476a9543891bap-3},
    {0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2},
    {0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2},  {0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2},
};
// __powf_log2_data.poly: log1p(r)/ln2 ~ A0 r^5 + A1 r^4 + A2 r^3 + A3 r^2 + A4 r
static constexpr double kLog2Poly[5] = {0x1.27616c9496e0bp-2, -0x1.71969a075c67ap-2, 0x1.ec70a6ca7baddp-2,
                                        -0x1.7154748bef6c8p-1, 0x1.71547652ab82bp0};
// __exp2f_data.tab
static constexpr uint64_t kExp2Tab[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
    0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
    0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
    0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
    0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
    0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
    0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull,
};
// __exp2f_data.poly: 2^r ~ C0 r^3 + C1 r^2 + C2 r + 1 on |r| <= 1/64
static constexpr double kExp2Poly[3] = {0x1.c6af84b912394p-5, 0x1.ebfce50fac4f3p-3, 0x1.62e42ff0c52d6p-1};

SPT_POWF_HD inline uint32_t f2u(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
SPT_POWF_HD inline float u2f(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}
SPT_POWF_HD inline uint64_t d2u(double f)
{
    uint64_t u;
    memcpy(&u, &f, 8);
    return u;
}
SPT_POWF_HD inline double u2d(uint64_t u)
{
    double f;
    memcpy(&f, &u, 8);
    return f;
}

// 0: not an integer, 1: odd integer, 2: even integer (e_powf.c checkint)
SPT_POWF_HD inline int checkint(uint32_t iy)
{
    const int e = (int)(iy >> 23 & 0xff);
    if (e < 0x7f) return 0;
    if (e > 0x7f + 23) return 2;
    if (iy & ((1u << (0x7f + 23 - e)) - 1)) return 0;
    if (iy & (1u << (0x7f + 23 - e))) return 1;
    return 2;
}
SPT_POWF_HD inline bool zeroinfnan(uint32_t ix) { return 2u * ix - 1u >= 2u * 0x7f800000u - 1u; }

// A polynomial coefficient formed where it is used.  In a kernel the compiler otherwise
// hoists the coefficients that are fma addends into vector registers for the kernel's
// whole lifetime and then spills them to scratch; two scalar moves it may not move
// keep them out of both.  Same value on the host.
#if defined(__HIP_DEVICE_COMPILE__)
template <uint64_t BITS>
__device__ __forceinline__ double lit_bits()
{
    uint32_t lo, hi;
    asm volatile("s_mov_b32 %0, %2\n\ts_mov_b32 %1, %3"
                 : "=s"(lo), "=s"(hi)
                 : "i"((uint32_t)BITS), "i"((uint32_t)(BITS >> 32)));
    return u2d(((uint64_t)hi << 32) | lo);
}
#define SPT_POWF_LIT(c) (::spt_powf_detail::lit_bits<__builtin_bit_cast(uint64_t, (double)(c))>())
#else
#define SPT_POWF_LIT(c) (c)
#endif

}  // namespace spt_powf_detail

// powf(x, y) of glibc 2.35 (FMA variant) for finite nonzero y and any x; the
// y = 0 / inf / NaN cases (never reached: the reference's exponents are the
// constants 5 and 2) return NaN here instead of glibc's special values.
SPT_POWF_HD inline float spt_glibc_powf(float x, float y)
{
    using namespace spt_powf_detail;
    uint32_t sign_bias = 0;
    uint32_t ix = f2u(x);
    const uint32_t iy = f2u(y);
    if (zeroinfnan(iy)) return __builtin_nanf("");
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
        // x < 0x1p-126, or inf, or NaN
        if (zeroinfnan(ix)) {
            float x2 = x * x;
            if ((ix & 0x80000000u) && checkint(iy) == 1) x2 = -x2;
            return (iy & 0x80000000u) ? 1.0f / x2 : x2;
        }
        if (ix & 0x80000000u) {
            const int yint = checkint(iy);
            if (yint == 0) return __builtin_nanf("");
            if (yint == 1) sign_bias = 1u << (5 + 11);
            ix &= 0x7fffffffu;
        }
        if (ix < 0x00800000u) {  // subnormal: normalise
            ix = f2u(u2f(ix) * 0x1p23f);
            ix &= 0x7fffffffu;
            ix -= 23u << 23;
        }
    }
    // log2_inline: x = 2^k z, z in [OFF, 2 OFF], log2(x) = log1p(z/c - 1)/ln2 + log2(c) + k
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (int)((tmp >> 19) % 16);
    const uint32_t top = tmp & 0xff800000u;
    const uint32_t iz = ix - top;
    const int k = (int32_t)top >> 23;
    const double invc = kLog2Tab[i].invc, logc = kLog2Tab[i].logc;
    const double z = (double)u2f(iz);
    const double r = __builtin_fma(z, invc, -1.0);
    const double y0 = logc + (double)k;
    const double r2 = r * r;
    double yy = __builtin_fma(kLog2Poly[0], r, SPT_POWF_LIT(kLog2Poly[1]));
    const double p = __builtin_fma(kLog2Poly[2], r, SPT_POWF_LIT(kLog2Poly[3]));
    const double r4 = r2 * r2;
    double q = __builtin_fma(kLog2Poly[4], r, y0);
    q = __builtin_fma(p, r2, q);
    yy = __builtin_fma(yy, r4, q);
    const double ylogx = (double)y * yy;
    if (((d2u(ylogx) >> 47) & 0xffff) >= (d2u(126.0) >> 47)) {
        // |y log2 x| >= 126
        if (ylogx > 0x1.fffffffd1d571p+6) return sign_bias ? -__builtin_inff() : __builtin_inff();
        if (ylogx <= -150.0) return sign_bias ? -0.0f : 0.0f;
    }
    // exp2_inline: x = k/32 + r, r in [-1/64, 1/64]
    const double shift = 0x1.8p+52 / 32;
    double kd = ylogx + shift;
    const uint64_t ki = d2u(kd);
    kd -= shift;
    const double rr = ylogx - kd;
    uint64_t t = kExp2Tab[ki % 32];
    const uint64_t ski = ki + sign_bias;
    t += ski << (52 - 5);
    const double s = u2d(t);
    const double zz = __builtin_fma(kExp2Poly[0], rr, SPT_POWF_LIT(kExp2Poly[1]));
    const double rr2 = rr * rr;
    double e = __builtin_fma(kExp2Poly[2], rr, 1.0);
    e = __builtin_fma(zz, rr2, e);
    e = e * s;
    return (float)e;
}
