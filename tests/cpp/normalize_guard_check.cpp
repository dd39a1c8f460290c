// Host check of Normalize's range guard (spt_device.h normalize_slow_mask): the one
// predicate that sends a lane down the short division-free path,
//     ok3(a) = min3(|x|, |y|, |z|) >= 2^-40 && max3(|x|, |y|, |z|) <= 2^40 && L <= 2^82,
//     L = (x*x + y*y) + z*z,
// must equal div_operand_ok(x) && div_operand_ok(y) && div_operand_ok(z) for every input.
// v_min3_f32 / v_max3_f32 return the minimum / maximum of the operands that are numbers
// (a NaN operand is dropped; all NaN gives NaN), so the two range compares alone pass a NaN
// component whose neighbours are in range: the L term is what rejects it.  The model is
// also run with a min3 / max3 that propagates NaN; the guard must not depend on which.
//
// Sweep 1: each component over every exponent field x mantissas {0, 1, 0x400000, 0x7FFFFE,
// 0x7FFFFF} x both signs, the other two components over in-range values.
// Sweep 2: all triples over an edge set: +-0, denormals, 2^-40 and 2^40 with their
// neighbours, FLT_MAX, inf, NaN, 1.
// Build with -ffp-contract=off (L's operation order is the device's).  Prints "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static float f32(uint32_t b)
{
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// spt_device.h div_operand_ok
static bool div_operand_ok(float x)
{
    const float ax = std::fabs(x);
    return ax >= 0x1p-40f && ax <= 0x1p40f;
}

// v_min3_f32 / v_max3_f32 on |operands|.  DROP: NaN operands are ignored (the instruction);
// otherwise any NaN operand gives NaN.
template <bool DROP>
static float min3(float a, float b, float c)
{
    if (DROP) return std::fmin(std::fmin(a, b), c);
    if (std::isnan(a) || std::isnan(b) || std::isnan(c)) return NAN;
    return std::fmin(std::fmin(a, b), c);
}
template <bool DROP>
static float max3(float a, float b, float c)
{
    if (DROP) return std::fmax(std::fmax(a, b), c);
    if (std::isnan(a) || std::isnan(b) || std::isnan(c)) return NAN;
    return std::fmax(std::fmax(a, b), c);
}

static float lensq(float x, float y, float z)
{
    const float xx = x * x, yy = y * y, zz = z * z;
    const float s = xx + yy;
    return s + zz;
}

// the guard as written: the slow mask is the union of three negated compares
template <bool DROP, bool WITH_L = true>
static bool short_ok(float x, float y, float z)
{
    const float lo = min3<DROP>(std::fabs(x), std::fabs(y), std::fabs(z));
    const float hi = max3<DROP>(std::fabs(x), std::fabs(y), std::fabs(z));
    const float L = lensq(x, y, z);
    const bool slow = !(lo >= 0x1p-40f) || !(hi <= 0x1p40f) || (WITH_L && !(L <= 0x1p82f));
    return !slow;
}

struct Tally {
    unsigned long long n = 0, ok = 0, nan_in_range = 0, two_compares_wrong = 0;
};

static bool check(float x, float y, float z, Tally &t)
{
    const bool want = div_operand_ok(x) && div_operand_ok(y) && div_operand_ok(z);
    const bool a = short_ok<true>(x, y, z), b = short_ok<false>(x, y, z);
    ++t.n;
    t.ok += want ? 1 : 0;
    if (short_ok<true, false>(x, y, z) != want) ++t.two_compares_wrong;
    if (a != want || b != want) {
        std::printf("guard differs at (%a, %a, %a): want %d, dropping min3 %d, propagating min3 %d\n", x, y, z, (int)want,
                    (int)a, (int)b);
        return false;
    }
    return true;
}

int main()
{
    Tally t;
    // sweep 1
    const uint32_t mant[5] = {0u, 1u, 0x400000u, 0x7FFFFEu, 0x7FFFFFu};
    const float in_range[5] = {0x1p-40f, 1.0f, 0x1p40f, 0x1.8p10f, -3.0f};
    for (int pos = 0; pos < 3; ++pos)
        for (uint32_t e = 0; e < 256u; ++e)
            for (uint32_t m : mant)
                for (uint32_t s = 0; s < 2u; ++s) {
                    const float v = f32((s << 31) | (e << 23) | m);
                    for (float p : in_range)
                        for (float q : in_range) {
                            const float c[3] = {pos == 0 ? v : p, pos == 1 ? v : (pos == 0 ? p : q), pos == 2 ? v : q};
                            if (!check(c[0], c[1], c[2], t)) return 1;
                        }
                }
    // sweep 2
    std::vector<float> edge;
    const uint32_t lo = 0x2B800000u, hi = 0x53800000u;  // 2^-40, 2^40
    if (f32(lo) != 0x1p-40f || f32(hi) != 0x1p40f) return 2;
    const uint32_t bits[] = {0u, 1u, 0x007FFFFFu, lo - 1u, lo, lo + 1u, hi - 1u, hi, hi + 1u,
                             0x7F7FFFFFu, 0x7F800000u, 0x7FC00000u, 0x7F800001u, 0x3F800000u};
    for (uint32_t b : bits) {
        edge.push_back(f32(b));
        edge.push_back(f32(b | 0x80000000u));
    }
    for (float x : edge)
        for (float y : edge)
            for (float z : edge) {
                if (std::isnan(x) && div_operand_ok(y) && div_operand_ok(z)) ++t.nan_in_range;
                if (!check(x, y, z, t)) return 1;
            }
    // liveness: both answers occur, a NaN beside in-range components is among the inputs,
    // and the two range compares alone get some input wrong (the NaN pitfall)
    if (t.ok == 0 || t.ok == t.n || t.nan_in_range == 0 || t.two_compares_wrong == 0) {
        std::printf("sweep too weak: %llu of %llu ok, %llu NaN cases, %llu told apart\n", t.ok, t.n, t.nan_in_range,
                    t.two_compares_wrong);
        return 3;
    }
    std::printf("ok\n");
    return 0;
}
