// spt_primcone.h -- the cone of a pixel block's primary rays and the candidate test of the
// primary-ray candidate lists (spt_accel.cpp "primary-ray candidate lists" has the proof),
// one definition for the host builder (build_prim_lists) and the device builder
// (spt_primlists.hip).  All fp64, contraction off: the host builder's tables are those of
// the functions as they stood in spt_accel.cpp, bit for bit; the device's differ from them
// only where its atan2 / asin round across a bound.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "spt_internal.h"

#pragma clang fp contract(off)

namespace spt {

struct PrimCone {
    double a[3];
    double theta, delta;
    bool ok;
};

constexpr double kPrimU = 1.0 / 16777216.0;  // 2^-24

// std::max / std::min as functions the device can call (the same operand order: a NaN
// second operand is dropped, as there)
__host__ __device__ inline double prim_max2(double a, double b) { return a < b ? b : a; }
__host__ __device__ inline double prim_min2(double a, double b) { return b < a ? b : a; }

__host__ __device__ inline double prim_norm3(const double v[3])
{
    return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}

// angle between unit a and v (any length), robust near 0 and pi
__host__ __device__ inline double prim_angle_to(const double a[3], const double v[3])
{
    const double cx = a[1] * v[2] - a[2] * v[1], cy = a[2] * v[0] - a[0] * v[2], cz = a[0] * v[1] - a[1] * v[0];
    const double s = std::sqrt(cx * cx + cy * cy + cz * cz), c = a[0] * v[0] + a[1] * v[1] + a[2] * v[2];
    return std::atan2(s, c);
}

struct PrimRange {
    double first, second;
};

// [lo, hi] widened by a relative and an absolute rounding allowance
__host__ __device__ inline PrimRange prim_widen(double lo, double hi, double rel, double abs_)
{
    const double m = prim_max2(std::fabs(lo), std::fabs(hi));
    return PrimRange{lo - m * rel - abs_, hi + m * rel + abs_};
}

// M (px, py, 1, 0) and the sum of the magnitudes of its terms
__host__ __device__ inline void prim_dir(const float *m, double px, double py, double out[3], double &mag)
{
    mag = 0;
    for (int r = 0; r < 3; ++r) {
        const double t0 = (double)m[4 * r] * px, t1 = (double)m[4 * r + 1] * py, t2 = (double)m[4 * r + 2];
        out[r] = t0 + t1 + t2;
        mag += std::fabs(t0) + std::fabs(t1) + std::fabs(t2);
    }
}

// Cone of the primary rays of pixel columns [x0, x1), rows [y0, y1).
__host__ __device__ inline PrimCone prim_cone(const Camera &cam, uint32_t W, uint32_t H, uint32_t x0, uint32_t x1,
                                              uint32_t y0, uint32_t y1)
{
    PrimCone pc{};
    // jittered row / column coordinates un = y + U, vn = x + U' (U in [-1, 1)), widened by
    // their fp rounding, then u = un / W, v = vn / H (correctly rounded), vy = -1 + 2u,
    // vx = -1 + 2v, each widened by its rounding
    const PrimRange un = prim_widen((double)y0 - 1.0, (double)y1, 4 * kPrimU, 1e-6);
    const PrimRange vn = prim_widen((double)x0 - 1.0, (double)x1, 4 * kPrimU, 1e-6);
    const PrimRange u = prim_widen(un.first / (double)W, un.second / (double)W, 4 * kPrimU, 1e-12);
    const PrimRange v = prim_widen(vn.first / (double)H, vn.second / (double)H, 4 * kPrimU, 1e-12);
    const PrimRange vy = prim_widen(-1.0 + 2.0 * u.first, -1.0 + 2.0 * u.second, 4 * kPrimU, 1e-7);
    const PrimRange vx = prim_widen(-1.0 + 2.0 * v.first, -1.0 + 2.0 * v.second, 4 * kPrimU, 1e-7);
    const float *m = cam.view;
    double c[3], cm;
    prim_dir(m, 0.5 * (vx.first + vx.second), 0.5 * (vy.first + vy.second), c, cm);
    const double cl = prim_norm3(c);
    if (!(cl > 0) || !std::isfinite(cl)) return pc;
    for (int k = 0; k < 3; ++k) pc.a[k] = c[k] / cl;
    double theta = 0, smax = cm, amin = 1e300;
    for (int k = 0; k < 4; ++k) {
        double d[3], dm;
        prim_dir(m, k & 1 ? vx.second : vx.first, k & 2 ? vy.second : vy.first, d, dm);
        const double along = pc.a[0] * d[0] + pc.a[1] * d[1] + pc.a[2] * d[2];
        if (!(along > 0) || !std::isfinite(along)) return pc;
        theta = prim_max2(theta, prim_angle_to(pc.a, d));
        smax = prim_max2(smax, dm);
        amin = prim_min2(amin, along);
    }
    if (!(theta < 0.5)) return pc;
    pc.theta = theta;
    pc.delta = 8 * kPrimU * smax / amin + 6 * kPrimU + 1e-6;
    pc.ok = std::isfinite(pc.delta) && pc.delta < 1e-3;
    return pc;
}

// Can a primary ray of cone pc pass the member test of slot s (eye e)?
__host__ __device__ inline bool prim_candidate(const PrimCone &pc, const float4 &sl, const double e[3])
{
    if (sl.w == -INFINITY) return false;  // dummy slot: never passes
    const double c[3] = {(double)sl.x - e[0], (double)sl.y - e[1], (double)sl.z - e[2]};
    const double L = prim_norm3(c), r2 = (double)sl.w;
    if (!std::isfinite(L) || !std::isfinite(r2)) return true;
    const double R = std::sqrt(prim_max2(r2 + 2.6e-6 * L * L, 0.0)) * 1.001 + 1e-4;
    if (!(L > R * 1.01 + 1e-3)) return true;
    const double alpha = std::asin(prim_min2(1.0, R / L));
    return prim_angle_to(pc.a, c) <= pc.theta + alpha + pc.delta + 1e-6;
}

}  // namespace spt
