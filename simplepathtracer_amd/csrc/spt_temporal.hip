// spt_temporal.hip -- temporal accumulation: the last frame's colour and luminance moments
// reprojected into this frame and blended with it, spt_temporal[_async] (spt_temporal.cpp;
// the definition is include/spt_hip.h "temporal accumulation").
//
// One launch, one lane per pixel, no LDS.  A block of 256 threads takes a 32x8 pixel tile:
// a wave is two rows of 32 pixels, so its current-frame loads are whole 512-byte runs of a
// row, and under a small camera motion its lanes' four taps fall in the same few lines of
// the history.  Every load and store of a colour, a moment or a feature half is 16 bytes.
//
// A lane loads its own pixel (rgba, mom, the two halves of feat, ids) first, reprojects its
// hit point (or, on the sky, its direction) through the previous camera while those loads are
// in flight, and then visits the four taps in stages, each stage's loads issued together
// before any is used and only for the taps still alive: the ids (4 bytes), then the moments,
// then the features, then the colour.  A tap that fails a cheap test never loads the rest.
//
// Arithmetic: fp32 without contraction in the definition's order; normalize and div_rn
// (spt_device.h) and __builtin_sqrtf are the IEEE operations the render uses.
// Lanes whose pixel lies past the image do nothing.
//
// The motion variant (kMotion; spt_temporal_motion[_async]) is the same body
// with one more gather: the lane's own ids word is loaded with the pixel, and its sphere's
// 32-byte record {C, r, Cp, rp} with two 16-byte loads right behind it, predicated on
// id < n_spheres, so they are in flight during the reprojection arithmetic.  ids is coherent
// within a tile and the table is a few KB, so the gather stays in cache.  A moved sphere's
// hit point is carried back, Pp = Cp + (P - C) * (rp / r), before it is reprojected; every
// other pixel takes the plain path, bits and all, and the static rule holds per pixel.
#include "spt_device.h"
#include "spt_internal.h"

namespace spt {

namespace {

constexpr uint32_t kTemporalTileX = 32, kTemporalTileY = 8;
constexpr uint32_t kTemporalBlock = kTemporalTileX * kTemporalTileY;

__device__ __forceinline__ bool finite3(float a, float b, float c)
{
    return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c);
}
__device__ __forceinline__ bool finite4(const float4 &v) { return finite3(v.x, v.y, v.z) && __builtin_isfinite(v.w); }

}  // namespace

template <bool kMotion>
__global__ __launch_bounds__(kTemporalBlock) void temporal_kernel(TemporalArgs a)
{
    const uint32_t by = blockIdx.x / a.tiles_x, bx = blockIdx.x - by * a.tiles_x;
    const uint32_t x = bx * kTemporalTileX + (threadIdx.x & (kTemporalTileX - 1u));
    const uint32_t y = by * kTemporalTileY + threadIdx.x / kTemporalTileX;
    if (x >= a.width || y >= a.height) return;  // past the image
    const size_t p = (size_t)y * a.width + x;
    const float4 c = a.rgba[p], m = a.mom[p], f0 = a.feat[2u * p], f1 = a.feat[2u * p + 1u];
    float4 oc = c, om = m;  // no history: the pixel passes through, bits and all
    uint32_t own_id = 0;
    float4 rec0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rec1 = rec0;  // an id outside the table: unmoved
    bool in_table = false;
    if constexpr (kMotion) {
        own_id = a.ids[p];
        in_table = own_id < a.n_spheres;  // the miss sentinel or garbage: nothing is read
        if (in_table) {
            rec0 = a.motion[2u * (size_t)own_id];
            rec1 = a.motion[2u * (size_t)own_id + 1u];
        }
    }
    if (a.h_rgba && finite3(c.x, c.y, c.z) && finite4(m) && finite4(f0) && finite4(f1) && m.w > 0.0f) {
        const uint32_t id = kMotion ? own_id : a.ids[p];
        const bool hit = f0.w > 0.0f;
        const float z = hit ? div_rn(f1.w, f0.w) : 0.0f;
        // the render's own quirk: x over the height, y over the width
        const float vx = -1.0f + 2.0f * div_rn((float)x, a.fh);
        const float vy = -1.0f + 2.0f * div_rn((float)y, a.fw);
        const f3 r = mk((a.m[0] * vx + a.m[1] * vy) + a.m[2], (a.m[3] * vx + a.m[4] * vy) + a.m[5],
                        (a.m[6] * vx + a.m[7] * vy) + a.m[8]);
        const f3 d = normalize(r);
        f3 w = d;  // the sky: a point at infinity, it follows the rotation only
        float L = 0.0f;
        bool mv = false, seek = true;
        if (hit) {
            const f3 P = add(mk(a.e[0], a.e[1], a.e[2]), mul(d, z));
            f3 from = P;
            if constexpr (kMotion) {
                mv = in_table && !(rec0.x == rec1.x && rec0.y == rec1.y && rec0.z == rec1.z && rec0.w == rec1.w);
                if (mv) {  // the sphere's own frame: the point keeps its place on the sphere
                    const float sc = div_rn(rec1.w, rec0.w);
                    const f3 u = sub(P, mk(rec0.x, rec0.y, rec0.z));
                    from = add(mk(rec1.x, rec1.y, rec1.z), mul(u, sc));
                    seek = finite3(from.x, from.y, from.z);
                }
            }
            w = sub(from, mk(a.ep[0], a.ep[1], a.ep[2]));
            L = __builtin_sqrtf(lensq(w));
        }
        const float qx = (a.minv[0] * w.x + a.minv[1] * w.y) + a.minv[2] * w.z;
        const float qy = (a.minv[3] * w.x + a.minv[4] * w.y) + a.minv[5] * w.z;
        const float qz = (a.minv[6] * w.x + a.minv[7] * w.y) + a.minv[8] * w.z;
        float fx = ((div_rn(qx, qz) + 1.0f) * 0.5f) * a.fh;
        float fy = ((div_rn(qy, qz) + 1.0f) * 0.5f) * a.fw;
        bool front = qz > 0.0f;
        if (a.is_static && !mv) {  // the same camera, the same sphere: the pixel's own place, exactly
            fx = (float)x;
            fy = (float)y;
            front = true;
        }
        if (seek && front && fx > -1.0f && fx < a.fw && fy > -1.0f && fy < a.fh) {  // NaN fails
            const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
            const float tx = fx - x0f, ty = fy - y0f;
            const int x0 = (int)x0f, y0 = (int)y0f;  // -1 .. width - 1, -1 .. height - 1
            float wt[4];
            bool ok[4];
            size_t t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // j outer, i inner
                const int i = k & 1, j = k >> 1;
                const int xi = x0 + i, yj = y0 + j;
                wt[k] = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                ok[k] = xi >= 0 && xi < (int)a.width && yj >= 0 && yj < (int)a.height && wt[k] > 0.0f;
                t[k] = ok[k] ? (size_t)yj * a.width + (size_t)xi : p;  // a dead tap reads nothing new
            }
            // the ids, then the moments: the cheap tests
            uint32_t hid[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) hid[k] = a.h_ids[t[k]];
#pragma unroll
            for (int k = 0; k < 4; ++k) ok[k] = ok[k] && hid[k] == id;
            float4 hm[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) hm[k] = a.h_mom[t[k]];
#pragma unroll
            for (int k = 0; k < 4; ++k) ok[k] = ok[k] && hm[k].w > 0.0f && finite3(hm[k].x, hm[k].y, hm[k].w);
            // the features: normal and depth
            float4 h0[4], h1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) {
                    h0[k] = a.h_feat[2u * t[k]];
                    h1[k] = a.h_feat[2u * t[k] + 1u];
                }
            const bool any_normal = a.tol_normal == __builtin_inff(), any_depth = !hit || a.tol_depth == __builtin_inff();
            const float lim = a.tol_depth * L, lim2 = lim * lim;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) {
                    const float dnx = h1[k].x - f1.x, dny = h1[k].y - f1.y, dnz = h1[k].z - f1.z;
                    const float dn = (dnx * dnx + dny * dny) + dnz * dnz;
                    const float zq = h0[k].w > 0.0f ? div_rn(h1[k].w, h0[k].w) : 0.0f;
                    const float dz = zq - L;
                    ok[k] = (any_normal || dn <= a.tol_normal) && (any_depth || dz * dz <= lim2);
                }
            // the colour
            float4 hc[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) hc[k] = a.h_rgba[t[k]];
            float ws = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, h1s = 0.0f, h2s = 0.0f, hn = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k] && finite3(hc[k].x, hc[k].y, hc[k].z)) {
                    ws = ws + wt[k];
                    ar = ar + wt[k] * hc[k].x;
                    ag = ag + wt[k] * hc[k].y;
                    ab = ab + wt[k] * hc[k].z;
                    h1s = h1s + wt[k] * hm[k].x;
                    h2s = h2s + wt[k] * hm[k].y;
                    hn = hn + wt[k] * hm[k].w;
                }
            if (ws > 0.0f) {
                ar = ar / ws;
                ag = ag / ws;
                ab = ab / ws;
                h1s = h1s / ws;
                h2s = h2s / ws;
                const float nh = __builtin_fminf(hn / ws, a.max_history);
                const float nc = m.w;
                const float nn = nh + nc;
                const float alpha = nc / nn;
                oc.x = ar + (c.x - ar) * alpha;
                oc.y = ag + (c.y - ag) * alpha;
                oc.z = ab + (c.z - ab) * alpha;
                const float m1 = h1s + (m.x - h1s) * alpha;
                const float m2 = h2s + (m.y - h2s) * alpha;
                const float dd = m2 - m1 * m1;
                om = make_float4(m1, m2, dd < 0.0f ? 0.0f : dd, nn);
            }
        }
    }
    a.out_rgba[p] = oc;
    a.out_mom[p] = om;
}

hipError_t launch_temporal(TemporalArgs a, bool motion, hipStream_t s)
{
    a.tiles_x = (a.width + kTemporalTileX - 1u) / kTemporalTileX;
    const uint64_t blocks = (uint64_t)a.tiles_x * ((a.height + kTemporalTileY - 1u) / kTemporalTileY);
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (motion)
        hipLaunchKernelGGL(temporal_kernel<true>, dim3((uint32_t)blocks), dim3(kTemporalBlock), 0, s, a);
    else
        hipLaunchKernelGGL(temporal_kernel<false>, dim3((uint32_t)blocks), dim3(kTemporalBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace spt
