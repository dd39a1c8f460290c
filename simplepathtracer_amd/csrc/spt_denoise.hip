// spt_denoise.hip -- the edge-avoiding a-trous filter guided by the feature buffers:
// spt_denoise[_async] (spt_denoise.cpp; the definition is include/spt_hip.h "denoiser",
// DESIGN.md §4.11), and its variance-guided variant spt_denoise_var[_async] ("variance-guided
// denoiser").  Both are one level body, denoise_level<kVar>: what the
// variance-guided form adds stands under `if constexpr (kVar)`, and denoise_level_kernel and
// denoise_var_level_kernel are its two instantiations.
//
// One launch per level.  Level k has step s = 2^k, and the 25 taps of a pixel all lie on the
// lattice of pixels congruent to it modulo s in x and in y.  A block of 256 threads takes a
// 16x16 tile of one lattice (rx, ry): lattice cell (lx, ly) is pixel (rx + s * lx, ry + s *
// ly).  It stages the tile and its halo of two cells, 20x20 cells, in LDS once: the level's
// input u, the albedo, and {normal, z} with z = dep / cov (cov > 0, else +0) worked out as
// the cell is staged -- 400 x 48 B = 19 200 B at every level.  A cell outside the image has
// its flag (albedo's w lane) clear and the taps that meet it are skipped; its values are
// zeros that nothing reads into a sum.  Then every thread walks its 5x5 cells in the
// definition's order (rows outer, columns inner), fp32 without contraction, one IEEE
// division per tap, and stores its pixel.  Level 0 is the contiguous case (s = 1, one
// lattice).
//
// Blocks: per lattice ceil(Lx / 16) x ceil(Ly / 16) tiles where Lx = ceil(W / s) is the
// longest lattice's width (rx = 0); a shorter lattice's surplus tile holds no pixel and its
// block returns before the barrier.  Lattices with rx >= W or ry >= H do not exist and get
// no blocks.  The logical block order is rx fastest, then the tile column, then ry, then the
// tile row: neighbouring lattices read neighbouring 16-byte pixels of the same cache lines,
// so blocks that share lines are consecutive; and the hardware block index is dealt so
// that each of the eight XCDs (blockIdx % 8) gets one contiguous run of logical blocks and
// those lines meet in one L2.  Placement changes speed only.
//
// Lanes whose pixel lies past the image stage their share of the cells (a cell is staged by
// index, not by owner) but compute nothing and store nothing.
#include "spt_device.h"
#include "spt_internal.h"

namespace spt {

namespace {

constexpr uint32_t kTile = 16, kHalo = 2, kCells = kTile + 2 * kHalo;  // 20
constexpr uint32_t kDenoiseBlock = kTile * kTile;

// the logical block of hardware block b of n: XCD x = b % 8 owns a contiguous run
__device__ __forceinline__ uint32_t xcd_run_block(uint32_t b, uint32_t n)
{
    const uint32_t per = n >> 3, rem = n & 7u, x = b & 7u, j = b >> 3;
    const uint32_t first = x < rem ? x * (per + 1u) : rem * (per + 1u) + (x - rem) * per;
    return first + j;
}

// One level, both forms.  kVar, the variance-guided form (spt_denoise_var):
// g, the variance of the pixel mean, rides in s_u's w lane -- level 0 works it out as the
// cell is staged (mom.z / mom.w, as z), later levels find it in the plane the previous level
// wrote -- the colour term is divided by var_floor + (g_p + g_q), two IEEE divisions per tap,
// and the last level takes the output's w lane from the caller's rgba.
template <bool kVar>
__device__ __forceinline__ void denoise_level(const DenoiseArgs &a)
{
    __shared__ float4 s_u[kCells * kCells];  // u.rgb, w = the pixel's own w lane (kVar: g)
    __shared__ float4 s_a[kCells * kCells];  // alb.rgb, w = 1 inside the image, 0 outside
    __shared__ float4 s_n[kCells * kCells];  // nrm.xyz, z

    uint32_t l = xcd_run_block(blockIdx.x, gridDim.x);
    const uint32_t rx = l % a.sx;
    l /= a.sx;
    const uint32_t tx = l % a.tiles_x;
    l /= a.tiles_x;
    const uint32_t ry = l % a.sy, ty = l / a.sy;
    // cells of this block's lattice
    const uint32_t lw = (a.width - rx + a.step - 1u) / a.step, lh = (a.height - ry + a.step - 1u) / a.step;
    if (tx * kTile >= lw || ty * kTile >= lh) return;  // the whole block

    for (uint32_t c = threadIdx.x; c < kCells * kCells; c += kDenoiseBlock) {
        const uint32_t cy = c / kCells, cx = c - cy * kCells;
        // lattice cell, then pixel: 64-bit, a far halo cell of a wide level may pass 2^32
        const int64_t lx = (int64_t)(tx * kTile + cx) - kHalo, ly = (int64_t)(ty * kTile + cy) - kHalo;
        const int64_t x = (int64_t)rx + lx * (int64_t)a.step, y = (int64_t)ry + ly * (int64_t)a.step;
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f), al = u, nz = u;
        if (lx >= 0 && ly >= 0 && x < (int64_t)a.width && y < (int64_t)a.height) {
            const size_t p = (size_t)y * a.width + (size_t)x;
            u = a.in[p];
            if constexpr (kVar) {
                if (a.first) {
                    const float4 m = a.mom[p];
                    const float g = m.z / m.w;
                    u.w = __builtin_isfinite(g) ? g : __builtin_nanf("");  // +-inf would not make X NaN
                }
            }
            al = a.feat[2u * p];
            nz = a.feat[2u * p + 1u];
            const float cov = al.w;
            nz.w = cov > 0.0f ? nz.w / cov : 0.0f;
            al.w = 1.0f;
        }
        s_u[c] = u;
        s_a[c] = al;
        s_n[c] = nz;
    }
    __syncthreads();

    const uint32_t i = threadIdx.x & (kTile - 1u), j = threadIdx.x >> 4;
    const uint32_t lx = tx * kTile + i, ly = ty * kTile + j;
    if (lx >= lw || ly >= lh) return;  // past the image
    const uint32_t cc = (j + kHalo) * kCells + (i + kHalo);
    const float4 up = s_u[cc], ap = s_a[cc], np = s_n[cc];
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, ws = 0.0f;
    [[maybe_unused]] float gacc = 0.0f;
    const float h[3] = {0.375f, 0.25f, 0.0625f};
#pragma unroll
    for (int dj = -2; dj <= 2; ++dj) {
#pragma unroll
        for (int di = -2; di <= 2; ++di) {
            const uint32_t q = (uint32_t)((int)cc + dj * (int)kCells + di);
            const float4 uq = s_u[q], aq = s_a[q], nq = s_n[q];
            const float du_r = uq.x - up.x, du_g = uq.y - up.y, du_b = uq.z - up.z;
            const float dc = (du_r * du_r + du_g * du_g) + du_b * du_b;
            const float da_r = aq.x - ap.x, da_g = aq.y - ap.y, da_b = aq.z - ap.z;
            const float d_a = (da_r * da_r + da_g * da_g) + da_b * da_b;
            const float dn_x = nq.x - np.x, dn_y = nq.y - np.y, dn_z = nq.z - np.z;
            const float d_n = (dn_x * dn_x + dn_y * dn_y) + dn_z * dn_z;
            const float dz = nq.w - np.w;
            const float d_z = dz * dz;
            float tc = dc * a.kc;
            if constexpr (kVar) {
                const float vn = a.var_floor + (up.w + uq.w);
                tc = tc / vn;
            }
            const float X = (tc + d_a * a.ka) + (d_n * a.kn + d_z * a.kz);
            const float w = (h[di < 0 ? -di : di] * h[dj < 0 ? -dj : dj]) / (1.0f + X);
            // a cell outside the image, a NaN and a zero weight all skip the tap
            if (aq.w != 0.0f && w > 0.0f) {
                acc_r = acc_r + w * uq.x;
                acc_g = acc_g + w * uq.y;
                acc_b = acc_b + w * uq.z;
                ws = ws + w;
                if constexpr (kVar) gacc = gacc + (w * w) * uq.w;
            }
        }
    }
    float4 o = up;  // no weight at all: the pixel (kVar: and g) passes through, bits and all
    if (ws > 0.0f) {
        o.x = acc_r / ws;
        o.y = acc_g / ws;
        o.z = acc_b / ws;
        if constexpr (kVar) o.w = gacc / (ws * ws);
    }
    const uint32_t x = rx + a.step * lx, y = ry + a.step * ly;
    const size_t p = (size_t)y * a.width + x;
    if constexpr (kVar) {
        if (a.rgba) {  // the last level
            if (a.out_var) a.out_var[p] = o.w;
            o.w = a.rgba[p].w;
        }
    }
    if (a.out) a.out[p] = o;
    if (a.rgb8) {
        // io::WritePixel's place in a g_data frame of the image's own size
        uint8_t *g = a.rgb8 + (size_t)3 * ((size_t)(a.height - 1u - y) * a.width + x);
        g[0] = gamma_byte(o.x);
        g[1] = gamma_byte(o.y);
        g[2] = gamma_byte(o.z);
    }
}

}  // namespace

// the two forms under the names that profiles and DESIGN.md §4.11 / §4.12 use
__global__ __launch_bounds__(kDenoiseBlock) void denoise_level_kernel(DenoiseArgs a) { denoise_level<false>(a); }
__global__ __launch_bounds__(kDenoiseBlock) void denoise_var_level_kernel(DenoiseArgs a) { denoise_level<true>(a); }

hipError_t launch_denoise_level(const DenoiseArgs &a, bool var, hipStream_t s)
{
    const uint64_t blocks = (uint64_t)a.sx * a.tiles_x * a.sy * a.tiles_y;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(var ? denoise_var_level_kernel : denoise_level_kernel, dim3((uint32_t)blocks), dim3(kDenoiseBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace spt
