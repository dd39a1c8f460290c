// spt_mathsweep.hip -- test-only sweeps of the device's exact fp32 primitives
// (tests/test_gpu_math_sweep.py); built into simplepathtracer_amd/lib/libspt_mathsweep.so
// with the product's own flags, never linked into libspt_hip.so.
//
// The functions of spt_device.h, spt_powf.h and spt_decode.h are called unchanged, each
// from a kernel of its own, over whole input domains:
//   unary ops over consecutive uint32 input patterns [first, first + count), as raw result
//   bits (spt_sweep_dump) or as one 64-bit digest per block of 2^20 patterns
//   (spt_sweep_digest; oracle/spt_oracle.c's spo_math_digest is the same sum on the host);
//   division, Normalize and the fold's halvings elementwise over caller-supplied arrays.
// Return codes: 0 ok, 1 bad argument, 3 HIP error.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "spt_decode.h"
#include "spt_device.h"
#include "spt_path.h"

#pragma clang fp contract(off)

namespace {

using namespace spt;

// op codes: oracle/spt_oracle.h's SPO_MATH_* and tests/math_sweep.py's OPS
enum : int {
    OP_SQRT = 0,
    OP_SQRT_POS = 1,
    OP_SQRT_RAW = 2,
    OP_POW5 = 3,
    OP_UNI_M1_1 = 4,
    OP_UNI_H = 5,
    OP_UNI_0_1 = 6,
    OP_REFR_AG = 7,
    OP_REFR_GA = 8,
    OP_GAMMA = 9,
    OP_F2U8 = 10,
    OP_COUNT = 11,
};

constexpr uint32_t kBlockLog2 = 20;                  // patterns per digest
constexpr uint32_t kThreads = 256;                   // 4 waves
constexpr uint32_t kCanonNaN = 0x7FC00000u;

__device__ __forceinline__ uint32_t fbits(float r)
{
    return r != r ? kCanonNaN : __float_as_uint(r);
}

// the result bits of op on input pattern u: NaN results canonical, bytes zero-extended
template <int OP>
__device__ __forceinline__ uint32_t eval(uint32_t u)
{
    const float x = __uint_as_float(u);
    if constexpr (OP == OP_SQRT) return fbits(__builtin_sqrtf(x));
    if constexpr (OP == OP_SQRT_POS) return fbits(sqrt_pos_normal(x));
    if constexpr (OP == OP_SQRT_RAW) return fbits(__builtin_amdgcn_sqrtf(x));
    if constexpr (OP == OP_POW5) return fbits(pow5f(x));
    if constexpr (OP == OP_UNI_M1_1) return fbits(uniform_bits(u, -1.f, 1.f));
    if constexpr (OP == OP_UNI_H) return fbits(uniform_bits(u, -0.5f, 0.5f));
    if constexpr (OP == OP_UNI_0_1) return fbits(uniform_bits(u, 0.f, 1.f));
    if constexpr (OP == OP_REFR_AG) return fbits(no_tir(kAirToGlass, x) ? refract_k(kAirToGlass, x) : -1e30f);
    if constexpr (OP == OP_REFR_GA) return fbits(no_tir(kGlassToAir, x) ? refract_k(kGlassToAir, x) : -1e30f);
    if constexpr (OP == OP_GAMMA) return (uint32_t)gamma_byte(x);
    if constexpr (OP == OP_F2U8) return (uint32_t)f2u8(x);
    return 0u;
}

// One workgroup per block of 2^20 patterns: digest[blockIdx.x] = wrapping sum of
// fmix64(u << 32 | r).  Reduced in the wave, then in LDS; thread 0 stores.
template <int OP>
__global__ __launch_bounds__(kThreads) void digest_kernel(uint32_t first, uint64_t count, uint64_t *digest)
{
    __shared__ uint64_t part[kThreads / 64];
    const uint64_t base = (uint64_t)blockIdx.x << kBlockLog2;
    const uint64_t left = count - base;  // > 0: the grid is ceil(count / 2^20)
    const uint32_t n = left < (1ull << kBlockLog2) ? (uint32_t)left : (1u << kBlockLog2);
    uint64_t sum = 0;
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
        const uint32_t u = first + (uint32_t)base + i;  // wraps with the pattern
        sum += fmix64(((uint64_t)u << 32) | (uint64_t)eval<OP>(u));
    }
    for (int off = 32; off > 0; off >>= 1) sum += (uint64_t)__shfl_down((unsigned long long)sum, off, 64);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint64_t total = 0;
        for (uint32_t w = 0; w < kThreads / 64; ++w) total += part[w];
        digest[blockIdx.x] = total;
    }
}

template <int OP>
__global__ __launch_bounds__(kThreads) void dump_kernel(uint32_t first, uint64_t count, uint32_t *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += stride)
        out[i] = eval<OP>(first + (uint32_t)i);
}

uint32_t grid_for(uint64_t n)
{
    const uint64_t blocks = (n + kThreads - 1) / kThreads;
    return (uint32_t)(blocks < 4096 ? (blocks ? blocks : 1) : 4096);
}

template <int OP>
void launch_digest(uint32_t first, uint64_t count, uint64_t *digest, hipStream_t s)
{
    const uint32_t blocks = (uint32_t)((count + (1ull << kBlockLog2) - 1) >> kBlockLog2);
    hipLaunchKernelGGL(digest_kernel<OP>, dim3(blocks), dim3(kThreads), 0, s, first, count, digest);
}
template <int OP>
void launch_dump(uint32_t first, uint64_t count, uint32_t *out, hipStream_t s)
{
    hipLaunchKernelGGL(dump_kernel<OP>, dim3(grid_for(count)), dim3(kThreads), 0, s, first, count, out);
}

// a / b three ways: the gated division, the ungated core, and the unrefined reciprocal
__global__ __launch_bounds__(kThreads) void div_kernel(const float *a, const float *b, uint64_t n, uint32_t *out_rn,
                                                        uint32_t *out_core, uint32_t *out_raw)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const float x = a[i], y = b[i];
        out_rn[i] = __float_as_uint(div_rn(x, y));
        out_core[i] = __float_as_uint(div_core(x, recip(y)));
        out_raw[i] = __float_as_uint(x * __builtin_amdgcn_rcpf(y));
    }
}

__global__ __launch_bounds__(kThreads) void normalize_kernel(const float *x, const float *y, const float *z, uint64_t n,
                                                              uint32_t *out3)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const f3 v = normalize(mk(x[i], y[i], z[i]));
        out3[3 * i + 0] = __float_as_uint(v.x);
        out3[3 * i + 1] = __float_as_uint(v.y);
        out3[3 * i + 2] = __float_as_uint(v.z);
    }
}

__global__ __launch_bounds__(kThreads) void halve_kernel(const float *x, const uint32_t *j, uint64_t n, uint32_t *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride)
        out[i] = __float_as_uint(halve_n(x[i], j[i]));
}

int done() { return hipGetLastError() == hipSuccess ? 0 : 3; }

}  // namespace

#define SPT_SWEEP_API extern "C" __attribute__((visibility("default")))

#define SPT_SWEEP_DISPATCH(fn, ...)                         \
    switch (op) {                                           \
    case OP_SQRT: fn<OP_SQRT>(__VA_ARGS__); break;          \
    case OP_SQRT_POS: fn<OP_SQRT_POS>(__VA_ARGS__); break;  \
    case OP_SQRT_RAW: fn<OP_SQRT_RAW>(__VA_ARGS__); break;  \
    case OP_POW5: fn<OP_POW5>(__VA_ARGS__); break;          \
    case OP_UNI_M1_1: fn<OP_UNI_M1_1>(__VA_ARGS__); break;  \
    case OP_UNI_H: fn<OP_UNI_H>(__VA_ARGS__); break;        \
    case OP_UNI_0_1: fn<OP_UNI_0_1>(__VA_ARGS__); break;    \
    case OP_REFR_AG: fn<OP_REFR_AG>(__VA_ARGS__); break;    \
    case OP_REFR_GA: fn<OP_REFR_GA>(__VA_ARGS__); break;    \
    case OP_GAMMA: fn<OP_GAMMA>(__VA_ARGS__); break;        \
    case OP_F2U8: fn<OP_F2U8>(__VA_ARGS__); break;          \
    default: return 1;                                      \
    }

// d_digest: ceil(count / 2^20) words; count in 1 ... 2^32
SPT_SWEEP_API int spt_sweep_digest(int op, uint32_t first, uint64_t count, uint64_t *d_digest, void *stream)
{
    if (count == 0 || count > (1ull << 32) || !d_digest) return 1;
    SPT_SWEEP_DISPATCH(launch_digest, first, count, d_digest, (hipStream_t)stream)
    return done();
}

// d_out: count words, on the null stream
SPT_SWEEP_API int spt_sweep_dump(int op, uint32_t first, uint64_t count, uint32_t *d_out)
{
    if (count == 0 || count > (1ull << 32) || !d_out) return 1;
    SPT_SWEEP_DISPATCH(launch_dump, first, count, d_out, (hipStream_t) nullptr)
    return done();
}

// every array: n words (out3: 3 n), on the null stream
SPT_SWEEP_API int spt_sweep_div(const float *a, const float *b, uint64_t n, uint32_t *out_rn, uint32_t *out_core,
                                uint32_t *out_raw)
{
    if (n == 0 || !a || !b || !out_rn || !out_core || !out_raw) return 1;
    hipLaunchKernelGGL(div_kernel, dim3(grid_for(n)), dim3(kThreads), 0, nullptr, a, b, n, out_rn, out_core, out_raw);
    return done();
}

SPT_SWEEP_API int spt_sweep_normalize(const float *x, const float *y, const float *z, uint64_t n, uint32_t *out3)
{
    if (n == 0 || !x || !y || !z || !out3) return 1;
    hipLaunchKernelGGL(normalize_kernel, dim3(grid_for(n)), dim3(kThreads), 0, nullptr, x, y, z, n, out3);
    return done();
}

SPT_SWEEP_API int spt_sweep_halve(const float *x, const uint32_t *j, uint64_t n, uint32_t *out)
{
    if (n == 0 || !x || !j || !out) return 1;
    hipLaunchKernelGGL(halve_kernel, dim3(grid_for(n)), dim3(kThreads), 0, nullptr, x, j, n, out);
    return done();
}
