// Test hook of tests/test_gpu_normalize_guard.py: spt::normalize (spt_device.h) and the
// plain IEEE form it stands for, a / sqrtf(lensq(a)), one element per lane, so that the
// test decides which lanes share a wave (element i is lane i % 64 of wave i / 64; blocks
// are whole waves).  Built with the product's flags, which are part of what is tested.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spt_device.h"

using namespace spt;

namespace {

constexpr uint32_t kThreads = 256;

template <bool PLAIN>
__global__ __launch_bounds__(kThreads) void normalize_hook_kernel(const float *x, const float *y, const float *z, uint32_t n,
                                                                   uint32_t *out3)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const f3 a = mk(x[i], y[i], z[i]);
    f3 v;
    if (PLAIN) {
        const float l = __builtin_sqrtf(lensq(a));
        v = mk(a.x / l, a.y / l, a.z / l);
    } else {
        v = normalize(a);
    }
    out3[3 * i + 0] = __float_as_uint(v.x);
    out3[3 * i + 1] = __float_as_uint(v.y);
    out3[3 * i + 2] = __float_as_uint(v.z);
}

}  // namespace

// x, y, z: n floats; out3: 3 n words; plain != 0: the IEEE form.  Null stream.
extern "C" __attribute__((visibility("default"))) int spt_hook_normalize(const float *x, const float *y, const float *z,
                                                                        uint32_t n, uint32_t *out3, int plain)
{
    if (n == 0 || !x || !y || !z || !out3) return 1;
    const dim3 grid((n + kThreads - 1) / kThreads), block(kThreads);
    if (plain)
        hipLaunchKernelGGL(normalize_hook_kernel<true>, grid, block, 0, nullptr, x, y, z, n, out3);
    else
        hipLaunchKernelGGL(normalize_hook_kernel<false>, grid, block, 0, nullptr, x, y, z, n, out3);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}
