// temporal.hip — spt_temporal_accumulate's kernel: one thread per pixel of the
// new history, the arithmetic of temporal.h.  Its own namespace: the kernels of
// namespace spt are the render's.
#include "temporal.h"

namespace spt_temporal {

// 32 x 8 pixel blocks like denoise_kernel: a thread's own planes are read and
// written coalesced, and the four taps of neighbouring pixels land in the same
// few cache lines of the previous frame's planes wherever the motion is smooth.
__global__ __launch_bounds__(256) void temporal_kernel(TemporalArgs a) {
    const uint32_t x = blockIdx.x * 32u + (threadIdx.x & 31u);
    const uint32_t y = blockIdx.y * 8u + (threadIdx.x >> 5);
    if (x >= a.width || y >= a.height) return;
    temporal_store(a, x, y, temporal_pixel(a, x, y));
}

hipError_t launch_temporal(const TemporalArgs& a, hipStream_t s) {
    if (a.width == 0 || a.height == 0) return hipSuccess;
    const dim3 g((a.width + 31u) / 32u, (a.height + 7u) / 8u), b(256);
    hipLaunchKernelGGL(temporal_kernel, g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace spt_temporal
