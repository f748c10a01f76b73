// adapt.hip — spt_adapt_select's kernels: which pixels of an accumulation
// still need samples (include/spt.h), compacted in ascending order.  Not in
// the reference (it renders a fixed spp, main.cpp:385-429).
//
// An ordered stream compaction in three launches, one pixel per lane:
//   1. adapt_count_kernel   the predicate from coalesced plane reads; a wave's
//                           ballot to masks[], the block's total (its four
//                           waves' popcounts through LDS) to totals[block];
//   2. adapt_scan_kernel    one block turns totals[0 .. blocks) into their
//                           exclusive scan, 256 at a time with a running carry,
//                           and leaves the sum in totals[blocks];
//   3. adapt_write_kernel   a lane's rank is its block's offset, plus the
//                           popcounts of the block's earlier waves, plus mbcnt
//                           of its own wave's ballot below it: list[rank] = p.
// Every rank is a function of the ballots alone, so the list is the same on
// every run whatever the block scheduling, and neighbouring lanes of a sparse
// pass keep neighbouring pixels.  No atomics.
#include "spt_internal.h"

namespace spt {

// fmaxf(x, lo) that returns a NaN x as it is
__device__ __forceinline__ float max_keep_nan(float x, float lo) { return x != x ? x : fmaxf(x, lo); }

// active(p) of spt.h, each operation rounded to f32 (-ffp-contract=off), the
// mean and variance as accum_finish computes them (kernels.hip) but for the
// NaN that the two maxima let through.
__device__ __forceinline__ bool adapt_active(const AdaptArgs& a, uint32_t p) {
    if (a.count[p] != a.n) return false;
    if (a.n < a.min_spp) return true;
    if (a.n >= a.max_spp) return false;
    const size_t P = a.npix;
    const float n = (float)a.n;
    float v[3], m[3];
    for (uint32_t c = 0; c < 3; c++) {
        m[c] = a.sum[c * P + p] / n;
        const float q = a.sum_sq[c * P + p] / n;
        v[c] = a.n < 2u ? 0.0f : max_keep_nan(q - m[c] * m[c], 0.0f) / (float)(a.n - 1u);
    }
    const float vs = (v[0] + v[1]) + v[2];
    const float ms = (m[0] + m[1]) + m[2];
    const float t = a.tolerance * max_keep_nan(ms, a.floor);
    return !(vs <= t * t);  // a NaN: not converged
}

__device__ __forceinline__ uint32_t lane_id() {
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

__global__ __launch_bounds__(kAdaptBlock) void adapt_count_kernel(AdaptArgs a) {
    __shared__ uint32_t wave_n[kAdaptBlock / 64];
    const uint32_t p = blockIdx.x * kAdaptBlock + threadIdx.x;
    const bool act = p < a.npix && adapt_active(a, p);
    const unsigned long long b = __ballot(act);
    const uint32_t wave = threadIdx.x >> 6;
    if (lane_id() == 0) {
        const uint32_t w = blockIdx.x * (kAdaptBlock / 64) + wave;
        if (w * 64u < a.npix) {  // masks[] holds the waves that cover a pixel
            a.masks[2 * w] = (uint32_t)b;
            a.masks[2 * w + 1] = (uint32_t)(b >> 32);
        }
        wave_n[wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t k = 0; k < kAdaptBlock / 64; k++) t += wave_n[k];
        a.totals[blockIdx.x] = t;
    }
}

// One block: totals[0 .. blocks) -> exclusive scan in place, totals[blocks] = sum.
__global__ __launch_bounds__(kAdaptBlock) void adapt_scan_kernel(uint32_t* totals, uint32_t blocks) {
    __shared__ uint32_t wave_sum[kAdaptBlock / 64];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < blocks; base += kAdaptBlock) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t x = i < blocks ? totals[i] : 0u;
        // inclusive scan inside the wave
        uint32_t s = x;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)s, d);
            if (lane >= d) s += y;
        }
        if (lane == 63u) wave_sum[wave] = s;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t k = 0; k < kAdaptBlock / 64; k++) {
            const uint32_t ws = wave_sum[k];
            if (k < wave) before += ws;
            all += ws;
        }
        if (i < blocks) totals[i] = carry + before + (s - x);
        carry += all;
        __syncthreads();  // wave_sum is rewritten by the next round
    }
    if (threadIdx.x == 0) totals[blocks] = carry;
}

__global__ __launch_bounds__(kAdaptBlock) void adapt_write_kernel(AdaptArgs a) {
    const uint32_t p = blockIdx.x * kAdaptBlock + threadIdx.x;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t w0 = blockIdx.x * (kAdaptBlock / 64);
    uint32_t rank = a.totals[blockIdx.x];
    uint32_t lo = 0, hi = 0;
    for (uint32_t k = 0; k <= wave; k++) {
        const uint32_t w = w0 + k;
        uint32_t ml = 0, mh = 0;
        if (w * 64u < a.npix) {
            ml = a.masks[2 * w];
            mh = a.masks[2 * w + 1];
        }
        if (k < wave) rank += __popc(ml) + __popc(mh);
        else { lo = ml; hi = mh; }
    }
    const uint32_t lane = threadIdx.x & 63u;
    const bool act = lane < 32u ? (lo >> lane) & 1u : (hi >> (lane - 32u)) & 1u;
    if (!act || p >= a.npix) return;
    rank += __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
    a.list[rank] = p;  // rank < the active count <= npix
}

// sample_base == 0: every pixel, no input read
__global__ __launch_bounds__(kAdaptBlock) void adapt_identity_kernel(uint32_t* list, uint32_t npix) {
    const uint32_t p = blockIdx.x * kAdaptBlock + threadIdx.x;
    if (p < npix) list[p] = p;
}

hipError_t launch_adapt_select(const AdaptArgs& a, hipStream_t s) {
    if (a.npix == 0) return hipSuccess;
    const uint32_t blocks = (a.npix + kAdaptBlock - 1) / kAdaptBlock;
    if (a.n == 0) {
        hipLaunchKernelGGL(adapt_identity_kernel, dim3(blocks), dim3(kAdaptBlock), 0, s, a.list, a.npix);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(adapt_count_kernel, dim3(blocks), dim3(kAdaptBlock), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e) return e;
    hipLaunchKernelGGL(adapt_scan_kernel, dim3(1), dim3(kAdaptBlock), 0, s, a.totals, blocks);
    if ((e = hipGetLastError())) return e;
    hipLaunchKernelGGL(adapt_write_kernel, dim3(blocks), dim3(kAdaptBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace spt
