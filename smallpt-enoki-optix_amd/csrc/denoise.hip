// denoise.hip — spt_denoise's and spt_denoise_var's kernels: the edge-avoiding
// a-trous wavelet filter of Dammertz et al. 2010 ("Edge-Avoiding A-Trous Wavelet Transform for fast
// Global Illumination Filtering"), guided by the first-hit buffers of
// spt_render_aov.  Not in the reference (its film is saved as rendered,
// main.cpp:431-433).
#include "spt_internal.h"

namespace spt {

// One iteration, one thread per pixel p: the 5 x 5 taps q = p + step (dx, dy)
// inside the image, kernel weight k = h[|dx|] h[|dy|] with the B3 spline
// h = {3/8, 1/4, 1/16}, weight w = k expf(-(e_c + e_n + e_a + e_z)) with
//   e_c = |c(p) - c(q)|^2 inv_color,    e_n = |n(p) - n(q)|^2 inv_normal,
//   e_a = |a(p) - a(q)|^2 inv_albedo,   e_z = (z(p) - z(q))^2 inv_depth / max(z(p)^2, 1e-12),
// and dst(p) = sum w c(q) / sum w.  The centre tap has every e = 0 and so the
// weight k(0, 0) exactly: the denominator is never 0.  A term whose inv is 0
// is off (its planes are not read and may be NULL).
__global__ __launch_bounds__(256) void denoise_kernel(DenoiseArgs a) {
    const uint32_t x = blockIdx.x * 32u + (threadIdx.x & 31u);
    const uint32_t y = blockIdx.y * 8u + (threadIdx.x >> 5);
    if (x >= a.width || y >= a.height) return;
    const size_t P = (size_t)a.width * a.height;
    const size_t p = (size_t)y * a.width + x;
    const bool on_c = a.inv_color > 0.0f, on_n = a.inv_normal > 0.0f, on_a = a.inv_albedo > 0.0f,
               on_z = a.inv_depth > 0.0f;
    const float cr = a.src[p], cg = a.src[P + p], cb = a.src[2 * P + p];
    float pnx = 0.0f, pny = 0.0f, pnz = 0.0f, par = 0.0f, pag = 0.0f, pab = 0.0f, pz = 0.0f, inv_z = 0.0f;
    if (on_n) { pnx = a.normal_x[p]; pny = a.normal_y[p]; pnz = a.normal_z[p]; }
    if (on_a) { par = a.albedo_r[p]; pag = a.albedo_g[p]; pab = a.albedo_b[p]; }
    if (on_z) { pz = a.depth[p]; inv_z = a.inv_depth / fmaxf(pz * pz, 1e-12f); }
    const float h[3] = {0.375f, 0.25f, 0.0625f};
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = (int64_t)y + (int64_t)dy * (int64_t)a.step;
        if (qy < 0 || qy >= (int64_t)a.height) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = (int64_t)x + (int64_t)dx * (int64_t)a.step;
            if (qx < 0 || qx >= (int64_t)a.width) continue;
            const size_t q = (size_t)qy * a.width + (size_t)qx;
            const float qr = a.src[q], qg = a.src[P + q], qb = a.src[2 * P + q];
            float e = 0.0f;
            if (on_c) {
                const float d0 = cr - qr, d1 = cg - qg, d2 = cb - qb;
                e = e + ((d0 * d0 + d1 * d1) + d2 * d2) * a.inv_color;
            }
            if (on_n) {
                const float d0 = pnx - a.normal_x[q], d1 = pny - a.normal_y[q], d2 = pnz - a.normal_z[q];
                e = e + ((d0 * d0 + d1 * d1) + d2 * d2) * a.inv_normal;
            }
            if (on_a) {
                const float d0 = par - a.albedo_r[q], d1 = pag - a.albedo_g[q], d2 = pab - a.albedo_b[q];
                e = e + ((d0 * d0 + d1 * d1) + d2 * d2) * a.inv_albedo;
            }
            if (on_z) {
                const float d0 = pz - a.depth[q];
                e = e + (d0 * d0) * inv_z;
            }
            const float w = (h[dx < 0 ? -dx : dx] * h[dy < 0 ? -dy : dy]) * expf(-e);
            sr = sr + w * qr;
            sg = sg + w * qg;
            sb = sb + w * qb;
            sw = sw + w;
        }
    }
    a.dst[p] = sr / sw;
    a.dst[P + p] = sg / sw;
    a.dst[2 * P + p] = sb / sw;
}

// spt_denoise_var's first step: v_0 = max((var_r + var_g) + var_b, 0), one plane.
__global__ __launch_bounds__(256) void denoise_var_init_kernel(const float* __restrict__ var3, float* __restrict__ v0,
                                                               uint32_t P) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= P) return;
    v0[p] = fmaxf((var3[p] + var3[(size_t)P + p]) + var3[2 * (size_t)P + p], 0.0f);
}

// One iteration of spt_denoise_var (the spatial filter of Schied et al. 2017,
// "Spatiotemporal Variance-Guided Filtering"): denoise_kernel with the colour
// distance measured against the pixel's own variance estimate,
//   e_c = |c(p) - c(q)|^2 / (sigma_variance^2 vt(p) + 1e-10),
// vt(p) the 3 x 3 Gaussian {1/2, 1/4} x {1/2, 1/4} of the variance plane over the
// adjacent pixels inside the image, normalised by the weights that took part;
// and with the variance filtered along: vdst(p) = sum w^2 v(q) / (sum w)^2.
// sv2 = sigma_variance^2, 0: no colour term.  vdst may be null (the last
// iteration of a call that does not want the variance).
__global__ __launch_bounds__(256) void denoise_var_kernel(DenoiseVarArgs a) {
    const uint32_t x = blockIdx.x * 32u + (threadIdx.x & 31u);
    const uint32_t y = blockIdx.y * 8u + (threadIdx.x >> 5);
    if (x >= a.width || y >= a.height) return;
    const size_t P = (size_t)a.width * a.height;
    const size_t p = (size_t)y * a.width + x;
    const bool on_c = a.sv2 > 0.0f, on_n = a.inv_normal > 0.0f, on_a = a.inv_albedo > 0.0f, on_z = a.inv_depth > 0.0f;
    const float cr = a.src[p], cg = a.src[P + p], cb = a.src[2 * P + p];
    float pnx = 0.0f, pny = 0.0f, pnz = 0.0f, par = 0.0f, pag = 0.0f, pab = 0.0f, pz = 0.0f, inv_z = 0.0f;
    if (on_n) { pnx = a.normal_x[p]; pny = a.normal_y[p]; pnz = a.normal_z[p]; }
    if (on_a) { par = a.albedo_r[p]; pag = a.albedo_g[p]; pab = a.albedo_b[p]; }
    if (on_z) { pz = a.depth[p]; inv_z = a.inv_depth / fmaxf(pz * pz, 1e-12f); }
    float den_c = 1.0f;
    if (on_c) {
        const float g1[2] = {0.5f, 0.25f};
        float gv = 0.0f, gs = 0.0f;
        for (int dy = -1; dy <= 1; dy++) {
            const int64_t qy = (int64_t)y + dy;
            if (qy < 0 || qy >= (int64_t)a.height) continue;
            for (int dx = -1; dx <= 1; dx++) {
                const int64_t qx = (int64_t)x + dx;
                if (qx < 0 || qx >= (int64_t)a.width) continue;
                const float g = g1[dx < 0 ? -dx : dx] * g1[dy < 0 ? -dy : dy];
                gv = gv + g * a.vsrc[(size_t)qy * a.width + (size_t)qx];
                gs = gs + g;
            }
        }
        den_c = a.sv2 * (gv / gs) + 1e-10f;
    }
    const float h[3] = {0.375f, 0.25f, 0.0625f};
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = (int64_t)y + (int64_t)dy * (int64_t)a.step;
        if (qy < 0 || qy >= (int64_t)a.height) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = (int64_t)x + (int64_t)dx * (int64_t)a.step;
            if (qx < 0 || qx >= (int64_t)a.width) continue;
            const size_t q = (size_t)qy * a.width + (size_t)qx;
            const float qr = a.src[q], qg = a.src[P + q], qb = a.src[2 * P + q];
            float e = 0.0f;
            if (on_c) {
                const float d0 = cr - qr, d1 = cg - qg, d2 = cb - qb;
                e = e + ((d0 * d0 + d1 * d1) + d2 * d2) / den_c;
            }
            if (on_n) {
                const float d0 = pnx - a.normal_x[q], d1 = pny - a.normal_y[q], d2 = pnz - a.normal_z[q];
                e = e + ((d0 * d0 + d1 * d1) + d2 * d2) * a.inv_normal;
            }
            if (on_a) {
                const float d0 = par - a.albedo_r[q], d1 = pag - a.albedo_g[q], d2 = pab - a.albedo_b[q];
                e = e + ((d0 * d0 + d1 * d1) + d2 * d2) * a.inv_albedo;
            }
            if (on_z) {
                const float d0 = pz - a.depth[q];
                e = e + (d0 * d0) * inv_z;
            }
            const float w = (h[dx < 0 ? -dx : dx] * h[dy < 0 ? -dy : dy]) * expf(-e);
            sr = sr + w * qr;
            sg = sg + w * qg;
            sb = sb + w * qb;
            sw = sw + w;
            sv = sv + (w * w) * a.vsrc[q];
        }
    }
    a.dst[p] = sr / sw;
    a.dst[P + p] = sg / sw;
    a.dst[2 * P + p] = sb / sw;
    if (a.vdst) a.vdst[p] = sv / (sw * sw);
}

hipError_t launch_denoise(const DenoiseArgs& a, hipStream_t s) {
    if (a.width == 0 || a.height == 0) return hipSuccess;
    const dim3 g((a.width + 31u) / 32u, (a.height + 7u) / 8u), b(256);
    hipLaunchKernelGGL(denoise_kernel, g, b, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_denoise_var_init(const float* var3, float* v0, uint32_t P, hipStream_t s) {
    if (P == 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_var_init_kernel, dim3((P + 255u) / 256u), dim3(256), 0, s, var3, v0, P);
    return hipGetLastError();
}

hipError_t launch_denoise_var(const DenoiseVarArgs& a, hipStream_t s) {
    if (a.width == 0 || a.height == 0) return hipSuccess;
    const dim3 g((a.width + 31u) / 32u, (a.height + 7u) / 8u), b(256);
    hipLaunchKernelGGL(denoise_var_kernel, g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace spt
