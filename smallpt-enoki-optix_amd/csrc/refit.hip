// refit.hip — in-place geometry update of a committed scene (gfx950):
// spt_scene_update_geometry's device side.  The tree's topology stays; the
// triangle records and normals are rewritten in their slots and every node's
// boxes are recomputed bottom-up with the builders' own arithmetic
// (bvh_refit.h), so a refitted tree has conservative boxes and — the closest
// hit not depending on the tree — gives the hits of a tree
// freshly built from the new vertices.
//
//   plan    one download of the nodes, a walk from the root (slot 0): the
//           reachable node slots grouped by level, 6 floats of scratch per
//           slot for the node's exact box
//   pass 1  one lane per original triangle t: gather its vertices, write the
//           record and the three normal quads of slot orig2slot[t]
//   pass 2  one lane per node, one launch per level, deepest first (kernel
//           boundaries order the levels; no host round trip between them);
//           the top levels, a few hundred nodes in all, share one single-block
//           launch with a barrier between levels
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "spt_internal.h"

#include "bvh_refit.h"

namespace spt {
namespace {

constexpr uint32_t kBlock = 256;
// levels from the root down are refitted by one block while each holds at most this many nodes
constexpr uint32_t kTopLevelNodes = 1024;

inline uint32_t blocks(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

#define RF_TRY(call)                          \
    do {                                      \
        hipError_t e_ = (call);               \
        if (e_ != hipSuccess) return e_;      \
    } while (0)

// ---- validation: spt_scene_create_cfg's index rules, counted on the device

__global__ __launch_bounds__(kBlock) void refit_validate_kernel(RefitMeshIn m, uint32_t ntri,
                                                                uint32_t* __restrict__ bad) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= ntri) return;
    uint32_t n = 0;
    for (int k = 0; k < 3; k++) {
        const int64_t pi = m.pos_tri[(size_t)t * 3 + k];
        if (pi < 0 || (uint64_t)pi >= m.nvert) n++;
        if (m.nrm_tri) {
            const int64_t ni = m.nrm_tri[(size_t)t * 3 + k];
            if (ni < -1 || (ni >= 0 && (uint64_t)ni >= m.nnrm)) n++;
        }
    }
    if (n) atomicAdd(bad, n);
}

// ---- pass 1: triangle records and normals, in place

__global__ __launch_bounds__(kBlock) void refit_tris_kernel(RefitMeshIn m, uint32_t ntri,
                                                            const int32_t* __restrict__ o2s,
                                                            float4* __restrict__ tris, float4* __restrict__ snrm) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= ntri) return;
    const uint32_t sl = (uint32_t)o2s[t];
    if (sl >= ntri) return;  // (a scene's own orig2slot: checked at load, never out of range)
    float v[9];
    for (int k = 0; k < 3; k++) {
        const int64_t pi = m.pos_tri[(size_t)t * 3 + k];
        for (int c = 0; c < 3; c++) v[k * 3 + c] = m.pos[pi * 3 + c];
    }
    float rec[kTriFloats];
    tri_record_fill(rec, v, t);
    for (int k = 0; k < 4; k++)
        tris[(size_t)sl * kTriQuads + k] = make_float4(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
    // geometric normal fallback for a missing vertex normal (as scene_slots_kernel)
    const V3 g = normalize(cross(v3(v[3] - v[0], v[4] - v[1], v[5] - v[2]), v3(v[6] - v[0], v[7] - v[1], v[8] - v[2])));
    const float mat = snrm[(size_t)sl * 3].w;  // the material id bits stay
    for (int k = 0; k < 3; k++) {
        const int64_t ni = m.nrm_tri ? m.nrm_tri[(size_t)t * 3 + k] : -1;
        const V3 nv = ni >= 0 ? v3(m.nrm[ni * 3], m.nrm[ni * 3 + 1], m.nrm[ni * 3 + 2]) : g;
        snrm[(size_t)sl * 3 + k] = make_float4(nv.x, nv.y, nv.z, k == 0 ? mat : 0.0f);
    }
}

// ---- pass 2: one node

struct RefitArgs {
    uint4* nodes;
    const float4* tris;
    float* boxes;                 // 6 floats per node slot
    const uint32_t* order;        // node slots, level by level
    const uint32_t* level_off;    // (top kernel) offsets into order
    double* area;
    uint32_t first, count;        // (level kernel) this launch's part of order
    uint32_t top_levels;          // (top kernel) levels top_levels - 1 .. 0
    uint32_t group_shift, write;
};

struct DeviceBoxes {
    const float4* tris;
    const float* boxes;
    __device__ __forceinline__ RefitBox leaf(uint32_t first, uint32_t count) const {
        RefitBox b = refit_box_empty();
        for (uint32_t i = 0; i < count; i++) {
            const float4* q = tris + (size_t)(first + i) * kTriQuads;
            const float4 a = q[0], c = q[1], d = q[2];
            // the three vertices' floats 0-2, 5-7, 10-12 of the record
            const float rec[13] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w, q[3].x};
            refit_box_grow(b, refit_tri_box(rec));
        }
        return b;
    }
    __device__ __forceinline__ RefitBox inner(uint32_t slot) const {
        const float2* p = (const float2*)(boxes + (size_t)slot * 6);
        const float2 a = p[0], c = p[1], d = p[2];
        RefitBox b;
        b.lo[0] = a.x; b.lo[1] = a.y; b.lo[2] = c.x; b.hi[0] = c.y; b.hi[1] = d.x; b.hi[2] = d.y;
        return b;
    }
};

// Refits node `slot` (whole 16-B quads in and out) and returns the half area
// of its exact box (0 for a box that is not finite).
template <int kFmt>
__device__ __forceinline__ double refit_one(const RefitArgs& a, uint32_t slot) {
    constexpr uint32_t kQuads = kFmt == kRefitFmt8 ? kNode8Quads : 4u;
    constexpr uint32_t kUsed = kFmt == kRefitFmt8 ? 5u : 4u;  // quads that hold node words
    uint4* np = a.nodes + (size_t)slot * kQuads;
    uint32_t w[kUsed * 4];
#pragma unroll
    for (uint32_t q = 0; q < kUsed; q++) {
        const uint4 x = np[q];
        w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w;
    }
    RefitKid kid[8];
    const DeviceBoxes src{a.tris, a.boxes};
    const RefitBox nb = refit_node(kFmt, w, a.group_shift, src, kid);
    float2* bp = (float2*)(a.boxes + (size_t)slot * 6);
    bp[0] = make_float2(nb.lo[0], nb.lo[1]);
    bp[1] = make_float2(nb.lo[2], nb.hi[0]);
    bp[2] = make_float2(nb.hi[1], nb.hi[2]);
    if (a.write) {
#pragma unroll
        for (uint32_t q = 0; q < kUsed; q++) {
            if (kFmt == kRefitFmt8 && q == 1) continue;  // w4-7: topology only
            if (kFmt == kRefitFmt2 && q == 3) continue;  // the child codes
            np[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
        }
    }
    const double h = refit_half_area(nb);
    return h >= 0.0 && h <= 1e300 ? h : 0.0;
}

// the wave's sum into *area: one atomic per wave
__device__ __forceinline__ void add_area(double* area, double h) {
    for (int off = 32; off > 0; off >>= 1) h += __shfl_down(h, off);
    if ((threadIdx.x & 63u) == 0u && h != 0.0) atomicAdd(area, h);
}

template <int kFmt>
__global__ __launch_bounds__(kBlock) void refit_level_kernel(RefitArgs a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    double h = 0.0;
    if (i < a.count) h = refit_one<kFmt>(a, a.order[a.first + i]);
    add_area(a.area, h);
}

// Levels top_levels - 1 .. 0 in one block: a level's boxes are written before
// the barrier and read after it by the same workgroup.
template <int kFmt>
__global__ __launch_bounds__(kBlock) void refit_top_kernel(RefitArgs a) {
    double h = 0.0;
    for (uint32_t l = a.top_levels; l-- > 0;) {
        const uint32_t b = a.level_off[l], e = a.level_off[l + 1];
        for (uint32_t i = b + threadIdx.x; i < e; i += kBlock) h += refit_one<kFmt>(a, a.order[i]);
        __threadfence_block();
        __syncthreads();
    }
    add_area(a.area, h);
}

template <int kFmt>
hipError_t launch_levels(const RefitArgs& base, const RefitPlan& plan, hipStream_t s) {
    for (uint32_t l = plan.levels; l-- > plan.top_levels;) {
        RefitArgs a = base;
        a.first = plan.h_level_off[l];
        a.count = plan.h_level_off[l + 1] - a.first;
        if (!a.count) continue;
        hipLaunchKernelGGL(refit_level_kernel<kFmt>, dim3(blocks(a.count)), dim3(kBlock), 0, s, a);
    }
    if (plan.top_levels) hipLaunchKernelGGL(refit_top_kernel<kFmt>, dim3(1), dim3(kBlock), 0, s, base);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_refit_validate(const RefitScene& sc, const RefitMeshIn& m, uint32_t* bad, hipStream_t s) {
    RF_TRY(hipMemsetAsync(bad, 0, sizeof(uint32_t), s));
    if (sc.ntri == 0) return hipSuccess;
    hipLaunchKernelGGL(refit_validate_kernel, dim3(blocks(sc.ntri)), dim3(kBlock), 0, s, m, sc.ntri, bad);
    return hipGetLastError();
}

hipError_t launch_refit_update(const RefitScene& sc, const RefitMeshIn* m, const RefitPlan& plan, bool write,
                               hipStream_t s) {
    RF_TRY(hipMemsetAsync(plan.area, 0, sizeof(double), s));
    if (sc.ntri == 0 || plan.levels == 0) return hipSuccess;
    if (m) {
        hipLaunchKernelGGL(refit_tris_kernel, dim3(blocks(sc.ntri)), dim3(kBlock), 0, s, *m, sc.ntri, sc.orig2slot,
                           sc.tris, sc.snrm);
        RF_TRY(hipGetLastError());
    }
    RefitArgs a{};
    a.nodes = sc.nodes;
    a.tris = sc.tris;
    a.boxes = plan.boxes;
    a.order = plan.order;
    a.level_off = plan.level_off;
    a.area = plan.area;
    a.top_levels = plan.top_levels;
    a.group_shift = sc.group_shift;
    a.write = write ? 1u : 0u;
    if (sc.fmt == kRefitFmt8) return launch_levels<kRefitFmt8>(a, plan, s);
    if (sc.fmt == kRefitFmt6) return launch_levels<kRefitFmt6>(a, plan, s);
    return launch_levels<kRefitFmt2>(a, plan, s);
}

void refit_plan_release(RefitPlan& p) {
    if (p.order) (void)hipFree(p.order);
    if (p.level_off) (void)hipFree(p.level_off);
    if (p.boxes) (void)hipFree(p.boxes);
    if (p.area) (void)hipFree(p.area);
    if (p.ev0) (void)hipEventDestroy(p.ev0);
    if (p.ev1) (void)hipEventDestroy(p.ev1);
    p = RefitPlan{};
}

hipError_t refit_plan_build(const RefitScene& sc, uint64_t expected_nodes, hipStream_t s, RefitPlan* plan,
                            const char** why) {
    *why = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    RefitPlan p;
    const auto bail = [&](hipError_t e) {
        refit_plan_release(p);
        return e;
    };
    const uint32_t stride = refit_node_words(sc.fmt);
    const uint64_t nslots = sc.node_bytes / ((uint64_t)stride * 4);
    std::vector<uint32_t> order;
    std::vector<uint32_t>& off = p.h_level_off;
    off.push_back(0u);
    if (sc.ntri && nslots) {
        std::vector<uint32_t> w((size_t)nslots * stride);
        hipError_t e = hipMemcpyAsync(w.data(), sc.nodes, sc.node_bytes, hipMemcpyDeviceToHost, s);
        if (!e) e = hipStreamSynchronize(s);
        if (e) return bail(e);
        // breadth first from the root: level l's nodes are order[off[l] .. off[l + 1])
        std::vector<uint8_t> seen(nslots, 0);
        order.reserve(expected_nodes);
        order.push_back(0u);
        seen[0] = 1;
        size_t b = 0;
        while (b < order.size()) {
            const size_t e2 = order.size();
            off.push_back((uint32_t)e2);
            for (size_t i = b; i < e2; i++) {
                RefitKid kid[8];
                const uint32_t* n = &w[(size_t)order[i] * stride];
                const int nk = sc.fmt == kRefitFmt8 ? 8 : (sc.fmt == kRefitFmt6 ? 6 : 2);
                if (sc.fmt == kRefitFmt8) refit_kids8(n, sc.group_shift, kid);
                else if (sc.fmt == kRefitFmt6) refit_kids6(n, sc.group_shift, kid);
                else refit_kids2(n, kid);
                for (int c = 0; c < nk; c++) {
                    if (kid[c].inner) {
                        if (kid[c].index >= nslots || seen[kid[c].index]) {
                            *why = "an inner child lies outside the nodes or is reached twice";
                            return bail(hipErrorInvalidValue);
                        }
                        seen[kid[c].index] = 1;
                        order.push_back(kid[c].index);
                    } else if ((uint64_t)kid[c].index + kid[c].count > sc.ntri) {
                        *why = "a leaf lies beyond the triangles";
                        return bail(hipErrorInvalidValue);
                    }
                }
            }
            b = e2;
        }
        if (order.size() != expected_nodes) {
            *why = "the nodes reachable from the root are not the scene's node count";
            return bail(hipErrorInvalidValue);
        }
    }
    p.levels = (uint32_t)off.size() - 1;
    p.nodes = order.size();
    while (p.top_levels < p.levels && off[p.top_levels + 1] - off[p.top_levels] <= kTopLevelNodes &&
           off[p.top_levels + 1] <= 4 * kTopLevelNodes)
        p.top_levels++;
    const size_t order_bytes = std::max<size_t>(order.size(), 1) * sizeof(uint32_t);
    const size_t off_bytes = off.size() * sizeof(uint32_t);
    const size_t box_bytes = std::max<uint64_t>(nslots, 1) * 6 * sizeof(float);
    hipError_t e = hipMalloc((void**)&p.order, order_bytes);
    if (!e) e = hipMalloc((void**)&p.level_off, off_bytes);
    if (!e) e = hipMalloc((void**)&p.boxes, box_bytes);
    if (!e) e = hipMalloc((void**)&p.area, sizeof(double));
    if (!e && !order.empty()) e = hipMemcpyAsync(p.order, order.data(), order.size() * 4, hipMemcpyHostToDevice, s);
    if (!e) e = hipMemcpyAsync(p.level_off, off.data(), off_bytes, hipMemcpyHostToDevice, s);
    if (!e) e = hipEventCreate(&p.ev0);
    if (!e) e = hipEventCreate(&p.ev1);
    if (!e) e = hipStreamSynchronize(s);  // (the uploads read host vectors that end with this call)
    if (e) return bail(e);
    p.bytes = order_bytes + off_bytes + box_bytes + sizeof(double);
    // the areas as built: the refit's own pass over the records the scene
    // holds, nothing written (an identity update reproduces the build)
    e = launch_refit_update(sc, nullptr, p, false, s);
    if (!e) e = hipMemcpyAsync(&p.area_built, p.area, sizeof(double), hipMemcpyDeviceToHost, s);
    if (!e) e = hipStreamSynchronize(s);
    if (e) return bail(e);
    p.built = true;
    p.plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *plan = std::move(p);
    return hipSuccess;
}

// ---- the light table's inputs (spt_scene_set_light_sampling, capi.cpp): the
// host keeps no copy of the triangles, so the material id of every triangle
// and the vertices of the emissive ones are read back from the records, in
// original triangle id order (orig2slot).

__global__ __launch_bounds__(256) void light_mats_kernel(const float4* __restrict__ snrm,
                                                         const int32_t* __restrict__ orig2slot, uint32_t ntri,
                                                         int32_t* __restrict__ mat) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= ntri) return;
    mat[t] = (int32_t)f2u(snrm[(size_t)orig2slot[t] * 3].w);
}

__global__ __launch_bounds__(256) void light_tris_kernel(const float4* __restrict__ tris,
                                                         const int32_t* __restrict__ orig2slot,
                                                         const uint32_t* __restrict__ ids, uint32_t n,
                                                         float* __restrict__ tv) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float* rec = (const float*)(tris + (size_t)orig2slot[ids[i]] * kTriQuads);  // tri_record_fill
    for (uint32_t k = 0; k < 3; k++)
        for (uint32_t c = 0; c < 3; c++) tv[(size_t)i * 9 + 3 * k + c] = rec[5 * k + c];
}

hipError_t launch_light_mats(const float4* snrm, const int32_t* orig2slot, uint32_t ntri, int32_t* mat,
                             hipStream_t s) {
    if (!ntri) return hipSuccess;
    hipLaunchKernelGGL(light_mats_kernel, dim3((ntri + 255u) / 256u), dim3(256), 0, s, snrm, orig2slot, ntri, mat);
    return hipGetLastError();
}

hipError_t launch_light_tris(const float4* tris, const int32_t* orig2slot, const uint32_t* ids, uint32_t n,
                             float* tv, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(light_tris_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, tris, orig2slot, ids, n, tv);
    return hipGetLastError();
}

}  // namespace spt
