// camera_entry.hip — the entry table of a render's tile (camera_entry.h,
// DESIGN.md §4 "Camera entry"): one word per tile pixel, built once per
// (geometry, camera, tile) on the render's stream before the camera cast.
#include <hip/hip_runtime.h>

#include "spt_internal.h"
#include "camera_entry.h"

namespace spt {

// One lane per tile pixel, no stack: from node 0 down while the pixel's beam is
// accepted into exactly one child and that child is an inner node.  f64, a few
// nodes per pixel: its cost does not matter (a 1024 x 1024 tile: well under a
// millisecond, once per view).
__global__ __launch_bounds__(256) void camera_entry_kernel(CameraEntryArgs a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.P) return;
    const uint32_t ly = udiv(p, a.W), lx = p - ly * a.W;
    const uint32_t gy = tile_global_row(ly, a.tile_index, a.tile_count, a.rows_per_group);  // camera_ray's row
    uint32_t word = 0;
    EntryBeam b;
    if (entry_beam(a.cam, lx, gy, b)) {
        uint32_t node = 0;
        for (uint32_t depth = 0; depth < kEntryMaxDepth; depth++) {
            const uint4* np = a.nodes + (size_t)node * kNode6Quads;
            const uint4 q0 = np[0], q1 = np[1], q2 = np[2], q3 = np[3];
            const uint32_t w[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                    q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
            uint32_t next, rank;
            if (!entry_descend6(w, b, next, rank)) break;
            const uint64_t child = ((uint64_t)(next & 0x00ffffffu) << a.group_shift) + (next >> 24);
            if (child == 0 || child >= a.nslots) break;  // (never in a sound tree: no read outside the nodes)
            word = next;
            node = (uint32_t)child;
        }
    }
    a.entry[p] = word;
}

hipError_t launch_camera_entry(const CameraEntryArgs& a, hipStream_t s) {
    if (a.P == 0) return hipSuccess;
    if (!a.nodes || !a.entry || a.nslots == 0 || a.W == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(camera_entry_kernel, dim3((a.P + 255u) / 256u), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace spt
