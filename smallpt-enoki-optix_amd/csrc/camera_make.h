// camera_make.h — the Camera constants of a view, evaluated once on the host:
// shared by the render loop (render.cpp) and spt_temporal_accumulate
// (temporal.cpp), which reprojects through the constants the renders used.
#pragma once
#include <cmath>

#include "../../include/spt.h"
#include "spt_math.h"

namespace spt {

// ThinlensCamera constructor (pinhole.h:9-25) + the per-call constants of
// sample_dir (pinhole.h:40-41), evaluated once on the host.
inline Camera make_camera(const spt_camera& c, uint32_t width, uint32_t height) {
    Camera cam;
    V3 from = v3(c.look_from[0], c.look_from[1], c.look_from[2]);
    V3 at = v3(c.look_at[0], c.look_at[1], c.look_at[2]);
    V3 up = v3(c.up[0], c.up[1], c.up[2]);
    cam.origin = from;
    V3 z = normalize(at - from);
    V3 x = normalize(cross(up, z));
    V3 y = normalize(cross(z, x));
    cam.frame.bx = x; cam.frame.by = y; cam.frame.bz = z;
    cam.lens_radius = c.lens_radius;
    cam.focal_dist = c.focal_dist;
    cam.film_y = c.film_size_y;
    cam.dist_lens_to_film = (c.film_size_y * 0.5f) / std::tan(c.fov_y * 0.5f);
    cam.ratio = (float)width / (float)height;
    cam.fw = (float)width;
    cam.fh = (float)height;
    // exact reciprocals of power-of-two sizes (camera_sample_dir), else 0
    cam.inv_fw = width && (width & (width - 1u)) == 0u ? 1.0f / cam.fw : 0.0f;
    cam.inv_fh = height && (height & (height - 1u)) == 0u ? 1.0f / cam.fh : 0.0f;
    {
        volatile float fz = cam.dist_lens_to_film;  // the device's operation order, no folding
        volatile float num = cam.focal_dist * fz;
        cam.focal_z = num / fz;
    }
    return cam;
}

}  // namespace spt
