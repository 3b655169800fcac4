// pt_host_reproject.cpp -- the host side of the reprojection (include/mi3pt.h: mi3pt_reproject): the camera frame of a raytrace uniform
// block, the one input of the gather kernel (pt_reproject.hip) that is computed and not stored.  Plain C++, no device: the CPU builds and
// tests/test_reproject_host.py cover it.
#include <cmath>
#include "pt_internal.h"

// camera_frame's rule (pt_kernels.hip; cameraToRay, raytrace.wgsl:217-236), in double from the block's fp32 fields, each output rounded
// to fp32 once: position, aspect | fwd, t | u, r | v, 0
extern "C" int mi3pt_host_view_frame(const void *raytrace_uniforms, size_t nbytes, float out[16])
{
    if (!raytrace_uniforms || !out) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (nbytes != MI3PT_RAYTRACE_UNIFORMS_SIZE) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_host_view_frame: the raytrace uniform block is 96 bytes");
    const uint8_t *u = static_cast<const uint8_t *>(raytrace_uniforms);
    const double aspect = ldf(u, 8), fov = ldf(u, 60);
    double pos[3], dir[3];
    for (int k = 0; k < 3; k++) { pos[k] = ldf(u, 32 + 4 * k); dir[k] = ldf(u, 48 + 4 * k); }
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(pos[k])) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_host_view_frame: the camera position is not finite");
    const double len = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
    if (!std::isfinite(len) || !(len > 0.0)) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_host_view_frame: the camera direction is zero or not finite");
    if (!(fov > 0.0 && fov < 180.0)) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_host_view_frame: fov must lie in (0, 180)");
    const double w[3] = { -dir[0] / len, -dir[1] / len, -dir[2] / len };
    double up[3] = { 0.0, 1.0, 0.0 };
    if (std::fabs(w[1]) > 0.99999) { up[1] = 0.0; up[2] = 1.0; }
    double uu[3] = { up[1] * w[2] - up[2] * w[1], up[2] * w[0] - up[0] * w[2], up[0] * w[1] - up[1] * w[0] };
    const double ulen = std::sqrt(uu[0] * uu[0] + uu[1] * uu[1] + uu[2] * uu[2]);
    for (int k = 0; k < 3; k++) uu[k] /= ulen;
    const double vv[3] = { w[1] * uu[2] - w[2] * uu[1], w[2] * uu[0] - w[0] * uu[2], w[0] * uu[1] - w[1] * uu[0] };
    const double t = std::tan(fov * 3.14159265358979323846 / 360.0);
    const double r = aspect * t;
    const double all[16] = { pos[0], pos[1], pos[2], aspect, -w[0], -w[1], -w[2], t, uu[0], uu[1], uu[2], r, vv[0], vv[1], vv[2], 0.0 };
    for (int k = 0; k < 16; k++) out[k] = (float)all[k];
    return MI3PT_OK;
}
