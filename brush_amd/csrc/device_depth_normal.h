// device_depth_normal.h — the normal of a depth map at one pixel and its chain rule (include/brush_hip_normal.h): the
// ONE copy of the stencil that normal.hip's depth -> normal kernels and normal_loss.hip's fused normal-consistency kernel share.
#pragma once
#include "device_math.h"

namespace bh {

struct PinholeK {
    float fx, fy, cx, cy;
    uint32_t w, h;
};

BH_DEV bool depth_ok(float d) { return is_finite_f32(d) && d > 0.0f; }

// The stencil centred at (x, y): valid, the cross product c = gy x gx and the pieces its backward needs.
struct Stencil {
    bool valid;
    float kxl, kxr, kx, kyu, kyd, ky;
    Vec3A gx, gy, c;
};

BH_DEV Stencil depth_stencil(const PinholeK& k, const float* __restrict__ depth, uint32_t x, uint32_t y) {
    Stencil s;
    s.valid = false;
    if (x < 1u || y < 1u || x + 2u > k.w || y + 2u > k.h) return s;   // 1 <= x <= W-2, 1 <= y <= H-2
    const size_t p = (size_t)x + (size_t)y * k.w;
    const float dc = depth[p], dl = depth[p - 1], dr = depth[p + 1], du = depth[p - k.w], dd = depth[p + k.w];
    if (!(depth_ok(dc) && depth_ok(dl) && depth_ok(dr) && depth_ok(du) && depth_ok(dd))) return s;
    s.valid = true;
    const float fxc = ((float)x + 0.5f) - k.cx, fyc = ((float)y + 0.5f) - k.cy;
    s.kx = fxc / k.fx; s.kxl = (fxc - 1.0f) / k.fx; s.kxr = (fxc + 1.0f) / k.fx;
    s.ky = fyc / k.fy; s.kyu = (fyc - 1.0f) / k.fy; s.kyd = (fyc + 1.0f) / k.fy;
    s.gx = v3(s.kxr * dr - s.kxl * dl, s.ky * dr - s.ky * dl, dr - dl);
    s.gy = v3(s.kx * dd - s.kx * du, s.kyd * dd - s.kyu * du, dd - du);
    // c = gy x gx
    s.c = v3(s.gy.y * s.gx.z - s.gy.z * s.gx.y, s.gy.z * s.gx.x - s.gy.x * s.gx.z, s.gy.x * s.gx.y - s.gy.y * s.gx.x);
    return s;
}

// d <v, c / |c|> / d (the depth of neighbour `which` of the valid stencil s): 0 left, 1 right, 2 up, 3 down; u = c / |c|, inv = 1 / |c|
BH_DEV float stencil_chain(const Stencil& s, float inv, const Vec3A& u, const Vec3A& v, int which) {
    const Vec3A vc = scale(sub(v, scale(u, dot(v, u))), inv);
    if (which < 2) {
        // c = gy x gx: v_gx = vc x gy
        const Vec3A vg = v3(vc.y * s.gy.z - vc.z * s.gy.y, vc.z * s.gy.x - vc.x * s.gy.z, vc.x * s.gy.y - vc.y * s.gy.x);
        return which == 0 ? -dot(vg, v3(s.kxl, s.ky, 1.0f)) : dot(vg, v3(s.kxr, s.ky, 1.0f));
    }
    // v_gy = gx x vc
    const Vec3A vg = v3(s.gx.y * vc.z - s.gx.z * vc.y, s.gx.z * vc.x - s.gx.x * vc.z, s.gx.x * vc.y - s.gx.y * vc.x);
    return which == 2 ? -dot(vg, v3(s.kx, s.kyu, 1.0f)) : dot(vg, v3(s.kx, s.kyd, 1.0f));
}

// the same with the cotangent read from a map [H,W,3]; 0 for an invalid stencil and where |c| == 0
BH_DEV float stencil_grad(const PinholeK& k, const float* __restrict__ depth, const float* __restrict__ v_normal, uint32_t x, uint32_t y, int which) {
    const Stencil s = depth_stencil(k, depth, x, y);
    if (!s.valid) return 0.0f;
    const float len = length(s.c);
    if (len == 0.0f) return 0.0f;
    const float inv = 1.0f / len;
    const Vec3A u = scale(s.c, inv);
    const size_t p = ((size_t)x + (size_t)y * k.w) * 3;
    const Vec3A v = v3(v_normal[p], v_normal[p + 1], v_normal[p + 2]);
    return stencil_chain(s, inv, u, v, which);
}

}  // namespace bh
