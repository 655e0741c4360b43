// test_intrinsics.cpp — camera intrinsics gradients through the C++ host mirror (include/brush_hip.hpp RenderNode::backward_intrinsics,
// backward_camera, train_set_intrinsics_grad, camera_set_intrinsics):
//   * host arithmetic (no device needed): camera_set_intrinsics with the camera's own f64 focals reproduces the set-up's BhCamera byte
//     for byte, other intrinsics move the pinhole clamp limits to the image edges +-15 % and leave the pose alone, and zero, negative
//     or non-finite values throw and leave the camera as it was;
//   * on the GPU, a 16x16 frame (one tile: the backward repeats itself bit for bit): backward_intrinsics' splat outputs are
//     backward's bits, the four repeat bit for bit with and without the pose pass, the v_viewmat beside them is backward_pose's, and
//     an empty view overwrites NaN with zeros.
// Build + run: tests/test_intrinsics_cpp.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "brush_hip.hpp"

namespace bh = brush_hip;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                                        \
    do {                                                                                                                        \
        if (!(cond)) { std::printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); ++g_failed; } \
    } while (0)

struct Sm64 {
    uint64_t s;
    uint64_t next() {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    float uni(float lo, float hi) { return lo + (float)((double)next() / 18446744073709551615.0) * (hi - lo); }
};

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0;
}

static bh::Camera default_camera(uint32_t w, uint32_t h) {
    bh::Camera cam;
    cam.fov_x = 60.0 * 3.14159265358979323846 / 180.0;
    const double fx = (w / 2.0) / std::tan(cam.fov_x / 2.0);
    cam.fov_y = 2.0 * std::atan((h / 2.0) / fx);
    return cam;
}

static bool throws(BhCamera cam, double fx, double fy, double cx, double cy) {
    const BhCamera before = cam;
    try {
        bh::camera_set_intrinsics(cam, fx, fy, cx, cy);
    } catch (const bh::Error&) {
        return std::memcmp(&cam, &before, sizeof cam) == 0;
    }
    return false;
}

static void host_checks(uint32_t w, uint32_t h) {
    const bh::Camera c = default_camera(w, h);
    const BhCamera base = c.uniforms(w, h);
    const double fx = bh_fov_to_focal(c.fov_x, w, BH_CAMERA_PINHOLE, nullptr), fy = bh_fov_to_focal(c.fov_y, h, BH_CAMERA_PINHOLE, nullptr);
    BhCamera cam = base;
    cam.fx = 1.0f; cam.lim_pos_x = 7.0f; cam.lim_neg_y = 7.0f; cam.half_max_render_fov = 9.0f;
    bh::camera_set_intrinsics(cam, fx, fy, base.cx, base.cy);
    CHECK(std::memcmp(&cam, &base, sizeof cam) == 0, "the camera's own intrinsics do not reproduce its set-up");
    bh::camera_set_intrinsics(cam, 1.25 * fx, fy, base.cx + 2.0, base.cy);
    CHECK(cam.fx == (float)(1.25 * fx) && cam.fy == base.fy && cam.cx == base.cx + 2.0f && cam.cy == base.cy, "the four are not what was set");
    CHECK(cam.lim_pos_x == (1.15f * (float)w - cam.cx) / cam.fx && cam.lim_neg_x == (-0.15f * (float)w - cam.cx) / cam.fx &&
              cam.lim_pos_y == base.lim_pos_y && cam.lim_neg_y == base.lim_neg_y,
          "the clamp limits are not the image edges +-15 %% at the new intrinsics");
    CHECK(cam.half_max_render_fov < base.half_max_render_fov, "a longer focal length did not narrow the cull angle");
    CHECK(std::memcmp(cam.vm, base.vm, sizeof cam.vm) == 0 && std::memcmp(cam.cam_pos, base.cam_pos, sizeof cam.cam_pos) == 0 && cam.img_w == w &&
              cam.img_h == h && cam.model == base.model,
          "set_intrinsics touched another field");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(throws(base, 0.0, fy, 1.0, 1.0) && throws(base, fx, -1.0, 1.0, 1.0) && throws(base, nan, fy, 1.0, 1.0) && throws(base, fx, inf, 1.0, 1.0) &&
              throws(base, fx, fy, nan, 1.0) && throws(base, fx, fy, 1.0, -inf),
          "a value that is no focal length or no centre was accepted, or the camera changed");
    std::printf("ok intrinsics host arithmetic\n");
}

int main() {
    const uint32_t n = 2000, w = 16, h = 16;
    try {
        host_checks(123, 82);
        int dev_count = 0;
        if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
            std::printf("no HIP device: host checks only\n");
            return g_failed ? 1 : 0;
        }
        bh::Context ctx(0);
        Sm64 r{0x1A7};
        std::vector<float> tr((size_t)n * 10), sh((size_t)n * 4 * 3), op(n);
        for (uint32_t i = 0; i < n; ++i) {
            float* row = &tr[(size_t)i * 10];
            row[2] = r.uni(2.0f, 9.0f);
            row[0] = r.uni(-0.6f, 0.6f) * row[2]; row[1] = r.uni(-0.6f, 0.6f) * row[2];
            row[3] = 1.0f; row[4] = r.uni(-0.3f, 0.3f); row[5] = r.uni(-0.3f, 0.3f); row[6] = r.uni(-0.3f, 0.3f);
            for (int k = 7; k < 10; ++k) row[k] = r.uni(std::log(0.05f), std::log(0.4f));
            op[i] = r.uni(-2.0f, 2.5f);
            for (int c = 0; c < 12; ++c) sh[(size_t)i * 12 + c] = r.uni(-0.5f, 0.5f);
        }
        const bh::Splats s = bh::Splats::from_host(tr, sh, op);
        const bh::Camera cam = default_camera(w, h);
        const float black[3] = {0.0f, 0.0f, 0.0f};
        std::vector<float> v((size_t)w * h * 4);
        for (float& x : v) x = r.uni(-1.0f, 1.0f) / (float)(w * h);
        const bh::DeviceBuffer<float> v_dev(v);
        bh::DeviceBuffer<float> vi(4), vi2(4), vi3(4), vv(12), vv2(12);
        {
            bh::RenderNode a(ctx, s, cam, w, h, black, /*retain=*/true), b(ctx, s, cam, w, h, black, /*retain=*/true), c(ctx, s, cam, w, h, black, /*retain=*/true);
            const bh::SplatGrads plain = a.backward(v_dev.data());
            const bh::SplatGrads intr = b.backward_intrinsics(v_dev.data(), vi.data());
            (void)b.backward_intrinsics(v_dev.data(), vi2.data(), vv.data());
            (void)c.backward_pose(v_dev.data(), vv2.data());
            CHECK(same_bits(plain.v_transforms.download(), intr.v_transforms.download()) && same_bits(plain.v_sh_coeffs.download(), intr.v_sh_coeffs.download()) &&
                      same_bits(plain.v_raw_opacities.download(), intr.v_raw_opacities.download()) &&
                      same_bits(plain.v_refine_weight.download(), intr.v_refine_weight.download()),
                  "the splat outputs of backward_intrinsics are not backward's");
            const std::vector<float> g = vi.download();
            CHECK(same_bits(g, vi2.download()), "the four differ with the pose pass beside them");
            CHECK(same_bits(vv.download(), vv2.download()), "the v_viewmat beside the four is not backward_pose's");
            bool live = true;
            for (float x : g) live = live && std::isfinite(x) && x != 0.0f;
            CHECK(live, "v_intrinsics %g %g %g %g", g[0], g[1], g[2], g[3]);
            // no term given: the general entry is the colour-only one
            BhCameraGradTerms none{};
            (void)b.backward_camera(v_dev.data(), none, vi3.data());
            CHECK(same_bits(g, vi3.download()), "backward_camera without a term is not backward_intrinsics");
            std::printf("ok intrinsics backward (%.6g %.6g %.6g %.6g)\n", g[0], g[1], g[2], g[3]);
        }
        {
            // turned away from the scene: nothing visible, four zeros over NaN
            bh::Camera away = cam;
            away.rotation[0] = 0.0f; away.rotation[1] = 1.0f; away.rotation[2] = 0.0f; away.rotation[3] = 0.0f;
            bh::RenderNode node(ctx, s, away, w, h, black);
            CHECK(node.aux.raw.num_visible == 0, "the turned camera still sees %u splats", node.aux.raw.num_visible);
            bh::DeviceBuffer<float> nan4(std::vector<float>(4, std::nanf("")));
            (void)node.backward_intrinsics(v_dev.data(), nan4.data());
            bool zero = true;
            for (float x : nan4.download()) zero = zero && x == 0.0f;
            CHECK(zero, "an empty view did not write four zeros");
            bh::train_set_intrinsics_grad(ctx, nan4.data());
            bh::train_set_intrinsics_grad(ctx, nullptr);
            std::printf("ok intrinsics empty view\n");
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (g_failed) { std::printf("%d C++ intrinsics check(s) FAILED\n", g_failed); return 1; }
    std::printf("all C++ intrinsics checks passed\n");
    return 0;
}
