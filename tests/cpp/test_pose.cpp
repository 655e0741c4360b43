// test_pose.cpp — camera pose gradients through the C++ host mirror (include/brush_hip.hpp RenderNode::backward_pose,
// train_set_pose_grad, pose_twist, camera_apply_twist):
//   * host arithmetic (no device needed): a zero twist is the identity, a twist leaves W orthonormal and cam_pos = -W^T t, pose_twist
//     of a pure translation gradient is (t x v_t, v_t);
//   * on the GPU: backward_pose's splat outputs are backward's bits on a retained forward rendered twice (v_output in one tile), the
//     twelve repeat bit for bit, v_t = W sum v_mean within 1e-4 of its L1 mass, and an empty view overwrites NaN with zeros.
// Build + run: tests/test_pose_cpp.py.
#include <cmath>
#include <cstdio>
#include <cstring>

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

static void host_checks(uint32_t w, uint32_t h) {
    const BhCamera base = default_camera(w, h).uniforms(w, h);
    BhCamera cam = base;
    bh::camera_apply_twist(cam, {0, 0, 0, 0, 0, 0});
    CHECK(std::memcmp(&cam, &base, sizeof cam) == 0, "a zero twist changed the camera");
    bh::camera_apply_twist(cam, {0.03, -0.02, 0.05, 0.2, -0.1, 0.15});
    double worst = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double d = 0.0;
            for (int i = 0; i < 3; ++i) d += (double)cam.vm[3 * a + i] * cam.vm[3 * b + i];
            worst = std::fmax(worst, std::fabs(d - (a == b ? 1.0 : 0.0)));
        }
    CHECK(worst <= 4 * std::ldexp(1.0, -24), "W is not orthonormal after a twist (%.3e)", worst);
    for (int j = 0; j < 3; ++j) {
        double p = 0.0;
        for (int i = 0; i < 3; ++i) p -= (double)cam.vm[3 * j + i] * cam.vm[9 + i];
        CHECK(std::fabs(p - cam.cam_pos[j]) <= 1e-6, "cam_pos[%d] %g is not -W^T t = %g", j, cam.cam_pos[j], p);
    }
    CHECK(cam.fx == base.fx && cam.img_w == base.img_w && cam.model == base.model, "apply_twist touched another field");
    float v[12] = {0};
    v[9] = 0.5f; v[10] = -1.0f; v[11] = 2.0f;
    const std::array<double, 6> tw = bh::pose_twist(cam.vm, v);
    const double t[3] = {cam.vm[9], cam.vm[10], cam.vm[11]};
    CHECK(std::fabs(tw[0] - (t[1] * 2.0 - t[2] * -1.0)) <= 1e-12 && std::fabs(tw[1] - (t[2] * 0.5 - t[0] * 2.0)) <= 1e-12 &&
              std::fabs(tw[2] - (t[0] * -1.0 - t[1] * 0.5)) <= 1e-12 && tw[3] == 0.5 && tw[4] == -1.0 && tw[5] == 2.0,
          "pose_twist of a translation gradient");
    std::printf("ok pose host arithmetic\n");
}

int main() {
    const uint32_t n = 3000, w = 123, h = 82;
    try {
        host_checks(w, h);
        int dev_count = 0;
        if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
            std::printf("no HIP device: host checks only\n");
            return g_failed ? 1 : 0;
        }
        bh::Context ctx(0);
        Sm64 r{0x9053};
        std::vector<float> tr((size_t)n * 10), sh((size_t)n * 4 * 3), op(n);
        for (uint32_t i = 0; i < n; ++i) {
            float* row = &tr[(size_t)i * 10];
            row[2] = r.uni(2.0f, 9.0f);
            row[0] = r.uni(-0.6f, 0.6f) * row[2]; row[1] = r.uni(-0.4f, 0.4f) * row[2];
            row[3] = 1.0f; row[4] = r.uni(-0.3f, 0.3f); row[5] = r.uni(-0.3f, 0.3f); row[6] = r.uni(-0.3f, 0.3f);
            for (int k = 7; k < 10; ++k) row[k] = r.uni(std::log(0.02f), std::log(0.2f));
            op[i] = r.uni(-2.0f, 2.5f);
            for (int c = 0; c < 12; ++c) sh[(size_t)i * 12 + c] = r.uni(-0.5f, 0.5f);
        }
        const bh::Splats s = bh::Splats::from_host(tr, sh, op);
        const bh::Camera cam = default_camera(w, h);
        const float black[3] = {0.0f, 0.0f, 0.0f};
        // v_output confined to one tile: every splat gets one addition, so the backward repeats itself bit for bit
        std::vector<float> v((size_t)w * h * 4, 0.0f);
        for (uint32_t y = 16; y < 32; ++y)
            for (uint32_t x = 32; x < 48; ++x)
                for (int c = 0; c < 4; ++c) v[((size_t)y * w + x) * 4 + c] = r.uni(-1.0f, 1.0f) / (float)(w * h);
        const bh::DeviceBuffer<float> v_dev(v);
        bh::DeviceBuffer<float> vv(12), vv2(12);
        {
            bh::RenderNode a(ctx, s, cam, w, h, black, /*retain=*/true), b(ctx, s, cam, w, h, black, /*retain=*/true);
            const bh::SplatGrads plain = a.backward(v_dev.data());
            const bh::SplatGrads posed = b.backward_pose(v_dev.data(), vv.data());
            (void)b.backward_pose(v_dev.data(), vv2.data());
            CHECK(same_bits(plain.v_transforms.download(), posed.v_transforms.download()) && same_bits(plain.v_sh_coeffs.download(), posed.v_sh_coeffs.download()) &&
                      same_bits(plain.v_raw_opacities.download(), posed.v_raw_opacities.download()) &&
                      same_bits(plain.v_refine_weight.download(), posed.v_refine_weight.download()),
                  "the splat outputs of backward_pose are not backward's");
            const std::vector<float> g = vv.download(), vt = posed.v_transforms.download();
            CHECK(same_bits(g, vv2.download()), "two calls on one retained forward give different v_viewmat bits");
            // W = I for this camera: v_t = sum v_mean, within 1e-4 of the L1 mass of the summands
            double top = 0.0;
            for (int k = 0; k < 3; ++k) {
                double sum = 0.0, mass = 0.0;
                for (uint32_t i = 0; i < n; ++i) { sum += vt[(size_t)i * 10 + k]; mass += std::fabs(vt[(size_t)i * 10 + k]); }
                CHECK(std::fabs(g[9 + k] - sum) <= 1e-4 * mass, "v_t[%d] = %.9g, sum v_mean = %.9g (mass %.3e)", k, g[9 + k], sum, mass);
                top = std::fmax(top, std::fabs(sum));
            }
            CHECK(top > 0.0, "the gradient is empty");
            std::printf("ok pose backward (v_t %.6g %.6g %.6g)\n", g[9], g[10], g[11]);
        }
        {
            // turned away from the scene: nothing visible, twelve zeros over NaN
            bh::Camera away = cam;
            away.rotation[0] = 0.0f; away.rotation[1] = 1.0f; away.rotation[2] = 0.0f; away.rotation[3] = 0.0f;
            bh::RenderNode node(ctx, s, away, w, h, black);
            CHECK(node.aux.raw.num_visible == 0, "the turned camera still sees %u splats", node.aux.raw.num_visible);
            bh::DeviceBuffer<float> nan12(std::vector<float>(12, std::nanf("")));
            (void)node.backward_pose(v_dev.data(), nan12.data());
            const std::vector<float> z = nan12.download();
            bool zero = true;
            for (float x : z) zero = zero && x == 0.0f;
            CHECK(zero, "an empty view did not write twelve zeros");
            bh::train_set_pose_grad(ctx, nan12.data());
            bh::train_set_pose_grad(ctx, nullptr);
            std::printf("ok pose empty view\n");
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (g_failed) { std::printf("%d C++ pose check(s) FAILED\n", g_failed); return 1; }
    std::printf("all C++ pose checks passed\n");
    return 0;
}
