// test_normal.cpp — normal maps through the C++ host mirror (include/brush_hip.hpp RenderNode::normal / backward_normal,
// splat_normals, depth_to_normal, depth_to_normal_backward):
//   * the forward: the accumulated map is no longer than the image's alpha (unit splat normals), the unit map is the accumulated one
//     over its length (0 where that is 0), and a pixel's normal is a blend of normals that face the camera;
//   * bit identity: two calls on one saved state, a retained forward after another forward;
//   * the backward: the normal term alone (quaternion gradients arrive, SH and refine weight stay 0), all three terms against the
//     sum of the three, a 3D-filter floor;
//   * normals of a fronto-parallel depth plane are (0, 0, -1) inside and 0 on the border, and their backward repeats bit for bit.
// Build + run: tests/test_normal_cpp.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

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

template <class T>
static std::vector<T> download(const T* dev, size_t n) {
    std::vector<T> out(n);
    bh::hip_check(hipMemcpy(out.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    return out;
}

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0;
}

// the default camera of brush_amd/synth.py: origin, identity rotation, 60 degrees across, square pixels
static bh::Camera default_camera(uint32_t w, uint32_t h) {
    bh::Camera cam;
    cam.fov_x = 60.0 * 3.14159265358979323846 / 180.0;
    const double fx = (w / 2.0) / std::tan(cam.fov_x / 2.0);
    cam.fov_y = 2.0 * std::atan((h / 2.0) / fx);
    return cam;
}

int main() {
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        std::printf("no HIP device: compile-only run\n");
        return 0;
    }
    try {
        bh::Context ctx(0);
        const uint32_t n = 3000, w = 123, h = 82;
        std::vector<float> tr((size_t)n * 10), sh((size_t)n * 3), op(n);
        Sm64 r{0x9A11};
        for (uint32_t i = 0; i < n; ++i) {
            float* row = &tr[(size_t)i * 10];
            row[2] = r.uni(2.0f, 12.0f);
            row[0] = r.uni(-0.6f, 0.6f) * row[2]; row[1] = r.uni(-0.4f, 0.4f) * row[2];
            row[3] = 1.0f; row[4] = r.uni(-0.3f, 0.3f); row[5] = r.uni(-0.3f, 0.3f); row[6] = r.uni(-0.3f, 0.3f);
            for (int k = 7; k < 10; ++k) row[k] = r.uni(std::log(0.03f), std::log(0.3f));
            op[i] = r.uni(-2.0f, 2.5f);
            for (int c = 0; c < 3; ++c) sh[(size_t)i * 3 + c] = r.uni(-1.0f, 1.0f);
        }
        const size_t hw = (size_t)w * h;
        const bh::Splats s = bh::Splats::from_host(tr, sh, op);
        const bh::Camera cam = default_camera(w, h);
        const float black[3] = {0.0f, 0.0f, 0.0f};

        // ---- splat normals: unit length, facing the camera (at the origin: n . mean <= 0) ----
        {
            const std::vector<float> sn = bh::splat_normals(ctx, s, cam).download();
            CHECK(sn.size() == (size_t)n * 3, "splat_normals returned %zu floats", sn.size());
            double worst_len = 0.0;
            size_t away = 0;
            for (uint32_t i = 0; i < n; ++i) {
                const float* v = &sn[(size_t)i * 3];
                const float* m = &tr[(size_t)i * 10];
                worst_len = std::fmax(worst_len, std::fabs(std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]) - 1.0));
                away += ((double)v[0] * m[0] + (double)v[1] * m[1] + (double)v[2] * m[2]) > 0.0;
            }
            CHECK(worst_len <= 1e-6 && away == 0, "splat normals: |len - 1| %.3e, %zu face away", worst_len, away);
            std::printf("ok splat normals\n");
        }
        // ---- the forward ----
        {
            bh::RenderNode node(ctx, s, cam, w, h, black);
            ctx.sync();   // (the node's image is read with a blocking copy, which does not wait for the ctx stream)
            const std::vector<float> img = download(node.aux.raw.out_img, hw * 4);
            const std::vector<float> acc = node.normal(BH_NORMAL_ACCUMULATED).download();
            const std::vector<float> unit = node.normal(BH_NORMAL_UNIT).download();
            CHECK(acc.size() == hw * 3 && unit.size() == hw * 3, "map sizes %zu %zu", acc.size(), unit.size());
            double top = 0.0, over = 0.0, unit_err = 0.0;
            size_t toward = 0, seen = 0;
            for (size_t p = 0; p < hw; ++p) {
                const float* a = &acc[p * 3];
                const double len = std::sqrt((double)a[0] * a[0] + (double)a[1] * a[1] + (double)a[2] * a[2]);
                top = std::fmax(top, len);
                over = std::fmax(over, len - (double)img[p * 4 + 3]);   // |sum of w n| <= sum of w = alpha
                for (int c = 0; c < 3; ++c) {
                    const float lf = std::sqrt(std::fma(a[2], a[2], std::fma(a[1], a[1], a[0] * a[0])));
                    const float want = lf == 0.0f ? 0.0f : a[c] * (1.0f / lf);
                    unit_err = std::fmax(unit_err, std::fabs((double)unit[p * 3 + c] - want));
                }
                if (len > 0.0) { ++seen; toward += a[2] < 0.0f; }
            }
            CHECK(top > 0.5, "the frame is empty (longest normal %g)", top);
            CHECK(over <= 1e-5, "an accumulated normal is longer than its alpha by %.3e", over);
            CHECK(unit_err <= 2e-7, "unit != accumulated / length (%.3e)", unit_err);
            // near the optical axis the camera-facing normals have z < 0; over the frame most blended normals do
            CHECK(seen > hw / 2 && toward * 10 > seen * 6, "%zu of %zu covered pixels face the camera", toward, seen);
            std::printf("ok normal forward (longest %.3f, %zu covered pixels)\n", top, seen);
            // ---- bit identity ----
            CHECK(same_bits(node.normal(BH_NORMAL_ACCUMULATED).download(), acc), "two calls on one saved state differ");
            CHECK(same_bits(node.normal(BH_NORMAL_UNIT).download(), unit), "two calls on one saved state differ (unit)");
            bool refused = false;
            try { (void)node.normal(2u); } catch (const bh::Error&) { refused = true; }
            CHECK(refused, "an unknown mode was accepted");
            bh::RenderNode kept(ctx, s, cam, w, h, black, /*retain=*/true);
            bh::Camera other = cam;
            other.position[0] = 0.8f;
            (void)bh::render_splats(ctx, s, other, w, h, black, bh::RasterPass::Backward);
            CHECK(same_bits(kept.normal(BH_NORMAL_ACCUMULATED).download(), acc), "retained forward: accumulated normals differ");
            CHECK(same_bits(kept.normal(BH_NORMAL_UNIT).download(), unit), "retained forward: unit normals differ");
            refused = false;
            try { (void)node.normal(BH_NORMAL_UNIT); } catch (const bh::Error& e) { refused = std::strstr(e.what(), "stale") != nullptr; }
            CHECK(refused, "a stale node was accepted");
            std::printf("ok normal bit identity\n");

            // ---- the backward (on the retained node) ----
            Sm64 q{0xBAC};
            std::vector<float> vn(hw * 3), vd(hw), vo(hw * 4);
            for (auto& v : vn) v = q.uni(-1.0f, 1.0f) / (float)hw;
            for (auto& v : vd) v = q.uni(-1.0f, 1.0f) / (float)hw;
            for (auto& v : vo) v = q.uni(-1.0f, 1.0f) / (float)hw;
            bh::DeviceBuffer<float> vn_dev(vn), vd_dev(vd), vo_dev(vo);
            for (uint32_t mode : {BH_NORMAL_ACCUMULATED, BH_NORMAL_UNIT}) {
                const bh::SplatGrads gn = kept.backward_normal(vn_dev.data(), mode);
                const bh::SplatGrads gc = kept.backward(vo_dev.data());
                const bh::SplatGrads gd = kept.backward(nullptr, vd_dev.data(), BH_DEPTH_EXPECTED);
                const bh::SplatGrads ga = kept.backward_normal(vo_dev.data(), vd_dev.data(), BH_DEPTH_EXPECTED, vn_dev.data(), mode);
                const std::vector<float> nn = gn.v_transforms.download(), c = gc.v_transforms.download(), d = gd.v_transforms.download(),
                                         a = ga.v_transforms.download();
                double top_q = 0.0, top_a = 0.0, diff = 0.0;
                bool finite = true;
                for (size_t i = 0; i < nn.size(); ++i) {
                    finite = finite && std::isfinite(nn[i]) && std::isfinite(a[i]);
                    if (i % 10 >= 3 && i % 10 < 7) top_q = std::fmax(top_q, std::fabs(nn[i]));
                    top_a = std::fmax(top_a, std::fabs(a[i]));
                    diff = std::fmax(diff, std::fabs((double)a[i] - ((double)c[i] + (double)d[i] + (double)nn[i])));
                }
                CHECK(finite && top_q > 0.0, "mode %u: normal-only quaternion gradient (max %g)", mode, top_q);
                CHECK(diff <= 1e-4 * top_a, "mode %u: three terms differ from the sum of the three by %.3e of %.3e", mode, diff, top_a);
                double rf = 0.0, shg = 0.0;
                for (float v : gn.v_refine_weight.download()) rf = std::fmax(rf, std::fabs(v));
                for (float v : gn.v_sh_coeffs.download()) shg = std::fmax(shg, std::fabs(v));
                CHECK(rf == 0.0 && shg == 0.0, "mode %u: a normal-only backward wrote refine %g / sh %g", mode, rf, shg);
            }
            refused = false;
            try { (void)kept.backward_normal(nullptr, vd_dev.data(), BH_DEPTH_MEDIAN, vn_dev.data()); } catch (const bh::Error&) { refused = true; }
            CHECK(refused, "a median depth term was accepted");
            std::printf("ok normal backward\n");
        }
        // ---- a 3D-filter floor: the fold's chain behind the normal backward ----
        {
            bh::Splats f = bh::Splats::from_host(tr, sh, op, /*render_mip=*/true);
            f.min_scale.emplace(std::vector<float>(n, 0.02f));
            bh::RenderNode node(ctx, f, cam, w, h, black);
            std::vector<float> vn(hw * 3, 1.0f / (float)hw);
            bh::DeviceBuffer<float> vn_dev(vn);
            const bh::SplatGrads g = node.backward_normal(vn_dev.data(), BH_NORMAL_UNIT);
            double top = 0.0;
            bool finite = true;
            for (float v : g.v_transforms.download()) { finite = finite && std::isfinite(v); top = std::fmax(top, std::fabs(v)); }
            for (float v : g.v_raw_opacities.download()) finite = finite && std::isfinite(v);
            CHECK(finite && top > 0.0, "min_scale: gradient max %g", top);
            std::printf("ok normal backward with a 3D-filter floor\n");
        }
        // ---- depth -> normal: a fronto-parallel plane ----
        {
            std::vector<float> depth(hw, 3.0f);
            bh::DeviceBuffer<float> d_dev(depth);
            const std::vector<float> nd = bh::depth_to_normal(ctx, cam, d_dev.data(), h, w).download();
            double err = 0.0;
            size_t border_bad = 0;
            for (uint32_t y = 0; y < h; ++y)
                for (uint32_t x = 0; x < w; ++x) {
                    const float* v = &nd[((size_t)y * w + x) * 3];
                    if (x == 0 || y == 0 || x == w - 1 || y == h - 1) border_bad += v[0] != 0.0f || v[1] != 0.0f || v[2] != 0.0f;
                    else err = std::fmax(err, std::fmax(std::fabs(v[0]), std::fmax(std::fabs(v[1]), std::fabs(v[2] + 1.0f))));
                }
            CHECK(border_bad == 0 && err <= 1e-5, "plane normals: %zu border pixels set, max error %.3e", border_bad, err);
            std::vector<float> vn(hw * 3);
            Sm64 q{0x77};
            for (auto& v : vn) v = q.uni(-1.0f, 1.0f);
            bh::DeviceBuffer<float> vn_dev(vn);
            const std::vector<float> g1 = bh::depth_to_normal_backward(ctx, cam, d_dev.data(), vn_dev.data(), h, w).download();
            const std::vector<float> g2 = bh::depth_to_normal_backward(ctx, cam, d_dev.data(), vn_dev.data(), h, w).download();
            double top = 0.0;
            for (float v : g1) top = std::fmax(top, std::fabs(v));
            CHECK(same_bits(g1, g2) && top > 0.0 && std::isfinite(top), "depth -> normal backward (max %g)", top);
            std::printf("ok depth to normal\n");
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        ++g_failed;
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all C++ normal checks passed\n");
    return 0;
}
