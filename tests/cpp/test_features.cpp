// test_features.cpp — feature maps through the C++ host mirror (include/brush_hip.hpp RenderNode::features / backward_features,
// brush_hip::feature_loss_value_and_grad):
//   * bit identity with the colour image: a degree-0 scene over black, features = the projected rgb of the listed splats, alone
//     and as the first three of 19 channels; two calls; a retained forward after another forward; a stale node is refused;
//   * one backward: the feature-only backward of those features with v_map = v_output[..., :3] against the colour-only backward
//     (2e-4 of the block's maximum), v_features finite and non-zero, rows of unlisted splats 0;
//   * one loss: cross-entropy of the 19-channel map against labels with an ignored block, value and count against a double
//     restatement here, the gradient's rows summing to 0.
// Build + run: tests/test_features_cpp.py.
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

// the default camera of brush_amd/synth.py: origin, identity rotation, 60 degrees across, square pixels
static bh::Camera default_camera(uint32_t w, uint32_t h) {
    bh::Camera cam;
    cam.fov_x = 60.0 * 3.14159265358979323846 / 180.0;
    const double fx = (w / 2.0) / std::tan(cam.fov_x / 2.0);
    cam.fov_y = 2.0 * std::atan((h / 2.0) / fx);
    return cam;
}

// rows [n, c]: the projected rgb of the listed splats in the first three channels, noise elsewhere
static std::vector<float> colour_rows(const bh::RenderNode& node, uint32_t n, uint32_t c, std::vector<char>* listed) {
    const uint32_t nl = node.aux.raw.num_listed_splats;
    const std::vector<float> proj = download(node.aux.raw.projected, (size_t)nl * 9);
    const std::vector<uint32_t> gid = download(node.aux.raw.global_from_compact_gid, nl);
    Sm64 r{0xFEA7 + c};
    std::vector<float> f((size_t)n * c);
    for (auto& v : f) v = r.uni(-2.0f, 2.0f);
    listed->assign(n, 0);
    for (uint32_t i = 0; i < nl; ++i) {
        (*listed)[gid[i]] = 1;
        for (int k = 0; k < 3; ++k) f[(size_t)gid[i] * c + k] = proj[(size_t)i * 9 + 6 + k];
    }
    return f;
}

static size_t rgb_mismatches(const std::vector<float>& map, uint32_t c, const std::vector<float>& img, size_t hw) {
    size_t bad = 0;
    for (size_t p = 0; p < hw; ++p)
        for (int k = 0; k < 3; ++k) bad += std::memcmp(&map[p * c + k], &img[p * 4 + k], 4) != 0;
    return bad;
}

int main() {
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        std::printf("no HIP device: compile-only run\n");
        return 0;
    }
    try {
        bh::Context ctx(0);
        const uint32_t n = 3000, w = 123, h = 82, C = 19;
        const size_t hw = (size_t)w * h;
        Sm64 r{0xFE47};
        std::vector<float> tr((size_t)n * 10), sh((size_t)n * 3), op(n);
        for (uint32_t i = 0; i < n; ++i) {
            float* row = &tr[(size_t)i * 10];
            row[2] = r.uni(2.0f, 12.0f);
            row[0] = r.uni(-0.8f, 0.8f) * row[2]; row[1] = r.uni(-0.5f, 0.5f) * row[2];   // (some fall outside the frame)
            row[3] = 1.0f; row[4] = r.uni(-0.3f, 0.3f); row[5] = r.uni(-0.3f, 0.3f); row[6] = r.uni(-0.3f, 0.3f);
            for (int k = 7; k < 10; ++k) row[k] = r.uni(std::log(0.03f), std::log(0.3f));
            op[i] = r.uni(-2.0f, 2.5f);
            for (int c = 0; c < 3; ++c) sh[(size_t)i * 3 + c] = r.uni(-1.0f, 1.5f);
        }
        const bh::Splats s = bh::Splats::from_host(tr, sh, op);
        const bh::Camera cam = default_camera(w, h);
        const float black[3] = {0.0f, 0.0f, 0.0f};

        bh::RenderNode node(ctx, s, cam, w, h, black, /*retain=*/true);
        ctx.sync();
        const std::vector<float> img = download(node.aux.raw.out_img, hw * 4);
        std::vector<char> listed;
        const std::vector<float> f3 = colour_rows(node, n, 3, &listed), f19 = colour_rows(node, n, C, &listed);
        const bh::DeviceBuffer<float> f3_dev(f3), f19_dev(f19);
        // ---- bit identity with the colour image ----
        const std::vector<float> m3 = node.features(f3_dev.data(), 3).download();
        const std::vector<float> m19 = node.features(f19_dev.data(), C).download();
        float top = 0.0f;
        for (size_t p = 0; p < hw; ++p) top = std::fmax(top, img[p * 4]);
        CHECK(top > 0.1f, "the frame is empty (max red %g)", top);
        CHECK(rgb_mismatches(m3, 3, img, hw) == 0, "3 channels: %zu values differ from the colour image", rgb_mismatches(m3, 3, img, hw));
        CHECK(rgb_mismatches(m19, C, img, hw) == 0, "19 channels: %zu values differ from the colour image", rgb_mismatches(m19, C, img, hw));
        CHECK(node.features(f19_dev.data(), C).download() == m19, "two calls on one saved state differ");
        bh::Camera other = cam;
        other.position[0] = 0.8f;
        (void)bh::render_splats(ctx, s, other, w, h, black, bh::RasterPass::Backward);
        CHECK(node.features(f19_dev.data(), C).download() == m19, "retained forward: the map differs");
        bool refused = false;
        try { (void)node.features(f3_dev.data(), 0); } catch (const bh::Error&) { refused = true; }
        CHECK(refused, "0 channels were accepted");
        refused = false;
        try { (void)node.features(f3_dev.data(), BH_FEATURE_MAX_CHANNELS + 1); } catch (const bh::Error&) { refused = true; }
        CHECK(refused, "257 channels were accepted");
        {
            bh::RenderNode loose(ctx, s, cam, w, h, black);
            (void)bh::render_splats(ctx, s, other, w, h, black, bh::RasterPass::Backward);
            refused = false;
            try { (void)loose.features(f3_dev.data(), 3); } catch (const bh::Error& e) { refused = std::strstr(e.what(), "stale") != nullptr; }
            CHECK(refused, "a stale node was accepted");
        }
        std::printf("ok feature bit identity\n");

        // ---- one backward ----
        {
            Sm64 q{0xBAC};
            std::vector<float> vo(hw * 4, 0.0f), vm(hw * 3);
            for (size_t p = 0; p < hw; ++p)
                for (int k = 0; k < 3; ++k) vo[p * 4 + k] = vm[p * 3 + k] = q.uni(-1.0f, 1.0f) / (float)hw;
            const bh::DeviceBuffer<float> vo_dev(vo), vm_dev(vm);
            bh::DeviceBuffer<float> vf_dev;
            const bh::SplatGrads gc = node.backward(vo_dev.data());
            const bh::SplatGrads gf = node.backward_features(nullptr, f3_dev.data(), 3, vm_dev.data(), vf_dev);
            const std::vector<float> a = gf.v_transforms.download(), b = gc.v_transforms.download();
            double diff = 0.0, mag = 0.0;
            bool finite = true;
            for (size_t i = 0; i < a.size(); ++i) {
                finite = finite && std::isfinite(a[i]);
                diff = std::fmax(diff, std::fabs((double)a[i] - (double)b[i]));
                mag = std::fmax(mag, std::fabs((double)b[i]));
            }
            CHECK(finite && mag > 0.0 && diff <= 2e-4 * mag, "feature-only v_transforms differ from the colour backward's by %.3e of %.3e", diff, mag);
            const std::vector<float> vf = vf_dev.download();
            CHECK(vf.size() == (size_t)n * 3, "v_features has %zu floats", vf.size());
            double vtop = 0.0;
            size_t stray = 0, unlisted = 0;
            for (uint32_t i = 0; i < n; ++i)
                for (int k = 0; k < 3; ++k) {
                    const float v = vf[(size_t)i * 3 + k];
                    finite = finite && std::isfinite(v);
                    vtop = std::fmax(vtop, std::fabs(v));
                    if (!listed[i]) { ++unlisted; uint32_t bits; std::memcpy(&bits, &v, 4); stray += bits != 0u; }
                }
            CHECK(finite && vtop > 0.0, "v_features (max %g)", vtop);
            CHECK(unlisted > 0 && stray == 0, "%zu of %zu values of unlisted splats are not +0", stray, unlisted);
            double rf = 0.0, shg = 0.0;
            for (float v : gf.v_refine_weight.download()) rf = std::fmax(rf, std::fabs(v));
            for (float v : gf.v_sh_coeffs.download()) shg = std::fmax(shg, std::fabs(v));
            CHECK(rf == 0.0 && shg == 0.0, "a feature-only backward wrote refine %g / sh %g", rf, shg);
            std::printf("ok feature backward (v_transforms within %.3e of the colour backward's maximum)\n", diff / mag);
        }

        // ---- one loss ----
        {
            std::vector<uint8_t> lab(hw);
            Sm64 q{0x1AB};
            for (size_t p = 0; p < hw; ++p) lab[p] = (uint8_t)(q.next() % C);
            for (size_t p = 0; p < 40; ++p) lab[p] = p % 2 ? 255 : (uint8_t)C;
            const float weight = 0.5f;
            double sum = 0.0, count = 0.0;
            for (size_t p = 0; p < hw; ++p) {
                if (lab[p] >= C) continue;
                const float* F = &m19[p * C];
                double m = F[0], se = 0.0;
                for (uint32_t c = 1; c < C; ++c) m = std::fmax(m, (double)F[c]);
                for (uint32_t c = 0; c < C; ++c) se += std::exp((double)F[c] - m);
                sum += std::log(se) + (m - (double)F[lab[p]]);
                count += 1.0;
            }
            const double want = (double)weight / (double)hw * sum;
            const bh::DeviceBuffer<float> map_dev(m19);
            const bh::DeviceBuffer<uint8_t> lab_dev(lab);
            bh::DeviceBuffer<float> loss_dev, v_dev;
            loss_dev.resize(2);
            v_dev.resize(hw * C);
            bh::feature_loss_value_and_grad(ctx, map_dev.data(), bh::feature_target(lab_dev.data(), h, w, C, BH_FEATURE_LOSS_CROSS_ENTROPY, weight), loss_dev.data(),
                                            v_dev.data());
            ctx.sync();
            const std::vector<float> loss = loss_dev.download(), v = v_dev.download();
            CHECK(std::fabs((double)loss[0] - want) <= 1e-6 * want, "loss %.9g, restatement %.9g", loss[0], want);
            CHECK((double)loss[1] == count, "count %g, restatement %g", loss[1], count);
            double worst = 0.0, vtop = 0.0;
            size_t stray = 0;
            for (size_t p = 0; p < hw; ++p) {
                double row = 0.0;
                for (uint32_t c = 0; c < C; ++c) { row += v[p * C + c]; vtop = std::fmax(vtop, std::fabs(v[p * C + c])); if (lab[p] >= C) stray += v[p * C + c] != 0.0f; }
                worst = std::fmax(worst, std::fabs(row));
            }
            CHECK(vtop > 0.0 && worst <= 1e-6 * vtop && stray == 0, "gradient rows sum to %.3e of %.3e, %zu values at ignored pixels", worst, vtop, stray);
            std::printf("ok feature loss (%.9g against %.9g)\n", loss[0], want);
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        ++g_failed;
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all C++ feature checks passed\n");
    return 0;
}
