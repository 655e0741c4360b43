// test_eval.cpp — held-out evaluation through the C++ host mirror (include/brush_hip.hpp):
//   * eval_metrics of a random image (values in [-0.1, 1.2]) against a random GT: mse from a host restatement of the quantise and the
//     L1 map, ssim from the device SSIM map of the host-quantised image (image_loss, l1 0, ssim 1), psnr from the f32 formula; the
//     rgb8 copy exactly clip(rint(x * 255), 0, 255);
//   * eval_stats of a small scene equals eval_metrics of render_splats(Backward, black) bit for bit;
//   * run_eval over loader views equals eval_stats per view, averaged in f32.
// Build + run: tests/test_eval_cpp.py.
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

static bool within_ulp(float got, float want) {
    return std::fabs((double)got - (double)want) <= (double)(std::nextafter(std::fabs(want), INFINITY) - std::fabs(want));
}

static void test_metrics(const bh::Context& ctx) {
    const uint32_t h = 45, w = 70;
    const size_t hw = (size_t)h * w;
    Sm64 r{0xE7A1};
    std::vector<float> img(hw * 4);
    for (auto& v : img) v = r.uni(-0.1f, 1.2f);
    std::vector<uint32_t> gt(hw);
    for (auto& p : gt) p = (uint32_t)r.next();
    // host: q = rint(x * 255) / 255, g = byte * (1/255), the squared L1 map summed in f64; q goes to the device as CHW for the SSIM map
    std::vector<float> q_chw(hw * 3);
    std::vector<uint32_t> want_rgb8(hw);
    double sq = 0.0;
    for (size_t p = 0; p < hw; ++p) {
        uint32_t packed = 0xFF000000u;
        for (uint32_t c = 0; c < 3; ++c) {
            const float k = std::rint(img[p * 4 + c] * 255.0f);
            const float q = k / 255.0f;
            const float g = (float)((gt[p] >> (8 * c)) & 0xFFu) * (1.0f / 255.0f);
            const float d = std::fabs(q - g);
            sq += (double)(d * d);
            q_chw[c * hw + p] = q;
            packed |= (uint32_t)std::fmin(std::fmax(k, 0.0f), 255.0f) << (8 * c);
        }
        want_rgb8[p] = packed;
    }
    const float want_mse = (float)(sq / (double)(hw * 3));
    bh::DeviceBuffer<float> img_dev(img), q_dev(q_chw), metrics(3);
    bh::DeviceBuffer<uint32_t> gt_dev(gt), rgb8(hw);
    bh::LossConfig ssim_only;
    ssim_only.l1_weight = 0.0f;
    ssim_only.ssim_weight = 1.0f;
    const std::vector<float> ssim_map = bh::image_loss(ctx, q_dev.data(), gt_dev.data(), 3, h, w, ssim_only).download();
    double ss = 0.0;
    for (float v : ssim_map) ss += (double)v;
    const float want_ssim = (float)(ss / (double)(hw * 3));
    bh::eval_metrics(ctx, img_dev.data(), gt_dev.data(), h, w, metrics.data(), rgb8.data());
    ctx.sync();
    const std::vector<float> m = metrics.download();
    const float want_psnr = std::log(1.0f / m[0]) * 10.0f / 2.30258509299404568402f;
    CHECK(within_ulp(m[0], want_mse), "mse %.9g vs %.9g", m[0], want_mse);
    CHECK(within_ulp(m[2], want_ssim), "ssim %.9g vs %.9g", m[2], want_ssim);
    CHECK(std::fabs(m[1] - want_psnr) <= 1e-6f * std::fabs(want_psnr), "psnr %.9g vs %.9g", m[1], want_psnr);
    CHECK(rgb8.download() == want_rgb8, "rgb8 copy differs from clip(rint(x * 255), 0, 255)");
    std::printf("ok eval_metrics (mse %.6g psnr %.4f ssim %.6f)\n", m[0], m[1], m[2]);
}

static bh::Splats small_scene(uint32_t n) {
    Sm64 r{0x5CE7E};
    std::vector<float> tr((size_t)n * 10), sh((size_t)n * 4 * 3), op(n);
    for (uint32_t i = 0; i < n; ++i) {
        float* row = &tr[(size_t)i * 10];
        row[0] = r.uni(-1.5f, 1.5f); row[1] = r.uni(-1.0f, 1.0f); row[2] = r.uni(2.0f, 5.0f);
        row[3] = 1.0f; row[4] = r.uni(-0.3f, 0.3f); row[5] = r.uni(-0.3f, 0.3f); row[6] = r.uni(-0.3f, 0.3f);
        for (int k = 7; k < 10; ++k) row[k] = r.uni(std::log(0.02f), std::log(0.15f));
        op[i] = r.uni(-1.0f, 2.0f);
    }
    for (auto& v : sh) v = r.uni(-0.6f, 0.6f);
    return bh::Splats::from_host(tr, sh, op);
}

static bh::Camera turned(float yaw) {
    bh::Camera cam;
    cam.fov_x = 1.0;
    cam.fov_y = 0.75;
    cam.rotation[1] = std::sin(yaw / 2);
    cam.rotation[3] = std::cos(yaw / 2);
    return cam;
}

static void test_view(const bh::Context& ctx) {
    const uint32_t w = 88, h = 60;
    bh::Splats s = small_scene(2000);
    Sm64 r{0x6EE};
    std::vector<uint32_t> gt((size_t)w * h);
    for (auto& p : gt) p = (uint32_t)(r.next() & 0x00FFFFFFu) | 0xFF000000u;
    bh::DeviceBuffer<uint32_t> gt_dev(gt);
    const float black[3] = {0.0f, 0.0f, 0.0f};
    for (int v = 0; v < 3; ++v) {
        const bh::Camera cam = turned(0.05f * (float)(v - 1));
        const bh::EvalSample es = bh::eval_stats(ctx, s, cam, gt_dev.data(), w, h, true);
        const bh::RenderAux aux = bh::render_splats(ctx, s, cam, w, h, black, bh::RasterPass::Backward);
        bh::DeviceBuffer<float> m(3);
        bh::DeviceBuffer<uint32_t> rgb8((size_t)w * h);
        bh::eval_metrics(ctx, aux.raw.out_img, gt_dev.data(), h, w, m.data(), rgb8.data());
        ctx.sync();
        const std::vector<float> mm = m.download();
        CHECK(std::memcmp(mm.data(), &es.mse, 4) == 0 && std::memcmp(mm.data() + 1, &es.psnr, 4) == 0 && std::memcmp(mm.data() + 2, &es.ssim, 4) == 0,
              "view %d: eval_stats (%.9g %.9g %.9g) vs render + eval_metrics (%.9g %.9g %.9g)", v, es.mse, es.psnr, es.ssim, mm[0], mm[1], mm[2]);
        CHECK(es.image && es.image->download() == rgb8.download(), "view %d: rgb8 copies differ", v);
        CHECK(std::isfinite(es.psnr) && es.psnr > 3.0f && es.ssim > -1.0f && es.ssim < 1.0f, "view %d: psnr %g ssim %g", v, es.psnr, es.ssim);
    }
    std::printf("ok eval_view\n");

    // run_eval over loader views: RGBA and RGB, two sizes
    std::vector<bh::LoaderView> views;
    for (int v = 0; v < 3; ++v) {
        bh::LoaderView lv;
        lv.w = v == 2 ? 64 : w;
        lv.h = v == 2 ? 48 : h;
        lv.channels = v == 1 ? 3 : 4;
        lv.camera = turned(0.04f * (float)v);
        const uint32_t vw = lv.w, vh = lv.h, ch = lv.channels, seed = 100 + v;
        lv.decode = [vw, vh, ch, seed](uint8_t* dst) {
            Sm64 g{seed};
            for (size_t i = 0; i < (size_t)vw * vh * ch; ++i) dst[i] = (ch == 4 && i % 4 == 3) ? 255 : (uint8_t)(g.next() & 0xFF);
        };
        views.push_back(lv);
    }
    const bh::EvalResult res = bh::run_eval(ctx, s, views, true);
    CHECK(res.per_view.size() == views.size() && res.images.size() == views.size(), "run_eval: %zu rows", res.per_view.size());
    float psnr = 0.0f, ssim = 0.0f;
    for (size_t v = 0; v < views.size(); ++v) {
        const bh::LoaderView& lv = views[v];
        std::vector<uint8_t> px((size_t)lv.w * lv.h * lv.channels);
        lv.decode(px.data());
        bh::BatchUploader up(ctx, (uint64_t)lv.w * lv.h, 2);
        const int slot = up.submit(px.data(), lv.w, lv.h, lv.channels, true);
        const bh::BatchUploader::Packed p = up.acquire(slot);
        const bh::EvalSample es = bh::eval_stats(ctx, s, lv.camera, p.img, lv.w, lv.h, true);
        up.release(slot);
        CHECK(res.per_view[v][0] == es.mse && res.per_view[v][1] == es.psnr && res.per_view[v][2] == es.ssim, "run_eval row %zu differs from eval_stats", v);
        CHECK(res.images[v].download() == es.image->download(), "run_eval image %zu differs", v);
        psnr += es.psnr;
        ssim += es.ssim;
    }
    CHECK(res.avg_psnr == psnr / 3.0f && res.avg_ssim == ssim / 3.0f, "averages %g %g vs %g %g", res.avg_psnr, res.avg_ssim, psnr / 3.0f, ssim / 3.0f);
    std::printf("ok run_eval (avg psnr %.4f ssim %.6f)\n", res.avg_psnr, res.avg_ssim);
}

int main() {
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        std::printf("no HIP device: compile-only run\n");
        return 0;
    }
    try {
        bh::Context ctx(0);
        test_metrics(ctx);
        test_view(ctx);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        ++g_failed;
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all C++ eval checks passed\n");
    return 0;
}
