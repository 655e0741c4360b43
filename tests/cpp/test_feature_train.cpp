// test_feature_train.cpp — feature fields trained with the splats through the C++ host mirror (include/brush_hip.hpp FeatureField /
// train_set_features / refine_carry_rows / SplatTrainer::refine(.., FeatureField*)):
//   * one step with the term: its loss is the f32 sum (image, then feature) of the hand-composed RenderNode -> features ->
//     feature_loss_value_and_grad / image_loss_value_and_grad, bit for bit; the field moved and its first moments are non-zero; a step
//     with the field detached leaves it alone;
//   * the carry pin: a field whose features AND first moments are the splats' own SH rows goes through SplatTrainer::refine; the
//     carried features are the new sh_coeffs bit for bit, and every carried moment row is either its SH row or all +0, two rows
//     (parent and child) per split.
// Build + run: tests/test_feature_train_cpp.py.
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

// the default camera of brush_amd/synth.py: origin, identity rotation, 60 degrees across, square pixels
static bh::Camera default_camera(uint32_t w, uint32_t h) {
    bh::Camera cam;
    cam.fov_x = 60.0 * 3.14159265358979323846 / 180.0;
    const double fx = (w / 2.0) / std::tan(cam.fov_x / 2.0);
    cam.fov_y = 2.0 * std::atan((h / 2.0) / fx);
    return cam;
}

static bool all_zero_bits(const float* p, size_t n) {
    for (size_t i = 0; i < n; ++i) { uint32_t b; std::memcpy(&b, p + i, 4); if (b) return false; }
    return true;
}

int main() {
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        std::printf("no HIP device: compile-only run\n");
        return 0;
    }
    try {
        bh::Context ctx(0);
        const uint32_t n = 3000, w = 64, h = 48, C = 5;
        const size_t hw = (size_t)w * h;
        Sm64 r{0xFE48};
        std::vector<float> tr((size_t)n * 10), sh((size_t)n * 3), op(n);
        for (uint32_t i = 0; i < n; ++i) {
            float* row = &tr[(size_t)i * 10];
            row[2] = r.uni(2.0f, 12.0f);
            row[0] = r.uni(-0.8f, 0.8f) * row[2]; row[1] = r.uni(-0.5f, 0.5f) * row[2];
            row[3] = 1.0f; row[4] = r.uni(-0.3f, 0.3f); row[5] = r.uni(-0.3f, 0.3f); row[6] = r.uni(-0.3f, 0.3f);
            for (int k = 7; k < 10; ++k) row[k] = r.uni(std::log(0.05f), std::log(0.4f));
            op[i] = i % 7 == 0 ? -7.0f : r.uni(-2.0f, 2.5f);   // (dead splats: the refine below prunes them and splits to refill)
            for (int c = 0; c < 3; ++c) sh[(size_t)i * 3 + c] = r.uni(-1.0f, 1.5f);
        }
        bh::Splats s = bh::Splats::from_host(tr, sh, op);
        const bh::Camera cam = default_camera(w, h);
        std::vector<uint32_t> gt(hw);
        for (size_t p = 0; p < hw; ++p) gt[p] = 0xFF000000u | (uint32_t)((p * 37u) & 0xFFu) | (uint32_t)(((p / w) * 5u) & 0xFFu) << 8 | 0x400000u;
        const bh::DeviceBuffer<uint32_t> gt_dev(gt);
        std::vector<float> target(hw * C);
        for (auto& v : target) v = r.uni(-1.0f, 1.0f);
        const bh::DeviceBuffer<float> target_dev(target);

        bh::TrainConfig cfg;
        cfg.exact_lists = true;
        bh::FeatureField field(n, C, 1e-2f);
        std::vector<float> rows((size_t)n * C);
        for (auto& v : rows) v = r.uni(-1.0f, 1.0f);
        field.features.upload(rows);
        const BhFeatureTarget ft = bh::feature_target(target_dev.data(), h, w, C, BH_FEATURE_LOSS_L1, 1.0f);

        // ---- one step with the term against the hand-composed loss ----
        float want = 0.0f;
        {
            bh::RenderNode node(ctx, s, cam, w, h, cfg.background_color);
            const bh::DeviceBuffer<float> map = node.features(field.features.data(), C);
            bh::DeviceBuffer<float> loss_dev(2);
            bh::feature_loss_value_and_grad(ctx, map.data(), ft, loss_dev.data(), nullptr);
            bh::LossConfig lc;
            lc.l1_weight = 1.0f - cfg.ssim_weight;
            lc.ssim_weight = -cfg.ssim_weight;
            const float l_img = bh::image_loss_value_and_grad(ctx, node.aux.raw.out_img, gt_dev.data(), h, w, lc).first;
            ctx.sync();
            const std::vector<float> fl = loss_dev.download();
            CHECK(fl[0] > 0.0f && fl[1] == (float)hw, "feature loss %g over %g pixels", fl[0], fl[1]);
            want = l_img + fl[0];   // (image) + feature, in f32, in this order
        }
        bh::SplatTrainer trainer(ctx, cfg, 3.0f);
        bh::SceneBatch batch;
        batch.img_packed = gt_dev.data(); batch.img_w = w; batch.img_h = h; batch.camera = cam; batch.view_id = 1;
        bh::train_set_features(ctx, &field, &ft);
        const bh::TrainStepStats st = trainer.step(batch, s);
        field.step += 1;
        CHECK(std::memcmp(&st.loss, &want, 4) == 0, "the step's loss %.9g, hand-composed %.9g", st.loss, want);
        const std::vector<float> moved = field.features.download(), m1 = field.m1.download();
        CHECK(moved != rows && !all_zero_bits(m1.data(), m1.size()), "the step did not update the field");
        bh::train_set_features(ctx, nullptr, nullptr);
        (void)trainer.step(batch, s);
        CHECK(field.features.download() == moved, "a step without the term touched the field");
        bool refused = false;
        try { bh::FeatureField wide(n, BH_FEATURE_MAX_CHANNELS + 1); bh::train_set_features(ctx, &wide, nullptr); } catch (const bh::Error&) { refused = true; }
        CHECK(refused, "257 channels were accepted");
        std::printf("ok feature train step (loss %.9g)\n", st.loss);

        // ---- the carry pin ----
        {
            bh::FeatureField pin(n, 3);
            const std::vector<float> sh_now = s.sh_coeffs.download();
            pin.features.upload(sh_now);
            pin.m1.upload(sh_now);
            refused = false;
            try { bh::refine_carry_rows(ctx, pin.features.data(), pin.m2.data(), 3); } catch (const bh::Error&) { refused = true; }
            CHECK(refused, "a carry without a pending plan was accepted");
            const BhRefineStats rs = trainer.refine(2, s, 99, &pin);
            CHECK(rs.num_pruned > 0 && rs.num_added > 0, "the refine pruned %u and added %u", rs.num_pruned, rs.num_added);
            CHECK(pin.n == rs.total_splats && s.num_splats() == rs.total_splats, "rows %u, splats %u, plan %u", pin.n, s.num_splats(), rs.total_splats);
            const std::vector<float> sh_new = s.sh_coeffs.download(), f = pin.features.download(), m = pin.m1.download();
            CHECK(f.size() == sh_new.size() && std::memcmp(f.data(), sh_new.data(), f.size() * 4) == 0, "the carried features are not the new sh_coeffs");
            size_t zero_rows = 0, other = 0;
            for (uint32_t i = 0; i < rs.total_splats; ++i) {
                if (all_zero_bits(&m[(size_t)i * 3], 3)) ++zero_rows;
                else if (std::memcmp(&m[(size_t)i * 3], &sh_new[(size_t)i * 3], 12) != 0) ++other;
            }
            CHECK(zero_rows == 2 * (size_t)rs.num_added && other == 0, "%zu zero rows for %u splits, %zu rows that are neither", zero_rows, rs.num_added, other);
            std::printf("ok refine carry (pruned %u, added %u)\n", rs.num_pruned, rs.num_added);
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        ++g_failed;
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all C++ feature-train checks passed\n");
    return 0;
}
