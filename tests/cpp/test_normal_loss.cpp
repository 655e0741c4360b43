// test_normal_loss.cpp — normal consistency through the C++ host mirror (include/brush_hip.hpp normal_consistency_value_and_grad /
// train_set_normal; include/brush_hip_normal_loss.h):
//   * the fused operator on a node's accumulated normals, expected depth and image against the three-call composition it replaces
//     (depth_to_normal, the header's per-pixel arithmetic restated here, depth_to_normal_backward): the exact valid count, v_normal
//     within two roundings, v_depth within 1e-4 of its largest entry, the loss within its derived bound, two calls to the same bits,
//     accumulate = the map plus the overwrite result to the bit, weight 0 -> zeros, a null argument and an aliased output refused;
//   * one bh_train_step with the term: its loss is the step's loss without it + the hand-composed term, in f32, and the splats move
//     differently; with a pose-gradient buffer attached the step is refused and leaves step_count alone.
// Build + run: tests/test_normal_loss_cpp.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
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

int main() {
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        std::printf("no HIP device: compile-only run\n");
        return 0;
    }
    try {
        bh::Context ctx(0);
        const uint32_t n = 1500, w = 37, h = 23;
        const size_t hw = (size_t)w * h;
        Sm64 r{0x6E0A};
        std::vector<float> tr((size_t)n * 10), sh((size_t)n * 3), op(n);
        for (uint32_t i = 0; i < n; ++i) {
            float* row = &tr[(size_t)i * 10];
            row[2] = r.uni(2.0f, 12.0f);
            row[0] = r.uni(-0.35f, 0.35f) * row[2]; row[1] = r.uni(-0.4f, 0.4f) * row[2];   // (the frame's edge columns stay empty)
            row[3] = 1.0f; row[4] = r.uni(-0.3f, 0.3f); row[5] = r.uni(-0.3f, 0.3f); row[6] = r.uni(-0.3f, 0.3f);
            for (int k = 7; k < 10; ++k) row[k] = r.uni(std::log(0.03f), std::log(0.3f));
            op[i] = r.uni(-2.0f, 2.5f);
            for (int c = 0; c < 3; ++c) sh[(size_t)i * 3 + c] = r.uni(0.0f, 2.0f);
        }
        bh::Splats s = bh::Splats::from_host(tr, sh, op);
        const bh::Camera cam = default_camera(w, h);
        const float black[3] = {0.0f, 0.0f, 0.0f};
        std::vector<float> e, nrm, img(hw * 4);
        {
            bh::RenderNode node(ctx, s, cam, w, h, black);
            e = node.depth(BH_DEPTH_EXPECTED).download();
            nrm = node.normal(BH_NORMAL_ACCUMULATED).download();
            ctx.sync();
            if (hipMemcpy(img.data(), node.aux.raw.out_img, hw * 16, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("image copy failed");
        }
        const bh::DeviceBuffer<float> e_dev(e), n_dev(nrm), img_dev(img);
        bh::DeviceBuffer<float> vn_dev(hw * 3), vd_dev(hw), loss_dev(2);
        const double eps = std::ldexp(1.0, -24);
        const float weight = 0.4f;
        const float c = (float)((double)weight / (double)hw);
        // ---- the operator against the composition it replaces ----
        const std::vector<float> u = bh::depth_to_normal(ctx, cam, e_dev.data(), h, w).download();
        std::vector<float> want_vn(hw * 3, 0.0f), v_u(hw * 3, 0.0f);
        double sum = 0.0, count = 0.0;
        for (size_t p = 0; p < hw; ++p) {
            const uint32_t x = (uint32_t)(p % w), y = (uint32_t)(p / w);
            bool valid = x >= 1 && y >= 1 && x + 2 <= w && y + 2 <= h;
            if (valid)
                for (size_t q : {p, p - 1, p + 1, p - w, p + w}) valid = valid && std::isfinite(e[q]) && e[q] > 0.0f;
            if (!valid) continue;
            const float al = img[p * 4 + 3];
            volatile float t0 = nrm[p * 3] * u[p * 3];
            const float d = std::fmaf(nrm[p * 3 + 2], u[p * 3 + 2], std::fmaf(nrm[p * 3 + 1], u[p * 3 + 1], t0));
            volatile float one_minus = 1.0f - d;
            volatile float l = al * one_minus;
            volatile float ca = c * al;
            const float m = -ca;
            for (int k = 0; k < 3; ++k) {
                volatile float a = m * u[p * 3 + k], b = m * nrm[p * 3 + k];
                want_vn[p * 3 + k] = a;
                v_u[p * 3 + k] = b;
            }
            sum += (double)l;
            count += 1.0;
        }
        const bh::DeviceBuffer<float> vu_dev(v_u);
        const std::vector<float> want_vd = bh::depth_to_normal_backward(ctx, cam, e_dev.data(), vu_dev.data(), h, w).download();
        bh::normal_consistency_value_and_grad(ctx, cam, n_dev.data(), e_dev.data(), img_dev.data(), h, w, weight, false, loss_dev.data(), vn_dev.data(), vd_dev.data());
        ctx.sync();
        const std::vector<float> vn = vn_dev.download(), vd = vd_dev.download(), loss = loss_dev.download();
        CHECK(count > hw / 4 && loss[1] == (float)count, "valid count %g, restated %g of %zu", loss[1], count, hw);
        double worst = 0.0, vd_max = 0.0, vd_err = 0.0;
        for (size_t i = 0; i < hw * 3; ++i) worst = std::fmax(worst, std::fabs((double)vn[i] - want_vn[i]) / (eps * std::fmax(std::fabs((double)want_vn[i]), 1e-30)));
        CHECK(worst <= 2.0, "v_normal: %.2f roundings (bound 2)", worst);
        for (size_t p = 0; p < hw; ++p) { vd_max = std::fmax(vd_max, std::fabs((double)want_vd[p])); vd_err = std::fmax(vd_err, std::fabs((double)vd[p] - want_vd[p])); }
        CHECK(vd_max > 0.0 && vd_err <= 1e-4 * vd_max, "v_depth: max error %.3g of %.3g", vd_err, vd_max);
        const double want = (double)c * sum;
        CHECK(std::fabs(loss[0] - want) <= 2.0 * eps * std::fabs(want) + eps * (double)c * count, "loss %.9g, restated %.9g", loss[0], want);
        bh::normal_consistency_value_and_grad(ctx, cam, n_dev.data(), e_dev.data(), img_dev.data(), h, w, weight, false, loss_dev.data(), vn_dev.data(), vd_dev.data());
        ctx.sync();
        CHECK(same_bits(vn_dev.download(), vn) && same_bits(vd_dev.download(), vd) && same_bits(loss_dev.download(), loss), "two calls give different bits");
        std::printf("ok normal loss operator (loss %.6g, %g valid, v_normal within %.2f roundings, v_depth within %.2e of its largest)\n", loss[0], loss[1], worst,
                    vd_err / vd_max);
        // ---- accumulate, no term, refusals ----
        {
            std::vector<float> base(hw), sum_map(hw);
            for (size_t p = 0; p < hw; ++p) { base[p] = r.uni(-1e-3f, 1e-3f); volatile float t = base[p] + vd[p]; sum_map[p] = t; }
            bh::DeviceBuffer<float> acc_dev(base);
            bh::normal_consistency_value_and_grad(ctx, cam, n_dev.data(), e_dev.data(), img_dev.data(), h, w, weight, true, loss_dev.data(), vn_dev.data(), acc_dev.data());
            ctx.sync();
            CHECK(same_bits(acc_dev.download(), sum_map), "accumulate is not the map plus the overwrite result");
            bh::normal_consistency_value_and_grad(ctx, cam, n_dev.data(), e_dev.data(), img_dev.data(), h, w, 0.0f, true, loss_dev.data(), vn_dev.data(), acc_dev.data());
            ctx.sync();
            CHECK(same_bits(acc_dev.download(), sum_map) && same_bits(vn_dev.download(), std::vector<float>(hw * 3, 0.0f)) && same_bits(loss_dev.download(), {0.0f, 0.0f}),
                  "weight 0 under accumulate wrote something");
            bh::normal_consistency_value_and_grad(ctx, cam, n_dev.data(), e_dev.data(), img_dev.data(), h, w, 0.0f, false, loss_dev.data(), vn_dev.data(), vd_dev.data());
            ctx.sync();
            CHECK(same_bits(vd_dev.download(), std::vector<float>(hw, 0.0f)), "weight 0 left a v_depth");
            int refused = 0;
            try { bh::normal_consistency_value_and_grad(ctx, cam, n_dev.data(), e_dev.data(), nullptr, h, w, weight, false, loss_dev.data(), vn_dev.data(), vd_dev.data()); }
            catch (const bh::Error& err) { refused += err.code == BH_ERR_INVALID_ARG; }
            try { bh::normal_consistency_value_and_grad(ctx, cam, n_dev.data(), e_dev.data(), img_dev.data(), h, w, weight, false, loss_dev.data(), vn_dev.data(), const_cast<float*>(e_dev.data())); }
            catch (const bh::Error& err) { refused += err.code == BH_ERR_INVALID_ARG; }
            try { bh::normal_consistency_value_and_grad(ctx, cam, n_dev.data(), e_dev.data(), img_dev.data(), 0, w, weight, false, loss_dev.data(), vn_dev.data(), vd_dev.data()); }
            catch (const bh::Error& err) { refused += err.code == BH_ERR_INVALID_ARG; }
            CHECK(refused == 3, "a null argument, an aliased v_depth or h == 0 was accepted (%d of 3 refused)", refused);
            std::printf("ok normal loss arguments\n");
        }
        // ---- one step with the term ----
        {
            std::vector<uint32_t> gt(hw);
            for (auto& px : gt) px = 0xFF000000u | (uint32_t)(r.next() & 0xFFFFFFu);
            const bh::DeviceBuffer<uint32_t> gt_dev(gt);
            bh::SceneBatch batch;
            batch.img_packed = gt_dev.data(); batch.img_w = w; batch.img_h = h; batch.camera = cam; batch.view_id = 1;
            bh::TrainConfig cfg;
            cfg.exact_lists = true;
            const float term = loss[0];
            bh::Splats a = bh::Splats::from_host(tr, sh, op), b = bh::Splats::from_host(tr, sh, op);
            bh::SplatTrainer plain(ctx, cfg, 3.0f), with(ctx, cfg, 3.0f);
            const bh::TrainStepStats sp = plain.step(batch, a);
            bh::train_set_normal(ctx, weight);
            bh::DeviceBuffer<float> pose(12);
            ctx.check(bh_train_set_pose_grad(ctx.get(), pose.data()));
            bool refused = false;
            try { (void)with.step(batch, b); } catch (const bh::Error& err) { refused = err.code == BH_ERR_INVALID_ARG; }
            ctx.check(bh_train_set_pose_grad(ctx.get(), nullptr));
            CHECK(refused && with.step_count() == 0, "a pose buffer beside the normal term was accepted (step_count %u)", with.step_count());
            const bh::TrainStepStats sw = with.step(batch, b);
            bh::train_set_normal(ctx, nullptr);
            volatile float want_loss = sp.loss + term;
            const float want_f = want_loss;
            CHECK(term > 0.0f && std::memcmp(&sw.loss, &want_f, 4) == 0, "step loss %.9g, image term %.9g + normal term %.9g", sw.loss, sp.loss, term);
            CHECK(!same_bits(a.transforms.download(), b.transforms.download()), "the normal term moved nothing");
            bool finite = true;
            for (float x : b.transforms.download()) finite = finite && std::isfinite(x);
            CHECK(finite, "a step with the term left a non-finite parameter");
            std::printf("ok train step with a normal term (loss %.6g = %.6g + %.6g)\n", sw.loss, sp.loss, term);
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        ++g_failed;
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all C++ normal loss checks passed\n");
    return 0;
}
