// test_depth_loss.cpp — depth supervision through the C++ host mirror (include/brush_hip.hpp depth_loss_value_and_grad /
// eval_depth_metrics / train_set_depth; include/brush_hip_depth_loss.h):
//   * the fused loss of a node's expected depth against a perturbed copy, against the header's definitions restated here in
//     double: v_depth (L1: to the bit; disparity: four roundings), the loss within its derived bound, the exact valid count,
//     two calls to the same bits, weight 0 -> zeros, an unknown kind refused;
//   * the metrics against the same restatement;
//   * one bh_train_step with a target: its loss is the step's loss without the target + the hand-composed term, in f32, and the
//     splats move differently; a target of another size is refused and leaves step_count alone.
// Build + run: tests/test_depth_loss_cpp.py.
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

struct Ref { std::vector<float> v; double sum = 0.0, count = 0.0, ar = 0.0, se = 0.0, inl = 0.0; };

// the header's definitions (volatile: every f32 step is rounded to f32, whatever the host compiler would like to fuse)
static Ref restate(const std::vector<float>& e, const std::vector<float>& gt, uint32_t kind, float weight, float scale, float offset) {
    Ref r;
    r.v.assign(e.size(), 0.0f);
    const float c = (float)((double)weight / (double)e.size());
    for (size_t p = 0; p < e.size(); ++p) {
        const float t = std::fmaf(scale, gt[p], offset);
        if (!(std::isfinite(gt[p]) && t > 0.0f && e[p] > 0.0f)) continue;
        volatile float x = kind == BH_DEPTH_LOSS_L1 ? e[p] : 1.0f / e[p];
        volatile float d = x - t;
        const float s = d > 0.0f ? c : (d < 0.0f ? -c : 0.0f);
        if (kind == BH_DEPTH_LOSS_L1) r.v[p] = s;
        else if (d != 0.0f) { volatile float ee = e[p] * e[p]; r.v[p] = -s / ee; }
        r.sum += std::fabs((double)d);
        r.count += 1.0;
        volatile float zt = kind == BH_DEPTH_LOSS_L1 ? t : 1.0f / t;
        const double dz = (double)e[p] - (double)zt;
        r.ar += std::fabs(dz) / (double)zt;
        r.se += dz * dz;
        r.inl += std::fmax((double)e[p] / (double)zt, (double)zt / (double)e[p]) < 1.25 ? 1.0 : 0.0;
    }
    return r;
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
        Sm64 r{0xDE97};
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
        std::vector<float> e, gt(hw);
        {
            bh::RenderNode node(ctx, s, cam, w, h, black);
            e = node.depth(BH_DEPTH_EXPECTED).download();
        }
        size_t covered = 0;
        for (size_t p = 0; p < hw; ++p) { covered += e[p] > 0.0f; gt[p] = e[p] * r.uni(0.8f, 1.25f) + (e[p] > 0.0f ? 0.0f : 3.0f); }
        gt[5] = NAN; gt[6] = INFINITY; gt[7] = 0.0f; gt[8] = -1.0f;
        CHECK(covered > hw / 4, "the frame is almost empty (%zu of %zu)", covered, hw);
        const bh::DeviceBuffer<float> e_dev(e);
        bh::DeviceBuffer<float> v_dev(hw), loss_dev(2), met_dev(4);
        const double eps = std::ldexp(1.0, -24);
        for (uint32_t kind : {BH_DEPTH_LOSS_L1, BH_DEPTH_LOSS_DISPARITY}) {
            std::vector<float> g = gt;
            if (kind == BH_DEPTH_LOSS_DISPARITY) for (auto& x : g) x = 1.0f / x;
            const bh::DeviceBuffer<float> g_dev(g);
            const BhDepthTarget t = bh::depth_target(g_dev.data(), h, w, kind, 0.5f, 0.7f, 0.05f);
            const Ref ref = restate(e, g, kind, 0.5f, 0.7f, 0.05f);
            bh::depth_loss_value_and_grad(ctx, e_dev.data(), t, loss_dev.data(), v_dev.data());
            ctx.sync();
            const std::vector<float> v = v_dev.download(), loss = loss_dev.download();
            double worst = 0.0;
            for (size_t p = 0; p < hw; ++p) worst = std::fmax(worst, std::fabs((double)v[p] - ref.v[p]) / (eps * std::fmax(std::fabs((double)ref.v[p]), 1e-30)));
            if (kind == BH_DEPTH_LOSS_L1) CHECK(same_bits(v, ref.v), "L1 v_depth differs (worst %.2f roundings)", worst);
            else CHECK(worst <= 4.0, "disparity v_depth: %.2f roundings (bound 4)", worst);
            const double want = (double)(float)((double)0.5f / (double)hw) * ref.sum;
            CHECK(ref.count > 0 && loss[1] == (float)ref.count, "valid count %g, reference %g", loss[1], ref.count);
            CHECK(std::fabs(loss[0] - want) <= 2.0 * eps * want, "loss %.9g, reference %.9g", loss[0], want);
            bh::depth_loss_value_and_grad(ctx, e_dev.data(), t, loss_dev.data(), v_dev.data());
            ctx.sync();
            CHECK(same_bits(v_dev.download(), v) && same_bits(loss_dev.download(), loss), "two calls give different bits");
            bh::eval_depth_metrics(ctx, e_dev.data(), t, met_dev.data());
            ctx.sync();
            const std::vector<float> m = met_dev.download();
            CHECK(m[3] == (float)ref.count, "metrics: valid count %g, reference %g", m[3], ref.count);
            CHECK(std::fabs(m[0] - ref.ar / ref.count) <= 4 * eps * m[0] && std::fabs(m[1] - std::sqrt(ref.se / ref.count)) <= 4 * eps * m[1] &&
                      std::fabs(m[2] - ref.inl / ref.count) <= 4 * eps, "metrics %g %g %g", m[0], m[1], m[2]);
            std::printf("ok depth loss kind %u (loss %.6g, %g valid, v_depth within %.2f roundings)\n", kind, loss[0], loss[1], worst);
        }
        const bh::DeviceBuffer<float> gt_dev(gt);
        {
            BhDepthTarget t = bh::depth_target(gt_dev.data(), h, w, BH_DEPTH_LOSS_L1, 0.0f);
            bh::depth_loss_value_and_grad(ctx, e_dev.data(), t, loss_dev.data(), v_dev.data());
            ctx.sync();
            CHECK(same_bits(v_dev.download(), std::vector<float>(hw, 0.0f)) && same_bits(loss_dev.download(), {0.0f, 0.0f}), "weight 0 wrote something");
            t.kind = 2u;
            bool refused = false;
            try { bh::depth_loss_value_and_grad(ctx, e_dev.data(), t, loss_dev.data(), v_dev.data()); } catch (const bh::Error& err) { refused = err.code == BH_ERR_INVALID_ARG; }
            CHECK(refused, "an unknown kind was accepted");
            std::printf("ok depth loss arguments\n");
        }
        // ---- one step with a target ----
        {
            std::vector<uint32_t> img(hw);
            for (auto& px : img) px = 0xFF000000u | (uint32_t)(r.next() & 0xFFFFFFu);
            const bh::DeviceBuffer<uint32_t> img_dev(img);
            bh::SceneBatch batch;
            batch.img_packed = img_dev.data(); batch.img_w = w; batch.img_h = h; batch.camera = cam; batch.view_id = 1;
            bh::TrainConfig cfg;
            cfg.exact_lists = true;
            const float weight = 0.3f;
            const BhDepthTarget t = bh::depth_target(gt_dev.data(), h, w, BH_DEPTH_LOSS_L1, weight);
            bh::depth_loss_value_and_grad(ctx, e_dev.data(), t, loss_dev.data(), nullptr);
            ctx.sync();
            const float term = loss_dev.download()[0];
            bh::Splats a = bh::Splats::from_host(tr, sh, op), b = bh::Splats::from_host(tr, sh, op);
            bh::SplatTrainer plain(ctx, cfg, 3.0f), with(ctx, cfg, 3.0f);
            const bh::TrainStepStats sp = plain.step(batch, a);
            BhDepthTarget bad = t;
            bad.h = h + 1;
            bh::train_set_depth(ctx, &bad);
            bool refused = false;
            try { (void)with.step(batch, b); } catch (const bh::Error& err) { refused = err.code == BH_ERR_INVALID_ARG; }
            CHECK(refused && with.step_count() == 0, "a target of another size was accepted (step_count %u)", with.step_count());
            bh::train_set_depth(ctx, &t);
            const bh::TrainStepStats sw = with.step(batch, b);
            bh::train_set_depth(ctx, nullptr);
            volatile float want = sp.loss + term;
            const float want_f = want;
            CHECK(term > 0.0f && std::memcmp(&sw.loss, &want_f, 4) == 0, "step loss %.9g, image term %.9g + depth term %.9g", sw.loss, sp.loss, term);
            CHECK(!same_bits(a.transforms.download(), b.transforms.download()), "the depth term moved nothing");
            bool finite = true;
            for (float x : b.transforms.download()) finite = finite && std::isfinite(x);
            CHECK(finite, "a step with a target left a non-finite parameter");
            std::printf("ok train step with a depth target (loss %.6g = %.6g + %.6g)\n", sw.loss, sp.loss, term);
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        ++g_failed;
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all C++ depth loss checks passed\n");
    return 0;
}
