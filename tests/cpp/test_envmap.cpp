// test_envmap.cpp — environment maps through the C++ host mirror (include/brush_hip.hpp EnvironmentMap, train_set_envmap):
//   * without a device: the surface compiles and links, and a null context is refused before the device is touched;
//   * on the GPU: a new map is black (composite and backward return their input bit for bit), a map of one colour c gives
//     img + (1 - A) c within the roundings of the bilinear weights, the table's gradient sums to the frame's sum of (1 - A) v, two runs
//     give the same bits, one Adam step at t = 1 moves every texel some pixel reaches by lr against the sign of its gradient and
//     leaves every other texel's bits, a checkpointed map resumes to the same bits, and a fisheye camera is refused.
// Build + run: tests/test_envmap_cpp.py.
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

static void host_checks() {
    bh_envmap* m = nullptr;
    CHECK(bh_envmap_create(nullptr, 8, &m) == BH_ERR_INVALID_ARG && m == nullptr, "create took a null context");
    CHECK(bh_envmap_destroy(nullptr, nullptr) == BH_ERR_INVALID_ARG, "destroy took a null context");
    CHECK(bh_envmap_set_adam(nullptr, nullptr, 1e-3, 0.9, 0.999, 1e-15) == BH_ERR_INVALID_ARG, "set_adam took a null context");
    CHECK(bh_envmap_composite(nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr) == BH_ERR_INVALID_ARG, "composite took a null context");
    CHECK(bh_envmap_backward(nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, 0) == BH_ERR_INVALID_ARG, "backward took a null context");
    CHECK(bh_train_set_envmap(nullptr, nullptr) == BH_ERR_INVALID_ARG, "train_set_envmap took a null context");
    std::printf("ok envmap host checks\n");
}

int main() {
    const uint32_t w = 61, h = 45, px = w * h, res = 4;
    const double eps = std::ldexp(1.0, -24), lr = 0.01;
    try {
        host_checks();
        int dev_count = 0;
        if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
            std::printf("no HIP device: host checks only\n");
            return g_failed ? 1 : 0;
        }
        bh::Context ctx(0);
        BhCamera cam{};
        const float pos[3] = {0.0f, 0.0f, 0.0f}, rot[4] = {0.2f, -0.3f, 0.1f, 0.9f};   // (normalised below)
        const float rn = std::sqrt(rot[0] * rot[0] + rot[1] * rot[1] + rot[2] * rot[2] + rot[3] * rot[3]);
        const float rot_n[4] = {rot[0] / rn, rot[1] / rn, rot[2] / rn, rot[3] / rn};
        CHECK(bh_camera_setup(pos, rot_n, 1.6, 1.3, 0.5f, 0.5f, w, h, &cam) == 0, "camera setup");
        Sm64 r{0xE47A9};
        std::vector<float> x((size_t)px * 4), v((size_t)px * 4);
        for (auto& e : x) e = r.uni(0.0f, 1.0f);
        for (uint32_t p = 0; p < px; p += 3) x[4 * p + 3] = 1.0f;   // a third of the pixels is covered
        for (auto& e : v) e = r.uni(-1.0f, 1.0f) + 0.25f;
        const bh::DeviceBuffer<float> x_dev(x), v_dev(v);
        bh::DeviceBuffer<float> y_dev((size_t)px * 4), g_dev((size_t)px * 4);
        {
            bh::EnvironmentMap map(ctx, res, lr);
            CHECK(map.floats() == 6u * res * res * 3u && map.resolution() == res, "the map's size");
            map.composite(cam, x_dev.data(), h, w, y_dev.data());
            map.backward(cam, x_dev.data(), v_dev.data(), h, w, g_dev.data());
            ctx.sync();
            CHECK(same_bits(y_dev.download(), x) && same_bits(g_dev.download(), v), "a black map changed its input");
            std::printf("ok envmap black\n");

            const float c[3] = {0.2f, 0.5f, 0.7f};
            std::vector<float> table(map.floats());
            for (size_t i = 0; i < table.size(); ++i) table[i] = c[i % 3];
            map.set_params(table);
            map.composite(cam, x_dev.data(), h, w, y_dev.data());
            map.backward(cam, x_dev.data(), v_dev.data(), h, w, g_dev.data());
            const std::vector<float> grad = map.grads();
            const std::vector<float> y = y_dev.download(), g = g_dev.download();
            double worst = 0.0, worst_a = 0.0, want_sum[3] = {0, 0, 0}, mass[3] = {0, 0, 0};
            for (uint32_t p = 0; p < px; ++p) {
                const double oma = 1.0 - (double)x[4 * p + 3];
                double sky = 0.0, sky_mass = 0.0;
                for (int k = 0; k < 3; ++k) {
                    const double ref = x[4 * p + k] + oma * c[k];
                    worst = std::fmax(worst, std::fabs(y[4 * p + k] - ref) / (eps * (std::fabs(x[4 * p + k]) + std::fabs(oma * c[k]))));
                    sky += (double)v[4 * p + k] * c[k];
                    sky_mass += std::fabs((double)v[4 * p + k] * c[k]);
                    want_sum[k] += oma * v[4 * p + k];
                    mass[k] += std::fabs(oma * v[4 * p + k]);
                    CHECK(g[4 * p + k] == v[4 * p + k], "v_rgb did not pass through at pixel %u", p);
                }
                CHECK(y[4 * p + 3] == x[4 * p + 3], "alpha did not pass through at pixel %u", p);
                worst_a = std::fmax(worst_a, std::fabs((double)g[4 * p + 3] - ((double)v[4 * p + 3] - sky)) / (eps * (std::fabs(v[4 * p + 3]) + sky_mass)));
            }
            // (the four weights sum to 1 within four roundings, the blend adds four, the composite one)
            CHECK(worst <= 10.0 && worst_a <= 8.0, "composite %.3f / v_a %.3f roundings (bounds 10, 8)", worst, worst_a);
            double got_sum[3] = {0, 0, 0};
            size_t touched = 0;
            for (size_t i = 0; i < grad.size(); ++i) got_sum[i % 3] += grad[i];
            for (size_t i = 0; i < grad.size(); i += 3) touched += (grad[i] != 0.0f || grad[i + 1] != 0.0f || grad[i + 2] != 0.0f) ? 1 : 0;
            for (int k = 0; k < 3; ++k)
                CHECK(std::fabs(got_sum[k] - want_sum[k]) <= 16 * eps * mass[k], "sum of v_E[%d] = %.9g, the frame's %.9g (mass %.3e)", k, got_sum[k], want_sum[k], mass[k]);
            CHECK(touched > 0 && touched < grad.size() / 3, "%zu of %zu texels touched", touched, grad.size() / 3);
            map.backward(cam, x_dev.data(), v_dev.data(), h, w, g_dev.data());
            CHECK(same_bits(map.grads(), grad) && same_bits(g_dev.download(), g), "two runs give different bits");
            std::printf("ok envmap composite and backward (roundings %.2f / %.2f)\n", worst, worst_a);

            // Adam at t = 1: m1 / (1 - b1) = g and sqrt(m2 / (1 - b2)) = |g|, so a texel with a gradient moves by lr against its sign
            map.backward(cam, x_dev.data(), v_dev.data(), h, w, g_dev.data(), /*update=*/true);
            const std::vector<float> after = map.params();
            for (size_t i = 0; i < grad.size(); ++i) {
                if (grad[i] == 0.0f) {
                    CHECK(std::memcmp(&after[i], &table[i], 4) == 0, "an unreached texel moved (%zu)", i);
                } else {
                    const double want = (double)table[i] - lr * (grad[i] > 0 ? 1.0 : -1.0);
                    CHECK(std::fabs(after[i] - want) <= 1e-6, "param[%zu] %.9g, expected %.9g", i, after[i], want);
                }
            }
            const bh::EnvironmentMap::State st = map.state();
            CHECK(st.t == 1, "state after one step (t = %u)", st.t);
            std::printf("ok envmap adam\n");

            // checkpoint: params + state into a fresh map, one more step on both
            bh::EnvironmentMap copy(ctx, res, lr);
            copy.set_params(map.params());
            copy.set_state(map.state());
            map.backward(cam, x_dev.data(), v_dev.data(), h, w, g_dev.data(), true);
            copy.backward(cam, x_dev.data(), v_dev.data(), h, w, g_dev.data(), true);
            const bh::EnvironmentMap::State a = map.state(), b = copy.state();
            CHECK(same_bits(map.params(), copy.params()) && a.t == 2 && b.t == 2 && same_bits(a.m1, b.m1) && same_bits(a.m2, b.m2), "the resumed map differs");
            bh::train_set_envmap(ctx, &map);
            bh::train_set_envmap(ctx, nullptr);
            BhCamera fish = cam;
            fish.model = BH_CAMERA_KANNALA_BRANDT_4;
            bool threw = false;
            try { map.composite(fish, x_dev.data(), h, w, y_dev.data()); } catch (const bh::Error& e) { threw = e.code == BH_ERR_INVALID_ARG; }
            CHECK(threw, "a fisheye camera was accepted");
            std::printf("ok envmap checkpoint\n");
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (g_failed) { std::printf("%d C++ envmap check(s) FAILED\n", g_failed); return 1; }
    std::printf("all C++ envmap checks passed\n");
    return 0;
}
