// test_exposure.cpp — per-view exposure compensation through the C++ host mirror (include/brush_hip.hpp ExposureTable,
// train_set_exposure):
//   * without a device: the surface compiles and links, and a null context is refused before the device is touched;
//   * on the GPU: a new table is the identity (apply and backward return their input bit for bit), a perturbed row agrees with
//     a double-precision loop within the roundings of the f32 chain, v_m within 3 x 2^-24 of its L1 mass, two runs give the
//     same bits, one Adam step at t = 1 moves every entry by lr against the sign of its gradient, other rows stay, and a
//     checkpointed table resumes to the same bits.
// Build + run: tests/test_exposure_cpp.py.
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
    bh_exposure* t = nullptr;
    CHECK(bh_exposure_create(nullptr, 3, &t) == BH_ERR_INVALID_ARG && t == nullptr, "create took a null context");
    CHECK(bh_exposure_destroy(nullptr, nullptr) == BH_ERR_INVALID_ARG, "destroy took a null context");
    CHECK(bh_exposure_apply(nullptr, nullptr, 1, nullptr, 1, 1, nullptr) == BH_ERR_INVALID_ARG, "apply took a null context");
    CHECK(bh_exposure_backward(nullptr, nullptr, 1, nullptr, nullptr, 1, 1, nullptr, 0) == BH_ERR_INVALID_ARG, "backward took a null context");
    CHECK(bh_train_set_exposure(nullptr, nullptr) == BH_ERR_INVALID_ARG, "train_set_exposure took a null context");
    std::printf("ok exposure host checks\n");
}

int main() {
    const uint32_t w = 123, h = 82, px = w * h;
    const double eps = std::ldexp(1.0, -24);
    try {
        host_checks();
        int dev_count = 0;
        if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
            std::printf("no HIP device: host checks only\n");
            return g_failed ? 1 : 0;
        }
        bh::Context ctx(0);
        Sm64 r{0xE8905};
        std::vector<float> x((size_t)px * 4), v((size_t)px * 4);
        for (auto& e : x) e = r.uni(0.0f, 1.0f);
        for (auto& e : v) e = r.uni(-1.0f, 1.0f) + 0.25f;
        const bh::DeviceBuffer<float> x_dev(x), v_dev(v);
        bh::DeviceBuffer<float> y_dev((size_t)px * 4), g_dev((size_t)px * 4);
        {
            bh::ExposureTable tab(ctx, 3, /*lr=*/0.01);
            tab.apply(2, x_dev.data(), h, w, y_dev.data());
            tab.backward(2, x_dev.data(), v_dev.data(), h, w, g_dev.data());
            ctx.sync();
            CHECK(same_bits(y_dev.download(), x) && same_bits(g_dev.download(), v), "the identity row changed its input");
            std::printf("ok exposure identity\n");

            std::vector<float> m = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
            for (auto& e : m) e += r.uni(-0.3f, 0.3f);
            tab.set_params(m, 2);
            tab.apply(2, x_dev.data(), h, w, y_dev.data());
            tab.backward(2, x_dev.data(), v_dev.data(), h, w, g_dev.data());
            const std::vector<float> grad = tab.grads();
            const std::vector<float> y = y_dev.download(), g = g_dev.download();
            double worst_y = 0.0, worst_g = 0.0, vm[12] = {0}, mass[12] = {0};
            for (uint32_t p = 0; p < px; ++p) {
                for (int c = 0; c < 3; ++c) {
                    double ref = m[4 * c + 3], ma = std::fabs(m[4 * c + 3]), gref = 0.0, gma = 0.0;
                    for (int k = 0; k < 3; ++k) {
                        ref += (double)m[4 * c + k] * x[4 * p + k];
                        ma += std::fabs((double)m[4 * c + k] * x[4 * p + k]);
                        gref += (double)m[4 * k + c] * v[4 * p + k];
                        gma += std::fabs((double)m[4 * k + c] * v[4 * p + k]);
                        vm[4 * c + k] += (double)v[4 * p + c] * x[4 * p + k];
                        mass[4 * c + k] += std::fabs((double)v[4 * p + c] * x[4 * p + k]);
                    }
                    vm[4 * c + 3] += v[4 * p + c];
                    mass[4 * c + 3] += std::fabs(v[4 * p + c]);
                    worst_y = std::fmax(worst_y, std::fabs(y[4 * p + c] - ref) / (eps * ma));
                    worst_g = std::fmax(worst_g, std::fabs(g[4 * p + c] - gref) / (eps * gma));
                }
                CHECK(y[4 * p + 3] == x[4 * p + 3] && g[4 * p + 3] == v[4 * p + 3], "alpha did not pass through at pixel %u", p);
            }
            CHECK(worst_y <= 4.0 && worst_g <= 4.0, "apply %.3f / backward %.3f roundings (bound 4)", worst_y, worst_g);
            for (int k = 0; k < 12; ++k)
                CHECK(std::fabs(grad[12 + k] - vm[k]) <= 3 * eps * mass[k], "v_m[%d] = %.9g, reference %.9g (mass %.3e)", k, grad[12 + k], vm[k], mass[k]);
            tab.backward(2, x_dev.data(), v_dev.data(), h, w, g_dev.data());
            CHECK(same_bits(tab.grads(), grad) && same_bits(g_dev.download(), g), "two runs give different bits");
            std::printf("ok exposure apply and backward (roundings %.2f / %.2f)\n", worst_y, worst_g);

            // Adam at t = 1: m1 / (1 - b1) = g and sqrt(m2 / (1 - b2)) = |g|, so every entry moves by lr against the sign of g
            const std::vector<float> before = tab.params();
            tab.backward(2, x_dev.data(), v_dev.data(), h, w, g_dev.data(), /*update=*/true);
            const std::vector<float> after = tab.params();
            for (int k = 0; k < 12; ++k) {
                const double want = (double)before[12 + k] - 0.01 * (grad[12 + k] > 0 ? 1.0 : -1.0);
                CHECK(std::fabs(after[12 + k] - want) <= 2 * eps * std::fmax(std::fabs(want), 0.01) + 1e-9, "param[%d] %.9g, expected %.9g", k, after[12 + k], want);
            }
            CHECK(std::memcmp(before.data(), after.data(), 48) == 0 && std::memcmp(before.data() + 24, after.data() + 24, 48) == 0, "another row moved");
            const bh::ExposureTable::State st = tab.state(2);
            CHECK(st.t == 1 && tab.state(1).t == 0 && std::fabs(st.m1[0] - 0.1 * vm[0]) <= 1e-9 * std::fabs(vm[0]), "state after one step (t = %u)", st.t);
            std::printf("ok exposure adam\n");

            // checkpoint: params + state into a fresh table, one more step on both
            bh::ExposureTable copy(ctx, 3, 0.01);
            copy.set_params(tab.params());
            for (uint32_t k = 1; k <= 3; ++k) copy.set_state(k, tab.state(k));
            tab.backward(2, x_dev.data(), v_dev.data(), h, w, g_dev.data(), true);
            copy.backward(2, x_dev.data(), v_dev.data(), h, w, g_dev.data(), true);
            const bh::ExposureTable::State a = tab.state(2), b = copy.state(2);
            CHECK(same_bits(tab.params(), copy.params()) && a.t == 2 && b.t == 2 && a.m1 == b.m1 && a.m2 == b.m2, "the resumed table differs");
            bh::train_set_exposure(ctx, &tab);
            bh::train_set_exposure(ctx, nullptr);
            bool threw = false;
            try { tab.apply(4, x_dev.data(), h, w, y_dev.data()); } catch (const bh::Error& e) { threw = e.code == BH_ERR_INVALID_ARG; }
            CHECK(threw, "a view out of range was accepted");
            std::printf("ok exposure checkpoint\n");
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (g_failed) { std::printf("%d C++ exposure check(s) FAILED\n", g_failed); return 1; }
    std::printf("all C++ exposure checks passed\n");
    return 0;
}
