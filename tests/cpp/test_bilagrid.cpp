// test_bilagrid.cpp — per-view bilateral grids through the C++ host mirror (include/brush_hip.hpp BilateralGridTable,
// train_set_bilagrid):
//   * without a device: the surface compiles and links, and a null context is refused before the device is touched;
//   * on the GPU: a new table is the identity (slice and backward return their input bit for bit), a perturbed grid agrees with a
//     double-precision loop over the header's f32 coordinates within 8 x 2^-24 of each pixel's L1 mass, two runs give the same bits,
//     one Adam step at t = 1 moves every reached entry by lr against the sign of its gradient and leaves the others, other views
//     stay, and a checkpointed table resumes to the same bits.
// Build + run: tests/test_bilagrid_cpp.py.
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

// the header's coordinates of one axis, each operation rounded to f32 (volatile keeps the compiler from contracting them)
static void axis(float f, int n, int& i0, int& i1, double& t) {
    const int top = n >= 2 ? n - 2 : 0;
    const int fl = (int)std::floor(f);
    i0 = fl < top ? fl : top;
    i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
    volatile float d = f - (float)i0;
    t = d;
}

static void host_checks() {
    bh_bilagrid* t = nullptr;
    CHECK(bh_bilagrid_create(nullptr, 3, 16, 16, 8, &t) == BH_ERR_INVALID_ARG && t == nullptr, "create took a null context");
    CHECK(bh_bilagrid_destroy(nullptr, nullptr) == BH_ERR_INVALID_ARG, "destroy took a null context");
    CHECK(bh_bilagrid_dims(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == BH_ERR_INVALID_ARG, "dims took a null context");
    CHECK(bh_bilagrid_slice(nullptr, nullptr, 1, nullptr, 1, 1, nullptr) == BH_ERR_INVALID_ARG, "slice took a null context");
    CHECK(bh_bilagrid_backward(nullptr, nullptr, 1, nullptr, nullptr, 1, 1, nullptr, 0.0f, 0) == BH_ERR_INVALID_ARG, "backward took a null context");
    CHECK(bh_bilagrid_tv(nullptr, nullptr, 1, nullptr) == BH_ERR_INVALID_ARG, "tv took a null context");
    CHECK(bh_train_set_bilagrid(nullptr, nullptr, 0.0f) == BH_ERR_INVALID_ARG, "train_set_bilagrid took a null context");
    std::printf("ok bilagrid host checks\n");
}

int main() {
    const uint32_t w = 123, h = 82, px = w * h;
    const int gw = 4, gh = 3, gl = 2;
    const double eps = std::ldexp(1.0, -24);
    try {
        host_checks();
        int dev_count = 0;
        if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
            std::printf("no HIP device: host checks only\n");
            return g_failed ? 1 : 0;
        }
        bh::Context ctx(0);
        Sm64 r{0xB11A6};
        std::vector<float> x((size_t)px * 4), v((size_t)px * 4);
        for (auto& e : x) e = r.uni(0.05f, 0.95f);   // luminance strictly inside (0, 1)
        for (auto& e : v) e = r.uni(-1.0f, 1.0f);
        const bh::DeviceBuffer<float> x_dev(x), v_dev(v);
        bh::DeviceBuffer<float> y_dev((size_t)px * 4), g_dev((size_t)px * 4);
        {
            bh::BilateralGridTable tab(ctx, 3, gw, gh, gl, /*lr=*/0.01);
            const size_t row = tab.row_floats();
            CHECK(row == (size_t)gw * gh * gl * 12 && tab.grid()[0] == (uint32_t)gw && tab.grid()[1] == (uint32_t)gh && tab.grid()[2] == (uint32_t)gl, "dims");
            tab.slice(2, x_dev.data(), h, w, y_dev.data());
            tab.backward(2, x_dev.data(), v_dev.data(), h, w, g_dev.data());
            ctx.sync();
            CHECK(same_bits(y_dev.download(), x) && same_bits(g_dev.download(), v), "the identity grid changed its input");
            std::printf("ok bilagrid identity\n");

            std::vector<float> g = tab.params();
            for (size_t k = 0; k < row; ++k) g[row + k] += r.uni(-0.3f, 0.3f);
            tab.set_params(std::vector<float>(g.begin() + row, g.begin() + 2 * row), 2);
            tab.slice(2, x_dev.data(), h, w, y_dev.data());
            tab.backward(2, x_dev.data(), v_dev.data(), h, w, g_dev.data());
            const std::vector<float> grad = tab.grads();
            const std::vector<float> y = y_dev.download(), gi = g_dev.download();
            const volatile float sx = (float)(gw - 1) / (float)w, sy = (float)(gh - 1) / (float)h;
            std::vector<double> vg(row, 0.0), mass_g(row, 0.0);
            double worst_y = 0.0;
            for (uint32_t p = 0; p < px; ++p) {
                const uint32_t py = p / w, pxx = p % w;
                volatile float cx = (float)pxx + 0.5f, cy = (float)py + 0.5f;
                volatile float fx = cx * sx, fy = cy * sy;
                volatile float l0 = x[4 * p] * 0.299f, l1 = x[4 * p + 1] * 0.587f, l2 = x[4 * p + 2] * 0.114f;
                volatile float l01 = l0 + l1;
                volatile float lum = l01 + l2;
                volatile float fz = std::fmin(std::fmax(lum, 0.0f), 1.0f) * (float)(gl - 1);
                int i[2], j[2], l[2];
                double tx, ty, tz;
                axis(fx, gw, i[0], i[1], tx);
                axis(fy, gh, j[0], j[1], ty);
                axis(fz, gl, l[0], l[1], tz);
                const double wx[2] = {1.0 - tx, tx}, wy[2] = {1.0 - ty, ty}, wz[2] = {1.0 - tz, tz};
                double a[12] = {0}, ma[12] = {0};
                const double xs[4] = {x[4 * p], x[4 * p + 1], x[4 * p + 2], 1.0};
                for (int cyi = 0; cyi < 2; ++cyi)
                    for (int cxi = 0; cxi < 2; ++cxi)
                        for (int czi = 0; czi < 2; ++czi) {
                            const double wgt = wy[cyi] * wx[cxi] * wz[czi];
                            const size_t base = (((size_t)j[cyi] * gw + i[cxi]) * gl + l[czi]) * 12;
                            for (int q = 0; q < 12; ++q) {
                                a[q] += wgt * g[row + base + q];
                                ma[q] += std::fabs(wgt * g[row + base + q]);
                                const double o = (double)v[4 * p + q / 4] * xs[q % 4];
                                vg[base + q] += wgt * o;
                                mass_g[base + q] += std::fabs(wgt * o);
                            }
                        }
                for (int c = 0; c < 3; ++c) {
                    double ref = 0.0, m = 0.0;
                    for (int k = 0; k < 4; ++k) { ref += a[4 * c + k] * xs[k]; m += ma[4 * c + k] * std::fabs(xs[k]); }
                    worst_y = std::fmax(worst_y, std::fabs(y[4 * p + c] - ref) / (eps * m));
                }
                CHECK(y[4 * p + 3] == x[4 * p + 3] && gi[4 * p + 3] == v[4 * p + 3], "alpha did not pass through at pixel %u", p);
            }
            CHECK(worst_y <= 8.0, "slice %.3f roundings (bound 8)", worst_y);
            double worst_g = 0.0;
            for (size_t k = 0; k < row; ++k) worst_g = std::fmax(worst_g, std::fabs(grad[row + k] - vg[k]) / (eps * std::fmax(mass_g[k], 1e-300)));
            CHECK(worst_g <= 2.0, "v_g %.3f roundings of its mass (bound 2: the f64 sum is rounded to f32 once)", worst_g);
            tab.backward(2, x_dev.data(), v_dev.data(), h, w, g_dev.data());
            CHECK(same_bits(tab.grads(), grad) && same_bits(g_dev.download(), gi), "two runs give different bits");
            std::printf("ok bilagrid slice and backward (roundings %.2f / %.2f)\n", worst_y, worst_g);

            // Adam at t = 1: m1 / (1 - b1) = g and sqrt(m2 / (1 - b2)) = |g|, so every entry moves by lr against the sign of g
            const std::vector<float> before = tab.params();
            tab.backward(2, x_dev.data(), v_dev.data(), h, w, g_dev.data(), 0.0f, /*update=*/true);
            const std::vector<float> after = tab.params();
            for (size_t k = 0; k < row; ++k) {
                const double step = grad[row + k] > 0 ? 0.01 : grad[row + k] < 0 ? -0.01 : 0.0;
                const double want = (double)before[row + k] - step;
                CHECK(std::fabs(after[row + k] - want) <= 2 * eps * std::fmax(std::fabs(want), 0.01) + 1e-9, "param[%zu] %.9g, expected %.9g", k, after[row + k], want);
            }
            CHECK(std::memcmp(before.data(), after.data(), row * 4) == 0 && std::memcmp(before.data() + 2 * row, after.data() + 2 * row, row * 4) == 0,
                  "another view moved");
            const bh::BilateralGridTable::State st = tab.state(2);
            CHECK(st.t == 1 && tab.state(1).t == 0 && std::fabs(st.m1[0] - 0.1 * vg[0]) <= 1e-6 * std::fabs(vg[0]), "state after one step (t = %u)", st.t);
            std::printf("ok bilagrid adam\n");

            // checkpoint: params + state into a fresh table, one more step on both
            bh::BilateralGridTable copy(ctx, 3, gw, gh, gl, 0.01);
            copy.set_params(tab.params());
            for (uint32_t k = 1; k <= 3; ++k) copy.set_state(k, tab.state(k));
            tab.backward(2, x_dev.data(), v_dev.data(), h, w, g_dev.data(), 0.5f, true);
            copy.backward(2, x_dev.data(), v_dev.data(), h, w, g_dev.data(), 0.5f, true);
            const bh::BilateralGridTable::State a = tab.state(2), b = copy.state(2);
            CHECK(same_bits(tab.params(), copy.params()) && a.t == 2 && b.t == 2 && same_bits(a.m1, b.m1) && same_bits(a.m2, b.m2), "the resumed table differs");
            bh::train_set_bilagrid(ctx, &tab, 10.0f);
            bh::train_set_bilagrid(ctx, nullptr);
            bool threw = false;
            try { tab.slice(4, x_dev.data(), h, w, y_dev.data()); } catch (const bh::Error& e) { threw = e.code == BH_ERR_INVALID_ARG; }
            CHECK(threw, "a view out of range was accepted");
            std::printf("ok bilagrid checkpoint\n");
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (g_failed) { std::printf("%d C++ bilagrid check(s) FAILED\n", g_failed); return 1; }
    std::printf("all C++ bilagrid checks passed\n");
    return 0;
}
