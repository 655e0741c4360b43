// test_knn.cpp — point-cloud initialisation through the C++ host mirror (include/brush_hip.hpp):
//   * knn_log_scales of a small cloud (duplicates, a non-finite row) vs a host brute force in f32 with the reference's distance
//     ((dx*dx + dy*dy) + dz*dz, correctly rounded sqrt): d1 / d2 bit-exact, log-scales within 2 ulp of ln in double;
//   * to_init_splats: the reference's defaults (rotation 1 0 0 0, SH 0.5, raw opacity 0) and kNN log-scales;
//   * load_init_splats of a points-only PLY (x y z + uchar colour): the kNN runs over the loaded rows.
// Build + run: tests/test_knn_init_abi.py (compile) and tests/test_gpu_knn_init.py (run).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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

static uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static int64_t ulps(float a, float b) {
    if (a == b) return 0;
    auto ord = [](float f) { const int32_t i = (int32_t)f2u(f); return i < 0 ? -(int64_t)(i & 0x7FFFFFFF) : (int64_t)i; };
    return std::llabs(ord(a) - ord(b));
}

// f32 brute force: the two smallest (dx*dx + dy*dy) + dz*dz over finite rows j != i, then sqrt
static void brute(const std::vector<float>& xyz, std::vector<float>& nn) {
    const size_t n = xyz.size() / 3;
    const float inf = std::numeric_limits<float>::infinity();
    nn.assign(n * 2, inf);
    auto fin = [&](size_t i) { return std::isfinite(xyz[i * 3]) && std::isfinite(xyz[i * 3 + 1]) && std::isfinite(xyz[i * 3 + 2]); };
    for (size_t i = 0; i < n; ++i) {
        if (!fin(i)) continue;
        float b1 = inf, b2 = inf;
        for (size_t j = 0; j < n; ++j) {
            if (j == i || !fin(j)) continue;
            const float dx = xyz[i * 3] - xyz[j * 3], dy = xyz[i * 3 + 1] - xyz[j * 3 + 1], dz = xyz[i * 3 + 2] - xyz[j * 3 + 2];
            const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
            const float xy = xx + yy;
            const float s = xy + zz;
            if (s < b1) { b2 = b1; b1 = s; } else if (s < b2) { b2 = s; }
        }
        nn[i * 2] = std::sqrt(b1);
        nn[i * 2 + 1] = std::sqrt(b2);
    }
}

static std::vector<float> make_cloud(size_t n, uint64_t seed) {
    Sm64 r{seed};
    std::vector<float> xyz(n * 3);
    for (auto& v : xyz) v = r.uni(-1.0f, 1.0f);
    for (size_t i = 0; i < 40; ++i)   // duplicates: rows 0..39 repeated at 40..79
        for (int k = 0; k < 3; ++k) xyz[(40 + i) * 3 + k] = xyz[i * 3 + k];
    xyz[100 * 3 + 1] = std::numeric_limits<float>::quiet_NaN();   // a non-finite row
    return xyz;
}

static std::vector<float> means_to_transforms(const std::vector<float>& xyz) {
    const size_t n = xyz.size() / 3;
    std::vector<float> tr(n * 10, 0.0f);
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) tr[i * 10 + k] = xyz[i * 3 + k];
        tr[i * 10 + 3] = 1.0f;
    }
    return tr;
}

static void test_knn(const bh::Context& ctx) {
    const size_t n = 3000;
    const std::vector<float> xyz = make_cloud(n, 7);
    bh::Splats s = bh::Splats::from_host(means_to_transforms(xyz), std::vector<float>(n * 3, 0.5f), std::vector<float>(n, 0.0f));
    bh::DeviceBuffer<float> nn_dev;
    const uint64_t pairs = bh::knn_log_scales(ctx, s, &nn_dev);
    const std::vector<float> nn = nn_dev.download(), tr = s.transforms.download();
    std::vector<float> want;
    brute(xyz, want);
    size_t bad = 0;
    for (size_t i = 0; i < n * 2; ++i) bad += f2u(nn[i]) != f2u(want[i]);
    CHECK(bad == 0, "%zu of %zu distances differ from the f32 brute force", bad, n * 2);
    CHECK(nn[0] == 0.0f && nn[40 * 2] == 0.0f, "a duplicate is a neighbour at distance 0");
    CHECK(std::isinf(nn[100 * 2]) && std::isinf(nn[100 * 2 + 1]), "a non-finite row has no neighbour");
    CHECK(pairs > 0 && pairs < (uint64_t)n * n, "pairs_tested %llu", (unsigned long long)pairs);
    // median_size from the 0.75 box (extents ~0.75 on every axis: one value checked against the clamp, the rest by ulp)
    float center[3], extent[3];
    ctx.check(bh_splat_bounds(ctx.get(), s.transforms.data(), (uint32_t)n, 0.75f, center, extent));
    std::sort(extent, extent + 3);
    const float upper = std::fmax(extent[1] * 2.0f, 0.01f) * 0.1f;
    int64_t worst = 0;
    for (size_t i = 0; i < n; ++i) {
        float d = (want[i * 2] + want[i * 2 + 1]) / 4.0f;
        if (d < 1e-3f) d = 1e-3f;
        if (d > upper) d = upper;
        const float ref = (float)std::log((double)d);
        for (int k = 7; k < 10; ++k) worst = std::max(worst, ulps(tr[i * 10 + k], ref));
        for (int k = 0; k < 7; ++k) CHECK(f2u(tr[i * 10 + k]) == f2u(k < 3 ? xyz[i * 3 + k] : (k == 3 ? 1.0f : 0.0f)), "row %zu column %d changed", i, k);
        if (g_failed > 20) return;
    }
    CHECK(worst <= 2, "log-scale %lld ulp from ln", (long long)worst);
    if (!g_failed) std::printf("ok knn_log_scales n=%zu pairs/N=%.1f\n", n, (double)pairs / n);
}

static void test_to_init(const bh::Context& ctx) {
    const size_t n = 500;
    std::vector<float> xyz = make_cloud(n, 11);
    xyz[100 * 3 + 1] = 0.25f;
    bh::Splats s = bh::to_init_splats(ctx, xyz);
    const std::vector<float> tr = s.transforms.download(), sh = s.sh_coeffs.download(), op = s.raw_opacities.download();
    CHECK(s.num_splats() == n && s.num_coeffs() == 1, "shape");
    bh::Splats t = bh::Splats::from_host(means_to_transforms(xyz), std::vector<float>(n * 3, 0.5f), std::vector<float>(n, 0.0f));
    bh::knn_log_scales(ctx, t);
    const std::vector<float> tt = t.transforms.download();
    for (size_t i = 0; i < n * 10; ++i) CHECK(f2u(tr[i]) == f2u(tt[i]), "transforms[%zu]", i);
    for (float v : sh) CHECK(v == 0.5f, "SH default");
    for (float v : op) CHECK(v == 0.0f, "opacity default");
    std::vector<float> given(n * 3, -2.0f);
    bh::Splats g = bh::to_init_splats(ctx, xyz, {}, given);
    const std::vector<float> gt = g.transforms.download();
    for (size_t i = 0; i < n; ++i) CHECK(gt[i * 10 + 7] == -2.0f && gt[i * 10 + 9] == -2.0f, "given log-scales are kept");
    if (!g_failed) std::printf("ok to_init_splats\n");
}

static void test_load_init(const bh::Context& ctx) {
    const size_t n = 1000;
    std::vector<float> xyz = make_cloud(n, 13);
    xyz[100 * 3 + 1] = 0.5f;
    std::string head = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(n) +
                       "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n";
    std::vector<uint8_t> bytes(head.begin(), head.end());
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(&xyz[i * 3]);
        bytes.insert(bytes.end(), p, p + 12);
        const uint8_t rgb[3] = {(uint8_t)(i & 255), (uint8_t)(i * 7 & 255), 200};
        bytes.insert(bytes.end(), rgb, rgb + 3);
    }
    auto loaded = bh::load_init_splats(ctx, bytes, 1, 400);   // subsampled to 334 rows: the kNN runs over those
    bh::Splats& s = loaded.first;
    CHECK(loaded.second.num_splats == s.num_splats() && s.num_splats() == 334, "rows kept %u", s.num_splats());
    const std::vector<float> tr = s.transforms.download();
    std::vector<float> kept;
    for (size_t i = 0; i < s.num_splats(); ++i)
        for (int k = 0; k < 3; ++k) kept.push_back(tr[i * 10 + k]);
    bh::Splats t = bh::Splats::from_host(means_to_transforms(kept), std::vector<float>(kept.size(), 0.5f), std::vector<float>(kept.size() / 3, 0.0f));
    bh::knn_log_scales(ctx, t);
    const std::vector<float> tt = t.transforms.download();
    for (size_t i = 0; i < s.num_splats(); ++i)
        for (int k = 7; k < 10; ++k) CHECK(f2u(tr[i * 10 + k]) == f2u(tt[i * 10 + k]), "row %zu log-scale", i);
    CHECK(bh_ply_vertex_has_property(bytes.data(), bytes.size(), "scale_0") == 0 && bh_ply_vertex_has_property(bytes.data(), bytes.size(), "red") == 1,
          "has_property");
    if (!g_failed) std::printf("ok load_init_splats\n");
}

int main() {
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        std::printf("no HIP device: compile-only run\n");
        return g_failed ? 1 : 0;
    }
    try {
        bh::Context ctx(0);
        test_knn(ctx);
        test_to_init(ctx);
        test_load_init(ctx);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        ++g_failed;
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all C++ kNN checks passed\n");
    return 0;
}
