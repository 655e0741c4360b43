// test_lod.cpp — LOD decimation through the C++ host mirror (include/brush_hip.hpp):
//   * decimate_to_count of a small scene (scores with ties, +-0, -inf and NaN) vs std::stable_sort with the reference's comparator
//     (lod.rs:20: sort_by(|a, b| b.partial_cmp(a).unwrap_or(Equal)); NaN placed last, the library's documented choice), rows and
//     min_scale gathered exactly;
//   * pup_accumulate_view over 8 views + pup_scores: finite accumulator, -inf for splats no view reached, finite scores for others;
//   * lod_target_count on the reference's formula.
// Build + run: tests/test_lod_cpp.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>

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

// the host order decimate_to_count must reproduce
static std::vector<uint32_t> host_order(const std::vector<float>& s) {
    std::vector<uint32_t> idx(s.size());
    std::iota(idx.begin(), idx.end(), 0u);
    auto rank = [](float x) { return std::isnan(x) ? 1 : 0; };
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
        const float x = s[a], y = s[b];
        if (rank(x) != rank(y)) return rank(x) < rank(y);
        return !std::isnan(x) && x > y;   // descending; equal (incl. -0 == +0) keeps the index order
    });
    return idx;
}

static void test_decimate(const bh::Context& ctx) {
    const uint32_t n = 2053, coeffs = 4;
    Sm64 r{0x10D};
    std::vector<float> tr((size_t)n * 10), sh((size_t)n * coeffs * 3), op(n), ms(n), sc(n);
    for (auto& v : tr) v = r.uni(-2.0f, 2.0f);
    for (auto& v : sh) v = r.uni(-1.0f, 1.0f);
    for (auto& v : op) v = r.uni(-3.0f, 3.0f);
    for (auto& v : ms) v = r.uni(0.0f, 0.01f);
    const float inf = std::numeric_limits<float>::infinity();
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t c = r.next() % 8;
        sc[i] = c == 0 ? 0.0f : c == 1 ? -0.0f : c == 2 ? -inf : c == 3 ? std::nanf("") : c == 4 ? 1.5f : (float)(int)r.uni(-20.0f, 20.0f);
    }
    bh::Splats s = bh::Splats::from_host(tr, sh, op);
    s.with_min_scale(bh::DeviceBuffer<float>(ms));
    bh::DeviceBuffer<float> scores(sc);
    const std::vector<uint32_t> want = host_order(sc);
    for (uint32_t target : {1u, n / 2, n - 1, n, n + 7}) {
        std::vector<uint32_t> keep;
        bh::Splats d = bh::decimate_to_count(ctx, s, scores.data(), target, &keep);
        const uint32_t k = std::min(target, n);
        CHECK(d.num_splats() == k && keep.size() == k, "target %u: %u splats", target, d.num_splats());
        const std::vector<float> dt = d.transforms.download(), dsh = d.sh_coeffs.download(), dop = d.raw_opacities.download(), dms = d.min_scale->download();
        bool ok = true;
        for (uint32_t i = 0; i < k && ok; ++i) {
            const uint32_t src = target >= n ? i : want[i];
            ok = keep[i] == src && std::memcmp(&dt[(size_t)i * 10], &tr[(size_t)src * 10], 40) == 0 &&
                 std::memcmp(&dsh[(size_t)i * coeffs * 3], &sh[(size_t)src * coeffs * 3], coeffs * 12) == 0 && dop[i] == op[src] && dms[i] == ms[src];
            if (!ok) std::printf("  target %u row %u: kept %u, want %u\n", target, i, keep[i], src);
        }
        CHECK(ok, "target %u: gathered rows differ from the host stable sort", target);
    }
    std::printf("ok decimate_to_count\n");
}

static void test_pup_view(const bh::Context& ctx) {
    const uint32_t n = 3000, coeffs = 1, w = 96, h = 64;
    Sm64 r{0xC0FFEE};
    std::vector<float> tr((size_t)n * 10), sh((size_t)n * coeffs * 3), op(n);
    const float t = std::tan(0.5f);
    for (uint32_t i = 0; i < n; ++i) {
        float* row = &tr[(size_t)i * 10];
        const float z = r.uni(2.0f, 10.0f);
        // a third of the splats sits behind the camera: no gradient, zero H, score -inf
        row[0] = r.uni(-1.0f, 1.0f) * z * t;
        row[1] = r.uni(-1.0f, 1.0f) * z * t * 0.7f;
        row[2] = i % 3 == 0 ? -z : z;
        row[3] = 1.0f; row[4] = r.uni(-0.3f, 0.3f); row[5] = r.uni(-0.3f, 0.3f); row[6] = r.uni(-0.3f, 0.3f);
        for (int k = 7; k < 10; ++k) row[k] = r.uni(std::log(0.03f), std::log(0.2f));
        op[i] = r.uni(-1.0f, 2.0f);
    }
    for (auto& v : sh) v = r.uni(-1.0f, 1.0f);
    bh::Splats s = bh::Splats::from_host(tr, sh, op);
    std::vector<uint32_t> gt((size_t)w * h);
    for (auto& p : gt) p = (uint32_t)(r.next() & 0x00FFFFFFu) | 0xFF000000u;
    bh::DeviceBuffer<uint32_t> gt_dev(gt);
    // H is a sum of rank-1 terms: it needs >= 6 views to be positive definite.  Eight slightly turned cameras see the same splats.
    bh::DeviceBuffer<float> hess((size_t)bh::kPupPlanes * n);
    hess.zero();
    for (int v = 0; v < 8; ++v) {
        bh::Camera cam;
        cam.fov_x = 1.0;
        cam.fov_y = 0.7;
        const float yaw = 0.04f * (float)(v - 4), pitch = 0.03f * std::sin(2.7f * (float)v);
        // yaw about y after pitch about x (xyzw)
        const float cy = std::cos(yaw / 2), sy = std::sin(yaw / 2), cx = std::cos(pitch / 2), sx = std::sin(pitch / 2);
        cam.rotation[0] = cy * sx; cam.rotation[1] = sy * cx; cam.rotation[2] = -sy * sx; cam.rotation[3] = cy * cx;
        cam.position[0] = 0.02f * std::sin((float)v);
        bh::pup_accumulate_view(ctx, s, cam, gt_dev.data(), w, h, hess);
    }
    const std::vector<float> hh = hess.download();
    bool finite = true;
    for (float v : hh) finite = finite && std::isfinite(v);
    CHECK(finite, "accumulator holds a non-finite entry");
    const std::vector<float> sc = bh::pup_scores(ctx, hess, n).download();
    uint32_t behind_inf = 0, front_finite = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (i % 3 == 0) behind_inf += sc[i] == -std::numeric_limits<float>::infinity();
        else front_finite += std::isfinite(sc[i]);
    }
    CHECK(behind_inf == (n + 2) / 3, "splats behind the camera: %u of %u score -inf", behind_inf, (n + 2) / 3);
    CHECK(front_finite > n / 10, "only %u splats in front of the camera have a finite score", front_finite);
    std::printf("ok pup_view (finite scores: %u)\n", front_finite);
}

int main() {
    CHECK(bh::lod_target_count(1, 50) == 1u && bh::lod_target_count(3, 50) == 1u && bh::lod_target_count(16777217u, 100) == 16777216u &&
          bh::lod_target_count(1000, 50) == 500u, "lod_target_count");
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        std::printf("no HIP device: compile-only run\n");
        return g_failed ? 1 : 0;
    }
    try {
        bh::Context ctx(0);
        test_decimate(ctx);
        test_pup_view(ctx);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        ++g_failed;
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all C++ LOD checks passed\n");
    return 0;
}
