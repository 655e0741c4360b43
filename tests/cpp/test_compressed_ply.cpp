// test_compressed_ply.cpp — compressed PLY export through the C++ host mirror (include/brush_hip.hpp):
//   * splat_to_compressed_ply of a small scene: the file size is the restated 72 ceil(n/256) + 16 n + 3K n behind the header, the
//     order is a permutation, a second call gives the same bytes;
//   * load_splat_from_ply of the bytes: a compressed file of n splats and the same degree, positions within their chunk's step.
// Build + run: tests/test_compressed_ply_cpp.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

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

static void test_round_trip(const bh::Context& ctx, uint32_t n, uint32_t deg) {
    const uint32_t coeffs = (deg + 1) * (deg + 1), k = coeffs - 1;
    Sm64 r{0xC0FFEEull + n + deg};
    std::vector<float> tr((size_t)n * 10), sh((size_t)n * coeffs * 3), op(n);
    for (uint32_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) tr[(size_t)i * 10 + a] = r.uni(-5.0f, 5.0f);
        for (int a = 3; a < 7; ++a) tr[(size_t)i * 10 + a] = r.uni(-1.0f, 1.0f);
        for (int a = 7; a < 10; ++a) tr[(size_t)i * 10 + a] = r.uni(-6.0f, -1.0f);
        op[i] = r.uni(-4.0f, 4.0f);
    }
    for (auto& v : sh) v = r.uni(-1.0f, 1.0f);
    bh::Splats s = bh::Splats::from_host(tr, sh, op);
    bh::DeviceBuffer<uint32_t> order;
    const std::vector<uint8_t> a = bh::splat_to_compressed_ply(ctx, s, nullptr, &order);
    const std::vector<uint8_t> b = bh::splat_to_compressed_ply(ctx, s);
    const std::string text(a.begin(), a.end());
    const size_t end = text.find("end_header\n");
    CHECK(end != std::string::npos, "n %u: no header end", n);
    const uint64_t nch = (n + 255ull) / 256ull;
    const uint64_t body = 72ull * nch + 16ull * n + 3ull * k * n;
    CHECK(a.size() == end + 11 + body, "n %u d %u: %zu bytes, want %llu + %llu", n, deg, a.size(), (unsigned long long)(end + 11), (unsigned long long)body);
    CHECK(a == b, "n %u d %u: two calls differ", n, deg);
    const std::vector<uint32_t> ord = order.download();
    std::vector<char> seen(n, 0);
    bool perm = ord.size() == n;
    for (uint32_t v : ord) perm = perm && v < n && !seen[v]++;
    CHECK(perm, "n %u: order is not a permutation", n);
    auto loaded = bh::load_splat_from_ply(ctx, a);
    CHECK(loaded.second.compressed == 1 && loaded.second.num_splats == n && loaded.second.sh_degree == deg, "n %u d %u: header %d %llu %u", n, deg,
          loaded.second.compressed, (unsigned long long)loaded.second.num_splats, loaded.second.sh_degree);
    const std::vector<float> back = loaded.first.transforms.download();
    float worst = 0.0f;
    for (uint32_t i = 0; i < n && perm; ++i)
        for (int ax = 0; ax < 3; ++ax) worst = std::fmax(worst, std::fabs(back[(size_t)i * 10 + ax] - tr[(size_t)ord[i] * 10 + ax]));
    CHECK(worst <= 10.0f / 1023.0f, "n %u: position error %g", n, worst);   // half a 10-bit step of the widest possible chunk range, twice
    std::printf("ok round_trip n=%u d=%u bytes=%zu pos_err=%.3g\n", n, deg, a.size(), worst);
}

int main() {
    bh::Context ctx(0);
    test_round_trip(ctx, 1, 0);
    test_round_trip(ctx, 257, 3);
    test_round_trip(ctx, 5000, 4);
    test_round_trip(ctx, 3000, 1);
    if (g_failed) {
        std::printf("%d C++ compressed PLY checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("all C++ compressed PLY checks passed\n");
    return 0;
}
