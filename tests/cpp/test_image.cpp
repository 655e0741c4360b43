// test_image.cpp — mask merge and resampling of LoadImage::load through the C++ host mirror (include/brush_hip.hpp):
//   * view_output_size of hand-worked cases (the 1920 cap, portrait, LOD scales, the clamp to one pixel);
//   * resize_u8 of a generated RGB image (Lanczos3 and Triangle) and BatchUploader::submit_view of a generated RGBA view with a
//     smaller mask under the cap: each result's FNV-1a hash is printed, and tests/test_image_cpp.py compares it with the numpy
//     restatement tests/image_ref.py of the same inputs.
// Build + run: tests/test_image_cpp.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "brush_hip.hpp"

namespace bh = brush_hip;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                                        \
    do {                                                                                                                        \
        if (!(cond)) { std::printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); ++g_failed; } \
    } while (0)

// the generator tests/test_image_cpp.py restates
static std::vector<uint8_t> pattern(uint32_t w, uint32_t h, uint32_t c, uint32_t salt) {
    std::vector<uint8_t> v((size_t)w * h * c);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x)
            for (uint32_t k = 0; k < c; ++k) v[((size_t)y * w + x) * c + k] = (uint8_t)((x * 37u + y * 91u + k * 53u + salt + (x * y) % 17u) & 255u);
    return v;
}
static unsigned long long fnv(const void* p, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
    return h;
}

int main() {
    using P = std::pair<uint32_t, uint32_t>;
    CHECK(bh::view_output_size(4032, 3024) == P(1920, 1440), "cap");
    CHECK(bh::view_output_size(3024, 4032) == P(1440, 1920), "portrait");
    CHECK(bh::view_output_size(1920, 1080, 1920, 0.25f) == P(480, 270), "lod");
    CHECK(bh::view_output_size(2000, 3, 1920, 0.1f) == P(192, 1), "clamp");
    CHECK(bh::view_output_size(640, 480, 1920, 2.0f) == P(640, 480), "never enlarged");

    bh::Context ctx(0);
    {
        const uint32_t w = 211, h = 105, nw = 100, nh = 50;
        bh::DeviceBuffer<uint8_t> src(pattern(w, h, 3, 1)), dst((size_t)nw * nh * 3);
        for (uint32_t f : {BH_FILTER_LANCZOS3, BH_FILTER_TRIANGLE}) {
            bh::resize_u8(ctx, src.data(), w, h, 3, dst.data(), nw, nh, f);
            ctx.sync();
            const std::vector<uint8_t> out = dst.download();
            std::printf("resize filter=%u %016llx\n", f, fnv(out.data(), out.size()));
        }
    }
    {
        const uint32_t w = 160, h = 120, mw = 61, mh = 47;
        const std::vector<uint8_t> img = pattern(w, h, 4, 2), mask = pattern(mw, mh, 1, 3);
        bh::BatchUploader up(ctx, ((uint64_t)w * h * 4 + (uint64_t)mw * mh + 3) / 4, 2);   // image + mask bytes in one slot
        const int slot = up.submit_view(img.data(), w, h, 4, mask.data(), mw, mh, /*invert*/ true, /*max_resolution*/ 100, 1.0f, /*premultiply*/ true);
        const bh::BatchUploader::Packed p = up.acquire(slot);
        ctx.sync();
        std::vector<uint32_t> out((size_t)p.w * p.h);
        bh::hip_check(hipMemcpy(out.data(), p.img, out.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy D2H");
        up.release(slot);
        ctx.sync();
        CHECK(p.w == 100 && p.h == 75 && p.has_alpha, "%u x %u alpha %d", p.w, p.h, (int)p.has_alpha);
        std::printf("view %ux%u %016llx\n", p.w, p.h, fnv(out.data(), out.size() * 4));
    }
    if (g_failed) { std::printf("%d C++ image checks FAILED\n", g_failed); return 1; }
    std::printf("all C++ image checks passed\n");
    return 0;
}
