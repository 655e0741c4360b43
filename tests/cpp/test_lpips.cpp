// test_lpips.cpp — LPIPS through the C++ host mirror (include/brush_hip.hpp):
//   * a wrong parameter count throws; the model is move-only RAII;
//   * lpips and lpips_value_and_grad of the inputs tests/test_lpips_cpp.py writes (params, image, GT, composite background)
//     give one value, repeated calls are bit-identical, and LPIPS(x, x) == 0;
//   * the value and dL/dimg are written back for the Python side to compare with its own call.
// Usage: test_lpips <dir> with <dir>/{params.f32, img.f32, gt.u32, shape.txt}; writes <dir>/{value.f32, grad.f32}.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "brush_hip.hpp"

namespace bh = brush_hip;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                                        \
    do {                                                                                                                        \
        if (!(cond)) { std::printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); ++g_failed; } \
    } while (0)

template <class T>
static std::vector<T> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("cannot open " + path);
    const size_t bytes = (size_t)f.tellg();
    std::vector<T> v(bytes / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

template <class T>
static void write_file(const std::string& path, const std::vector<T>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: %s <dir>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    bh::Context ctx(0);
    const std::vector<float> params = read_file<float>(dir + "/params.f32");
    {
        bool threw = false;
        try {
            bh::Lpips bad(ctx, std::vector<float>(params.begin(), params.end() - 1));
        } catch (const bh::Error& e) {
            threw = e.code == BH_ERR_INVALID_ARG && std::strstr(e.what(), "expected") != nullptr;
        }
        CHECK(threw, "a short parameter vector must be refused");
        std::printf("ok wrong_count\n");
    }
    bh::Lpips model(ctx, params);
    uint32_t h = 0, w = 0;
    float bg[3] = {0, 0, 0};
    int composite = 0;
    {
        std::ifstream f(dir + "/shape.txt");
        f >> h >> w >> composite >> bg[0] >> bg[1] >> bg[2];
    }
    const std::vector<float> img = read_file<float>(dir + "/img.f32");
    const std::vector<uint32_t> gt = read_file<uint32_t>(dir + "/gt.u32");
    CHECK(img.size() == (size_t)h * w * 4 && gt.size() == (size_t)h * w, "input sizes");
    bh::DeviceBuffer<float> d_img(img), value(1), value2(1), v_out(std::vector<float>((size_t)h * w * 4, 0.0f)), v_out2(std::vector<float>((size_t)h * w * 4, 0.0f));
    bh::DeviceBuffer<uint32_t> d_gt(gt);
    const float* bgp = composite ? bg : nullptr;
    bh::lpips(ctx, model, d_img.data(), d_gt.data(), h, w, value.data(), bgp);
    ctx.sync();
    const float v_fwd = value.download()[0];
    bh::lpips_value_and_grad(ctx, model, d_img.data(), d_gt.data(), h, w, 1.0f, value.data(), v_out.data(), bgp);
    bh::lpips_value_and_grad(ctx, model, d_img.data(), d_gt.data(), h, w, 1.0f, value2.data(), v_out2.data(), bgp);
    ctx.sync();
    const float v1 = value.download()[0], v2 = value2.download()[0];
    const std::vector<float> g1 = v_out.download(), g2 = v_out2.download();
    CHECK(std::isfinite(v1) && v1 > 0.0f, "value %g", (double)v1);
    CHECK(v1 == v2 && v1 == v_fwd, "values differ: %.9g %.9g %.9g", (double)v1, (double)v2, (double)v_fwd);
    CHECK(std::memcmp(g1.data(), g2.data(), g1.size() * 4) == 0, "repeated gradients differ");
    bool alpha_zero = true;
    for (size_t p = 0; p < (size_t)h * w; ++p) alpha_zero = alpha_zero && g1[p * 4 + 3] == 0.0f;
    CHECK(alpha_zero, "the alpha channel of v_output must stay untouched");
    std::printf("ok value_and_grad %.9g\n", (double)v1);
    // identity: the image against its own 8-bit quantisation, fed back as the prediction
    {
        std::vector<float> q((size_t)h * w * 4);
        for (size_t p = 0; p < (size_t)h * w; ++p)
            for (int c = 0; c < 4; ++c) q[p * 4 + c] = c < 3 ? (float)((gt[p] >> (8 * c)) & 0xffu) * (1.0f / 255.0f) : 1.0f;
        bh::DeviceBuffer<float> d_q(q), v0(1);
        bh::lpips(ctx, model, d_q.data(), d_gt.data(), h, w, v0.data(), nullptr);
        ctx.sync();
        const float z = v0.download()[0];
        CHECK(z == 0.0f, "LPIPS(x, x) = %g", (double)z);
        std::printf("ok identity\n");
    }
    write_file(dir + "/value.f32", std::vector<float>{v1});
    write_file(dir + "/grad.f32", g1);
    if (g_failed) {
        std::printf("%d C++ LPIPS checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("all C++ lpips checks passed\n");
    return 0;
}
