// test_scene.cpp — scene editing through the C++ host mirror (include/brush_hip.hpp SceneTransform / transform_splats /
// transformed_splats / select_region / crop_splats; include/brush_hip_scene.h), against numbers the Python side wrote:
//   * argv[1] is a file tests/test_scene_cpp.py wrote: a scene, a transform, a region, and what brush_amd/host.py got for them on this
//     GPU — the transformed tensors, the keep flags and the cropped rows;
//   * the record: compose with the inverse is the identity, the operator applies its right-hand side first;
//   * transformed_splats and transform_splats (in place) give Python's bits; the camera's view of a moved point is s times the old one;
//   * select_region gives Python's flags and count, crop_splats its rows and indices;
//   * refusals: a zero quaternion, a bad band, an unknown region kind, an overlapping output.
// Without an argument or without a device it only proves that it compiles, links and starts.  Build + run: tests/test_scene_cpp.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "brush_hip.hpp"

namespace bh = brush_hip;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                                        \
    do {                                                                                                                        \
        if (!(cond)) { std::printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); ++g_failed; } \
    } while (0)

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0;
}

static std::vector<float> read_floats(FILE* f, size_t n) {
    std::vector<float> v(n);
    if (std::fread(v.data(), 4, n, f) != n) { std::printf("FAIL short read\n"); std::exit(1); }
    return v;
}

int main(int argc, char** argv) {
    int dev_count = 0;
    if (argc < 2 || hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        std::printf("no input file or no HIP device: compile-only run\n");
        return 0;
    }
    try {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::printf("FAIL cannot open %s\n", argv[1]); return 1; }
        uint32_t hdr[4];
        double qts[8];
        BhSceneRegion region;
        if (std::fread(hdr, 4, 4, f) != 4 || std::fread(qts, 8, 8, f) != 8 || std::fread(&region, sizeof(region), 1, f) != 1) { std::printf("FAIL short header\n"); return 1; }
        const uint32_t n = hdr[0], coeffs = hdr[1], kept = hdr[2];
        const std::vector<float> tr = read_floats(f, (size_t)n * 10), sh = read_floats(f, (size_t)n * coeffs * 3), op = read_floats(f, n), ms = read_floats(f, n);
        const std::vector<float> want_tr = read_floats(f, (size_t)n * 10), want_sh = read_floats(f, (size_t)n * coeffs * 3), want_ms = read_floats(f, n);
        const std::vector<float> want_keep = read_floats(f, n), want_crop = read_floats(f, (size_t)kept * 10), want_idx = read_floats(f, kept);
        std::fclose(f);

        // ---- the record ----
        const bh::SceneTransform T({qts[0], qts[1], qts[2], qts[3]}, {qts[4], qts[5], qts[6]}, qts[7]);
        {
            const bh::SceneTransform I = T.inverse() * T;
            double off = std::fabs(I.rec.q[0] - 1.0) + std::fabs(I.rec.s - 1.0);
            for (int k = 0; k < 3; ++k) off += std::fabs(I.rec.q[1 + k]) + std::fabs(I.rec.t[k]);
            CHECK(off <= 1e-12, "inverse * T is %.3e from the identity", off);
            const bh::SceneTransform U({0.5, 0.5, -0.5, 0.5}, {1.0, -2.0, 0.5}, 2.0), TU = T * U;
            CHECK(std::fabs(TU.rec.s - T.rec.s * 2.0) <= 1e-12 * TU.rec.s, "scale of a product");
            // U first: the origin goes to U.t, then through T
            double want[3];
            for (int i = 0; i < 3; ++i)
                want[i] = T.rec.s * ((double)T.rec.rot[3 * i] * 1.0 + (double)T.rec.rot[3 * i + 1] * -2.0 + (double)T.rec.rot[3 * i + 2] * 0.5) + T.rec.t[i];
            for (int i = 0; i < 3; ++i) CHECK(std::fabs(TU.rec.t[i] - want[i]) <= 1e-5 * (1.0 + std::fabs(want[i])), "translation of a product: %g against %g", TU.rec.t[i], want[i]);
            CHECK(T.sh_rotation(1) == T.rec.sh_rot && T.sh_rotation(4) == T.rec.sh_rot + 83, "sh_rotation offsets");
            std::printf("ok scene record\n");
        }

        bh::Context ctx(0);
        bh::Splats s = bh::Splats::from_host(tr, sh, op);
        s.with_min_scale(bh::DeviceBuffer<float>(ms));

        // ---- the transform ----
        {
            const bh::Splats moved = bh::transformed_splats(ctx, s, T);
            CHECK(same_bits(moved.transforms.download(), want_tr), "transformed_splats: transforms differ from Python's");
            CHECK(same_bits(moved.sh_coeffs.download(), want_sh), "transformed_splats: SH differs from Python's");
            CHECK(same_bits(moved.min_scale->download(), want_ms), "transformed_splats: min_scale differs from Python's");
            CHECK(same_bits(moved.raw_opacities.download(), op) && same_bits(s.transforms.download(), tr), "transformed_splats touched its input or the opacities");
            bh::Splats copy = bh::Splats::from_host(tr, sh, op);
            copy.with_min_scale(bh::DeviceBuffer<float>(ms));
            bh::transform_splats(ctx, copy, T);
            ctx.sync();
            CHECK(same_bits(copy.transforms.download(), want_tr) && same_bits(copy.sh_coeffs.download(), want_sh) && same_bits(copy.min_scale->download(), want_ms),
                  "in place differs from out of place");
            // the camera: W' x' + tv' = s (W x + tv) for the first splat's mean
            bh::Camera cam;
            cam.position[0] = 0.3f; cam.position[2] = -1.0f;
            const BhCamera u = cam.uniforms(64, 48), v = T.apply(u);
            for (int i = 0; i < 3; ++i) {
                double a = u.vm[9 + i], b = v.vm[9 + i];
                for (int j = 0; j < 3; ++j) { a += (double)u.vm[3 * j + i] * tr[j]; b += (double)v.vm[3 * j + i] * want_tr[j]; }
                CHECK(std::fabs(b - T.rec.s * a) <= 1e-5 * T.rec.s * (1.0 + std::fabs(a)), "camera space: %g against %g", b, T.rec.s * a);
            }
            CHECK(v.fx == u.fx && v.img_w == u.img_w && v.model == u.model, "the camera's other fields changed");
            std::printf("ok scene transform\n");
        }

        // ---- select and crop ----
        {
            uint32_t count = 0;
            const bh::DeviceBuffer<float> keep = bh::select_region(ctx, s, region, &count);
            CHECK(same_bits(keep.download(), want_keep) && count == kept, "select_region: flags or count (%u against %u) differ from Python's", count, kept);
            std::vector<uint32_t> idx;
            const bh::Splats crop = bh::crop_splats(ctx, s, region, &idx);
            CHECK(crop.num_splats() == kept && same_bits(crop.transforms.download(), want_crop), "crop_splats: rows differ from Python's");
            bool same_idx = idx.size() == kept;
            for (uint32_t k = 0; same_idx && k < kept; ++k) same_idx = idx[k] == (uint32_t)want_idx[k] && (k == 0 || idx[k] > idx[k - 1]);
            CHECK(same_idx, "crop_splats: indices differ from Python's or are out of order");
            std::printf("ok scene crop (%u of %u)\n", kept, n);
        }

        // ---- refusals ----
        {
            bool refused = false;
            try { (void)bh::SceneTransform({0.0, 0.0, 0.0, 0.0}); } catch (const bh::Error&) { refused = true; }
            CHECK(refused, "a zero quaternion was accepted");
            refused = false;
            try { (void)T.sh_rotation(5); } catch (const bh::Error&) { refused = true; }
            CHECK(refused, "band 5 was accepted");
            refused = false;
            BhSceneRegion bad = region;
            bad.kind = 2u;
            try { (void)bh::select_region(ctx, s, bad); } catch (const bh::Error&) { refused = true; }
            CHECK(refused, "an unknown region kind was accepted");
            CHECK(n < 2 || bh_splats_transform(ctx.get(), &T.rec, n - 1, coeffs, s.transforms.data(), nullptr, nullptr, s.transforms.data() + 10, nullptr, nullptr) == BH_ERR_INVALID_ARG,
                  "an overlapping output was accepted");
            CHECK(same_bits(s.transforms.download(), tr), "a refused call wrote");
            std::printf("ok scene arguments\n");
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        ++g_failed;
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all C++ scene checks passed\n");
    return 0;
}
