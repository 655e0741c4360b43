// test_depth.cpp — depth maps through the C++ host mirror (include/brush_hip.hpp RenderNode::depth / backward(v_output, v_depth, mode)):
//   * accumulated depth of a depth-coloured scene (SH degree 0 colour == camera z) against a reference image of its channel 0
//     within the derived bound (n + 3) 2^-24 (z_max + 0.5), n = the frame's longest tile list.  The driver
//     (tests/test_depth_cpp.py) writes the scene and the CPU oracle's image into a directory: test_depth <dir> <n> <w> <h>;
//     without arguments the scene is made here and the reference is the node's own colour image;
//   * bit identity: two calls on one saved state, a retained forward after another forward, expected == accumulated / alpha;
//   * the backward overload: v_output == nullptr, both terms against the sum of the two, the refine weight, a 3D-filter floor.
// Build + run: tests/test_depth_cpp.py.
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

static const float kC0 = 0.2820947917738781f;

static std::vector<float> read_floats(const std::string& path, size_t count) {
    std::vector<float> v(count);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(v.data(), 4, count, f) != count) throw std::runtime_error("cannot read " + path);
    std::fclose(f);
    return v;
}

template <class T>
static std::vector<T> download(const T* dev, size_t n) {
    std::vector<T> out(n);
    bh::hip_check(hipMemcpy(out.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    return out;
}

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0;
}

// the default camera of brush_amd/synth.py: origin, identity rotation, 60 degrees across, square pixels
static bh::Camera default_camera(uint32_t w, uint32_t h) {
    bh::Camera cam;
    cam.fov_x = 60.0 * 3.14159265358979323846 / 180.0;
    const double fx = (w / 2.0) / std::tan(cam.fov_x / 2.0);
    cam.fov_y = 2.0 * std::atan((h / 2.0) / fx);
    return cam;
}

int main(int argc, char** argv) {
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        std::printf("no HIP device: compile-only run\n");
        return 0;
    }
    try {
        bh::Context ctx(0);
        uint32_t n = 3000, w = 123, h = 82;
        std::vector<float> tr, sh, op, ref;
        if (argc == 5) {
            const std::string dir = argv[1];
            n = (uint32_t)std::atoi(argv[2]); w = (uint32_t)std::atoi(argv[3]); h = (uint32_t)std::atoi(argv[4]);
            tr = read_floats(dir + "/transforms.bin", (size_t)n * 10);
            sh = read_floats(dir + "/sh.bin", (size_t)n * 3);
            op = read_floats(dir + "/raw_opac.bin", n);
            ref = read_floats(dir + "/oracle_channel0.bin", (size_t)w * h);
        } else {
            Sm64 r{0xDE97};
            tr.resize((size_t)n * 10); sh.resize((size_t)n * 3); op.resize(n);
            for (uint32_t i = 0; i < n; ++i) {
                float* row = &tr[(size_t)i * 10];
                row[2] = r.uni(2.0f, 12.0f);
                row[0] = r.uni(-0.6f, 0.6f) * row[2]; row[1] = r.uni(-0.4f, 0.4f) * row[2];
                row[3] = 1.0f; row[4] = r.uni(-0.3f, 0.3f); row[5] = r.uni(-0.3f, 0.3f); row[6] = r.uni(-0.3f, 0.3f);
                for (int k = 7; k < 10; ++k) row[k] = r.uni(std::log(0.03f), std::log(0.3f));
                op[i] = r.uni(-2.0f, 2.5f);
                for (int c = 0; c < 3; ++c) sh[(size_t)i * 3 + c] = (row[2] - 0.5f) / kC0;
            }
        }
        const size_t hw = (size_t)w * h;
        float zmax = 0.0f;
        for (uint32_t i = 0; i < n; ++i) zmax = std::fmax(zmax, tr[(size_t)i * 10 + 2]);
        const bh::Splats s = bh::Splats::from_host(tr, sh, op);
        const bh::Camera cam = default_camera(w, h);
        const float black[3] = {0.0f, 0.0f, 0.0f};

        // ---- accumulated depth against the reference image, within the derived bound ----
        {
            bh::RenderNode node(ctx, s, cam, w, h, black);
            ctx.sync();   // (the node's image is read with a blocking copy, which does not wait for the ctx stream)
            const std::vector<float> img = download(node.aux.raw.out_img, hw * 4);
            if (ref.empty()) { ref.resize(hw); for (size_t p = 0; p < hw; ++p) ref[p] = img[p * 4]; }
            const std::vector<uint32_t> to = download(node.aux.raw.tile_offsets, (size_t)node.aux.raw.num_tiles * 2);
            uint32_t longest = 0;
            for (uint32_t t = 0; t < node.aux.raw.num_tiles; ++t) longest = std::max(longest, to[t * 2 + 1] - to[t * 2]);
            const double bound = (double)(longest + 3) * std::ldexp(1.0, -24) * ((double)zmax + 0.5);
            const std::vector<float> acc = node.depth(BH_DEPTH_ACCUMULATED).download();
            double err = 0.0, top = 0.0;
            for (size_t p = 0; p < hw; ++p) { err = std::fmax(err, std::fabs((double)acc[p] - (double)ref[p])); top = std::fmax(top, acc[p]); }
            CHECK(top > 1.0, "the frame is empty (max depth %g)", top);
            CHECK(err <= bound, "max |dD| %.3e beyond the bound %.3e (longest list %u)", err, bound, longest);
            std::printf("ok accumulated depth (max |dD| %.3e, bound %.3e, longest list %u, %s reference)\n", err, bound, longest, argc == 5 ? "oracle" : "colour-path");
            // ---- bit identity ----
            CHECK(same_bits(node.depth(BH_DEPTH_ACCUMULATED).download(), acc), "two calls on one saved state differ");
            const std::vector<float> exp = node.depth(BH_DEPTH_EXPECTED).download();
            size_t bad = 0;
            for (size_t p = 0; p < hw; ++p) {
                const float a = img[p * 4 + 3];
                const float want = a == 0.0f ? 0.0f : acc[p] / a;
                bad += std::memcmp(&want, &exp[p], 4) != 0;
            }
            CHECK(bad == 0, "expected != accumulated / alpha at %zu pixels", bad);
            const std::vector<float> med = node.depth(BH_DEPTH_MEDIAN).download();
            size_t found = 0;
            bad = 0;
            for (size_t p = 0; p < hw; ++p) {
                found += med[p] != 0.0f;
                if (med[p] != 0.0f && !(med[p] >= 2.0f && med[p] <= zmax && img[p * 4 + 3] >= 0.5f)) ++bad;
            }
            CHECK(found > 0 && bad == 0, "median: %zu found, %zu out of range", found, bad);
            bool refused = false;
            try { (void)node.depth(3u); } catch (const bh::Error&) { refused = true; }
            CHECK(refused, "an unknown mode was accepted");
            // a retained forward, after another forward has run
            bh::RenderNode kept(ctx, s, cam, w, h, black, /*retain=*/true);
            bh::Camera other = cam;
            other.position[0] = 0.8f;
            (void)bh::render_splats(ctx, s, other, w, h, black, bh::RasterPass::Backward);
            CHECK(same_bits(kept.depth(BH_DEPTH_ACCUMULATED).download(), acc), "retained forward: accumulated depth differs");
            CHECK(same_bits(kept.depth(BH_DEPTH_EXPECTED).download(), exp), "retained forward: expected depth differs");
            CHECK(same_bits(kept.depth(BH_DEPTH_MEDIAN).download(), med), "retained forward: median depth differs");
            refused = false;
            try { (void)node.depth(BH_DEPTH_EXPECTED); } catch (const bh::Error& e) { refused = std::strstr(e.what(), "stale") != nullptr; }
            CHECK(refused, "a stale node was accepted");
            std::printf("ok depth bit identity\n");

            // ---- the backward overload (on the retained node) ----
            Sm64 r{0xBAC};
            std::vector<float> vd(hw), vo(hw * 4);
            for (auto& v : vd) v = r.uni(-1.0f, 1.0f) / (float)hw;
            for (auto& v : vo) v = r.uni(-1.0f, 1.0f) / (float)hw;
            bh::DeviceBuffer<float> vd_dev(vd), vo_dev(vo);
            for (uint32_t mode : {BH_DEPTH_ACCUMULATED, BH_DEPTH_EXPECTED}) {
                const bh::SplatGrads gd = kept.backward(nullptr, vd_dev.data(), mode);
                const bh::SplatGrads gc = kept.backward(vo_dev.data());
                const bh::SplatGrads gb = kept.backward(vo_dev.data(), vd_dev.data(), mode);
                const std::vector<float> d = gd.v_transforms.download(), c = gc.v_transforms.download(), b = gb.v_transforms.download();
                double top_d = 0.0, top_b = 0.0, diff = 0.0;
                bool finite = true;
                for (size_t i = 0; i < d.size(); ++i) {
                    finite = finite && std::isfinite(d[i]) && std::isfinite(b[i]);
                    top_d = std::fmax(top_d, std::fabs(d[i]));
                    top_b = std::fmax(top_b, std::fabs(b[i]));
                    diff = std::fmax(diff, std::fabs((double)b[i] - ((double)c[i] + (double)d[i])));
                }
                CHECK(finite && top_d > 0.0, "mode %u: depth-only gradient (max %g)", mode, top_d);
                CHECK(diff <= 1e-4 * top_b, "mode %u: both terms differ from the sum of the two by %.3e of %.3e", mode, diff, top_b);
                double rf = 0.0, shg = 0.0;
                for (float v : gd.v_refine_weight.download()) rf = std::fmax(rf, std::fabs(v));
                for (float v : gd.v_sh_coeffs.download()) shg = std::fmax(shg, std::fabs(v));
                CHECK(rf == 0.0 && shg == 0.0, "mode %u: a depth-only backward wrote refine %g / sh %g", mode, rf, shg);
                const std::vector<float> rb = gb.v_refine_weight.download(), rc = gc.v_refine_weight.download();
                double rdiff = 0.0, rtop = 0.0;
                for (size_t i = 0; i < rb.size(); ++i) { rdiff = std::fmax(rdiff, std::fabs((double)rb[i] - rc[i])); rtop = std::fmax(rtop, std::fabs(rc[i])); }
                CHECK(rdiff <= 1e-6 * rtop, "mode %u: the refine weight moved with a depth term (%.3e of %.3e)", mode, rdiff, rtop);
            }
            refused = false;
            try { (void)kept.backward(nullptr, vd_dev.data(), BH_DEPTH_MEDIAN); } catch (const bh::Error&) { refused = true; }
            CHECK(refused, "a median backward was accepted");
            std::printf("ok depth backward\n");
        }
        // ---- a 3D-filter floor: the fold's chain behind the depth backward ----
        {
            bh::Splats f = bh::Splats::from_host(tr, sh, op, /*render_mip=*/true);
            f.min_scale.emplace(std::vector<float>(n, 0.02f));
            bh::RenderNode node(ctx, f, cam, w, h, black);
            std::vector<float> vd(hw, 1.0f / (float)hw);
            bh::DeviceBuffer<float> vd_dev(vd);
            const bh::SplatGrads g = node.backward(nullptr, vd_dev.data(), BH_DEPTH_EXPECTED);
            double top = 0.0;
            bool finite = true;
            for (float v : g.v_transforms.download()) { finite = finite && std::isfinite(v); top = std::fmax(top, std::fabs(v)); }
            for (float v : g.v_raw_opacities.download()) finite = finite && std::isfinite(v);
            CHECK(finite && top > 0.0, "min_scale: gradient max %g", top);
            std::printf("ok depth backward with a 3D-filter floor\n");
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        ++g_failed;
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all C++ depth checks passed\n");
    return 0;
}
