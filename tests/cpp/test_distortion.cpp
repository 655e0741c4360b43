// test_distortion.cpp — distortion maps through the C++ host mirror (include/brush_hip.hpp RenderNode::distortion /
// backward_distortion, distortion_loss, train_set_distortion; include/brush_hip_distortion.h), against numbers the Python side wrote:
//   * argv[1] is a file tests/test_distortion_cpp.py wrote: a scene, a cotangent, and what brush_amd/host.py got for them on this
//     GPU — the distortion map (both kinds), the loss, and the gradients of the distortion term alone;
//   * the forward: both maps within 1e-5 of their maximum (the two mirrors set the camera up on their own), non-negative up to
//     rounding, two calls and the moment map to the same bits;
//   * the loss: bh_distortion_loss of the map against Python's, and of the moment map to the same bits;
//   * the backward: v_transforms and v_raw_opacities within 1e-4 of Python's largest entry, SH and refine weight untouched, and the
//     term beside a colour term equals the sum of the two;
//   * refusals: an unknown kind, near >= far, a stale node; train_set_distortion attaches and detaches.
// Without an argument or without a device it only proves that it compiles, links and starts.  Build + run: tests/test_distortion_cpp.py.
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

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0;
}

static double max_abs(const std::vector<float>& v) {
    double m = 0.0;
    for (float x : v) m = std::fmax(m, std::fabs((double)x));
    return m;
}

static double max_diff(const std::vector<float>& a, const std::vector<float>& b) {
    if (a.size() != b.size()) return INFINITY;
    double m = 0.0;
    for (size_t i = 0; i < a.size(); ++i) m = std::fmax(m, std::isfinite(a[i]) ? std::fabs((double)a[i] - (double)b[i]) : INFINITY);
    return m;
}

// the default camera of brush_amd/synth.py: origin, identity rotation, 60 degrees across, square pixels
static bh::Camera default_camera(uint32_t w, uint32_t h) {
    bh::Camera cam;
    cam.fov_x = 60.0 * 3.14159265358979323846 / 180.0;
    const double fx = (w / 2.0) / std::tan(cam.fov_x / 2.0);
    cam.fov_y = 2.0 * std::atan((h / 2.0) / fx);
    return cam;
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
        float cfgf[4];
        if (std::fread(hdr, 4, 4, f) != 4 || std::fread(cfgf, 4, 4, f) != 4) { std::printf("FAIL short header\n"); return 1; }
        const uint32_t n = hdr[0], w = hdr[1], h = hdr[2], coeffs = hdr[3];
        const float near_z = cfgf[0], far_z = cfgf[1], weight = cfgf[2];
        const size_t hw = (size_t)w * h;
        const std::vector<float> tr = read_floats(f, (size_t)n * 10), sh = read_floats(f, (size_t)n * coeffs * 3), op = read_floats(f, n);
        const std::vector<float> v_dist = read_floats(f, hw), v_out = read_floats(f, hw * 4);
        const std::vector<float> want_z = read_floats(f, hw), want_ndc = read_floats(f, hw), want_loss = read_floats(f, 2);
        const std::vector<float> want_vt_z = read_floats(f, (size_t)n * 10), want_vo_z = read_floats(f, n);
        const std::vector<float> want_vt_ndc = read_floats(f, (size_t)n * 10), want_vo_ndc = read_floats(f, n);
        std::fclose(f);

        bh::Context ctx(0);
        const bh::Splats s = bh::Splats::from_host(tr, sh, op);
        const bh::Camera cam = default_camera(w, h);
        const float black[3] = {0.0f, 0.0f, 0.0f};
        BhDistortionConfig zc{};
        zc.kind = BH_DISTORTION_Z;
        BhDistortionConfig nc{};
        nc.kind = BH_DISTORTION_NDC;
        nc.near_z = near_z;
        nc.far_z = far_z;

        bh::RenderNode node(ctx, s, cam, w, h, black, /*retain=*/true);
        // ---- the forward ----
        const std::vector<float> dz = node.distortion(zc).download(), dn = node.distortion(nc).download();
        const std::vector<float> mo = node.distortion(zc, /*moments=*/true).download();
        CHECK(dz.size() == hw && dn.size() == hw && mo.size() == hw * 4, "map sizes %zu %zu %zu", dz.size(), dn.size(), mo.size());
        const double top_z = max_abs(want_z), top_n = max_abs(want_ndc);
        CHECK(top_z > 0.0 && top_n > 0.0, "Python's maps are empty");
        CHECK(max_diff(dz, want_z) <= 1e-5 * top_z, "kind z: the map differs from Python's by %.3e of %.3e", max_diff(dz, want_z), top_z);
        CHECK(max_diff(dn, want_ndc) <= 1e-5 * top_n, "kind ndc: the map differs from Python's by %.3e of %.3e", max_diff(dn, want_ndc), top_n);
        double low = 0.0;
        bool restated = true;
        for (size_t p = 0; p < hw; ++p) {
            low = std::fmin(low, (double)dz[p]);
            restated = restated && dz[p] == std::fma(mo[p * 4], mo[p * 4 + 2], -(mo[p * 4 + 1] * mo[p * 4 + 1]));
        }
        CHECK(low >= -1e-5 * top_z, "a distortion of %.3e", low);
        CHECK(restated, "the value map is not fma(A, M2', -(M1' M1')) of the moment map");
        CHECK(same_bits(node.distortion(zc).download(), dz) && same_bits(node.distortion(nc).download(), dn), "two calls on one saved state differ");
        std::printf("ok distortion forward (max %.4e / %.4e)\n", top_z, top_n);

        // ---- the loss ----
        {
            bh::DeviceBuffer<float> map(dz), moments(mo), loss, loss2;
            loss.resize(2);
            loss2.resize(2);
            bh::distortion_loss(ctx, map.data(), h, w, 1, weight, loss.data());
            bh::distortion_loss(ctx, moments.data(), h, w, 4, weight, loss2.data());
            ctx.sync();
            const std::vector<float> l = loss.download(), l2 = loss2.download();
            CHECK(std::fabs((double)l[0] - want_loss[0]) <= 1e-5 * std::fabs(want_loss[0]) && l[1] == (float)hw, "loss %.8e against Python's %.8e", l[0], want_loss[0]);
            CHECK(same_bits(l, l2), "the moment map's loss differs from the value map's");
            std::printf("ok distortion loss (%.6e)\n", l[0]);
        }

        // ---- the backward ----
        {
            bh::DeviceBuffer<float> vd_dev(v_dist), vo_dev(v_out);
            const bh::SplatGrads gz = node.backward_distortion(vd_dev.data(), zc), gn = node.backward_distortion(vd_dev.data(), nc);
            const std::vector<float> vt_z = gz.v_transforms.download(), vo_z = gz.v_raw_opacities.download();
            CHECK(max_diff(vt_z, want_vt_z) <= 1e-4 * max_abs(want_vt_z) && max_abs(want_vt_z) > 0.0, "kind z: v_transforms differ by %.3e of %.3e",
                  max_diff(vt_z, want_vt_z), max_abs(want_vt_z));
            CHECK(max_diff(vo_z, want_vo_z) <= 1e-4 * max_abs(want_vo_z), "kind z: v_raw_opacities differ by %.3e of %.3e", max_diff(vo_z, want_vo_z), max_abs(want_vo_z));
            CHECK(max_diff(gn.v_transforms.download(), want_vt_ndc) <= 1e-4 * max_abs(want_vt_ndc) && max_abs(want_vt_ndc) > 0.0, "kind ndc: v_transforms differ by %.3e of %.3e",
                  max_diff(gn.v_transforms.download(), want_vt_ndc), max_abs(want_vt_ndc));
            CHECK(max_diff(gn.v_raw_opacities.download(), want_vo_ndc) <= 1e-4 * max_abs(want_vo_ndc), "kind ndc: v_raw_opacities differ");
            CHECK(max_abs(gz.v_sh_coeffs.download()) == 0.0 && max_abs(gz.v_refine_weight.download()) == 0.0, "a distortion-only backward wrote SH or the refine weight");
            // beside a colour term: the sum of the two
            const bh::SplatGrads gc = node.backward(vo_dev.data());
            const bh::SplatGrads gb = node.backward_distortion(vo_dev.data(), nullptr, BH_DEPTH_EXPECTED, nullptr, BH_NORMAL_ACCUMULATED, vd_dev.data(), zc);
            const std::vector<float> c = gc.v_transforms.download(), b = gb.v_transforms.download();
            double diff = 0.0, top = 0.0;
            for (size_t i = 0; i < b.size(); ++i) {
                diff = std::fmax(diff, std::fabs((double)b[i] - ((double)c[i] + (double)vt_z[i])));
                top = std::fmax(top, std::fabs((double)b[i]));
            }
            CHECK(diff <= 1e-4 * top && top > 0.0, "two terms differ from the sum of the two by %.3e of %.3e", diff, top);
            std::printf("ok distortion backward\n");
        }

        // ---- refusals, and the train term's switch ----
        {
            bool refused = false;
            BhDistortionConfig bad{};
            bad.kind = 2u;
            try { (void)node.distortion(bad); } catch (const bh::Error&) { refused = true; }
            CHECK(refused, "an unknown kind was accepted");
            refused = false;
            bad.kind = BH_DISTORTION_NDC;
            bad.near_z = 2.0f;
            bad.far_z = 1.0f;
            try { (void)node.distortion(bad); } catch (const bh::Error&) { refused = true; }
            CHECK(refused, "far <= near was accepted");
            bh::RenderNode fresh(ctx, s, cam, w, h, black);
            bh::Camera other = cam;
            other.position[0] = 0.8f;
            (void)bh::render_splats(ctx, s, other, w, h, black, bh::RasterPass::Backward);
            refused = false;
            try { (void)fresh.distortion(zc); } catch (const bh::Error& e) { refused = std::strstr(e.what(), "stale") != nullptr; }
            CHECK(refused, "a stale node was accepted");
            CHECK(same_bits(node.distortion(zc).download(), dz), "retained forward: the map differs");
            bh::train_set_distortion(ctx, 0.5f, BH_DISTORTION_NDC, near_z, far_z);
            refused = false;
            try { bh::train_set_distortion(ctx, 0.5f, 2u); } catch (const bh::Error&) { refused = true; }
            CHECK(refused, "train_set_distortion accepted an unknown kind");
            bh::train_set_distortion(ctx, nullptr);
            std::printf("ok distortion arguments\n");
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        ++g_failed;
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("all C++ distortion checks passed\n");
    return 0;
}
