// test_mesh.cpp — mesh extraction through the C++ host mirror (include/brush_hip.hpp TsdfVolume, mesh_to_ply):
//   * without a device: the surface compiles and links, the structs have the header's sizes, a null context is refused before the
//     device is touched;
//   * on the GPU: a cleared volume extracts to nothing, an analytic sphere (20^3 samples, T = clip((|p| - 0.6) / 0.3)) extracts to the
//     2030 vertices and 4056 triangles of the rule in brush_hip_mesh.h — closed, consistently oriented, of positive volume, every
//     index in range, two runs the same bits —, one fronto-parallel view integrates to the header's running mean bit for bit (a host
//     loop with every f32 operation rounded on its own), a batch of views equals single-view calls, refusals leave the volume alone,
//     and the PLY has the header and the size the format states.
// Build + run: tests/test_mesh_cpp.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>

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

static BhCamera pinhole(uint32_t w, uint32_t h, float f, float tz) {
    BhCamera c{};
    c.vm[0] = c.vm[4] = c.vm[8] = 1.0f;   // identity rotation, column-major
    c.vm[11] = tz;
    c.fx = c.fy = f;
    c.cx = 0.5f * (float)w - 0.25f;
    c.cy = 0.5f * (float)h + 0.125f;
    c.img_w = w; c.img_h = h;
    c.model = BH_CAMERA_PINHOLE;
    return c;
}

static void host_checks() {
    static_assert(sizeof(BhTsdfGrid) == 56 && sizeof(BhTsdfIntegrateConfig) == 16 && BH_TSDF_MAX_BATCH == 8u, "brush_hip_mesh.h layout");
    BhTsdfGrid g{};
    g.voxel_size = 1.0f; g.nx = g.ny = g.nz = 4; g.trunc = 4.0f; g.max_weight = 8.0f;
    const BhTsdfIntegrateConfig cfg{0.0f, INFINITY, 0.5f, 0u};
    uint32_t nv = 7, nt = 7;
    uint64_t size = 7;
    CHECK(bh_tsdf_clear(nullptr, &g) == BH_ERR_INVALID_ARG, "clear took a null context");
    CHECK(bh_tsdf_integrate(nullptr, &g, 0, nullptr, nullptr, nullptr, &cfg) == BH_ERR_INVALID_ARG, "integrate took a null context");
    CHECK(bh_tsdf_extract_count(nullptr, &g, &nv, &nt) == BH_ERR_INVALID_ARG, "extract_count took a null context");
    CHECK(bh_tsdf_extract(nullptr, &g, nullptr, nullptr, nullptr, 0, 0, &nv, &nt) == BH_ERR_INVALID_ARG, "extract took a null context");
    CHECK(bh_mesh_to_ply(nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, &size) == BH_ERR_INVALID_ARG, "mesh_to_ply took a null context");
    CHECK(nv == 7 && nt == 7 && size == 7, "a refused call wrote its outputs");
    std::printf("ok mesh host checks\n");
}

int main() {
    try {
        host_checks();
        int dev_count = 0;
        if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
            std::printf("no HIP device: host checks only\n");
            return g_failed ? 1 : 0;
        }
        bh::Context ctx(0);
        {   // ---- extraction: the analytic sphere
            const uint32_t n = 20;
            const float org = -0.95f, vs = 0.1f, r = 0.6f;
            bh::TsdfVolume vol(ctx, {org, org, org}, vs, {n, n, n}, 0.0f, 64.0f, /*colour=*/false);
            CHECK(vol.count() == std::make_pair(0u, 0u), "a cleared volume has a surface");
            const bh::Mesh none = vol.extract();
            CHECK(none.n_vertices == 0 && none.n_triangles == 0, "a cleared volume extracted something");
            std::vector<float> tw((size_t)n * n * n * 2);
            for (uint32_t k = 0; k < n; ++k)
                for (uint32_t j = 0; j < n; ++j)
                    for (uint32_t i = 0; i < n; ++i) {
                        const double x = org + vs * (float)i, y = org + vs * (float)j, z = org + vs * (float)k;
                        const double t = (std::sqrt(x * x + y * y + z * z) - r) / 0.3;
                        const size_t s = ((size_t)k * n + j) * n + i;
                        tw[2 * s] = (float)std::fmin(std::fmax(t, -1.0), 1.0);
                        tw[2 * s + 1] = 1.0f;
                    }
            vol.set_tw(tw);
            const bh::Mesh m = vol.extract();
            CHECK(m.n_vertices == 2030 && m.n_triangles == 4056, "sphere: %u vertices, %u triangles (2030, 4056)", m.n_vertices, m.n_triangles);
            const std::vector<float> v = m.vertices.download();
            const std::vector<uint32_t> t = m.triangles.download();
            std::map<std::pair<uint32_t, uint32_t>, int> edges;
            std::vector<int> used(m.n_vertices, 0);
            double volume = 0.0, worst = 0.0;
            bool in_range = true;
            for (uint32_t f = 0; f < m.n_triangles && in_range; ++f) {
                const uint32_t* q = &t[3 * (size_t)f];
                in_range = q[0] < m.n_vertices && q[1] < m.n_vertices && q[2] < m.n_vertices;
                if (!in_range) break;
                for (int c = 0; c < 3; ++c) { ++edges[{q[c], q[(c + 1) % 3]}]; used[q[c]] = 1; }
                const float *a = &v[3 * (size_t)q[0]], *b = &v[3 * (size_t)q[1]], *c = &v[3 * (size_t)q[2]];
                volume += (a[0] * ((double)b[1] * c[2] - (double)b[2] * c[1]) - a[1] * ((double)b[0] * c[2] - (double)b[2] * c[0]) +
                           a[2] * ((double)b[0] * c[1] - (double)b[1] * c[0])) / 6.0;
            }
            CHECK(in_range, "a triangle index is out of range");
            if (in_range) {
                bool closed = edges.size() == 2 * 6084u;
                for (const auto& e : edges) closed = closed && e.second == 1 && edges.count({e.first.second, e.first.first}) == 1;
                CHECK(closed, "the sphere is not a closed, consistently oriented surface (%zu directed edges)", edges.size());
                bool all_used = true;
                for (int u : used) all_used = all_used && u;
                CHECK(all_used, "an unreferenced vertex");
                for (uint32_t p = 0; p < m.n_vertices; ++p)
                    worst = std::fmax(worst, std::fabs(std::sqrt((double)v[3 * p] * v[3 * p] + (double)v[3 * p + 1] * v[3 * p + 1] + (double)v[3 * p + 2] * v[3 * p + 2]) - r) / vs);
                const double ratio = volume / (4.0 / 3.0 * 3.14159265358979323846 * r * r * r);
                CHECK(ratio >= 0.98 && ratio < 1.0 && worst <= 0.07, "volume ratio %.5f, radial error %.4f voxel", ratio, worst);
                std::printf("ok mesh sphere (volume ratio %.5f, radial error %.4f voxel)\n", ratio, worst);
            }
            const bh::Mesh again = vol.extract();
            CHECK(same_bits(again.vertices.download(), v) && again.triangles.download() == t, "two extractions differ");
            uint32_t nv = 0, nt = 0;
            bh::DeviceBuffer<float> small_v(3 * 100);
            bh::DeviceBuffer<uint32_t> small_t(3 * 100);
            CHECK(bh_tsdf_extract(ctx.get(), &vol.grid(), small_v.data(), nullptr, small_t.data(), 100, 100, &nv, &nt) == BH_ERR_INVALID_ARG && nv == 2030 && nt == 4056,
                  "a capacity too small: counts %u, %u", nv, nt);
            const std::vector<uint8_t> ply = vol.to_ply();
            const std::string want = "ply\nformat binary_little_endian 1.0\ncomment Exported from Brush\nelement vertex 2030\nproperty float x\nproperty float y\n"
                                     "property float z\nelement face 4056\nproperty list uchar uint vertex_indices\nend_header\n";
            CHECK(ply.size() == want.size() + 2030u * 12u + 4056u * 13u && std::memcmp(ply.data(), want.data(), want.size()) == 0, "PLY header or size (%zu bytes)", ply.size());
            CHECK(std::memcmp(ply.data() + want.size(), v.data(), 2030u * 12u) == 0 && ply[want.size() + 2030u * 12u] == 3, "PLY body");
            std::printf("ok mesh ply\n");
        }
        {   // ---- integration: one view against a host loop of the header's rule, then batching
            const uint32_t nx = 9, ny = 7, nz = 6, w = 16, h = 12;
            const float org[3] = {-0.8f, -0.6f, 0.3f}, vs = 0.2f, trunc = 0.5f;
            const BhCamera cam = pinhole(w, h, 14.0f, 0.7f);
            std::vector<float> depth((size_t)w * h), image((size_t)w * h * 4);
            for (uint32_t p = 0; p < w * h; ++p) {
                depth[p] = 1.3f + 0.01f * (float)(p % w) - 0.02f * (float)(p / w);
                image[4 * p] = 0.1f * (float)(p % 7); image[4 * p + 1] = 0.3f; image[4 * p + 2] = 0.05f * (float)(p % 11);
                image[4 * p + 3] = (p % 5 == 0) ? 0.25f : 0.9f;
            }
            depth[5] = 0.0f; depth[6] = NAN; depth[7] = -1.0f;
            const bh::DeviceBuffer<float> depth_dev(depth), image_dev(image);
            bh::TsdfVolume vol(ctx, {org[0], org[1], org[2]}, vs, {nx, ny, nz}, trunc, 2.0f);
            vol.integrate({cam}, {depth_dev.data()}, {image_dev.data()}, 0.4f, 1.45f, 0.5f);
            vol.integrate({cam}, {depth_dev.data()}, {image_dev.data()}, 0.4f, 1.45f, 0.5f);
            vol.integrate({cam}, {depth_dev.data()}, {image_dev.data()}, 0.4f, 1.45f, 0.5f);
            const std::vector<float> tw = vol.tw(), rgb = vol.rgb();
            uint32_t touched = 0, wrong = 0;
            for (uint32_t k = 0; k < nz; ++k)
                for (uint32_t j = 0; j < ny; ++j)
                    for (uint32_t i = 0; i < nx; ++i) {
                        volatile float T = 1.0f, W = 0.0f, c[3] = {0.0f, 0.0f, 0.0f};
                        volatile float mx = vs * (float)i, my = vs * (float)j, mz = vs * (float)k;
                        volatile float px = org[0] + mx, py = org[1] + my, pz = org[2] + mz;
                        for (int rep = 0; rep < 3; ++rep) {
                            volatile float a0 = cam.vm[0] * px, a1 = cam.vm[3] * py, a2 = cam.vm[6] * pz;
                            volatile float b0 = cam.vm[1] * px, b1 = cam.vm[4] * py, b2 = cam.vm[7] * pz;
                            volatile float c0 = cam.vm[2] * px, c1 = cam.vm[5] * py, c2 = cam.vm[8] * pz;
                            volatile float a01 = a0 + a1, b01 = b0 + b1, c01 = c0 + c1;
                            volatile float a012 = a01 + a2, b012 = b01 + b2, c012 = c01 + c2;
                            volatile float X = a012 + cam.vm[9], Y = b012 + cam.vm[10], Z = c012 + cam.vm[11];
                            if (!(Z > 0.4f)) continue;
                            volatile float xz = X / Z, yz = Y / Z;
                            volatile float fu = cam.fx * xz, fv = cam.fy * yz;
                            volatile float u = fu + cam.cx, v = fv + cam.cy;
                            if (!(u >= 0.0f && u < (float)w && v >= 0.0f && v < (float)h)) continue;
                            const size_t p = (size_t)std::floor(v) * w + (size_t)std::floor(u);
                            const float d = depth[p];
                            if (!(std::isfinite(d) && d > 0.0f && d <= 1.45f)) continue;
                            if (image[4 * p + 3] < 0.5f) continue;
                            volatile float sdf = d - Z;
                            if (sdf < -trunc) continue;
                            volatile float q = sdf / trunc;
                            const float s = q < 1.0f ? q : 1.0f;
                            volatile float Wn = W + 1.0f;
                            volatile float wt = W * T;
                            volatile float num = wt + s;
                            T = num / Wn;
                            for (int ch = 0; ch < 3; ++ch) {
                                volatile float wc = W * c[ch];
                                volatile float nc = wc + image[4 * p + ch];
                                c[ch] = nc / Wn;
                            }
                            W = Wn < 2.0f ? Wn : 2.0f;
                        }
                        const size_t s = ((size_t)k * ny + j) * nx + i;
                        const float want[5] = {T, W, c[0], c[1], c[2]};
                        const float got[5] = {tw[2 * s], tw[2 * s + 1], rgb[3 * s], rgb[3 * s + 1], rgb[3 * s + 2]};
                        if (std::memcmp(want, got, sizeof(want)) != 0) ++wrong;
                        if (W > 0.0f) ++touched;
                    }
            CHECK(wrong == 0 && touched > 20 && touched < nx * ny * nz, "%u of %u samples differ from the header's rule (%u touched)", wrong, nx * ny * nz, touched);
            std::printf("ok mesh integrate (%u samples touched)\n", touched);

            // 11 views in one call == 11 single calls
            std::vector<BhCamera> cams;
            std::vector<const float*> depths, images;
            for (int n = 0; n < 11; ++n) {
                cams.push_back(pinhole(w, h, 12.0f + (float)n, 0.7f + 0.03f * (float)n));
                depths.push_back(depth_dev.data());
                images.push_back(image_dev.data());
            }
            bh::TsdfVolume batched(ctx, {org[0], org[1], org[2]}, vs, {nx, ny, nz}, trunc, 4.0f), single(ctx, {org[0], org[1], org[2]}, vs, {nx, ny, nz}, trunc, 4.0f);
            batched.integrate(cams, depths, images, 0.4f);
            for (int n = 0; n < 11; ++n) single.integrate({cams[n]}, {depths[n]}, {images[n]}, 0.4f);
            CHECK(same_bits(batched.tw(), single.tw()) && same_bits(batched.rgb(), single.rgb()), "a batch of 11 views differs from 11 single calls");
            float wmax = 0.0f;
            const std::vector<float> btw = batched.tw();
            for (size_t s = 0; s < batched.samples(); ++s) wmax = std::fmax(wmax, btw[2 * s + 1]);
            CHECK(wmax == 4.0f, "the weight did not saturate at max_weight (largest %g)", wmax);
            std::printf("ok mesh batching\n");

            // refusals leave the volume alone
            const std::vector<float> before = batched.tw();
            BhCamera fish = cams[0];
            fish.model = BH_CAMERA_KANNALA_BRANDT_4;
            BhCamera window = cams[0];
            window.tile_row_begin = 0; window.tile_row_end = 1;
            for (const BhCamera& bad : {fish, window}) {
                bool threw = false;
                try { batched.integrate({cams[1], bad}, {depths[0], depths[0]}, {images[0], images[0]}); } catch (const bh::Error& e) { threw = e.code == BH_ERR_INVALID_ARG; }
                CHECK(threw, "a camera that is no whole pinhole frame was accepted");
            }
            BhTsdfGrid g = batched.grid();
            g.trunc = 0.0f;
            CHECK(bh_tsdf_clear(ctx.get(), &g) == BH_ERR_INVALID_ARG, "trunc 0 was accepted");
            g = batched.grid();
            g.nx = 1;
            CHECK(bh_tsdf_clear(ctx.get(), &g) == BH_ERR_INVALID_ARG, "a dimension of 1 was accepted");
            g = batched.grid();
            g.nx = 2048; g.ny = 1024; g.nz = 1024;
            uint32_t nv = 0, nt = 0;
            CHECK(bh_tsdf_extract_count(ctx.get(), &g, &nv, &nt) == BH_ERR_INVALID_ARG, "2^31 samples were accepted");
            CHECK(same_bits(batched.tw(), before), "a refused call changed the volume");
            std::printf("ok mesh refusals\n");
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (g_failed) { std::printf("%d C++ mesh check(s) FAILED\n", g_failed); return 1; }
    std::printf("all C++ mesh checks passed\n");
    return 0;
}
