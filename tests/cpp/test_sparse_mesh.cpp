// test_sparse_mesh.cpp — sparse TSDF volumes through the C++ host mirror (include/brush_hip.hpp SparseTsdfVolume):
//   * without a device: the surface compiles and links, the struct has the header's size, a null context is refused before the device
//     is touched and no output is written;
//   * on the GPU: an analytic sphere written into the pool of a 24^3 grid (all 27 blocks, set through set_bits and commit(0)) scatters
//     to the dense volume bit for bit and extracts to as many vertices and triangles as the dense TsdfVolume holding the same field,
//     closed and consistently oriented; one view marked, committed and integrated equals the dense volume fused with the same view on
//     every allocated sample and is cleared elsewhere, with fewer blocks than the grid has; refusals; the PLY's size.
// Build + run: tests/test_sparse_mesh_cpp.py.
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

static BhCamera pinhole(uint32_t w, uint32_t h, float f, float tz) {
    BhCamera c{};
    c.vm[0] = c.vm[4] = c.vm[8] = 1.0f;   // identity rotation, column-major
    c.vm[11] = tz;
    c.cam_pos[2] = -tz;
    c.fx = c.fy = f;
    c.cx = 0.5f * (float)w - 0.25f;
    c.cy = 0.5f * (float)h + 0.125f;
    c.img_w = w; c.img_h = h;
    c.model = BH_CAMERA_PINHOLE;
    return c;
}

static void host_checks() {
    static_assert(sizeof(BhSparseTsdf) == 80 && BH_SPTSDF_BLOCK == 8u && BH_SPTSDF_MAX_DIM == 8192u && BH_SPTSDF_MAX_STEPS == 64u, "brush_hip_sparse_mesh.h layout");
    BhSparseTsdf v{};
    v.voxel_size = 1.0f; v.nx = v.ny = v.nz = 16; v.trunc = 4.0f; v.max_weight = 8.0f;
    BhTsdfGrid g{};
    const BhTsdfIntegrateConfig cfg{0.0f, INFINITY, 0.5f, 0u};
    uint32_t nv = 7, nt = 7, nb = 7;
    CHECK(bh_sptsdf_mark_clear(nullptr, &v) == BH_ERR_INVALID_ARG, "mark_clear took a null context");
    CHECK(bh_sptsdf_mark(nullptr, &v, 0, nullptr, nullptr, nullptr, &cfg) == BH_ERR_INVALID_ARG, "mark took a null context");
    CHECK(bh_sptsdf_commit(nullptr, &v, 1, &nb) == BH_ERR_INVALID_ARG, "commit took a null context");
    CHECK(bh_sptsdf_clear(nullptr, &v) == BH_ERR_INVALID_ARG, "clear took a null context");
    CHECK(bh_sptsdf_integrate(nullptr, &v, 0, nullptr, nullptr, nullptr, &cfg) == BH_ERR_INVALID_ARG, "integrate took a null context");
    CHECK(bh_sptsdf_extract_count(nullptr, &v, &nv, &nt) == BH_ERR_INVALID_ARG, "extract_count took a null context");
    CHECK(bh_sptsdf_extract(nullptr, &v, nullptr, nullptr, nullptr, 0, 0, &nv, &nt) == BH_ERR_INVALID_ARG, "extract took a null context");
    CHECK(bh_sptsdf_to_dense(nullptr, &v, 0, 0, 0, &g) == BH_ERR_INVALID_ARG, "to_dense took a null context");
    CHECK(nv == 7 && nt == 7 && nb == 7, "a refused call wrote its outputs");
    std::printf("ok sparse mesh host checks\n");
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
        {   // ---- extraction: an analytic sphere written into the pool
            const uint32_t n = 24;
            const float org = -1.15f, vs = 0.1f, r = 1.0f;
            bh::SparseTsdfVolume vol(ctx, {org, org, org}, vs, {n, n, n}, 0.0f, 64.0f, /*colour=*/false);
            CHECK(vol.n_words() == 1 && vol.bits() == std::vector<uint32_t>{0u}, "a new volume has marks");
            bool threw = false;
            try { vol.count(); } catch (const bh::Error& e) { threw = e.code == BH_ERR_INVALID_ARG; }
            CHECK(threw, "a volume before its commit was extracted");
            vol.set_bits({(1u << 27) - 1u});
            CHECK(vol.commit(0) == 27 && vol.n_blocks() == 27, "27 blocks, got %u", vol.n_blocks());
            const std::vector<uint32_t> keys = vol.keys();
            bool ascending = keys.size() == 27;
            for (size_t s = 0; s < keys.size(); ++s) ascending = ascending && keys[s] == s;
            CHECK(ascending && vol.rank() == std::vector<uint32_t>{0u}, "keys or rank");
            CHECK(vol.count() == std::make_pair(0u, 0u), "a cleared volume has a surface");
            std::vector<float> dense_tw((size_t)n * n * n * 2), pool((size_t)27 * 1024);
            for (uint32_t k = 0; k < n; ++k)
                for (uint32_t j = 0; j < n; ++j)
                    for (uint32_t i = 0; i < n; ++i) {
                        const double x = org + vs * (float)i, y = org + vs * (float)j, z = org + vs * (float)k;
                        const double t = (std::sqrt(x * x + y * y + z * z) - r) / 0.15;
                        const size_t s = ((size_t)k * n + j) * n + i;
                        const size_t p = (size_t)(((k / 8) * 3 + j / 8) * 3 + i / 8) * 512 + ((k % 8) * 8 + j % 8) * 8 + i % 8;
                        dense_tw[2 * s] = pool[2 * p] = (float)std::fmin(std::fmax(t, -1.0), 1.0);
                        dense_tw[2 * s + 1] = pool[2 * p + 1] = 1.0f;
                    }
            vol.set_tw(pool);
            bh::TsdfVolume dense(ctx, {org, org, org}, vs, {n, n, n}, 0.0f, 64.0f, false), image(ctx, {org, org, org}, vs, {n, n, n}, 0.0f, 64.0f, false);
            dense.set_tw(dense_tw);
            vol.to_dense({0, 0, 0}, image);
            const std::vector<float> image_tw = image.tw();
            CHECK(image_tw.size() == dense_tw.size() && std::memcmp(image_tw.data(), dense_tw.data(), dense_tw.size() * 4) == 0, "to_dense is not the field written");
            const bh::Mesh m = vol.extract();
            const auto want = dense.count();
            CHECK(m.n_vertices == want.first && m.n_triangles == want.second && m.n_triangles > 2000, "sphere: %u vertices, %u triangles (dense: %u, %u)", m.n_vertices,
                  m.n_triangles, want.first, want.second);
            const std::vector<float> v = m.vertices.download();
            const std::vector<uint32_t> t = m.triangles.download();
            std::map<std::pair<uint32_t, uint32_t>, int> edges;
            bool in_range = true;
            double volume = 0.0;
            for (uint32_t f = 0; f < m.n_triangles && in_range; ++f) {
                const uint32_t* q = &t[3 * (size_t)f];
                in_range = q[0] < m.n_vertices && q[1] < m.n_vertices && q[2] < m.n_vertices;
                if (!in_range) break;
                for (int c = 0; c < 3; ++c) ++edges[{q[c], q[(c + 1) % 3]}];
                const float *a = &v[3 * (size_t)q[0]], *b = &v[3 * (size_t)q[1]], *c = &v[3 * (size_t)q[2]];
                volume += (a[0] * ((double)b[1] * c[2] - (double)b[2] * c[1]) - a[1] * ((double)b[0] * c[2] - (double)b[2] * c[0]) +
                           a[2] * ((double)b[0] * c[1] - (double)b[1] * c[0])) / 6.0;
            }
            CHECK(in_range, "a triangle index is out of range");
            if (in_range) {
                bool closed = edges.size() == 3 * (size_t)m.n_triangles;
                for (const auto& e : edges) closed = closed && e.second == 1 && edges.count({e.first.second, e.first.first}) == 1;
                const double ratio = volume / (4.0 / 3.0 * 3.14159265358979323846 * r * r * r);
                CHECK(closed && ratio >= 0.98 && ratio < 1.0, "the sphere is not closed and consistently oriented, or its volume ratio %.5f is off", ratio);
                std::printf("ok sparse mesh sphere (%u vertices, %u triangles, volume ratio %.5f)\n", m.n_vertices, m.n_triangles, ratio);
            }
            const std::vector<uint8_t> ply = vol.to_ply();
            const std::string head = "ply\nformat binary_little_endian 1.0\ncomment Exported from Brush\nelement vertex " + std::to_string(m.n_vertices) + "\n";
            CHECK(ply.size() > head.size() && std::memcmp(ply.data(), head.data(), head.size()) == 0, "PLY header");
            const std::string rest = "property float x\nproperty float y\nproperty float z\nelement face " + std::to_string(m.n_triangles) +
                                     "\nproperty list uchar uint vertex_indices\nend_header\n";
            CHECK(ply.size() == head.size() + rest.size() + (size_t)m.n_vertices * 12u + (size_t)m.n_triangles * 13u, "PLY size (%zu bytes)", ply.size());
            std::printf("ok sparse mesh ply\n");
        }
        {   // ---- one view: mark, commit, integrate against the dense volume
            const uint32_t nx = 40, ny = 33, nz = 26, w = 32, h = 24;
            const float org[3] = {-1.9f, -1.6f, 0.2f}, vs = 0.1f;
            const BhCamera cam = pinhole(w, h, 40.0f, 0.5f);
            std::vector<float> depth((size_t)w * h), image((size_t)w * h * 4);
            for (uint32_t p = 0; p < w * h; ++p) {
                depth[p] = 1.9f + 0.01f * (float)(p % w) - 0.02f * (float)(p / w);
                image[4 * p] = 0.1f * (float)(p % 7); image[4 * p + 1] = 0.3f; image[4 * p + 2] = 0.05f * (float)(p % 11);
                image[4 * p + 3] = (p % 5 == 0) ? 0.25f : 0.9f;
            }
            depth[5] = 0.0f; depth[6] = NAN; depth[7] = -1.0f;
            const bh::DeviceBuffer<float> depth_dev(depth), image_dev(image);
            bh::SparseTsdfVolume vol(ctx, {org[0], org[1], org[2]}, vs, {nx, ny, nz});
            vol.mark({cam}, {depth_dev.data()}, {image_dev.data()});
            const uint32_t blocks = vol.commit();
            CHECK(blocks > 0 && blocks < 5 * 5 * 4, "%u of 100 blocks allocated", blocks);
            vol.integrate({cam}, {depth_dev.data()}, {image_dev.data()});
            vol.integrate({cam, cam}, {depth_dev.data(), depth_dev.data()}, {image_dev.data(), image_dev.data()});
            bh::TsdfVolume dense(ctx, {org[0], org[1], org[2]}, vs, {nx, ny, nz}), img(ctx, {org[0], org[1], org[2]}, vs, {nx, ny, nz});
            dense.integrate({cam, cam, cam}, {depth_dev.data(), depth_dev.data(), depth_dev.data()}, {image_dev.data(), image_dev.data(), image_dev.data()});
            vol.to_dense({0, 0, 0}, img);
            const std::vector<float> a = dense.tw(), b = img.tw(), ca = dense.rgb(), cb = img.rgb();
            const std::vector<uint32_t> bits = vol.bits();
            uint32_t wrong = 0, held = 0, inside = 0;
            for (uint32_t k = 0; k < nz; ++k)
                for (uint32_t j = 0; j < ny; ++j)
                    for (uint32_t i = 0; i < nx; ++i) {
                        const size_t s = ((size_t)k * ny + j) * nx + i;
                        const uint32_t key = ((k / 8) * 5 + j / 8) * 5 + i / 8;
                        if ((bits[key / 32] >> (key % 32)) & 1u) {
                            if (std::memcmp(&a[2 * s], &b[2 * s], 8) != 0 || std::memcmp(&ca[3 * s], &cb[3 * s], 12) != 0) ++wrong;
                            if (b[2 * s + 1] > 0.0f) ++held;
                            if (b[2 * s] < 0.0f) ++inside;
                        } else if (b[2 * s] != 1.0f || b[2 * s + 1] != 0.0f || cb[3 * s] != 0.0f || cb[3 * s + 1] != 0.0f || cb[3 * s + 2] != 0.0f) {
                            ++wrong;
                        }
                    }
            CHECK(wrong == 0 && held > 500 && inside > 50, "%u samples differ from the dense volume (%u observed, %u inside)", wrong, held, inside);
            const bh::Mesh m = vol.extract();
            // (every fifth pixel fails the alpha test, so few cubes have all eight corners observed: some surface, not much)
            CHECK(m.n_triangles > 0 && m.colours.download().size() == (size_t)m.n_vertices * 3, "%u triangles", m.n_triangles);
            std::printf("ok sparse mesh integrate (%u blocks, %u samples observed, %u triangles)\n", blocks, held, m.n_triangles);

            // refusals leave the volume alone
            const std::vector<float> before = vol.tw();
            BhCamera fish = cam;
            fish.model = BH_CAMERA_KANNALA_BRANDT_4;
            bool threw = false;
            try { vol.integrate({cam, fish}, {depth_dev.data(), depth_dev.data()}); } catch (const bh::Error& e) { threw = e.code == BH_ERR_INVALID_ARG; }
            CHECK(threw, "a fisheye camera was accepted");
            threw = false;
            try { vol.mark({cam}, {depth_dev.data()}); } catch (const bh::Error& e) { threw = e.code == BH_ERR_INVALID_ARG; }
            CHECK(threw, "marking after a commit was accepted");
            uint32_t nb = 7;
            CHECK(bh_sptsdf_commit(ctx.get(), &vol.vol(), 3, &nb) == BH_ERR_INVALID_ARG && nb == 7, "dilate 3 was accepted");
            BhSparseTsdf bad = vol.vol();
            bad.nx = 8193;
            CHECK(bh_sptsdf_clear(ctx.get(), &bad) == BH_ERR_INVALID_ARG, "a dimension of 8193 was accepted");
            bad = vol.vol();
            bad.n_blocks = 0;
            CHECK(bh_sptsdf_clear(ctx.get(), &bad) == BH_ERR_INVALID_ARG, "a volume without blocks was cleared");
            CHECK(vol.tw() == before, "a refused call changed the volume");
            vol.mark_clear();
            CHECK(vol.n_blocks() == 0 && vol.commit() == 0, "mark_clear left marks behind");
            std::printf("ok sparse mesh refusals\n");
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (g_failed) { std::printf("%d C++ sparse mesh check(s) FAILED\n", g_failed); return 1; }
    std::printf("all C++ sparse mesh checks passed\n");
    return 0;
}
