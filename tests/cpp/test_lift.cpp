// test_lift.cpp — mask lifting through the C++ host mirror (include/brush_hip.hpp LiftAccumulator / compact_splats):
//   * one view accumulated through the mirror against a loop here over the weights RenderNode::features returns for identity
//     blocks of 256 rows (the map IS w_ip, bit for bit: tests/test_gpu_lift.py A): votes, max_weight and pixel_count EQUAL;
//   * assign against the argmax of those rows (ties to the lowest label), select + compact_splats against the rows a loop picks;
//   * the refusals of the mirror.
// Build + run: tests/test_lift_cpp.py.
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

// the default camera of brush_amd/synth.py: origin, identity rotation, 60 degrees across, square pixels
static bh::Camera default_camera(uint32_t w, uint32_t h) {
    bh::Camera cam;
    cam.fov_x = 60.0 * 3.14159265358979323846 / 180.0;
    const double fx = (w / 2.0) / std::tan(cam.fov_x / 2.0);
    cam.fov_y = 2.0 * std::atan((h / 2.0) / fx);
    return cam;
}

int main() {
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
        std::printf("no HIP device: compile-only run\n");
        return 0;
    }
    try {
        bh::Context ctx(0);
        const uint32_t n = 600, w = 64, h = 48, L = 5, BLOCK = 256;
        const size_t hw = (size_t)w * h;
        Sm64 r{0x11F7};
        std::vector<float> tr((size_t)n * 10), sh((size_t)n * 3), op(n);
        for (uint32_t i = 0; i < n; ++i) {   // large, faint splats: long lists that are walked far
            float* row = &tr[(size_t)i * 10];
            row[2] = r.uni(2.0f, 9.0f);
            row[0] = r.uni(-0.6f, 0.6f) * row[2]; row[1] = r.uni(-0.45f, 0.45f) * row[2];
            row[3] = 1.0f; row[4] = r.uni(-0.3f, 0.3f); row[5] = r.uni(-0.3f, 0.3f); row[6] = r.uni(-0.3f, 0.3f);
            for (int k = 7; k < 10; ++k) row[k] = r.uni(std::log(0.2f), std::log(0.8f));
            op[i] = r.uni(-3.0f, -0.8f);
            for (int c = 0; c < 3; ++c) sh[(size_t)i * 3 + c] = r.uni(-1.0f, 1.5f);
        }
        const bh::Splats s = bh::Splats::from_host(tr, sh, op);
        const bh::Camera cam = default_camera(w, h);
        const float black[3] = {0.0f, 0.0f, 0.0f};
        bh::RenderNode node(ctx, s, cam, w, h, black, /*retain=*/true);
        ctx.sync();

        // labels: (x + 3 y) mod L, with ignored pixels (255, and L itself: the first value that is no label)
        std::vector<uint8_t> lab(hw);
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) lab[(size_t)y * w + x] = (x % 7 == 0 && y % 5 == 0) ? 255 : ((x % 11 == 3 && y % 4 == 1) ? (uint8_t)L : (uint8_t)((x + 3 * y) % L));
        const bh::DeviceBuffer<uint8_t> lab_dev(lab);

        // ---- the weights, and the tables a loop makes of them ----
        std::vector<uint64_t> votes((size_t)n * L, 0);
        std::vector<float> wmax(n, 0.0f);
        std::vector<uint32_t> count(n, 0);
        float top = 0.0f;
        for (uint32_t b = 0; b < n; b += BLOCK) {
            const uint32_t rows = std::min(BLOCK, n - b);
            std::vector<float> f((size_t)n * BLOCK, 0.0f);
            for (uint32_t j = 0; j < rows; ++j) f[(size_t)(b + j) * BLOCK + j] = 1.0f;
            const bh::DeviceBuffer<float> f_dev(f);
            const std::vector<float> map = node.features(f_dev.data(), BLOCK).download();
            for (size_t p = 0; p < hw; ++p)
                for (uint32_t j = 0; j < rows; ++j) {
                    const float wgt = map[p * BLOCK + j];
                    if (!(wgt > 0.0f)) continue;
                    const uint32_t i = b + j;
                    if (lab[p] < L) votes[(size_t)i * L + lab[p]] += (uint64_t)std::nearbyintf(wgt * 16777216.0f);
                    wmax[i] = std::fmax(wmax[i], wgt);
                    ++count[i];
                    top = std::fmax(top, wgt);
                }
        }
        CHECK(top > 0.02f && top <= 0.999f, "the frame is empty or the weights are no weights (max %g)", top);

        // ---- one view through the mirror ----
        bh::LiftAccumulator acc(ctx, n, L);
        acc.add(node, lab_dev.data());
        ctx.sync();
        const std::vector<uint64_t> got_votes = acc.votes.download();
        const std::vector<float> got_max = acc.max_weight.download();
        const std::vector<uint32_t> got_count = acc.pixel_count.download();
        size_t bad_v = 0, bad_m = 0, bad_c = 0, voted = 0;
        for (size_t k = 0; k < votes.size(); ++k) { bad_v += got_votes[k] != votes[k]; voted += votes[k] != 0; }
        for (uint32_t i = 0; i < n; ++i) { bad_m += std::memcmp(&got_max[i], &wmax[i], 4) != 0; bad_c += got_count[i] != count[i]; }
        CHECK(voted > n, "only %zu votes entries are not 0", voted);
        CHECK(bad_v == 0 && bad_m == 0 && bad_c == 0, "%zu votes, %zu maxima, %zu counts differ from the loop's", bad_v, bad_m, bad_c);
        // a retained node after another forward, into the same tables: twice the votes
        bh::Camera other = cam;
        other.position[0] = 0.8f;
        (void)bh::render_splats(ctx, s, other, w, h, black, bh::RasterPass::Backward);
        acc.add(node, lab_dev.data());
        ctx.sync();
        const std::vector<uint64_t> twice = acc.votes.download();
        size_t bad_t = 0;
        for (size_t k = 0; k < votes.size(); ++k) bad_t += twice[k] != 2 * votes[k];
        CHECK(bad_t == 0 && acc.max_weight.download() == got_max, "a second add of the same view: %zu votes are not doubled, or a maximum moved", bad_t);
        acc.clear();
        acc.add(node, lab_dev.data());
        std::printf("ok lift accumulate\n");

        // ---- assign, select, compact ----
        const float min_weight = 1.0f;
        bh::DeviceBuffer<float> share_dev;
        const std::vector<uint8_t> got_lab = acc.assign(min_weight, &share_dev).download();
        const std::vector<float> got_share = share_dev.download();
        BhLiftSelect sel{};
        sel.label = 1; sel.min_share = 0.2f; sel.min_weight = min_weight; sel.min_pixels = 8;   // (five interleaved labels: every share is near one fifth)
        const bh::DeviceBuffer<float> keep = acc.select(sel);
        const std::vector<float> got_keep = keep.download();
        std::vector<uint32_t> want_rows;
        size_t bad_l = 0, bad_s = 0, bad_k = 0, assigned = 0;
        for (uint32_t i = 0; i < n; ++i) {
            uint64_t total = 0, best = 0;
            uint32_t arg = 0;
            for (uint32_t l = 0; l < L; ++l) {
                const uint64_t v = votes[(size_t)i * L + l];
                total += v;
                if (v > best) { best = v; arg = l; }
            }
            const bool ok = total != 0 && total >= (uint64_t)std::rint((double)min_weight * 16777216.0);
            assigned += ok;
            bad_l += got_lab[i] != (ok ? arg : BH_LIFT_UNASSIGNED);
            const float share = ok ? (float)((double)best / (double)total) : 0.0f;
            bad_s += std::memcmp(&got_share[i], &share, 4) != 0;
            const bool k = ok && (double)votes[(size_t)i * L + 1] >= (double)sel.min_share * (double)total && count[i] >= sel.min_pixels;
            bad_k += got_keep[i] != (k ? 1.0f : 0.0f);
            if (k) want_rows.push_back(i);
        }
        CHECK(assigned > 20 && assigned < n, "%zu splats are assigned", assigned);
        CHECK(bad_l == 0 && bad_s == 0 && bad_k == 0, "%zu labels, %zu shares, %zu keep values differ from the loop's", bad_l, bad_s, bad_k);
        std::vector<uint32_t> rows;
        const bh::Splats kept = bh::compact_splats(ctx, s, keep, &rows);
        CHECK(!want_rows.empty() && want_rows.size() < n && rows == want_rows, "compact_splats kept %zu rows, the loop %zu", rows.size(), want_rows.size());
        const std::vector<float> kt = kept.transforms.download();
        size_t bad_r = 0;
        for (size_t j = 0; j < rows.size() && j * 10 + 9 < kt.size(); ++j) bad_r += std::memcmp(&kt[j * 10], &tr[(size_t)rows[j] * 10], 40) != 0;
        CHECK(kept.num_splats() == rows.size() && bad_r == 0, "%zu compacted rows are not their source rows", bad_r);
        std::printf("ok lift assign select compact\n");

        // ---- refusals ----
        bool refused = false;
        try { bh::LiftAccumulator bad(ctx, n, BH_LIFT_MAX_LABELS + 1); } catch (const bh::Error&) { refused = true; }
        CHECK(refused, "257 labels were accepted");
        refused = false;
        try { bh::LiftAccumulator bad(ctx, n + 1, L); bad.add(node, nullptr); } catch (const bh::Error&) { refused = true; }
        CHECK(refused, "tables of another size were accepted");
        refused = false;
        try { bh::LiftAccumulator bare(ctx, n, L, /*stats=*/false); BhLiftSelect t{}; t.label = BH_LIFT_ANY_LABEL; t.min_pixels = 1; (void)bare.select(t); }
        catch (const bh::Error&) { refused = true; }
        CHECK(refused, "a pixel test without the table was accepted");
        {
            bh::RenderNode loose(ctx, s, cam, w, h, black);
            (void)bh::render_splats(ctx, s, other, w, h, black, bh::RasterPass::Backward);
            refused = false;
            try { acc.add(loose, nullptr); } catch (const bh::Error& e) { refused = std::strstr(e.what(), "stale") != nullptr; }
            CHECK(refused, "a stale node was accepted");
        }
        std::printf("ok lift refusals\n");
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    if (g_failed) {
        std::printf("%d C++ lift check(s) FAILED\n", g_failed);
        return 1;
    }
    std::printf("all C++ lift checks passed\n");
    return 0;
}
