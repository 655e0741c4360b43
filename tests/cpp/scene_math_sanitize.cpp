// scene_math_sanitize.cpp — the host arithmetic of scene editing (brush_amd/csrc/scene_math.h) as a stand-alone program: g++ only, no
// HIP, no library.  tests/test_scene_cpp.py compiles it with -fsanitize=address,undefined and runs it: records for a few hundred random
// inputs (and the refused ones), composed, inverted and applied to a camera, with the properties that need no reference checked on the
// way — a unit quaternion with w >= 0, orthogonal D_l, invert composing to the identity.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../../brush_amd/csrc/scene_math.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform(double lo, double hi) {   // SplitMix64
    g_state += 0x9E3779B97F4A7C15ull;
    uint64_t z = g_state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return lo + (hi - lo) * ((double)(z >> 11) / 9007199254740992.0);
}

int main() {
    int failed = 0;
    double worst_orth = 0.0, worst_ident = 0.0;
    for (int it = 0; it < 300; ++it) {
        const double mag = it % 7 == 0 ? 1e160 : it % 5 == 0 ? 1e-170 : 1.0;   // squares that over- and underflow too
        const double q[4] = {uniform(-1, 1) * mag, uniform(-1, 1) * mag, uniform(-1, 1) * mag, uniform(-1, 1) * mag};
        const double t[3] = {uniform(-10, 10), uniform(-10, 10), uniform(-10, 10)};
        const double s = std::exp(uniform(-3, 3));
        BhSceneTransform a, b, inv, id;
        if (!bh_scene::fill_record(q, t, s, &a)) { std::printf("FAIL record %d refused\n", it); ++failed; continue; }
        const double n2 = a.q[0] * a.q[0] + a.q[1] * a.q[1] + a.q[2] * a.q[2] + a.q[3] * a.q[3];
        if (!(std::fabs(n2 - 1.0) <= 1e-14) || !(a.q[0] >= 0.0)) { std::printf("FAIL record %d: |q|^2 = %.17g, w = %g\n", it, n2, a.q[0]); ++failed; }
        for (int l = 1; l <= 4; ++l) {
            const int m = 2 * l + 1;
            const float* d = a.sh_rot + bh_scene::SH_ROT_OFFSET[l];
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < m; ++j) {
                    double dot = 0.0;
                    for (int k = 0; k < m; ++k) dot += (double)d[i * m + k] * (double)d[j * m + k];
                    worst_orth = std::fmax(worst_orth, std::fabs(dot - (i == j ? 1.0 : 0.0)));
                }
        }
        const double q2[4] = {uniform(-1, 1), uniform(-1, 1), uniform(-1, 1), uniform(-1, 1)};
        const double t2[3] = {uniform(-1, 1), uniform(-1, 1), uniform(-1, 1)};
        if (!bh_scene::fill_record(q2, t2, std::exp(uniform(-1, 1)), &b) || !bh_scene::compose(a, b, &b) || !bh_scene::invert(a, &inv) ||
            !bh_scene::compose(inv, a, &id)) {
            std::printf("FAIL compose / invert %d refused\n", it);
            ++failed;
            continue;
        }
        double off = std::fabs(id.q[0] - 1.0) + std::fabs(id.s - 1.0);
        for (int k = 0; k < 3; ++k) off += std::fabs(id.q[1 + k]) + std::fabs(id.t[k]);
        worst_ident = std::fmax(worst_ident, off);
        BhCamera cam{};
        cam.vm[0] = cam.vm[4] = cam.vm[8] = 1.0f;
        cam.vm[11] = 2.0f;
        cam.cam_pos[2] = -2.0f;
        cam.fx = 100.0f;
        bh_scene::camera_apply(cam, a, &cam);   // in place
        if (!std::isfinite(cam.vm[0]) || cam.fx != 100.0f) { std::printf("FAIL camera %d\n", it); ++failed; }
    }
    if (!(worst_orth <= 1e-6)) { std::printf("FAIL D D^T - I = %.3e\n", worst_orth); ++failed; }
    if (!(worst_ident <= 1e-12)) { std::printf("FAIL invert o make = identity + %.3e\n", worst_ident); ++failed; }
    // what make refuses leaves the record as it was
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double ok_q[4] = {1, 0, 0, 0}, ok_t[3] = {0, 0, 0};
    const double bad_q[3][4] = {{0, 0, 0, 0}, {nan, 0, 0, 1}, {inf, 0, 0, 0}};
    const double bad_t[3] = {0, inf, 0};
    BhSceneTransform r;
    r.s = -7.0;
    for (const auto& q : bad_q)
        if (bh_scene::fill_record(q, ok_t, 1.0, &r) || r.s != -7.0) { std::printf("FAIL a bad quaternion was accepted\n"); ++failed; }
    if (bh_scene::fill_record(ok_q, bad_t, 1.0, &r) || bh_scene::fill_record(ok_q, ok_t, 0.0, &r) || bh_scene::fill_record(ok_q, ok_t, nan, &r) ||
        bh_scene::fill_record(ok_q, ok_t, -1.0, &r) || bh_scene::fill_record(ok_q, ok_t, inf, &r) || r.s != -7.0) {
        std::printf("FAIL a bad translation or scale was accepted\n");
        ++failed;
    }
    if (failed) {
        std::printf("%d check(s) failed\n", failed);
        return 1;
    }
    std::printf("scene math ok: D D^T - I %.2e, invert o make %.2e\n", worst_orth, worst_ident);
    return 0;
}
