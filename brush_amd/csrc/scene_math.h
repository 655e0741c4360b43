// scene_math.h — the host arithmetic of brush_hip_scene.h in f64: the record of a similarity transform (with the rotation matrices of
// the spherical-harmonic bands 1..4), compose, invert, and the transform of a camera.  Plain C++: no HIP, no ctx, no device, so a
// stand-alone program can include it (tests/cpp/scene_math_sanitize.cpp does, under -fsanitize=address,undefined).
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/brush_hip_scene.h"

namespace bh_scene {

constexpr int SH_DIRS = 200;                        // Fibonacci directions of the least-squares fit (condition number <= 1.007 per band)
constexpr int SH_ROT_OFFSET[5] = {0, 0, 9, 34, 83};  // D_l in BhSceneTransform::sh_rot

// The 24 basis polynomials of degree 1..4 of device_sh.h at unit v — its constants (the f32 values) and signs — in f64; y[k] is basis
// k + 1.
inline void sh_basis_f64(const double v[3], double y[24]) {
    const double x = v[0], yy = v[1], z = v[2];
    const double f0a = (double)0.4886025f;
    y[0] = -f0a * yy;
    y[1] = f0a * z;
    y[2] = -f0a * x;
    const double z2 = z * z;
    const double f0b = (double)-1.0925485f * z;
    const double f1a = (double)0.54627424f;
    const double fc1 = x * x - yy * yy;
    const double fs1 = 2.0 * x * yy;
    y[3] = f1a * fs1;
    y[4] = f0b * yy;
    y[5] = (double)0.9461747f * z2 - (double)0.31539157f;
    y[6] = f0b * x;
    y[7] = f1a * fc1;
    const double f0c = (double)-2.285229f * z2 + (double)0.4570458f;
    const double f1b = (double)1.4453057f * z;
    const double f2a = (double)-0.5900436f;
    const double fc2 = x * fc1 - yy * fs1;
    const double fs2 = x * fs1 + yy * fc1;
    const double p12 = z * ((double)1.8658817f * z2 - (double)1.119529f);
    y[8] = f2a * fs2;
    y[9] = f1b * fs1;
    y[10] = f0c * yy;
    y[11] = p12;
    y[12] = f0c * x;
    y[13] = f1b * fc1;
    y[14] = f2a * fc2;
    const double f0d = z * ((double)-4.683326f * z2 + (double)2.0071396f);
    const double f1c = (double)3.3116114f * z2 - (double)0.47308735f;
    const double f2b = (double)-1.7701308f * z;
    const double f3a = (double)0.62583575f;
    const double fc3 = x * fc2 - yy * fs2;
    const double fs3 = x * fs2 + yy * fc2;
    y[15] = f3a * fs3;
    y[16] = f2b * fs2;
    y[17] = f1c * fs1;
    y[18] = f0d * yy;
    y[19] = (double)1.9843135f * z * p12 - (double)1.0062306f * y[5];
    y[20] = f0d * x;
    y[21] = f1c * fc1;
    y[22] = f2b * fc2;
    y[23] = f3a * fc3;
}

// R (row-major) of the unit quaternion (w,x,y,z)
inline void quat_to_matrix(const double q[4], double r[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    r[0] = 1.0 - 2.0 * (y * y + z * z);
    r[1] = 2.0 * (x * y - w * z);
    r[2] = 2.0 * (x * z + w * y);
    r[3] = 2.0 * (x * y + w * z);
    r[4] = 1.0 - 2.0 * (x * x + z * z);
    r[5] = 2.0 * (y * z - w * x);
    r[6] = 2.0 * (x * z - w * y);
    r[7] = 2.0 * (y * z + w * x);
    r[8] = 1.0 - 2.0 * (x * x + y * y);
}

// Hamilton product a (x) b, (w,x,y,z)
inline void quat_mul(const double a[4], const double b[4], double o[4]) {
    const double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    const double x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    const double y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    const double z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
    o[0] = w; o[1] = x; o[2] = y; o[3] = z;
}

// Solves the m x m system g X = h (g symmetric positive definite, overwritten; h m x m row-major, overwritten by X) by Gaussian
// elimination with partial pivoting.  false for a singular g.
inline bool solve_square(int m, double* g, double* h) {
    for (int c = 0; c < m; ++c) {
        int piv = c;
        for (int r = c + 1; r < m; ++r)
            if (std::fabs(g[r * m + c]) > std::fabs(g[piv * m + c])) piv = r;
        if (!(std::fabs(g[piv * m + c]) > 0.0)) return false;
        if (piv != c)
            for (int k = 0; k < m; ++k) {
                const double a = g[c * m + k]; g[c * m + k] = g[piv * m + k]; g[piv * m + k] = a;
                const double b = h[c * m + k]; h[c * m + k] = h[piv * m + k]; h[piv * m + k] = b;
            }
        for (int r = c + 1; r < m; ++r) {
            const double f = g[r * m + c] / g[c * m + c];
            if (f == 0.0) continue;
            for (int k = c; k < m; ++k) g[r * m + k] -= f * g[c * m + k];
            for (int k = 0; k < m; ++k) h[r * m + k] -= f * h[c * m + k];
        }
    }
    for (int c = m - 1; c >= 0; --c)
        for (int k = 0; k < m; ++k) {
            double s = h[c * m + k];
            for (int j = c + 1; j < m; ++j) s -= g[c * m + j] * h[j * m + k];
            h[c * m + k] = s / g[c * m + c];
        }
    return true;
}

// D_1..D_4 of the rotation r (row-major) into d[164], by least squares over SH_DIRS Fibonacci directions: with A = [Y_l(d_i)] and
// B = [Y_l(R^T d_i)], sum_k (D a)_k Y_k(d) = sum_k a_k Y_k(R^T d) for every a means A D = B, so D = (A^T A)^-1 A^T B.
inline bool sh_rotation_matrices(const double r[9], double d[164]) {
    double ya[SH_DIRS][24], yb[SH_DIRS][24];
    const double golden = 3.14159265358979323846 * (3.0 - std::sqrt(5.0));
    for (int i = 0; i < SH_DIRS; ++i) {
        const double z = 1.0 - (2.0 * i + 1.0) / SH_DIRS, rad = std::sqrt(1.0 - z * z), phi = golden * i;
        const double v[3] = {rad * std::cos(phi), rad * std::sin(phi), z};
        const double u[3] = {r[0] * v[0] + r[3] * v[1] + r[6] * v[2], r[1] * v[0] + r[4] * v[1] + r[7] * v[2],
                             r[2] * v[0] + r[5] * v[1] + r[8] * v[2]};   // R^T v
        sh_basis_f64(v, ya[i]);
        sh_basis_f64(u, yb[i]);
    }
    for (int l = 1; l <= 4; ++l) {
        const int m = 2 * l + 1, first = l * l - 1;
        double g[81], h[81];
        for (int a = 0; a < m; ++a)
            for (int b = 0; b < m; ++b) {
                double sg = 0.0, sh = 0.0;
                for (int i = 0; i < SH_DIRS; ++i) {
                    sg += ya[i][first + a] * ya[i][first + b];
                    sh += ya[i][first + a] * yb[i][first + b];
                }
                g[a * m + b] = sg;
                h[a * m + b] = sh;
            }
        if (!solve_square(m, g, h)) return false;
        std::memcpy(d + SH_ROT_OFFSET[l], h, sizeof(double) * m * m);
    }
    return true;
}

inline bool finite3(const double v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// Every field of the record from (q, t, s); q need not be normalised.  false (out untouched) when they are no transform.
inline bool fill_record(const double quat[4], const double trans[3], double scale, BhSceneTransform* out) {
    const double n2 = quat[0] * quat[0] + quat[1] * quat[1] + quat[2] * quat[2] + quat[3] * quat[3];
    if (!std::isfinite(quat[0]) || !std::isfinite(quat[1]) || !std::isfinite(quat[2]) || !std::isfinite(quat[3])) return false;
    double q[4];
    if (std::isfinite(n2) && n2 > 1e-300) {
        const double n = std::sqrt(n2);
        for (int k = 0; k < 4; ++k) q[k] = quat[k] / n;
    } else {
        // entries whose squares over- or underflow: scale by the largest first
        double top = 0.0;
        for (int k = 0; k < 4; ++k) top = std::fmax(top, std::fabs(quat[k]));
        if (!(top > 0.0)) return false;
        double m2 = 0.0;
        for (int k = 0; k < 4; ++k) { q[k] = quat[k] / top; m2 += q[k] * q[k]; }
        const double n = std::sqrt(m2);
        for (int k = 0; k < 4; ++k) q[k] /= n;
    }
    if (q[0] < 0.0)
        for (int k = 0; k < 4; ++k) q[k] = -q[k];
    if (!finite3(trans) || !std::isfinite(scale) || !(scale > 0.0)) return false;
    double r[9], d[164];
    quat_to_matrix(q, r);
    if (!sh_rotation_matrices(r, d)) return false;
    BhSceneTransform o;
    std::memset(&o, 0, sizeof(o));
    for (int k = 0; k < 4; ++k) { o.q[k] = q[k] + 0.0; o.quat[k] = (float)o.q[k]; }   // (+ 0.0: no -0 in the record)
    for (int k = 0; k < 3; ++k) { o.t[k] = trans[k]; o.trans[k] = (float)trans[k]; }
    o.s = scale;
    o.scale = (float)scale;
    o.log_scale = (float)std::log(scale);
    for (int k = 0; k < 9; ++k) o.rot[k] = (float)r[k];
    for (int k = 0; k < 164; ++k) o.sh_rot[k] = (float)d[k];
    *out = o;
    return true;
}

inline bool is_identity(const BhSceneTransform& T) {
    return T.q[0] == 1.0 && T.q[1] == 0.0 && T.q[2] == 0.0 && T.q[3] == 0.0 && T.t[0] == 0.0 && T.t[1] == 0.0 && T.t[2] == 0.0 && T.s == 1.0;
}

// a after b: s = sa sb, R = Ra Rb, t = sa Ra tb + ta
inline bool compose(const BhSceneTransform& a, const BhSceneTransform& b, BhSceneTransform* out) {
    double q[4], ra[9], t[3];
    quat_mul(a.q, b.q, q);
    quat_to_matrix(a.q, ra);
    for (int i = 0; i < 3; ++i) t[i] = a.s * (ra[3 * i] * b.t[0] + ra[3 * i + 1] * b.t[1] + ra[3 * i + 2] * b.t[2]) + a.t[i];
    return fill_record(q, t, a.s * b.s, out);
}

// x = R^T (x' - t) / s
inline bool invert(const BhSceneTransform& a, BhSceneTransform* out) {
    const double q[4] = {a.q[0], -a.q[1], -a.q[2], -a.q[3]};
    double r[9], t[3];
    quat_to_matrix(a.q, r);
    const double inv = 1.0 / a.s;
    for (int i = 0; i < 3; ++i) t[i] = -inv * (r[i] * a.t[0] + r[3 + i] * a.t[1] + r[6 + i] * a.t[2]);
    return fill_record(q, t, inv, out);
}

// W' = W R^T, tv' = s tv - W R^T t, cam_pos' = s R p + t (vm is column-major: W[i][j] = vm[3 j + i])
inline void camera_apply(const BhCamera& in, const BhSceneTransform& T, BhCamera* out) {
    double r[9], w[3][3];
    quat_to_matrix(T.q, r);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int l = 0; l < 3; ++l) s += (double)in.vm[3 * l + i] * r[3 * j + l];
            w[i][j] = s;
        }
    BhCamera o = in;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o.vm[3 * j + i] = (float)w[i][j];
        o.vm[9 + i] = (float)(T.s * (double)in.vm[9 + i] - (w[i][0] * T.t[0] + w[i][1] * T.t[1] + w[i][2] * T.t[2]));
        o.cam_pos[i] = (float)(T.s * (r[3 * i] * (double)in.cam_pos[0] + r[3 * i + 1] * (double)in.cam_pos[1] + r[3 * i + 2] * (double)in.cam_pos[2]) + T.t[i]);
    }
    *out = o;
}

}  // namespace bh_scene
