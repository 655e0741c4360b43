// pose.hip — the entry points of brush_hip_pose.h: the backward with a pose gradient (the pass itself is in project.hip, next to
// K18 whose per-splat chain it repeats), the train step's attachment, and the host arithmetic of a pose update in f64.
#include <cmath>

#include "../../include/brush_hip_pose.h"
#include "context.h"

namespace {

// exp([w]x) by Rodrigues' formula, row-major r[i][j]
void rodrigues(const double w[3], double r[3][3]) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
    // sin(th)/th and (1 - cos(th))/th^2, by their series below 1e-4 (the next terms are < 1e-17 relative)
    const double a = th < 1e-4 ? 1.0 - th2 / 6.0 : std::sin(th) / th;
    const double b = th < 1e-4 ? 0.5 - th2 / 24.0 : (1.0 - std::cos(th)) / th2;
    const double k[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0.0;
            for (int l = 0; l < 3; ++l) kk += k[i][l] * k[l][j];
            r[i][j] = (i == j ? 1.0 : 0.0) + a * k[i][j] + b * kk;
        }
}

}  // namespace

extern "C" {

int bh_render_backward_pose_saved(bh_ctx* ctx, const BhRenderOut* saved, const float* v_output, const float* transforms,
                                  const float* sh_coeffs, const float* raw_opacities, float* v_transforms, float* v_sh_coeffs,
                                  float* v_raw_opacities, float* v_refine_weight, float* v_viewmat) {
    bh::BackwardCall call{transforms, sh_coeffs, raw_opacities, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight};
    call.v_viewmat = v_viewmat;
    return bh::backward_entry(ctx, "render_backward_pose_saved", BH_ERR_STATE, bh::NEED_V_OUTPUT | bh::NEED_V_VIEWMAT, saved, v_output, call);
}

int bh_train_set_pose_grad(bh_ctx* ctx, float* v_viewmat) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    ctx->terms.pose_grad = v_viewmat;
    return 0;
}

int bh_pose_twist(const float vm[12], const float v_viewmat[12], double twist[6]) {
    if (!vm || !v_viewmat || !twist) return BH_ERR_INVALID_ARG;
    // column-major: entry (row i, column j) of W and of v_W is [3 j + i]
    double a[3][3];   // v_W W^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int l = 0; l < 3; ++l) s += (double)v_viewmat[3 * l + i] * (double)vm[3 * l + j];
            a[i][j] = s;
        }
    const double t[3] = {vm[9], vm[10], vm[11]}, vt[3] = {v_viewmat[9], v_viewmat[10], v_viewmat[11]};
    twist[0] = (a[2][1] - a[1][2]) + (t[1] * vt[2] - t[2] * vt[1]);
    twist[1] = (a[0][2] - a[2][0]) + (t[2] * vt[0] - t[0] * vt[2]);
    twist[2] = (a[1][0] - a[0][1]) + (t[0] * vt[1] - t[1] * vt[0]);
    twist[3] = vt[0];
    twist[4] = vt[1];
    twist[5] = vt[2];
    return 0;
}

int bh_camera_apply_twist(BhCamera* cam, const double twist[6]) {
    if (!cam || !twist) return BH_ERR_INVALID_ARG;
    bool zero = true;
    for (int k = 0; k < 6; ++k) zero = zero && twist[k] == 0.0;
    if (zero) return 0;   // the identity, to the bit
    double r[3][3];
    rodrigues(twist, r);
    double c[3][3];   // c[j] = column j of R W
    double t[3];
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) {
            double s = 0.0;
            for (int l = 0; l < 3; ++l) s += r[i][l] * (double)cam->vm[3 * j + l];
            c[j][i] = s;
        }
    for (int i = 0; i < 3; ++i) {
        double s = 0.0;
        for (int l = 0; l < 3; ++l) s += r[i][l] * (double)cam->vm[9 + l];
        t[i] = s + twist[3 + i];
    }
    // Gram-Schmidt on the columns: column 0 keeps its direction, column 2 = column 0 x column 1 (a proper rotation)
    // (a vm whose first two columns are zero, parallel or not finite is no pose: refused, the camera left as it was)
    const double n0 = std::sqrt(c[0][0] * c[0][0] + c[0][1] * c[0][1] + c[0][2] * c[0][2]);
    if (!(n0 > 0.0) || !std::isfinite(n0)) return BH_ERR_INVALID_ARG;
    for (int i = 0; i < 3; ++i) c[0][i] /= n0;
    const double d01 = c[0][0] * c[1][0] + c[0][1] * c[1][1] + c[0][2] * c[1][2];
    const double full1 = std::sqrt(c[1][0] * c[1][0] + c[1][1] * c[1][1] + c[1][2] * c[1][2]);
    for (int i = 0; i < 3; ++i) c[1][i] -= d01 * c[0][i];
    const double n1 = std::sqrt(c[1][0] * c[1][0] + c[1][1] * c[1][1] + c[1][2] * c[1][2]);
    // (parallel: what is left of column 1 is below 1e-6 of it, the rounding of f32 columns rather than a direction)
    if (!(n1 > 1e-6 * full1) || !std::isfinite(n1)) return BH_ERR_INVALID_ARG;
    for (int i = 0; i < 3; ++i) c[1][i] /= n1;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(t[i])) return BH_ERR_INVALID_ARG;
    c[2][0] = c[0][1] * c[1][2] - c[0][2] * c[1][1];
    c[2][1] = c[0][2] * c[1][0] - c[0][0] * c[1][2];
    c[2][2] = c[0][0] * c[1][1] - c[0][1] * c[1][0];
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) cam->vm[3 * j + i] = (float)c[j][i];
    for (int i = 0; i < 3; ++i) cam->vm[9 + i] = (float)t[i];
    for (int j = 0; j < 3; ++j) cam->cam_pos[j] = (float)-(c[j][0] * t[0] + c[j][1] * t[1] + c[j][2] * t[2]);   // -W^T t
    return 0;
}

}  // extern "C"
