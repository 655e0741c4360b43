// normal.hip — normal maps of a rendered frame, normals from a depth map, and their gradients (include/brush_hip_normal.h,
// DESIGN.md §6m).
//
// A normal map is one more blend over the lists a BH_FLAG_BWD_INFO forward saved, as a depth map is (depth.hip): the same splats in
// the same order with the same alpha, cut-off, clamp and saturation rule as the colour blend (device_blend.h holds the one copy of
// that arithmetic), folding a per-splat 3-vector where depth folds z.  K16 / K17 / K18 and the depth kernels are not touched.
//
//   * splat normals: one thread per splat, dense [N,3] (bh_splat_normals) or compact [Nv,3] over global_from_compact_gid (what
//     the two blends stage);
//   * forward and backward: device_map_blend.h's map_forward_kernel / map_backward_kernel, shared with depth.hip; NormalMap below is
//     what a normal map adds to them.  A staged splat is 12 floats (x y c00/2 c01 | c11/2 alpha0 sigma_cut nx | ny nz - -), three
//     uniform ds_read_b128 per splat, three fmas per contributing pair.  The backward replays with a 3-vector cotangent g per
//     pixel: the "colour" of splat i is g . n_i, the remaining sum S starts at g . N (an accumulated-normal forward into scratch
//     precedes the replay).  UNIT mode turns v into g = (v - (v . u) u) / |N| in the prologue, so both modes are one replay.
//     P Q R2 R3 R4 Vs join the [Nv,10] accumulator between K17 and K18 in the columns depth uses; Vn = sum of vis * g goes to a
//     compact [Nv,3] vector that a small kernel behind K18 carries to the quaternions;
//   * depth -> normal and its backward: streaming kernels, one thread per pixel; the backward is a gather without atomics.
#include "context.h"
#include "device_map_blend.h"
#include "device_depth_normal.h"
#include "../../include/brush_hip_depth.h"
#include "../../include/brush_hip_normal.h"

namespace bh {

namespace {

// the view a splat normal needs: rotation (column-major) and translation of the view matrix
struct NormalView {
    float vm[12];
};

// ---------------------------------------------------------------------------
// the normal of a splat
// ---------------------------------------------------------------------------
// k: the smallest log-scale (lowest index on a tie); qn: the normalised quaternion; sign: -1 where R_view col_k(qn) looks away from the camera
struct SplatFrame {
    Quat q, qn;
    float inv_len, sign;
    int k;
    Vec3A n;   // the oriented camera-space normal
};

BH_DEV SplatFrame splat_frame(const float* __restrict__ t, const NormalView& v) {
    SplatFrame f;
    const Vec3A mean = v3(t[0], t[1], t[2]);
    f.q = Quat{t[3], t[4], t[5], t[6]};
    const float s0 = t[7], s1 = t[8], s2 = t[9];
    f.k = 0;
    float best = s0;
    if (s1 < best) { best = s1; f.k = 1; }
    if (s2 < best) { best = s2; f.k = 2; }
    f.inv_len = 1.0f / __builtin_sqrtf(qdot(f.q, f.q));
    f.qn = qscale(f.q, f.inv_len);
    const Mat3 r = quat_to_mat3(f.qn);
    const Vec3A nw = f.k == 0 ? col0(r) : (f.k == 1 ? col1(r) : col2(r));
    const Mat3 rv = Mat3{v.vm[0], v.vm[1], v.vm[2], v.vm[3], v.vm[4], v.vm[5], v.vm[6], v.vm[7], v.vm[8]};
    const Vec3A nc = mul_vec3(rv, nw);
    const Vec3A mean_c = add(mul_vec3(rv, mean), v3(v.vm[9], v.vm[10], v.vm[11]));
    f.sign = dot(nc, mean_c) > 0.0f ? -1.0f : 1.0f;
    f.n = scale(nc, f.sign);
    return f;
}

// gid == NULL: the dense form (row i of transforms -> row i of out); else row gid[i] -> row i (the compact form)
__global__ __launch_bounds__(256) void splat_normals_kernel(uint64_t n, NormalView v, const uint32_t* __restrict__ gid,
                                                            const float* __restrict__ transforms, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t row = gid ? (uint64_t)gid[i] : i;
    const SplatFrame f = splat_frame(transforms + row * 10, v);
    float* o = out + i * 3;
    o[0] = f.n.x;
    o[1] = f.n.y;
    o[2] = f.n.z;
}

// What a normal map adds to the map skeleton.  MODE: BH_NORMAL_ACCUMULATED / UNIT (the backward does not read it).
//
// Backward.  Unit normals U = N / |N|: dU = (dN - (dN . u) u) / |N|, so both modes are ONE replay with a per-pixel cotangent g
// (accumulated: g = v; unit: g = (v - (v . u) u) / |N|, 0 where |N| == 0).  The "colour" of splat i at the pixel is cv = g . n_i and
// S = the remaining sum of w_j (g . n_j): it starts at g . N.
template <uint32_t MODE>
struct NormalMap : SinglePassMap<3> {
    static constexpr int STRIDE = 12, NACC = 3;
    struct Rec { float4 s0, s1, s2; };   // x y c00/2 c01 | c11/2 a sigma_cut nx | ny nz - -
    static BH_DEV Rec load(const float* p) {
        return Rec{*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4), *reinterpret_cast<const float4*>(p + 8)};
    }
    static BH_DEV float cut(const Rec& r) { return r.s1.z; }
    static BH_DEV void stage(float4* d, const float* v, float sigma_cut, Attr normals, uint32_t cg) {
        const float* nn = normals + (size_t)cg * 3;
        const float nx = nn[0], ny = nn[1], nz = nn[2];
        d[0] = make_float4(v[0], v[1], 0.5f * v[2], v[3]);
        d[1] = make_float4(0.5f * v[4], v[5], sigma_cut, nx);
        d[2] = make_float4(ny, nz, 0.0f, 0.0f);
    }
    static BH_DEV void fold(const Rec& r, bool ok, bool sat, float alpha_eff, float next_t, float& T, float* acc) {
        const float vis = (ok && !sat) ? alpha_eff * T : 0.0f;
        acc[0] = __builtin_fmaf(r.s1.w, vis, acc[0]);   // (one explicit fma per channel and term, as the colour channels)
        acc[1] = __builtin_fmaf(r.s2.x, vis, acc[1]);
        acc[2] = __builtin_fmaf(r.s2.y, vis, acc[2]);
        T = ok ? (sat ? -T : next_t) : T;
    }
    static BH_DEV void store(float* __restrict__ out, Attr, size_t pix, const float* acc, float T) {
        float x = acc[0], y = acc[1], z = acc[2];
        if (MODE == BH_NORMAL_UNIT) {
            const float len = __builtin_sqrtf(__builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x)));
            const float inv = len == 0.0f ? 0.0f : 1.0f / len;
            x *= inv; y *= inv; z *= inv;
        }
        float* o = out + pix * 3;
        o[0] = x; o[1] = y; o[2] = z;
    }

    struct BwdMaps {
        const float* __restrict__ normal_acc;   // [H,W,3] the frame's accumulated normals
        const float* __restrict__ v_normal;     // [H,W,3]
        uint32_t unit;
    };
    struct Pix { float g[3] = {0.0f, 0.0f, 0.0f}; };
    static BH_DEV float prologue(const BwdMaps& m, size_t pixel, Pix& px) {
        const size_t pix = pixel * 3;
        const float nx = m.normal_acc[pix], ny = m.normal_acc[pix + 1], nz = m.normal_acc[pix + 2];
        float vx = m.v_normal[pix], vy = m.v_normal[pix + 1], vz = m.v_normal[pix + 2];
        if (m.unit) {
            const float len = __builtin_sqrtf(__builtin_fmaf(nz, nz, __builtin_fmaf(ny, ny, nx * nx)));
            const float inv = len == 0.0f ? 0.0f : 1.0f / len;
            const float ux = nx * inv, uy = ny * inv, uz = nz * inv;
            const float vu = __builtin_fmaf(vz, uz, __builtin_fmaf(vy, uy, vx * ux));
            vx = __builtin_fmaf(-vu, ux, vx) * inv;
            vy = __builtin_fmaf(-vu, uy, vy) * inv;
            vz = __builtin_fmaf(-vu, uz, vz) * inv;
        }
        px.g[0] = vx; px.g[1] = vy; px.g[2] = vz;
        return __builtin_fmaf(vz, nz, __builtin_fmaf(vy, ny, vx * nx));
    }
    static BH_DEV float cv(const Rec& r, const Pix& px) { return __builtin_fmaf(px.g[2], r.s2.y, __builtin_fmaf(px.g[1], r.s2.x, px.g[0] * r.s1.w)); }
    static BH_DEV float vg(const Rec&, const Pix& px, int i) { return px.g[i]; }
};

// v_quat += the chain of Vn through the sign, R_view^T, column k of the rotation matrix and the quaternion's normalisation, behind
// K18 in its dense mode: a row K18 skipped (its ten sums are zero) is zero in the zero-filled dense output, so a splat that
// received only Vn is still written
// MARK (behind a K18 in marking mode: the single-GPU train step): a splat with a non-zero Vn may sit in a row K18 skipped, so the
// row is claimed first (device_map_blend.h claim_grad_row); a marked row (K18's, or depth's scatter, which runs in front of this one)
// is accumulated into as it is.
template <bool MARK>
BH_DEV void vn_scatter_row(uint32_t nv, const NormalView& v, uint32_t sh_floats, const uint32_t* __restrict__ global_from_compact,
                           const float* __restrict__ transforms, const float* __restrict__ v_n, float* __restrict__ v_transforms,
                           float* __restrict__ v_sh, float* __restrict__ v_raw_opac, float* __restrict__ v_refine) {
    const uint32_t cg = blockIdx.x * 256u + threadIdx.x;
    if (cg >= nv) return;
    const float vx = v_n[(size_t)cg * 3], vy = v_n[(size_t)cg * 3 + 1], vz = v_n[(size_t)cg * 3 + 2];
    if (vx == 0.0f && vy == 0.0f && vz == 0.0f) return;
    const uint32_t gid = global_from_compact[cg];
    const SplatFrame f = splat_frame(transforms + (size_t)gid * 10, v);
    const Mat3 rv = Mat3{v.vm[0], v.vm[1], v.vm[2], v.vm[3], v.vm[4], v.vm[5], v.vm[6], v.vm[7], v.vm[8]};
    const Vec3A a = transpose_mul_vec3(rv, scale(v3(vx, vy, vz), f.sign));   // d / d n_w
    const float w = f.qn.w, x = f.qn.x, y = f.qn.y, z = f.qn.z;
    Quat d;   // d / d (normalised quaternion): a . (d column k / d component)
    if (f.k == 0) {          // (1 - 2 (y2 + z2), 2 (xy + wz), 2 (xz - wy))
        d.w = 2.0f * (z * a.y - y * a.z);
        d.x = 2.0f * (y * a.y + z * a.z);
        d.y = 2.0f * ((x * a.y - w * a.z) - 2.0f * y * a.x);
        d.z = 2.0f * ((w * a.y + x * a.z) - 2.0f * z * a.x);
    } else if (f.k == 1) {   // (2 (xy - wz), 1 - 2 (x2 + z2), 2 (yz + wx))
        d.w = 2.0f * (x * a.z - z * a.x);
        d.x = 2.0f * ((y * a.x + w * a.z) - 2.0f * x * a.y);
        d.y = 2.0f * (x * a.x + z * a.z);
        d.z = 2.0f * ((y * a.z - w * a.x) - 2.0f * z * a.y);
    } else {                 // (2 (xz + wy), 2 (yz - wx), 1 - 2 (x2 + y2))
        d.w = 2.0f * (y * a.x - x * a.y);
        d.x = 2.0f * ((z * a.x - w * a.y) - 2.0f * x * a.z);
        d.y = 2.0f * ((w * a.x + z * a.y) - 2.0f * y * a.z);
        d.z = 2.0f * (x * a.x + y * a.y);
    }
    // qn = q / |q|: v_q = (d - qn (qn . d)) / |q|
    const float along = qdot(f.qn, d);
    float* vt = v_transforms + (size_t)gid * 10;
    if (MARK) claim_grad_row(gid, sh_floats, vt, v_sh, v_raw_opac, v_refine);
    vt[3] += (d.w - w * along) * f.inv_len;
    vt[4] += (d.x - x * along) * f.inv_len;
    vt[5] += (d.y - y * along) * f.inv_len;
    vt[6] += (d.z - z * along) * f.inv_len;
}

__global__ __launch_bounds__(256) void normal_vn_scatter_kernel(uint32_t nv, NormalView v, const uint32_t* __restrict__ global_from_compact,
                                                                const float* __restrict__ transforms, const float* __restrict__ v_n,
                                                                float* __restrict__ v_transforms) {
    vn_scatter_row<false>(nv, v, 0u, global_from_compact, transforms, v_n, v_transforms, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void normal_vn_scatter_marking_kernel(uint32_t nv, NormalView v, uint32_t sh_floats,
                                                                        const uint32_t* __restrict__ global_from_compact,
                                                                        const float* __restrict__ transforms, const float* __restrict__ v_n,
                                                                        float* __restrict__ v_transforms, float* __restrict__ v_sh,
                                                                        float* __restrict__ v_raw_opac, float* __restrict__ v_refine) {
    vn_scatter_row<true>(nv, v, sh_floats, global_from_compact, transforms, v_n, v_transforms, v_sh, v_raw_opac, v_refine);
}

// ---------------------------------------------------------------------------
// depth -> normal
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void depth_to_normal_kernel(PinholeK k, const float* __restrict__ depth, float* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= (size_t)k.w * k.h) return;
    const uint32_t x = (uint32_t)(p % k.w), y = (uint32_t)(p / k.w);
    const Stencil s = depth_stencil(k, depth, x, y);
    float ox = 0.0f, oy = 0.0f, oz = 0.0f;
    if (s.valid) {
        const float len = length(s.c);
        const float inv = len == 0.0f ? 0.0f : 1.0f / len;
        ox = s.c.x * inv; oy = s.c.y * inv; oz = s.c.z * inv;
    }
    out[p * 3] = ox;
    out[p * 3 + 1] = oy;
    out[p * 3 + 2] = oz;
}

// a gather in a fixed order (no atomics): pixel (x, y) is the right neighbour of the stencil at x-1, the left one of x+1, the lower
// one of y-1 and the upper one of y+1; its own stencil does not read its own depth
__global__ __launch_bounds__(256) void depth_to_normal_backward_kernel(PinholeK k, const float* __restrict__ depth, const float* __restrict__ v_normal,
                                                                       float* __restrict__ v_depth) {
    const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= (size_t)k.w * k.h) return;
    const uint32_t x = (uint32_t)(p % k.w), y = (uint32_t)(p / k.w);
    float g = 0.0f;
    if (x >= 1u) g += stencil_grad(k, depth, v_normal, x - 1u, y, 1);
    if (x + 1u < k.w) g += stencil_grad(k, depth, v_normal, x + 1u, y, 0);
    if (y >= 1u) g += stencil_grad(k, depth, v_normal, x, y - 1u, 3);
    if (y + 1u < k.h) g += stencil_grad(k, depth, v_normal, x, y + 1u, 2);
    v_depth[p] = g;
}

NormalView normal_view(const float* vm) {
    NormalView v;
    for (int i = 0; i < 12; ++i) v.vm[i] = vm[i];
    return v;
}

int launch_compact_normals(bh_ctx* ctx, const ForwardState& fs, const float* transforms, float* normals) {
    const uint32_t nv = fs.out.num_listed_splats;
    if (nv == 0) return 0;
    hipLaunchKernelGGL(splat_normals_kernel, dim3((nv + 255u) / 256u), dim3(256), 0, ctx->stream, (uint64_t)nv, normal_view(fs.uniforms.vm),
                       fs.out.global_from_compact_gid, transforms, normals);
    BH_LAUNCH_CHECK(ctx, "splat_normals_kernel");
    return 0;
}

// the blend over the saved lists (num_intersections > 0, num_listed_splats > 0, compact normals already queued)
int launch_normal_forward(bh_ctx* ctx, const ForwardState& fs, const float* normals, uint32_t mode, float* out_normal) {
    const BhRenderOut& r = fs.out;
    const MapUniforms u = map_uniforms(ctx, fs.uniforms);
    if (u.num_tiles == 0) return 0;
    const bool smooth = fs.flags & BH_FLAG_SMOOTH_CUTOFF;
    switch (mode) {
        case BH_NORMAL_ACCUMULATED: launch_map_forward<NormalMap<BH_NORMAL_ACCUMULATED>>(ctx, u, smooth, r, normals, out_normal); break;
        case BH_NORMAL_UNIT: launch_map_forward<NormalMap<BH_NORMAL_UNIT>>(ctx, u, smooth, r, normals, out_normal); break;
        default: return set_error(ctx, BH_ERR_INVALID_ARG, "render_normal: unknown normal mode");
    }
    BH_LAUNCH_CHECK(ctx, "normal_forward_kernel");
    return 0;
}

PinholeK pinhole_of(const BhCamera* cam, uint32_t h, uint32_t w) {
    PinholeK k;
    k.fx = cam->fx; k.fy = cam->fy; k.cx = cam->cx; k.cy = cam->cy;
    k.w = w; k.h = h;
    return k;
}

}  // namespace

// The normal map `mode` of the saved forward `fs` (something is listed); the compact splat normals go through SLOT_NORMAL.
int launch_normal_map(bh_ctx* ctx, const ForwardState& fs, const float* transforms, uint32_t mode, float* out) {
    MapScratch s;
    BH_TRY(map_scratch(ctx, SLOT_NORMAL, fs.out.num_listed_splats, 3, /*has_input=*/true, /*backward=*/false, 0, &s));
    BH_TRY(launch_compact_normals(ctx, fs, transforms, s.in));
    return launch_normal_forward(ctx, fs, s.in, mode, out);
}

// The normal term of a backward, between K17 and K18: v_combined += its raw sums, *v_n_out = Vn = sum of vis * g.
int launch_normal_backward(bh_ctx* ctx, const ForwardState& fs, const NormalTerm& term, const float* transforms, float* v_combined, const float** v_n_out) {
    const BhRenderOut& r = fs.out;
    const uint32_t nv = r.num_listed_splats;
    const MapUniforms u = map_uniforms(ctx, fs.uniforms);
    // SLOT_NORMAL: compact splat normals [Nv,3] | Vn [Nv,3] | the accumulated map [H,W,3]
    MapScratch s;
    BH_TRY(map_scratch(ctx, SLOT_NORMAL, nv, 3, /*has_input=*/true, /*backward=*/true, (size_t)u.img_w * u.img_h * 3, &s));
    *v_n_out = s.v;
    BH_HIP(ctx, hipMemsetAsync(s.v, 0, s.vec_floats * 4, ctx->stream));
    if (r.num_intersections == 0 || nv == 0 || u.num_tiles == 0) return 0;
    BH_TRY(launch_compact_normals(ctx, fs, transforms, s.in));
    BH_TRY(launch_normal_forward(ctx, fs, s.in, BH_NORMAL_ACCUMULATED, s.acc));
    using P = NormalMap<BH_NORMAL_ACCUMULATED>;
    const P::BwdMaps maps{s.acc, term.v_normal, term.mode == BH_NORMAL_UNIT ? 1u : 0u};
    launch_map_backward<P>(ctx, u, fs.flags & BH_FLAG_SMOOTH_CUTOFF, r, s.in, maps, v_combined, s.v);
    BH_LAUNCH_CHECK(ctx, "normal_backward_kernel");
    return 0;
}

// Vn -> the quaternion columns of v_transforms, behind K18 (and behind depth's scatter): dense and zero-filled, or (mark_rows, the
// single-GPU train step) row-marked
int launch_normal_vn_scatter(bh_ctx* ctx, const ForwardState& fs, const float* v_n, const float* transforms, float* v_transforms, bool mark_rows,
                             float* v_sh_coeffs, float* v_raw_opacities, float* v_refine_weight) {
    const BhRenderOut& r = fs.out;
    const uint32_t nv = r.num_listed_splats;
    if (nv == 0 || r.num_intersections == 0) return 0;
    if (mark_rows) {
        const uint32_t sh_floats = (fs.sh_degree + 1) * (fs.sh_degree + 1) * 3;
        hipLaunchKernelGGL(normal_vn_scatter_marking_kernel, dim3((nv + 255u) / 256u), dim3(256), 0, ctx->stream, nv, normal_view(fs.uniforms.vm), sh_floats,
                           r.global_from_compact_gid, transforms, v_n, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight);
        BH_LAUNCH_CHECK(ctx, "normal_vn_scatter_marking_kernel");
        return 0;
    }
    hipLaunchKernelGGL(normal_vn_scatter_kernel, dim3((nv + 255u) / 256u), dim3(256), 0, ctx->stream, nv, normal_view(fs.uniforms.vm),
                       r.global_from_compact_gid, transforms, v_n, v_transforms);
    BH_LAUNCH_CHECK(ctx, "normal_vn_scatter_kernel");
    return 0;
}

}  // namespace bh

extern "C" {

int bh_splat_normals(bh_ctx* ctx, const BhCamera* cam, const float* transforms, uint64_t n, float* out) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!cam) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "splat_normals: null camera");
    if (n == 0) return 0;
    if (!transforms || !out) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "splat_normals: null argument");
    if (n > 0xFFFFFFFFull) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "splat_normals: more than 2^32 - 1 splats");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(bh::splat_normals_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, ctx->stream, n, bh::normal_view(cam->vm),
                       (const uint32_t*)nullptr, transforms, out);
    BH_LAUNCH_CHECK(ctx, "splat_normals_kernel");
    return 0;
}

int bh_render_normal(bh_ctx* ctx, const BhRenderOut* saved, const float* transforms, uint32_t mode, float* out) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!saved || !out) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "render_normal: null argument");
    if (mode > BH_NORMAL_UNIT) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "render_normal: unknown normal mode");
    const bh::ForwardState* found = nullptr;
    BH_TRY(bh::find_saved_bwd_forward(ctx, saved, BH_ERR_INVALID_ARG, "render_normal", &found));
    const bh::ForwardState& fs = *found;
    // nothing listed: both modes are 0
    if (fs.out.num_intersections == 0 || fs.out.num_listed_splats == 0) return bh::clear_map_window(ctx, fs.uniforms, out, 3);
    if (!transforms) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "render_normal: null transforms");
    bh::ProfScope ps(ctx, "RenderNormal");
    return bh::launch_normal_map(ctx, fs, transforms, mode, out);
}

int bh_render_backward_normal_saved(bh_ctx* ctx, const BhRenderOut* saved, const float* v_output, const float* v_depth, uint32_t depth_mode,
                                    const float* v_normal, uint32_t normal_mode, const float* transforms, const float* sh_coeffs,
                                    const float* raw_opacities, float* v_transforms, float* v_sh_coeffs, float* v_raw_opacities,
                                    float* v_refine_weight) {
    bh::DepthTerm depth;
    depth.v_depth = v_depth;
    depth.mode = depth_mode;
    bh::NormalTerm normal;
    normal.v_normal = v_normal;
    normal.mode = normal_mode;
    bh::BackwardCall call{transforms, sh_coeffs, raw_opacities, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight};
    call.depth = &depth;
    call.normal = &normal;
    return bh::backward_entry(ctx, "render_backward_normal_saved", BH_ERR_INVALID_ARG, bh::NEED_V_NORMAL, saved, v_output, call);
}

int bh_depth_to_normal(bh_ctx* ctx, const BhCamera* cam, const float* depth, uint32_t h, uint32_t w, float* out) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!cam) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "depth_to_normal: null camera");
    if (cam->model != BH_CAMERA_PINHOLE) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "depth_to_normal: pinhole cameras only");
    const size_t pixels = (size_t)h * w;
    if (pixels == 0) return 0;
    if (!depth || !out) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "depth_to_normal: null argument");
    if (pixels > 0x7FFFFFFFull) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "depth_to_normal: more than 2^31 - 1 pixels");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(bh::depth_to_normal_kernel, dim3((uint32_t)((pixels + 255u) / 256u)), dim3(256), 0, ctx->stream, bh::pinhole_of(cam, h, w), depth, out);
    BH_LAUNCH_CHECK(ctx, "depth_to_normal_kernel");
    return 0;
}

int bh_depth_to_normal_backward(bh_ctx* ctx, const BhCamera* cam, const float* depth, const float* v_normal, uint32_t h, uint32_t w, float* v_depth) {
    if (!ctx) return BH_ERR_INVALID_ARG;
    if (!cam) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "depth_to_normal_backward: null camera");
    if (cam->model != BH_CAMERA_PINHOLE) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "depth_to_normal_backward: pinhole cameras only");
    const size_t pixels = (size_t)h * w;
    if (pixels == 0) return 0;
    if (!depth || !v_normal || !v_depth) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "depth_to_normal_backward: null argument");
    if (pixels > 0x7FFFFFFFull) return bh::set_error(ctx, BH_ERR_INVALID_ARG, "depth_to_normal_backward: more than 2^31 - 1 pixels");
    BH_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(bh::depth_to_normal_backward_kernel, dim3((uint32_t)((pixels + 255u) / 256u)), dim3(256), 0, ctx->stream, bh::pinhole_of(cam, h, w), depth,
                       v_normal, v_depth);
    BH_LAUNCH_CHECK(ctx, "depth_to_normal_backward_kernel");
    return 0;
}

}  // extern "C"
