// brush_hip.hpp — C++17 host-side mirror of Brush's operator surface over the C ABI of libbrush_hip.so.
//
// The reference's host language is Rust (not available in this image); where the reference is compiled code
// the host side above the C ABI is C++: this header restates, with the reference's names and argument
// meaning, what a Brush host sees (paths relative to /root/reference/crates/):
//
//   brush_hip::Camera            brush-render/src/camera.rs:12-58          (+ CameraModel, kernels/camera_model/mod.rs:31-38)
//   brush_hip::Splats            brush-render/src/gaussian_splats.rs:62-256 (transforms / sh_coeffs / raw_opacities / min_scale)
//   brush_hip::RasterPass        brush-render/src/gaussian_splats.rs:28-48
//   brush_hip::render_splats     brush-render/src/gaussian_splats.rs:365-446 -> (image, RenderAux)
//   brush_hip::render_splats_bwd brush-render/src/bwd/burn_glue.rs:223-311   (+ RenderBackwards::backward :121-182)
//   brush_hip::radix_argsort     brush-sort/src/lib.rs:16,  brush_hip::prefix_sum  brush-prefix-sum/src/lib.rs:11
//   brush_hip::tile_sort_offsets render.rs:228-243 + kernels/get_tile_offset.rs:11-58
//   brush_hip::SplatTrainer      brush-train/src/train.rs:140-893           (step, refine, set_view_cams)
//   brush_hip::splat_to_ply / load_splat_from_ply   brush-serde/src/export.rs:179-204, import.rs:166-170
//   brush_hip::splat_to_compressed_ply   the SuperSplat compressed.ply of import.rs:407-600 (brush_hip_compressed_ply.h)
//   brush_hip::image_loss / image_loss_backward      brush-loss/src/lib.rs:718-733, 1075-1104 (LossOps; [H,W,C] in, [H,W,C] out)
//   brush_hip::image_loss_value_and_grad             the composition SplatTrainer::step makes of it (train.rs:227-260)
//   brush_hip::adam_step / gather_stats              brush-train/src/adam_scaled.rs:75-147, stats.rs:40-50
//   brush_hip::BatchUploader / SceneLoader           brush-dataset/src/scene.rs:97-136, scene_loader.rs:59-174
//   brush_hip::view_output_size / resize_u8 / BatchUploader::submit_view   load_image.rs:60-131 (brush_hip_image.h)
//   brush_hip::sample_background / normal_samples    train.rs:896-908, 389-416 (the library's counter-based generator)
//   brush_hip::pup_accumulate[_view] / pup_scores / decimate_to_count / lod_target_count   brush-train/src/lod.rs:13-142, train_stream.rs:261
//   brush_hip::knn_log_scales / to_init_splats / load_init_splats   brush-train/src/splat_init.rs:179-242, train_stream.rs:100-123
//   brush_hip::eval_metrics / eval_stats / run_eval   brush-train/src/eval.rs:23-63, train_stream.rs:506-566 (held-out PSNR / SSIM)
//   brush_hip::Lpips / lpips / lpips_value_and_grad / train_set_lpips   crates/lpips/src/lib.rs, train.rs:265-273 (lpips_loss_weight)
//   RenderNode::backward_pose / train_set_pose_grad / pose_twist / camera_apply_twist   not in the reference: camera pose
//                                                   gradients (gsplat's v_viewmats) and the host arithmetic of a pose update
//   RenderNode::backward_intrinsics / backward_camera / train_set_intrinsics_grad / camera_set_intrinsics   not in the reference:
//                                                   camera intrinsics gradients (focal, principal point; brush_hip_intrinsics.h)
//   brush_hip::ExposureTable / train_set_exposure   not in the reference: per-view exposure compensation (an affine colour
//                                                   transform per training view, Adam on the device; brush_hip_exposure.h)
//   brush_hip::depth_loss_value_and_grad / eval_depth_metrics / train_set_depth   not in the reference: depth supervision (a fused
//                                                   depth loss, the step's depth term, held-out depth metrics; brush_hip_depth_loss.h)
//   brush_hip::normal_consistency_value_and_grad / train_set_normal   not in the reference: the normal-consistency regulariser (a fused
//                                                   loss with both gradients, the step's normal term; brush_hip_normal_loss.h)
//   RenderNode::distortion / backward_distortion, brush_hip::distortion_loss / train_set_distortion   not in the reference: distortion
//                                                   maps (2DGS's depth distortion), their gradient, the loss and the step's term
//                                                   (brush_hip_distortion.h)
//   brush_hip::BilateralGridTable / train_set_bilagrid   not in the reference: per-view bilateral grids (a grid of affine colour
//                                                   transforms per training view, sliced at (x, y, luminance), TV term, Adam on the
//                                                   device; gsplat's lib_bilagrid; brush_hip_bilagrid.h)
//   RenderNode::features / backward_features, brush_hip::feature_loss_value_and_grad   not in the reference: feature maps (caller-owned
//                                                   per-splat vectors of 1 .. 256 channels, gsplat's colors [N, D]), their gradient
//                                                   and the fused L1 / cross-entropy losses (brush_hip_features.h)
//   brush_hip::FeatureField / train_set_features / refine_carry_rows, SplatTrainer::refine(.., FeatureField*)   not in the reference:
//                                                   feature fields trained jointly with the splats (the step's feature term, Adam on
//                                                   the device, rows carried through refine; brush_hip_feature_train.h)
//   brush_hip::SceneTransform / transform_splats / transformed_splats / select_region / crop_splats   not in the reference: scene
//                                                   editing (a similarity transform with the rotation of the SH bands, the same
//                                                   transform of a camera, a box / ellipsoid / opacity crop; brush_hip_scene.h)
//   brush_hip::LiftAccumulator / compact_splats      not in the reference: mask lifting (per-splat blend-weight votes from 2-D label
//                                                   maps, the largest weight and the pixel count, argmax / threshold, compaction;
//                                                   brush_hip_lift.h)
//   brush_hip::EnvironmentMap / train_set_envmap  not in the reference: environment maps (a learned cubemap behind the splats,
//                                                   composited behind the frame before the loss, Adam on the device;
//                                                   brush_hip_envmap.h)
//   Context::comm_* / allreduce_* / exchange_strip_halos   not in the reference: RCCL behind the C ABI
//
// Errors are exceptions (brush_hip::Error carrying bh_last_error) where the reference panics.  Device memory is
// owned by DeviceBuffer<T> (hipMalloc/hipFree); nothing here computes — every operation is one C-ABI call.
// tests/cpp/test_host.cpp runs the reference-style checks through this header on the MI355X.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <numeric>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "brush_hip.h"
#include "brush_hip_lpips.h"
#include "brush_hip_compressed_ply.h"
#include "brush_hip_image.h"
#include "brush_hip_depth.h"
#include "brush_hip_pose.h"
#include "brush_hip_exposure.h"
#include "brush_hip_depth_loss.h"
#include "brush_hip_normal.h"
#include "brush_hip_normal_loss.h"
#include "brush_hip_distortion.h"
#include "brush_hip_bilagrid.h"
#include "brush_hip_mesh.h"
#include "brush_hip_sparse_mesh.h"
#include "brush_hip_features.h"
#include "brush_hip_feature_train.h"
#include "brush_hip_scene.h"
#include "brush_hip_lift.h"
#include "brush_hip_envmap.h"
#include "brush_hip_intrinsics.h"

namespace brush_hip {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error("brush_hip error " + std::to_string(c) + ": " + m), code(c) {}
};

inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw Error(BH_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// ---- device memory -------------------------------------------------------------------------------------------
template <class T>
class DeviceBuffer {
  public:
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t n) { resize(n); }
    explicit DeviceBuffer(const std::vector<T>& host) { upload(host); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DeviceBuffer() { release(); }
    void resize(size_t n) {
        release();
        if (n) hip_check(hipMalloc((void**)&p_, n * sizeof(T)), "hipMalloc");
        n_ = n;
    }
    void upload(const std::vector<T>& host) {
        if (host.size() != n_) resize(host.size());
        if (n_) hip_check(hipMemcpy(p_, host.data(), n_ * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy H2D");
    }
    std::vector<T> download() const {
        std::vector<T> out(n_);
        if (n_) hip_check(hipMemcpy(out.data(), p_, n_ * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy D2H");
        return out;
    }
    void zero() { if (n_) hip_check(hipMemset(p_, 0, n_ * sizeof(T)), "hipMemset"); }
    T* data() { return p_; }
    const T* data() const { return p_; }
    size_t size() const { return n_; }

  private:
    void release() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <class T>
std::vector<T> download(const T* dev, size_t n) {
    std::vector<T> out(n);
    if (n) hip_check(hipMemcpy(out.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy D2H");
    return out;
}

// ---- context: one per thread / per GPU (brush-async/src/lib.rs:1-17) ---------------------------------------
class Context {
  public:
    explicit Context(int device = 0) : h_(nullptr) {
        check_abi();
        h_ = bh_create(device, nullptr, /*own_stream=*/1);
        if (!h_) throw Error(BH_ERR_HIP, "bh_create failed: no HIP device " + std::to_string(device));
    }
    // the library fills the header's structs with the layout IT was built with: refuse a library of another revision
    static void check_abi() {
        if (bh_abi_version() != BH_ABI_VERSION)
            throw Error(BH_ERR_UNSUPPORTED, "libbrush_hip.so speaks ABI " + std::to_string(bh_abi_version()) + ", this header ABI " + std::to_string(BH_ABI_VERSION));
        const size_t mine[BH_STRUCT_COUNT] = {sizeof(BhCamera), sizeof(BhRenderOut), sizeof(BhLossConfig), sizeof(BhTrainConfig), sizeof(BhTrainState),
                                              sizeof(BhTrainBatch), sizeof(BhTrainStats), sizeof(BhRefineConfig), sizeof(BhRefineStats), sizeof(BhPlyInfo)};
        for (uint32_t i = 0; i < BH_STRUCT_COUNT; ++i)
            if (bh_struct_size(i) != mine[i])
                throw Error(BH_ERR_UNSUPPORTED, "libbrush_hip.so: struct " + std::to_string(i) + " is " + std::to_string(bh_struct_size(i)) + " bytes in the library, " +
                                                    std::to_string(mine[i]) + " in this header");
    }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    ~Context() { bh_destroy(h_); }
    bh_ctx* get() const { return h_; }
    void check(int rc) const { if (rc != 0) throw Error(rc, bh_last_error(h_)); }
    void sync() const { check(bh_sync(h_)); }

    // ---- per-tile list controls (include/brush_hip.h "depth-sliced lists"): only the TIME of a render depends on them
    void set_list_slicing(float near_share) const { check(bh_set_list_slicing(h_, near_share)); }       // <= 0: automatic (per-tile cuts)
    void set_list_cut_threshold(uint32_t min_pairs) const { check(bh_set_list_cut_threshold(h_, min_pairs)); }
    void set_view_id(uint32_t view_id) const { check(bh_set_view_id(h_, view_id)); }                     // sticky; 0 = keyed by the camera
    void forget_views() const { check(bh_forget_views(h_)); }                                            // after loading another scene
    // bh_set_option: select one of the library's alternative paths (same results; the keys: bh_option_name / include/brush_hip.h)
    void set_option(const std::string& key, const std::string& value) const { check(bh_set_option(h_, key.c_str(), value.c_str())); }
    static std::vector<std::pair<std::string, std::string>> options() {   // (key, one line of documentation)
        std::vector<std::pair<std::string, std::string>> out;
        for (int i = 0; i < bh_option_count(); ++i) out.emplace_back(bh_option_name(i), bh_option_help(i));
        return out;
    }
    float last_list_share() const { return bh_last_list_share(h_); }
    uint32_t far_slices_queued() const { return bh_far_slices_queued(h_); }
    uint32_t view_table_count() const { return bh_view_table_count(h_); }
    std::pair<uint32_t, uint32_t> last_list_counts() const {   // (near pairs, far pairs) of the last forward
        uint32_t a = 0, b = 0;
        check(bh_last_list_counts(h_, &a, &b));
        return {a, b};
    }
    BhRenderOut last_render_out() const {
        BhRenderOut o{};
        check(bh_last_render_out(h_, &o));
        return o;
    }

    // ---- per-stage profile (HIP events around every pipeline stage; 2 = only the dominant kernel)
    void profile(int level = 1) const { check(bh_profile_enable(h_, level)); }
    struct StageTime { std::string name; float ms; uint32_t calls; };
    std::vector<StageTime> profile_fetch() const {
        const char* names[64]; float ms[64]; uint32_t calls[64];
        const int n = bh_profile_fetch(h_, names, ms, calls, 64);
        if (n < 0) check(n);
        std::vector<StageTime> out;
        for (int i = 0; i < n; ++i) out.push_back({names[i], ms[i], calls[i]});
        return out;
    }

    // ---- the library's communicator (RCCL, resolved at first use; SURVEY §8e — not in the reference, which is single-GPU).
    // Rank 0 calls comm_unique_id() and hands the 128 bytes to every rank by its own means; every rank calls comm_init.  With a
    // communicator of world > 1 and no hook, SplatTrainer::step sums its gradients (and, for a tile-row window, exchanges the strips'
    // halos) through it.
    static std::array<uint8_t, 128> comm_unique_id() {
        std::array<uint8_t, 128> id{};
        const int rc = bh_comm_unique_id(id.data());
        if (rc != 0) throw Error(rc, "bh_comm_unique_id failed (is librccl.so loadable?)");
        return id;
    }
    void comm_init(int rank, int world, const std::array<uint8_t, 128>& id) const { check(bh_comm_init(h_, rank, world, id.data())); }
    void comm_destroy() const { check(bh_comm_destroy(h_)); }
    int comm_world() const { return bh_comm_world(h_); }
    int comm_rank() const { return bh_comm_rank(h_); }
    void comm_selftest() const { check(bh_comm_selftest(h_)); }   // collective: every rank calls it once after comm_init
    void allreduce_sum(float* dev, uint64_t count) const { check(bh_allreduce_sum_f32(h_, dev, count)); }
    void allreduce_max(float* dev, uint64_t count) const { check(bh_allreduce_max_f32(h_, dev, count)); }   // RefineRecord maxima before refine
    void allgather_bytes(const void* send_dev, void* recv_dev, uint64_t bytes_per_rank) const { check(bh_allgather_bytes(h_, send_dev, recv_dev, bytes_per_rank)); }
    // one frame split into strips of tile rows: fetch the 21 pixel rows above and below this rank's strip from its neighbours
    void exchange_strip_halos(float* img_hwc4, uint32_t h, uint32_t w, uint32_t row_begin_px, uint32_t row_end_px) const {
        check(bh_exchange_strip_halos(h_, img_hwc4, h, w, row_begin_px, row_end_px));
    }
    static std::vector<BhHaloOp> strip_halo_plan(uint32_t img_h, uint32_t row_begin_px, uint32_t row_end_px, int rank, int world) {
        BhHaloOp ops[4];
        const int n = bh_strip_halo_plan(img_h, row_begin_px, row_end_px, rank, world, ops);
        if (n < 0) throw Error(n, "strip_halo_plan: bad strip");
        return std::vector<BhHaloOp>(ops, ops + n);
    }

  private:
    bh_ctx* h_;
};

// ---- Camera (camera.rs:12-58) ------------------------------------------------------------------------------------
enum class CameraModel : uint32_t {
    Pinhole = BH_CAMERA_PINHOLE,
    KannalaBrandt4 = BH_CAMERA_KANNALA_BRANDT_4,
    RadialTangential8 = BH_CAMERA_RADIAL_TANGENTIAL_8,
    ThinPrismFisheye = BH_CAMERA_THIN_PRISM_FISHEYE
};

struct Camera {
    double fov_x = 1.0, fov_y = 1.0;
    float center_uv[2] = {0.5f, 0.5f};
    float position[3] = {0.0f, 0.0f, 0.0f};
    float rotation[4] = {0.0f, 0.0f, 0.0f, 1.0f};  // glam order x, y, z, w
    CameraModel camera_model = CameraModel::Pinhole;
    float dist[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // the model's parameter struct in field order (brush_hip.h)

    bool is_valid() const {  // camera.rs:41-47
        bool ok = std::isfinite(fov_x) && std::isfinite(fov_y) && std::isfinite(center_uv[0]) && std::isfinite(center_uv[1]);
        for (float v : position) ok = ok && std::isfinite(v);
        for (float v : rotation) ok = ok && std::isfinite(v);
        return ok;
    }
    // kernel uniforms for an (img_w, img_h) render: focal from fov through the lens law, view matrix, clamp limits
    BhCamera uniforms(uint32_t img_w, uint32_t img_h) const {
        BhCamera cam{};
        const int rc = bh_camera_setup_model(position, rotation, fov_x, fov_y, center_uv[0], center_uv[1], img_w, img_h,
                                             (uint32_t)camera_model, dist, &cam);
        if (rc != 0) throw Error(rc, "Can't render images with 0 size.");  // render.rs:50-53
        return cam;
    }
};
inline double fov_to_focal(double fov, uint32_t pixels, CameraModel m = CameraModel::Pinhole, const float* dist = nullptr) {
    return bh_fov_to_focal(fov, pixels, (uint32_t)m, dist);
}
inline double focal_to_fov(double focal, uint32_t pixels, CameraModel m = CameraModel::Pinhole, const float* dist = nullptr) {
    return bh_focal_to_fov(focal, pixels, (uint32_t)m, dist);
}

// ---- Splats (gaussian_splats.rs:62-256) --------------------------------------------------------------------
inline uint32_t sh_degree_from_coeffs(uint32_t coeffs) {  // sh.rs
    uint32_t d = 0;
    while ((d + 1) * (d + 1) < coeffs) ++d;
    if ((d + 1) * (d + 1) != coeffs || d > 4) throw Error(BH_ERR_INVALID_ARG, "sh_coeffs must have (d+1)^2 coefficients, d <= 4");
    return d;
}

struct Splats {
    DeviceBuffer<float> transforms;     // [N,10] means(3) quat wxyz(4) log-scales(3)
    DeviceBuffer<float> sh_coeffs;      // [N,C,3]
    DeviceBuffer<float> raw_opacities;  // [N] logits
    std::optional<DeviceBuffer<float>> min_scale;  // [N] Mip-Splatting 3D-filter floor
    bool render_mip = false;

    static Splats from_host(const std::vector<float>& transforms, const std::vector<float>& sh, const std::vector<float>& raw_opac,
                            bool render_mip = false) {
        const size_t n = raw_opac.size();
        if (transforms.size() != n * 10 || (n && sh.size() % (3 * n) != 0)) throw Error(BH_ERR_INVALID_ARG, "Splats: transforms [N,10], sh [N,C,3], raw_opacities [N]");
        Splats s;
        s.transforms.upload(transforms);
        s.sh_coeffs.upload(sh);
        s.raw_opacities.upload(raw_opac);
        s.render_mip = render_mip;
        (void)s.sh_degree();
        return s;
    }
    uint32_t num_splats() const { return (uint32_t)raw_opacities.size(); }
    uint32_t num_coeffs() const { return num_splats() ? (uint32_t)(sh_coeffs.size() / (3 * (size_t)num_splats())) : 1u; }
    uint32_t sh_degree() const { return sh_degree_from_coeffs(num_coeffs()); }
    Splats& with_min_scale(DeviceBuffer<float> f) {  // gaussian_splats.rs:188-194
        if (f.size() != num_splats()) throw Error(BH_ERR_INVALID_ARG, "min_scale must have one entry per splat");
        min_scale = std::move(f);
        return *this;
    }
    // Splats::bake_min_scale (gaussian_splats.rs:245-256): fold the floor into the raw parameters, in place
    Splats& bake_min_scale(const Context& ctx) {
        if (min_scale) {
            ctx.check(bh_fold_min_scale(ctx.get(), transforms.data(), raw_opacities.data(), min_scale->data(), num_splats(), transforms.data(),
                                        raw_opacities.data()));
            ctx.sync();  // the floor buffer is freed next
            min_scale.reset();
        }
        return *this;
    }
};

// ---- RasterPass / render (gaussian_splats.rs:28-48, 365-446) ---------------------------------------------------
enum class RasterPass { Forward, Backward, BackwardSmoothCutoff };
inline bool bwd_info(RasterPass p) { return p != RasterPass::Forward; }

struct RenderAux {  // render_aux.rs:17-68: host scalars + ctx-owned device pointers (valid until the next render on the ctx)
    BhRenderOut raw{};
    uint32_t img_w = 0, img_h = 0, num_splats = 0;
    uint32_t num_visible() const { return raw.num_visible; }
    uint32_t num_listed_splats() const { return raw.num_listed_splats; }   // entries of the compact (depth-ordered) arrays
    uint32_t num_intersections() const { return raw.num_intersections; }
    std::vector<float> image() const { return download(raw.out_img, (size_t)img_w * img_h * 4); }             // [H,W,4] f32
    std::vector<uint32_t> image_packed() const { return download(raw.out_img_packed, (size_t)img_w * img_h); }  // [H,W] rgba8
    void validate() const {  // render_aux.rs:30-45
        if (raw.num_visible > num_splats) throw Error(BH_ERR_STATE, "num_visible exceeds the splat count");
    }
};

namespace detail {
struct Folded {  // what the renderer sees: fold_min_scale(params) when a floor is set (gaussian_splats.rs:379-386)
    const float* t;
    const float* o;
    DeviceBuffer<float> ft, fo;
};
inline Folded fold(const Context& ctx, const Splats& s) {
    Folded f{s.transforms.data(), s.raw_opacities.data(), {}, {}};
    if (s.min_scale) {
        f.ft.resize(s.transforms.size());
        f.fo.resize(s.raw_opacities.size());
        ctx.check(bh_fold_min_scale(ctx.get(), s.transforms.data(), s.raw_opacities.data(), s.min_scale->data(), s.num_splats(), f.ft.data(), f.fo.data()));
        f.t = f.ft.data();
        f.o = f.fo.data();
    }
    return f;
}
inline uint32_t flags_of(const Splats& s, RasterPass pass) {
    return (s.render_mip ? BH_FLAG_MIP : 0u) | (bwd_info(pass) ? BH_FLAG_BWD_INFO : 0u) |
           (pass == RasterPass::BackwardSmoothCutoff ? BH_FLAG_SMOOTH_CUTOFF : 0u);
}
}  // namespace detail

inline RenderAux render_splats(const Context& ctx, const Splats& splats, const Camera& camera, uint32_t img_w, uint32_t img_h,
                               const float background[3], RasterPass pass = RasterPass::Forward) {
    const BhCamera cam = camera.uniforms(img_w, img_h);
    const detail::Folded f = detail::fold(ctx, splats);
    RenderAux aux;
    aux.img_w = img_w; aux.img_h = img_h; aux.num_splats = splats.num_splats();
    ctx.check(bh_render_forward(ctx.get(), &cam, splats.num_splats(), splats.sh_degree(), f.t, splats.sh_coeffs.data(), f.o, background,
                                detail::flags_of(splats, pass), &aux.raw));
    ctx.sync();  // the folded temporaries die with this scope
    return aux;
}

struct SplatGrads {  // SplatGrads + the refine weight (bwd/burn_glue.rs:184-193, 165-180)
    DeviceBuffer<float> v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight;
};

// forward (Backward pass flags) + backward for a given dL/d(out_img) [H,W,4] on the device
inline std::pair<RenderAux, SplatGrads> render_splats_bwd(const Context& ctx, const Splats& splats, const Camera& camera, uint32_t img_w,
                                                          uint32_t img_h, const float background[3], const float* v_output,
                                                          RasterPass pass = RasterPass::Backward) {
    if (!bwd_info(pass)) throw Error(BH_ERR_INVALID_ARG, "render_splats_bwd requires a Backward variant");  // bwd/burn_glue.rs:281-284
    const BhCamera cam = camera.uniforms(img_w, img_h);
    const detail::Folded f = detail::fold(ctx, splats);
    RenderAux aux;
    aux.img_w = img_w; aux.img_h = img_h; aux.num_splats = splats.num_splats();
    const uint32_t n = splats.num_splats();
    ctx.check(bh_render_forward(ctx.get(), &cam, n, splats.sh_degree(), f.t, splats.sh_coeffs.data(), f.o, background,
                                detail::flags_of(splats, pass), &aux.raw));
    SplatGrads g;
    g.v_transforms.resize((size_t)n * 10);
    g.v_sh_coeffs.resize(splats.sh_coeffs.size());
    g.v_raw_opacities.resize(n);
    g.v_refine_weight.resize(n);
    // the saved state goes in explicitly (SplatBwdOps::{rasterize_bwd, project_bwd}, bwd/burn_glue.rs:62-92)
    ctx.check(bh_render_backward_saved(ctx.get(), &aux.raw, v_output, f.t, splats.sh_coeffs.data(), f.o, g.v_transforms.data(), g.v_sh_coeffs.data(),
                                       g.v_raw_opacities.data(), g.v_refine_weight.data()));
    if (splats.min_scale)  // chain through the fold (the autodiff of bwd/burn_glue.rs:260-270)
        ctx.check(bh_fold_min_scale_backward(ctx.get(), splats.transforms.data(), splats.raw_opacities.data(), splats.min_scale->data(), n,
                                             g.v_transforms.data(), g.v_raw_opacities.data()));
    ctx.sync();
    return {std::move(aux), std::move(g)};
}

// One differentiable render as the autodiff node the reference registers (bwd/burn_glue.rs:223-311): the forward now, the backward
// later from the node's SAVED state (:336-371).  retain = true keeps the node replayable while other renders run on the ctx
// (bh_render_retain); without it a later forward makes the node stale and backward() throws (BH_ERR_STATE) instead of returning
// another frame's gradients.
class RenderNode {
  public:
    RenderNode(const Context& ctx, const Splats& splats, const Camera& camera, uint32_t img_w, uint32_t img_h, const float background[3],
               bool retain = false, RasterPass pass = RasterPass::Backward)
        : ctx_(ctx), splats_(splats), folded_(detail::fold(ctx, splats)) {
        if (!bwd_info(pass)) throw Error(BH_ERR_INVALID_ARG, "RenderNode requires a Backward variant");
        const BhCamera cam = camera.uniforms(img_w, img_h);
        aux.img_w = img_w; aux.img_h = img_h; aux.num_splats = splats.num_splats();
        ctx.check(bh_render_forward(ctx.get(), &cam, splats.num_splats(), splats.sh_degree(), folded_.t, splats.sh_coeffs.data(), folded_.o, background,
                                    detail::flags_of(splats, pass), &aux.raw));
        if (retain) {
            ctx.check(bh_render_retain(ctx.get(), &aux.raw));
            retained_ = true;
        }
    }
    RenderNode(const RenderNode&) = delete;
    RenderNode& operator=(const RenderNode&) = delete;
    ~RenderNode() { if (retained_) (void)bh_render_release(ctx_.get(), &aux.raw); }
    SplatGrads backward(const float* v_output) const {
        return run_backward([&](float* v_t, float* v_sh, float* v_op, float* v_rf) {
            return bh_render_backward_saved(ctx_.get(), &aux.raw, v_output, folded_.t, splats_.sh_coeffs.data(), folded_.o, v_t, v_sh, v_op, v_rf);
        });
    }
    // The node's depth map [H,W] f32 (brush_hip_depth.h): BH_DEPTH_ACCUMULATED, BH_DEPTH_EXPECTED or BH_DEPTH_MEDIAN.  Rows outside a
    // tile-row window stay 0.
    DeviceBuffer<float> depth(uint32_t mode = BH_DEPTH_EXPECTED) const {
        DeviceBuffer<float> d;
        d.resize((size_t)aux.img_w * aux.img_h);
        d.zero();
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // the fill is ordered before the ctx stream's kernel
        ctx_.check(bh_render_depth(ctx_.get(), &aux.raw, mode, d.data()));
        ctx_.sync();
        return d;
    }
    // gradients of <v_output, image> + <v_depth, depth(mode)>; v_output may be nullptr (the depth term alone)
    SplatGrads backward(const float* v_output, const float* v_depth, uint32_t mode = BH_DEPTH_EXPECTED) const {
        return run_backward([&](float* v_t, float* v_sh, float* v_op, float* v_rf) {
            return bh_render_backward_depth_saved(ctx_.get(), &aux.raw, v_output, v_depth, mode, folded_.t, splats_.sh_coeffs.data(), folded_.o, v_t, v_sh,
                                                  v_op, v_rf);
        });
    }
    // The node's normal map [H,W,3] f32 in camera space (brush_hip_normal.h): BH_NORMAL_ACCUMULATED or BH_NORMAL_UNIT.  Rows outside a
    // tile-row window stay 0.
    DeviceBuffer<float> normal(uint32_t mode = BH_NORMAL_ACCUMULATED) const {
        DeviceBuffer<float> d;
        d.resize((size_t)aux.img_w * aux.img_h * 3);
        d.zero();
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // the fill is ordered before the ctx stream's kernel
        ctx_.check(bh_render_normal(ctx_.get(), &aux.raw, folded_.t, mode, d.data()));
        ctx_.sync();
        return d;
    }
    // gradients of <v_output, image> + <v_depth, depth(depth_mode)> + <v_normal, normal(normal_mode)> in one backward; v_output and
    // v_depth may be nullptr
    SplatGrads backward_normal(const float* v_output, const float* v_depth, uint32_t depth_mode, const float* v_normal,
                               uint32_t normal_mode = BH_NORMAL_ACCUMULATED) const {
        return run_backward([&](float* v_t, float* v_sh, float* v_op, float* v_rf) {
            return bh_render_backward_normal_saved(ctx_.get(), &aux.raw, v_output, v_depth, depth_mode, v_normal, normal_mode, folded_.t,
                                                   splats_.sh_coeffs.data(), folded_.o, v_t, v_sh, v_op, v_rf);
        });
    }
    SplatGrads backward_normal(const float* v_normal, uint32_t normal_mode = BH_NORMAL_ACCUMULATED) const {
        return backward_normal(nullptr, nullptr, BH_DEPTH_EXPECTED, v_normal, normal_mode);
    }
    // The node's distortion map [H,W] f32 (brush_hip_distortion.h): sum over pairs of w_i w_j (m_i - m_j)^2, m = z (BH_DISTORTION_Z) or
    // 2DGS's far (z - near) / ((far - near) z) (BH_DISTORTION_NDC).  moments: the moment map [H,W,4] = (A, M1', M2', r) instead.  Rows
    // outside a tile-row window stay 0.
    DeviceBuffer<float> distortion(const BhDistortionConfig& cfg = BhDistortionConfig{}, bool moments = false) const {
        static_assert(sizeof(BhDistortionConfig) == 16, "BhDistortionConfig layout");
        DeviceBuffer<float> d;
        d.resize((size_t)aux.img_w * aux.img_h * (moments ? 4 : 1));
        d.zero();
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // the fill is ordered before the ctx stream's kernel
        ctx_.check(moments ? bh_render_distortion_moments(ctx_.get(), &aux.raw, &cfg, d.data()) : bh_render_distortion(ctx_.get(), &aux.raw, &cfg, d.data()));
        ctx_.sync();
        return d;
    }
    // gradients of <v_output, image> + <v_depth, depth(depth_mode)> + <v_normal, normal(normal_mode)> + <v_distortion, distortion(cfg)>
    // in one backward; every cotangent but v_distortion may be nullptr
    SplatGrads backward_distortion(const float* v_output, const float* v_depth, uint32_t depth_mode, const float* v_normal, uint32_t normal_mode,
                                   const float* v_distortion, const BhDistortionConfig& cfg = BhDistortionConfig{}) const {
        return run_backward([&](float* v_t, float* v_sh, float* v_op, float* v_rf) {
            return bh_render_backward_distortion_saved(ctx_.get(), &aux.raw, v_output, v_depth, depth_mode, v_normal, normal_mode, v_distortion, &cfg,
                                                       folded_.t, splats_.sh_coeffs.data(), folded_.o, v_t, v_sh, v_op, v_rf);
        });
    }
    SplatGrads backward_distortion(const float* v_distortion, const BhDistortionConfig& cfg = BhDistortionConfig{}) const {
        return backward_distortion(nullptr, nullptr, BH_DEPTH_EXPECTED, nullptr, BH_NORMAL_ACCUMULATED, v_distortion, cfg);
    }
    // The node's feature map [H,W,C] f32 (brush_hip_features.h): the blend of `features` [N,C] (device, 1 <= C <= 256) with the colour
    // blend's own weights.  Rows outside a tile-row window stay 0.
    DeviceBuffer<float> features(const float* features, uint32_t channels) const {
        DeviceBuffer<float> d;
        d.resize((size_t)aux.img_w * aux.img_h * channels);
        d.zero();
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // the fill is ordered before the ctx stream's kernel
        ctx_.check(bh_render_features(ctx_.get(), &aux.raw, features, channels, d.data()));
        ctx_.sync();
        return d;
    }
    // gradients of <v_output, image> + <v_map, features(features)>; v_output may be nullptr.  v_features: [N,C] = the gradient with
    // respect to `features` (dense, rows of unlisted splats 0)
    SplatGrads backward_features(const float* v_output, const float* features, uint32_t channels, const float* v_map,
                                 DeviceBuffer<float>& v_features) const {
        v_features.resize((size_t)splats_.num_splats() * channels);
        return run_backward([&](float* v_t, float* v_sh, float* v_op, float* v_rf) {
            return bh_render_backward_features_saved(ctx_.get(), &aux.raw, v_output, features, channels, v_map, folded_.t, splats_.sh_coeffs.data(),
                                                     folded_.o, v_t, v_sh, v_op, v_rf, v_features.data());
        });
    }
    // gradients of <v_output, image> and, into v_viewmat (device, 12 floats in the layout of BhCamera.vm), its gradient with respect
    // to the camera's view matrix (brush_hip_pose.h); the four splat outputs are backward(v_output)'s
    SplatGrads backward_pose(const float* v_output, float* v_viewmat) const {
        return run_backward([&](float* v_t, float* v_sh, float* v_op, float* v_rf) {
            return bh_render_backward_pose_saved(ctx_.get(), &aux.raw, v_output, folded_.t, splats_.sh_coeffs.data(), folded_.o, v_t, v_sh, v_op, v_rf,
                                                 v_viewmat);
        });
    }
    // ... and v_intrinsics [4] (device): (v_fx, v_fy, v_cx, v_cy) (brush_hip_intrinsics.h); v_viewmat may be nullptr (no pose pass)
    SplatGrads backward_intrinsics(const float* v_output, float* v_intrinsics, float* v_viewmat = nullptr) const {
        return run_backward([&](float* v_t, float* v_sh, float* v_op, float* v_rf) {
            return bh_render_backward_intrinsics_saved(ctx_.get(), &aux.raw, v_output, folded_.t, splats_.sh_coeffs.data(), folded_.o, v_t, v_sh, v_op, v_rf,
                                                       v_viewmat, v_intrinsics);
        });
    }
    // ... with the optional depth, rendered-normal and distortion cotangents of `terms` (v_output may then be nullptr)
    SplatGrads backward_camera(const float* v_output, const BhCameraGradTerms& terms, float* v_intrinsics, float* v_viewmat = nullptr) const {
        return run_backward([&](float* v_t, float* v_sh, float* v_op, float* v_rf) {
            return bh_render_backward_camera_saved(ctx_.get(), &aux.raw, v_output, &terms, folded_.t, splats_.sh_coeffs.data(), folded_.o, v_t, v_sh, v_op,
                                                   v_rf, v_viewmat, v_intrinsics);
        });
    }
    RenderAux aux;

  private:
    // what every backward shares: the four gradient buffers, ONE C entry point on them (entry(v_transforms, v_sh_coeffs,
    // v_raw_opacities, v_refine_weight) -> status), the chain through the fold (the autodiff of bwd/burn_glue.rs:260-270), the sync
    template <class Entry>
    SplatGrads run_backward(Entry entry) const {
        const uint32_t n = splats_.num_splats();
        SplatGrads g;
        g.v_transforms.resize((size_t)n * 10);
        g.v_sh_coeffs.resize(splats_.sh_coeffs.size());
        g.v_raw_opacities.resize(n);
        g.v_refine_weight.resize(n);
        ctx_.check(entry(g.v_transforms.data(), g.v_sh_coeffs.data(), g.v_raw_opacities.data(), g.v_refine_weight.data()));
        if (splats_.min_scale)
            ctx_.check(bh_fold_min_scale_backward(ctx_.get(), splats_.transforms.data(), splats_.raw_opacities.data(), splats_.min_scale->data(), n,
                                                  g.v_transforms.data(), g.v_raw_opacities.data()));
        ctx_.sync();
        return g;
    }

    const Context& ctx_;
    const Splats& splats_;
    detail::Folded folded_;
    bool retained_ = false;
};

// ---- primitives --------------------------------------------------------------------------------------------------
inline void radix_argsort(const Context& ctx, const DeviceBuffer<uint32_t>& keys, const DeviceBuffer<uint32_t>& vals, uint32_t bits,
                          DeviceBuffer<uint32_t>& out_keys, DeviceBuffer<uint32_t>& out_vals) {
    if (keys.size() != vals.size()) throw Error(BH_ERR_INVALID_ARG, "Input keys and values must have the same number of elements");  // brush-sort/src/lib.rs:21-33
    if (bits > 32) throw Error(BH_ERR_INVALID_ARG, "Can only sort up to 32 bits");
    out_keys.resize(keys.size());
    out_vals.resize(keys.size());
    ctx.check(bh_radix_argsort(ctx.get(), keys.data(), vals.data(), (uint32_t)keys.size(), bits, out_keys.data(), out_vals.data()));
    ctx.sync();  // the ctx owns a non-blocking stream: DeviceBuffer::download (default stream) must not overtake it
}
// the forward's tile sort and its offsets table as one operator (render.rs:228-243 + kernels/get_tile_offset.rs:11-58)
inline void tile_sort_offsets(const Context& ctx, const DeviceBuffer<uint32_t>& tile_ids, const DeviceBuffer<uint32_t>& compact_gids, uint32_t num_tiles,
                              DeviceBuffer<uint32_t>& tile_ids_sorted, DeviceBuffer<uint32_t>& compact_gids_sorted, DeviceBuffer<uint32_t>& tile_offsets) {
    if (tile_ids.size() != compact_gids.size()) throw Error(BH_ERR_INVALID_ARG, "tile ids and splat ids must have the same number of elements");
    tile_ids_sorted.resize(tile_ids.size());
    compact_gids_sorted.resize(tile_ids.size());
    tile_offsets.resize((size_t)num_tiles * 2);
    ctx.check(bh_tile_sort_offsets(ctx.get(), tile_ids.data(), compact_gids.data(), (uint32_t)tile_ids.size(), num_tiles, tile_ids_sorted.data(),
                                   compact_gids_sorted.data(), tile_offsets.data()));
    ctx.sync();
}
inline void prefix_sum(const Context& ctx, const DeviceBuffer<uint32_t>& in, DeviceBuffer<uint32_t>& out) {
    out.resize(in.size());
    ctx.check(bh_prefix_sum(ctx.get(), in.data(), (uint32_t)in.size(), out.data()));
    ctx.sync();
}

// ---- image loss (brush-loss) ---------------------------------------------------------------------------------------
struct LossConfig {  // image_loss's arguments (brush-loss/src/lib.rs:1075-1104)
    float l1_weight = 0.8f, ssim_weight = -0.2f;
    std::optional<std::array<float, 3>> composite_bg;  // Some(bg): the GT is composited over bg first (gt + (1 - gt.a) * bg)
    bool mask = false;                                  // loss *= gt.a
    BhLossConfig c() const {
        BhLossConfig k{};
        k.l1_weight = l1_weight; k.ssim_weight = ssim_weight;
        if (composite_bg) { k.bg[0] = (*composite_bg)[0]; k.bg[1] = (*composite_bg)[1]; k.bg[2] = (*composite_bg)[2]; }
        k.composite_bg = composite_bg ? 1 : 0;
        k.mask = mask ? 1 : 0;
        return k;
    }
};
// LossOps::image_loss_forward (lib.rs:718-725): pred [C,H,W] (C = 3, or 4 with the alpha-match plane), gt [H,W] rgba8 -> loss map [C,H,W]
inline DeviceBuffer<float> image_loss(const Context& ctx, const float* pred_chw, const uint32_t* gt_packed, uint32_t channels, uint32_t h, uint32_t w,
                                      const LossConfig& cfg = {}) {
    if (channels != 3 && channels != 4) throw Error(BH_ERR_INVALID_ARG, "image_loss: 3 or 4 channels");
    DeviceBuffer<float> out((size_t)channels * h * w);
    const BhLossConfig k = cfg.c();
    ctx.check(bh_image_loss_forward(ctx.get(), pred_chw, gt_packed, channels, h, w, &k, out.data()));
    ctx.sync();
    return out;
}
// LossOps::image_loss_backward (lib.rs:726-733): dL/d(loss map) [C,H,W] -> dL/d(pred) [C,H,W]
inline DeviceBuffer<float> image_loss_backward(const Context& ctx, const float* pred_chw, const uint32_t* gt_packed, const float* dl_dmap, uint32_t channels,
                                               uint32_t h, uint32_t w, const LossConfig& cfg = {}) {
    if (channels != 3 && channels != 4) throw Error(BH_ERR_INVALID_ARG, "image_loss_backward: 3 or 4 channels");
    DeviceBuffer<float> out((size_t)channels * h * w);
    const BhLossConfig k = cfg.c();
    ctx.check(bh_image_loss_backward(ctx.get(), pred_chw, gt_packed, dl_dmap, channels, h, w, &k, out.data()));
    ctx.sync();
    return out;
}
// What SplatTrainer::step composes from image_loss + mean (+ the alpha term) + autodiff (train.rs:227-260), fused: the rasterizer's
// [H,W,4] image in, (loss, dloss/dimg [H,W,4]) out.
inline std::pair<float, DeviceBuffer<float>> image_loss_value_and_grad(const Context& ctx, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w,
                                                                       const LossConfig& cfg = {}, float alpha_weight = 0.0f) {
    DeviceBuffer<float> v_out((size_t)h * w * 4), loss(1);
    const BhLossConfig k = cfg.c();
    ctx.check(bh_image_loss_value_and_grad(ctx.get(), img_hwc4, gt_packed, h, w, &k, alpha_weight, loss.data(), v_out.data()));
    ctx.sync();
    return {loss.download()[0], std::move(v_out)};
}

// ---- optimizer / statistics (brush-train) -------------------------------------------------------------------------
// AdamScaled::step on one [rows, row_len] parameter, in place (adam_scaled.rs:75-147).  t = state.time AFTER this step (1 on the
// first call); col_scale: per-column learning-rate scale or null; reduce_m2: one second moment per row (m2 has `rows` entries).
// Queued on the ctx stream like every call that returns no host value: Context::sync() before touching the buffers from elsewhere.
inline void adam_step(const Context& ctx, float* param, const float* grad, float* m1, float* m2, uint64_t rows, uint32_t row_len, float lr, uint32_t t,
                      const float* col_scale = nullptr, bool reduce_m2 = false, float beta1 = 0.9f, float beta2 = 0.999f, float eps = 1e-15f) {
    ctx.check(bh_adam_step(ctx.get(), param, grad, m1, m2, rows, row_len, col_scale, lr, t, reduce_m2 ? 1 : 0, beta1, beta2, eps));
}
// RefineRecord::gather_stats (stats.rs:40-50): running maxima of the refine weight and the screen radius, running sum of visibility
inline void gather_stats(const Context& ctx, float* refine_weight_norm, float* vis_weight, float* max_screen_size, const float* refine_weight, const float* visible,
                         const float* screen_radius, uint64_t n) {
    ctx.check(bh_gather_stats(ctx.get(), refine_weight_norm, vis_weight, max_screen_size, refine_weight, visible, screen_radius, n));
}

// ---- the stochastic terms of step() (train.rs:389-416, 896-908) as pure functions of (seed, step) -------------------------
inline std::array<float, 3> sample_background(uint64_t seed, uint32_t step, const float base[3], float strength) {
    std::array<float, 3> out{};
    bh_sample_background(seed, step, base, strength, out.data());
    return out;
}
inline DeviceBuffer<float> normal_samples(const Context& ctx, uint64_t seed, uint32_t step, uint64_t n) {   // [n,3] N(0,1): what a device_noise step draws
    DeviceBuffer<float> out((size_t)n * 3);
    ctx.check(bh_normal_samples(ctx.get(), seed, step, n, out.data()));
    ctx.sync();
    return out;
}
inline std::array<uint32_t, 4> philox4x32_10(const std::array<uint32_t, 4>& ctr, const std::array<uint32_t, 2>& key) {   // Random123's generator, host
    std::array<uint32_t, 4> out{};
    bh_philox4x32_10(ctr.data(), key.data(), out.data());
    return out;
}

// ---- PLY (brush-serde) -------------------------------------------------------------------------------------------
inline std::vector<uint8_t> splat_to_ply(const Context& ctx, const Splats& s, const float* up_axis = nullptr) {
    uint64_t need = 0;
    const float* f = s.min_scale ? s.min_scale->data() : nullptr;
    ctx.check(bh_splat_to_ply(ctx.get(), s.transforms.data(), s.sh_coeffs.data(), s.raw_opacities.data(), f, s.num_splats(), s.sh_degree(),
                              s.render_mip ? 1 : 0, up_axis, nullptr, 0, &need));
    std::vector<uint8_t> out(need);
    ctx.check(bh_splat_to_ply(ctx.get(), s.transforms.data(), s.sh_coeffs.data(), s.raw_opacities.data(), f, s.num_splats(), s.sh_degree(),
                              s.render_mip ? 1 : 0, up_axis, out.data(), need, &need));
    return out;
}
// SuperSplat compressed.ply (brush_hip_compressed_ply.h): Morton-ordered rows, per-chunk ranges; order, when given, is resized to
// n and receives file row -> input row
inline std::vector<uint8_t> splat_to_compressed_ply(const Context& ctx, const Splats& s, const float* up_axis = nullptr,
                                                    DeviceBuffer<uint32_t>* order = nullptr) {
    uint64_t need = 0;
    const float* f = s.min_scale ? s.min_scale->data() : nullptr;
    if (order && order->size() != s.num_splats()) order->resize(s.num_splats());
    uint32_t* o = order ? order->data() : nullptr;
    ctx.check(bh_splat_to_compressed_ply(ctx.get(), s.transforms.data(), s.sh_coeffs.data(), s.raw_opacities.data(), f, s.num_splats(),
                                         s.sh_degree(), s.render_mip ? 1 : 0, up_axis, o, nullptr, 0, &need));
    std::vector<uint8_t> out(need);
    ctx.check(bh_splat_to_compressed_ply(ctx.get(), s.transforms.data(), s.sh_coeffs.data(), s.raw_opacities.data(), f, s.num_splats(),
                                         s.sh_degree(), s.render_mip ? 1 : 0, up_axis, o, out.data(), need, &need));
    return out;
}
// subsample_points = s keeps every s-th file row (s-1, 2s-1, ...: import.rs:346-349), max_splats then caps the count the way
// SplatData::subsample does (rows 0, step, 2 step, ...; import.rs:49-74).  info.num_splats is the number of rows kept.
inline std::pair<Splats, BhPlyInfo> load_splat_from_ply(const Context& ctx, const std::vector<uint8_t>& bytes, uint32_t subsample_points = 1,
                                                        size_t max_splats = 0) {
    BhPlyInfo info{};
    const int rc = bh_ply_parse_header(bytes.data(), bytes.size(), &info);
    if (rc != 0) throw Error(rc, rc == BH_ERR_UNSUPPORTED ? "unsupported PLY variant" : "malformed PLY");
    if (subsample_points < 1) throw Error(BH_ERR_INVALID_ARG, "subsample_points must be >= 1");
    uint64_t first = subsample_points - 1, step = subsample_points, n = info.num_splats / subsample_points;
    if (max_splats != 0 && n > max_splats) {
        const uint64_t step2 = (n + max_splats - 1) / max_splats;
        n = (n + step2 - 1) / step2;
        step *= step2;
    }
    Splats s;
    const size_t c = (size_t)(info.sh_degree + 1) * (info.sh_degree + 1);
    s.transforms.resize(n * 10);
    s.sh_coeffs.resize(n * c * 3);
    s.raw_opacities.resize(n);
    s.render_mip = info.render_mode == 1;
    ctx.check(bh_splats_from_ply_strided(ctx.get(), bytes.data(), bytes.size(), first, step, n, s.transforms.data(), s.sh_coeffs.data(),
                                         s.raw_opacities.data()));
    info.num_splats = n;
    return {std::move(s), info};
}

// ---- training (brush-train) ---------------------------------------------------------------------------------------
struct TrainConfig {  // config.rs:7-132 subset, same defaults
    uint32_t total_train_iters = 30000;
    double lr_mean = 2e-5, lr_mean_end = 2e-7, lr_coeffs_dc = 2e-3, lr_opac = 0.012, lr_scale = 5e-3, lr_rotation = 2e-3;
    float lr_coeffs_sh_scale = 10.0f, ssim_weight = 0.2f, match_alpha_weight = 0.1f, mean_noise_weight = 50.0f;
    float background_color[3] = {0.0f, 0.0f, 0.0f};
    float background_noise_strength = 0.1f;
    bool render_mip = false;
    bool exact_lists = false;  // not in the reference: false = depth-sliced per-tile lists in step() (BH_FLAG_SLICED_LISTS, same results)
    uint32_t max_splats = 10000000, refine_every = 200, growth_stop_iter = 15000;
    float growth_grad_threshold = 0.0025f, growth_select_fraction = 0.25f, split_at_screen_size = 0.5f, opac_decay = 0.004f;
};

struct SceneBatch {  // brush-dataset/src/scene.rs:139-147
    const uint32_t* img_packed = nullptr;  // device [H,W] rgba8
    uint32_t img_w = 0, img_h = 0;
    bool has_alpha = false, alpha_is_mask = false;
    Camera camera;
    uint32_t view_id = 0;  // which view of the dataset this is (its index + 1; 0 = unknown): keys the forward's per-tile depth cuts (time only)
};

struct TrainStepStats { uint32_t num_visible, num_intersections; double lr_mean; float loss; };

// ---- host image -> packed device batch (brush-dataset) ---------------------------------------------------------------
// LoadImage::output_scale (load_image.rs): the (width, height) load() resizes a w x h view to; max_resolution 0: no cap
inline std::pair<uint32_t, uint32_t> view_output_size(uint32_t w, uint32_t h, uint32_t max_resolution = 1920, float scale = 1.0f) {
    uint32_t ow = 0, oh = 0;
    const int rc = bh_view_output_size(w, h, max_resolution, scale, &ow, &oh);
    if (rc != 0) throw Error(rc, "view_output_size: w, h > 0 and a finite scale > 0");
    return {ow, oh};
}
// image::imageops::resize of device bytes [h][w][channels] -> [nh][nw][channels] on the ctx stream (channels 1 | 3 | 4)
inline void resize_u8(const Context& ctx, const uint8_t* src, uint32_t w, uint32_t h, uint32_t channels, uint8_t* dst, uint32_t nw, uint32_t nh,
                      uint32_t filter = BH_FILTER_LANCZOS3) {
    ctx.check(bh_resize_u8(ctx.get(), src, w, h, channels, dst, nw, nh, filter));
}

// view_to_packed_data (scene.rs:97-136) on the device behind a ring of pinned staging slots and a copy stream: the decoded RGB8 / RGBA8
// bytes cross PCIe unpacked, widening (a = 255), the byte-space premultiply of AlphaMode::Transparent and the packing run in a kernel
// on the copy stream while the previous batch trains.  Life of a slot: map -> (decode into the pinned bytes) -> commit -> acquire
// (the ctx stream waits for the upload on the device: no host block) -> queue the train step -> release.
class BatchUploader {
  public:
    BatchUploader(const Context& ctx, uint64_t max_pixels, uint32_t slots = 3) : slots_(slots) {
        up_ = bh_uploader_create(ctx.get(), max_pixels, slots);
        if (!up_) throw Error(BH_ERR_INVALID_ARG, "bh_uploader_create failed (max_pixels > 0, 2 <= slots <= 16, enough pinned memory)");
    }
    BatchUploader(const BatchUploader&) = delete;
    BatchUploader& operator=(const BatchUploader&) = delete;
    ~BatchUploader() { bh_uploader_destroy(up_); }
    uint32_t slots() const { return slots_; }
    // the next slot's pinned buffer to decode straight into (blocks only when the ring wraps onto a slot whose step is still running)
    std::pair<int, uint8_t*> map(uint64_t bytes) {
        void* p = nullptr;
        const int slot = check(bh_uploader_begin(up_, bytes, &p));
        return {slot, (uint8_t*)p};
    }
    void commit(int slot, uint32_t w, uint32_t h, uint32_t channels, bool premultiply) { check(bh_uploader_commit(up_, slot, w, h, channels, premultiply ? 1 : 0)); }
    // map + memcpy + commit for pixels that already live elsewhere: tightly packed [H,W,3|4] bytes; returns the slot
    int submit(const uint8_t* pixels, uint32_t w, uint32_t h, uint32_t channels, bool premultiply = true) {
        if (channels != 3 && channels != 4) throw Error(BH_ERR_INVALID_ARG, "image must be [H,W,3] or [H,W,4] uint8");
        return check(bh_uploader_submit(up_, pixels, w, h, channels, (premultiply && channels == 4) ? 1 : 0));
    }
    // LoadImage::load of a decoded view (brush_hip_image.h): pixels [H,W,3|4]; mask (or nullptr) one channel [mask_h][mask_w], merged
    // into alpha; then Lanczos3 to view_output_size(w, h, max_resolution, scale) and the pack.  acquire() gives the output size.
    int submit_view(const uint8_t* pixels, uint32_t w, uint32_t h, uint32_t channels, const uint8_t* mask = nullptr, uint32_t mask_w = 0,
                    uint32_t mask_h = 0, bool invert_mask = false, uint32_t max_resolution = 1920, float scale = 1.0f, bool premultiply = true) {
        if (channels != 3 && channels != 4) throw Error(BH_ERR_INVALID_ARG, "image must be [H,W,3] or [H,W,4] uint8");
        const uint64_t img_bytes = (uint64_t)w * h * channels, mask_bytes = mask ? (uint64_t)mask_w * mask_h : 0;
        const std::pair<int, uint8_t*> m = map(img_bytes + mask_bytes);
        std::memcpy(m.second, pixels, (size_t)img_bytes);
        if (mask_bytes) std::memcpy(m.second + img_bytes, mask, (size_t)mask_bytes);
        BhViewLoad d{};
        d.w = w; d.h = h; d.channels = channels;
        d.mask_w = mask ? mask_w : 0; d.mask_h = mask ? mask_h : 0; d.invert_mask = invert_mask ? 1 : 0;
        d.mask_offset = mask ? img_bytes : 0;
        d.max_resolution = max_resolution; d.scale = scale; d.premultiply = premultiply ? 1 : 0;
        check(bh_uploader_commit_view(up_, m.first, &d));
        return m.first;
    }
    struct Packed { const uint32_t* img; uint32_t w, h; bool has_alpha; };   // device [H,W] rgba8, aliasing the slot
    Packed acquire(int slot) {
        Packed r{};
        int ha = 0;
        check(bh_uploader_acquire(up_, slot, &r.img, &r.w, &r.h, &ha));
        r.has_alpha = ha != 0;
        return r;
    }
    void release(int slot) { check(bh_uploader_release(up_, slot)); }   // once the step that reads the slot is queued

  private:
    int check(int rc) const {
        if (rc < 0) throw Error(rc, std::string("uploader: ") + bh_uploader_last_error(up_));
        return rc;
    }
    bh_uploader* up_ = nullptr;
    uint32_t slots_;
};

// SceneLoader (scene_loader.rs:59-174): an endless shuffled stream of SceneBatch over a list of views, the upload of the NEXT views
// in flight while the current one trains.  Every epoch is a seeded Fisher-Yates permutation (SplitMix64) of this rank's views — the
// reference's order comes from rand::StdRng inside racing loader tasks and is not reproducible, so only "every view once per epoch"
// is kept.  rank / world shard the view list for data-parallel training (view i belongs to rank i % world).  No loader thread here:
// next_batch() submits the views that follow before it hands the current one out (the copies and the packing kernel run on the
// uploader's stream; what the host does per view is one memcpy into pinned memory, or the caller's decode straight into it).
struct LoaderView {
    uint32_t w = 0, h = 0, channels = 3;
    std::function<void(uint8_t* dst)> decode;   // writes w * h * channels tightly packed bytes
    Camera camera;
    bool alpha_is_mask = false;
};

class SceneLoader {
  public:
    SceneLoader(const Context& ctx, std::vector<LoaderView> views, uint64_t seed = 0, uint32_t slots = 3, uint32_t rank = 0, uint32_t world = 1)
        : seed_(seed) {
        for (size_t i = 0; i < views.size(); ++i)
            if (world == 0 || i % world == rank) { views_.push_back(std::move(views[i])); ids_.push_back((uint32_t)i + 1u); }
        if (views_.empty()) throw Error(BH_ERR_INVALID_ARG, "Need at least one view in dataset");  // scene_loader.rs:130
        for (const LoaderView& v : views_)
            if (!v.decode || v.w == 0 || v.h == 0 || (v.channels != 3 && v.channels != 4))
                throw Error(BH_ERR_INVALID_ARG, "LoaderView: needs a decode function, a size and 3 or 4 channels");
        uint64_t mp = 0;
        for (const LoaderView& v : views_) mp = std::max<uint64_t>(mp, (uint64_t)v.w * v.h);
        up_.emplace(ctx, mp, slots);
        depth_ = slots > 1 ? slots - 1 : 1;   // slots in flight = submitted + the one being trained on
    }
    // the view order of `epoch` (deterministic in seed, epoch and the shard)
    std::vector<uint32_t> epoch_order(uint64_t epoch) const {
        std::vector<uint32_t> order(views_.size());
        std::iota(order.begin(), order.end(), 0u);
        uint64_t st = seed_ ^ (0xD1B54A32D192ED03ull * (epoch + 1));
        for (size_t i = order.size(); i-- > 1;) {
            st += 0x9E3779B97F4A7C15ull;
            uint64_t z = st;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            std::swap(order[i], order[(size_t)(z % (i + 1))]);
        }
        return order;
    }
    // -> the next batch (its img_packed aliases an uploader slot that stays valid until the NEXT next_batch call).  Call after queuing
    // the train step of the previous batch: that is what releases its slot.
    SceneBatch next_batch() {
        if (held_ >= 0) { up_->release(held_); held_ = -1; }
        // slots - 1 views submitted ahead: the slot mapped here was released one call ago, i.e. behind a step that has finished by
        // the time the NEXT step is running — map() does not wait for the GPU in steady state
        while (inflight_.size() < depth_) submit_next();
        const InFlight f = inflight_.front();
        inflight_.erase(inflight_.begin());
        const BatchUploader::Packed p = up_->acquire(f.slot);
        held_ = f.slot;
        const LoaderView& v = views_[f.idx];
        SceneBatch b;
        b.img_packed = p.img; b.img_w = p.w; b.img_h = p.h;
        b.has_alpha = p.has_alpha; b.alpha_is_mask = v.alpha_is_mask;
        b.camera = v.camera;
        b.view_id = ids_[f.idx];
        last_index_ = f.idx;
        return b;
    }
    uint32_t last_view_index() const { return last_index_; }   // index (within this rank's shard) of the batch just handed out
    size_t num_views() const { return views_.size(); }

  private:
    struct InFlight { int slot; uint32_t idx; };
    void submit_next() {
        if (cursor_ >= order_.size()) { order_ = epoch_order(epoch_++); cursor_ = 0; }
        const uint32_t idx = order_[cursor_++];
        const LoaderView& v = views_[idx];
        auto [slot, dst] = up_->map((uint64_t)v.w * v.h * v.channels);
        v.decode(dst);
        up_->commit(slot, v.w, v.h, v.channels, v.channels == 4 && !v.alpha_is_mask);
        inflight_.push_back({slot, idx});
    }
    std::vector<LoaderView> views_;
    std::vector<uint32_t> ids_;
    std::optional<BatchUploader> up_;
    uint64_t seed_;
    uint64_t epoch_ = 0;
    std::vector<uint32_t> order_;
    size_t cursor_ = 0;
    std::vector<InFlight> inflight_;
    size_t depth_ = 2;
    int held_ = -1;
    uint32_t last_index_ = 0;
};

// ---- feature fields trained with the splats (brush_hip_feature_train.h; not in the reference) ---------------------------------------
// Carries a per-splat table [N,channels] through the ctx's pending refine plan (between bh_refine_plan and bh_refine_apply): `out` has
// the plan's total_splats rows.  BH_CARRY_COPY: rows follow their splats, a split parent's row goes to both halves;
// BH_CARRY_ZERO_SPLIT: both halves of a split are +0
inline void refine_carry_rows(const Context& ctx, const float* in, float* out, uint32_t channels, uint32_t mode = BH_CARRY_COPY) {
    static_assert(BH_CARRY_COPY == 0u && BH_CARRY_ZERO_SPLIT == 1u && BH_CARRY_MAX_CHANNELS == 4096u, "carry modes");
    ctx.check(bh_refine_carry_rows(ctx.get(), in, out, channels, mode));
}

// Per-splat feature vectors [n,channels] with their Adam moments, zero-initialised: what bh_train_step trains beside the splats once
// train_set_features has attached it.  `step` counts the Adam updates applied so far: the caller adds one after every successful
// step that carried the term (the library counts in its own copy, which the next train_set_features replaces).
struct FeatureField {
    DeviceBuffer<float> features, m1, m2;
    uint32_t n = 0, channels = 0, step = 0;
    float lr = 1e-2f, beta1 = 0.9f, beta2 = 0.999f, eps = 1e-15f;

    FeatureField() = default;
    FeatureField(uint32_t n_, uint32_t channels_, float lr_ = 1e-2f) : n(n_), channels(channels_), lr(lr_) {
        for (auto* b : {&features, &m1, &m2}) { b->resize((size_t)n * channels); b->zero(); }
    }
    BhFeatureField as_struct() {
        BhFeatureField f{};
        f.features = features.data(); f.m1 = m1.data(); f.m2 = m2.data();
        f.n = n; f.channels = channels; f.step = step;
        f.lr = lr; f.beta1 = beta1; f.beta2 = beta2; f.eps = eps;
        return f;
    }
    // between bh_refine_plan and bh_refine_apply: the features follow the plan, the moments of both halves of a split start at zero
    void carry(const Context& ctx, uint32_t total_splats) {
        DeviceBuffer<float> f2((size_t)total_splats * channels), a2((size_t)total_splats * channels), b2((size_t)total_splats * channels);
        refine_carry_rows(ctx, features.data(), f2.data(), channels, BH_CARRY_COPY);
        refine_carry_rows(ctx, m1.data(), a2.data(), channels, BH_CARRY_ZERO_SPLIT);
        refine_carry_rows(ctx, m2.data(), b2.data(), channels, BH_CARRY_ZERO_SPLIT);
        ctx.sync();   // the old tables are freed below
        features = std::move(f2); m1 = std::move(a2); m2 = std::move(b2);
        n = total_splats;
    }
};

// bh_train_step on this ctx trains `field` against `target` (both copied; nullptr field detaches; a nullptr target or a weight <= 0
// is no term).  Call it before every step — the target changes per batch — and add one to field->step after a step that succeeded
// with the term.
inline void train_set_features(const Context& ctx, FeatureField* field, const BhFeatureTarget* target) {
    if (!field) { ctx.check(bh_train_set_features(ctx.get(), nullptr, nullptr)); return; }
    const BhFeatureField f = field->as_struct();
    ctx.check(bh_train_set_features(ctx.get(), &f, target));
}

class SplatTrainer {
  public:
    SplatTrainer(const Context& ctx, TrainConfig config, float median_scene_scale = 1.0f) : ctx_(ctx), cfg_(config), median_(median_scene_scale) {}

    void set_view_cams(std::vector<float> centre_xyz_focal /*[K,4]*/) { view_cams_ = std::move(centre_xyz_focal); }  // train.rs:170-174
    uint32_t step_count() const { return step_count_; }

    // SplatTrainer::step (train.rs:176-429): forward, L1+SSIM (+alpha) loss, backward, statistics, Adam, optional noise.
    // The two stochastic terms (mean noise train.rs:389-416, background jitter :896-908): with a seed (set_seed) they are
    // drawn by the library's counter-based generator as functions of (seed, step) — the reference's default behaviour;
    // without one they only appear when injected: `noise_samples` device [N,3] N(0,1) or null, `background` the colour
    // actually used this step (parity tests).
    void set_seed(uint64_t seed) { seed_ = seed; have_seed_ = true; }
    TrainStepStats step(const SceneBatch& batch, Splats& splats, const float* noise_samples = nullptr, const float* background = nullptr) {
        ensure_state(splats);
        BhTrainConfig c = c_config(splats);
        BhTrainState st = c_state(splats);
        BhTrainBatch b{};
        b.camera = batch.camera.uniforms(batch.img_w, batch.img_h);
        b.gt_packed = batch.img_packed;
        b.has_alpha = batch.has_alpha;
        b.alpha_is_mask = batch.alpha_is_mask;
        b.view_id = batch.view_id;
        for (int k = 0; k < 3; ++k) b.background[k] = background ? background[k] : cfg_.background_color[k];
        if (!background && have_seed_) bh_sample_background(seed_, step_count_ + 1, cfg_.background_color, cfg_.background_noise_strength, b.background);
        b.noise_samples = noise_samples;
        b.device_noise = (!noise_samples && have_seed_) ? 1 : 0;
        b.noise_seed = seed_;
        BhTrainStats stats{};
        ctx_.check(bh_train_step(ctx_.get(), &c, &st, &b, nullptr, nullptr, 1.0f, &stats));
        step_count_ = st.step_count;
        ctx_.sync();  // delivers stats.loss
        return {stats.num_visible, stats.num_intersections, stats.lr_mean, stats.loss};
    }

    // SplatTrainer::refine (train.rs:431-663); `seed` replaces rand::rng().  Replaces `splats` and the optimizer state; a feature
    // field trained beside the splats is carried through the plan (brush_hip_feature_train.h).
    BhRefineStats refine(uint32_t iter, Splats& splats, uint64_t seed, FeatureField* feature_field = nullptr) {
        if (!have_state_) throw Error(BH_ERR_STATE, "Can only refine if refine stats are initialized");  // train.rs:445
        splats.bake_min_scale(ctx_);
        if (!have_bounds_) update_bounds(splats);
        BhRefineConfig rc{};
        rc.iter = iter;
        rc.total_train_iters = cfg_.total_train_iters ? cfg_.total_train_iters : 1;
        rc.growth_stop_iter = cfg_.growth_stop_iter < cfg_.total_train_iters ? cfg_.growth_stop_iter : cfg_.total_train_iters;
        rc.max_splats = cfg_.max_splats;
        rc.growth_grad_threshold = cfg_.growth_grad_threshold;
        rc.growth_select_fraction = cfg_.growth_select_fraction;
        rc.split_at_screen_size = cfg_.split_at_screen_size;
        rc.opac_decay = cfg_.opac_decay;
        for (int k = 0; k < 3; ++k) { rc.bounds_center[k] = center_[k]; rc.bounds_extent[k] = extent_[k]; }
        rc.seed = seed;
        BhTrainState in = c_state(splats);
        if (feature_field && feature_field->n != in.n) throw Error(BH_ERR_INVALID_ARG, "refine: the feature field's rows differ from the splats'");
        BhRefineStats rs{};
        ctx_.check(bh_refine_plan(ctx_.get(), &rc, &in, &rs));
        const size_t n2 = rs.total_splats, c3 = (size_t)splats.num_coeffs() * 3;
        Splats out;
        out.render_mip = splats.render_mip;
        out.transforms.resize(n2 * 10);
        out.sh_coeffs.resize(n2 * c3);
        out.raw_opacities.resize(n2);
        State ns;
        ns.alloc(n2, c3);
        BhTrainState o = in;
        o.n = (uint32_t)n2;
        o.transforms = out.transforms.data(); o.sh_coeffs = out.sh_coeffs.data(); o.raw_opacities = out.raw_opacities.data();
        ns.fill(o);
        o.min_scale = nullptr;
        if (feature_field) feature_field->carry(ctx_, rs.total_splats);
        ctx_.check(bh_refine_apply(ctx_.get(), &rc, &in, &o));
        ctx_.sync();
        splats = std::move(out);
        state_ = std::move(ns);
        update_bounds(splats);  // train.rs:634
        if ((float)iter / (float)rc.total_train_iters < 0.9f && !view_cams_.empty()) {  // train.rs:636-648, MIN_SCALE_FREEZE_FRAC
            DeviceBuffer<float> f(splats.num_splats());
            ctx_.check(bh_compute_min_scale(ctx_.get(), splats.transforms.data(), splats.num_splats(), view_cams_.data(),
                                            (uint32_t)(view_cams_.size() / 4), 0.1f, f.data()));
            splats.with_min_scale(std::move(f));
        }
        return rs;
    }

  private:
    struct State {
        DeviceBuffer<float> m1_t, m2_t, m1_sh, m2_sh, m1_o, m2_o, refine_weight_norm, vis_weight, max_screen_size;
        void alloc(size_t n, size_t c3) {
            m1_t.resize(n * 10); m2_t.resize(n * 10); m1_sh.resize(n * c3); m2_sh.resize(n); m1_o.resize(n); m2_o.resize(n);
            refine_weight_norm.resize(n); vis_weight.resize(n); max_screen_size.resize(n);
        }
        void zero() { for (auto* b : {&m1_t, &m2_t, &m1_sh, &m2_sh, &m1_o, &m2_o, &refine_weight_norm, &vis_weight, &max_screen_size}) b->zero(); }
        void fill(BhTrainState& s) {
            s.m1_transforms = m1_t.data(); s.m2_transforms = m2_t.data(); s.m1_sh = m1_sh.data(); s.m2_sh = m2_sh.data();
            s.m1_opac = m1_o.data(); s.m2_opac = m2_o.data();
            s.refine_weight_norm = refine_weight_norm.data(); s.vis_weight = vis_weight.data(); s.max_screen_size = max_screen_size.data();
        }
    };
    void ensure_state(const Splats& s) {
        if (have_state_ && state_.m2_o.size() == s.num_splats()) return;
        state_.alloc(s.num_splats(), (size_t)s.num_coeffs() * 3);
        state_.zero();
        have_state_ = true;
    }
    void update_bounds(const Splats& s) {  // get_splat_bounds (train.rs:124-133), BOUND_PERCENTILE 0.8; median_size = 2 * median extent
        ctx_.check(bh_splat_bounds(ctx_.get(), s.transforms.data(), s.num_splats(), 0.8f, center_, extent_));
        float e[3] = {extent_[0], extent_[1], extent_[2]};
        if (e[0] > e[1]) std::swap(e[0], e[1]);
        if (e[1] > e[2]) std::swap(e[1], e[2]);
        if (e[0] > e[1]) std::swap(e[0], e[1]);
        median_ = e[1] * 2.0f;
        have_bounds_ = true;
    }
    BhTrainConfig c_config(const Splats& s) const {
        BhTrainConfig c{};
        c.lr_mean = cfg_.lr_mean; c.lr_mean_end = cfg_.lr_mean_end; c.total_train_iters = cfg_.total_train_iters;
        c.lr_coeffs_dc = cfg_.lr_coeffs_dc; c.lr_coeffs_sh_scale = cfg_.lr_coeffs_sh_scale; c.lr_opac = cfg_.lr_opac;
        c.lr_scale = cfg_.lr_scale; c.lr_rotation = cfg_.lr_rotation; c.ssim_weight = cfg_.ssim_weight;
        c.match_alpha_weight = cfg_.match_alpha_weight; c.mean_noise_weight = cfg_.mean_noise_weight;
        for (int k = 0; k < 3; ++k) c.background[k] = cfg_.background_color[k];
        c.median_scene_scale = median_;
        c.render_mip = (cfg_.render_mip || s.render_mip) ? 1 : 0;
        c.exact_lists = cfg_.exact_lists ? 1 : 0;
        c.growth_stop_iter = cfg_.growth_stop_iter;   // from that step on nobody reads the refine weight (train.rs:589-614)
        return c;
    }
    BhTrainState c_state(Splats& s) {
        BhTrainState st{};
        st.n = s.num_splats(); st.sh_degree = s.sh_degree();
        st.transforms = s.transforms.data(); st.sh_coeffs = s.sh_coeffs.data(); st.raw_opacities = s.raw_opacities.data();
        state_.fill(st);
        st.step_count = step_count_;
        st.min_scale = s.min_scale ? s.min_scale->data() : nullptr;
        return st;
    }
    const Context& ctx_;
    TrainConfig cfg_;
    float median_;
    State state_;
    bool have_state_ = false, have_bounds_ = false;
    float center_[3] = {0, 0, 0}, extent_[3] = {1, 1, 1};
    uint32_t step_count_ = 0;
    uint64_t seed_ = 0;
    bool have_seed_ = false;
    std::vector<float> view_cams_;
};

// ---- LOD decimation (brush-train/src/lod.rs; the LOD boundary of brush-process/src/train_stream.rs:248-303) -------------------
constexpr uint32_t kPupPlanes = 21;  // the [21,N] accumulator: entry (i,k), i >= k, of a splat's 6x6 H in plane i(i+1)/2 + k
// `(n as f32 * keep_pct as f32 / 100.0).max(1.0) as u32` (train_stream.rs:261)
inline uint32_t lod_target_count(uint32_t n, uint32_t keep_pct) {
    const float v = std::max((float)n * (float)keep_pct / 100.0f, 1.0f);
    return v >= 4294967295.0f ? UINT32_MAX : (uint32_t)v;
}
// hessian [21,N] += J Jᵀ of v_transforms' rows (lod.rs:120-126); rows: optional device list of row ids
inline void pup_accumulate(const Context& ctx, const float* v_transforms, uint32_t n, DeviceBuffer<float>& hessian, const uint32_t* rows = nullptr,
                           uint32_t num_rows = 0) {
    if (hessian.size() != (size_t)kPupPlanes * n) throw Error(BH_ERR_INVALID_ARG, "pup_accumulate: hessian must hold [21,N] floats");
    ctx.check(bh_pup_accumulate(ctx.get(), v_transforms, n, rows, num_rows, hessian.data()));
    ctx.sync();
}
// one view of compute_pup_scores (lod.rs:91-127): forward, L1 loss against gt_packed ([h,w] rgba8 device), backward, accumulate
inline void pup_accumulate_view(const Context& ctx, const Splats& splats, const Camera& camera, const uint32_t* gt_packed, uint32_t img_w, uint32_t img_h,
                                DeviceBuffer<float>& hessian) {
    if (hessian.size() != (size_t)kPupPlanes * splats.num_splats()) throw Error(BH_ERR_INVALID_ARG, "pup_accumulate_view: hessian must hold [21,N] floats");
    const BhCamera cam = camera.uniforms(img_w, img_h);
    ctx.check(bh_pup_accumulate_view(ctx.get(), &cam, splats.num_splats(), splats.sh_degree(), splats.transforms.data(), splats.sh_coeffs.data(),
                                     splats.raw_opacities.data(), splats.min_scale ? splats.min_scale->data() : nullptr,
                                     splats.render_mip ? BH_FLAG_MIP : 0u, gt_packed, hessian.data()));
    ctx.sync();
}
// log_det_6x6 (lod.rs:44-70) of every splat's H -> scores [N]
inline DeviceBuffer<float> pup_scores(const Context& ctx, const DeviceBuffer<float>& hessian, uint32_t n) {
    if (hessian.size() != (size_t)kPupPlanes * n) throw Error(BH_ERR_INVALID_ARG, "pup_scores: hessian must hold [21,N] floats");
    DeviceBuffer<float> scores(n);
    ctx.check(bh_pup_scores(ctx.get(), hessian.data(), n, scores.data()));
    ctx.sync();
    return scores;
}
// decimate_to_count (lod.rs:13-38): the target_count highest-scored splats, score-descending (ties: ascending index; NaN last),
// min_scale gathered too.  keep_idx (optional): the source row of every kept splat.  target_count >= N: a copy of the splats.
inline Splats decimate_to_count(const Context& ctx, const Splats& splats, const float* scores, uint32_t target_count,
                                std::vector<uint32_t>* keep_idx = nullptr) {
    const uint32_t n = splats.num_splats(), k = std::min(target_count, n), c = splats.num_coeffs();
    Splats out;
    out.render_mip = splats.render_mip;
    out.transforms.resize((size_t)k * 10);
    out.sh_coeffs.resize((size_t)k * c * 3);
    out.raw_opacities.resize(k);
    if (splats.min_scale) out.min_scale.emplace(k);
    DeviceBuffer<uint32_t> idx(k);
    ctx.check(bh_decimate_to_count(ctx.get(), scores, n, target_count, c, splats.transforms.data(), splats.sh_coeffs.data(), splats.raw_opacities.data(),
                                   splats.min_scale ? splats.min_scale->data() : nullptr, out.transforms.data(), out.sh_coeffs.data(),
                                   out.raw_opacities.data(), out.min_scale ? out.min_scale->data() : nullptr, idx.data()));
    ctx.sync();
    if (keep_idx) *keep_idx = idx.download();
    return out;
}

// ---- scene editing (include/brush_hip_scene.h; not in the reference) ---------------------------------------------
// The similarity x' = s R x + t as the library's record.  Nothing is computed here: every operator is one C call.
struct SceneTransform {
    BhSceneTransform rec;

    SceneTransform() : SceneTransform(std::array<double, 4>{1.0, 0.0, 0.0, 0.0}) {}
    explicit SceneTransform(const std::array<double, 4>& quat_wxyz, const std::array<double, 3>& trans = {0.0, 0.0, 0.0}, double scale = 1.0) {
        static_assert(sizeof(BhSceneTransform) == 800 && offsetof(BhSceneTransform, rot) == 64 && offsetof(BhSceneTransform, sh_rot) == 136, "BhSceneTransform layout");
        if (bh_scene_transform_make(quat_wxyz.data(), trans.data(), scale, &rec) != 0)
            throw Error(BH_ERR_INVALID_ARG, "SceneTransform: the quaternion must be finite and not zero, the translation finite, the scale a finite number > 0");
    }
    SceneTransform inverse() const {
        SceneTransform out;
        if (bh_scene_transform_invert(&rec, &out.rec) != 0) throw Error(BH_ERR_INVALID_ARG, "SceneTransform::inverse: not a transform");
        return out;
    }
    // (*this) * other applies `other` first
    SceneTransform operator*(const SceneTransform& other) const {
        SceneTransform out;
        if (bh_scene_transform_compose(&rec, &other.rec, &out.rec) != 0) throw Error(BH_ERR_INVALID_ARG, "SceneTransform: the product is no transform");
        return out;
    }
    // D_l (band 1..4), (2l+1) x (2l+1) row-major, inside the record
    const float* sh_rotation(uint32_t l) const {
        if (l < 1 || l > 4) throw Error(BH_ERR_INVALID_ARG, "SceneTransform::sh_rotation: band 1..4");
        const uint32_t first[5] = {0, 0, 9, 34, 83};
        return rec.sh_rot + first[l];
    }
    // the uniforms of the camera that sees the moved scene as `cam` saw the original
    BhCamera apply(const BhCamera& cam) const {
        BhCamera out{};
        if (bh_camera_apply_scene_transform(&cam, &rec, &out) != 0) throw Error(BH_ERR_INVALID_ARG, "camera_apply_scene_transform: not a transform");
        return out;
    }
};

// Splats moved by T in place (means, rotations, log-scales, SH bands >= 1, min_scale); queued on the ctx stream
inline void transform_splats(const Context& ctx, Splats& s, const SceneTransform& T) {
    float* ms = s.min_scale ? s.min_scale->data() : nullptr;
    ctx.check(bh_splats_transform(ctx.get(), &T.rec, s.num_splats(), s.num_coeffs(), s.transforms.data(), s.sh_coeffs.data(), ms, s.transforms.data(),
                                  s.sh_coeffs.data(), ms));
}
// ... and into new Splats
inline Splats transformed_splats(const Context& ctx, const Splats& s, const SceneTransform& T) {
    const uint32_t n = s.num_splats();
    Splats out;
    out.render_mip = s.render_mip;
    out.transforms.resize(s.transforms.size());
    out.sh_coeffs.resize(s.sh_coeffs.size());
    out.raw_opacities.resize(n);
    if (n) hip_check(hipMemcpy(out.raw_opacities.data(), s.raw_opacities.data(), (size_t)n * 4, hipMemcpyDeviceToDevice), "hipMemcpy D2D");
    if (s.min_scale) out.min_scale.emplace(n);
    ctx.check(bh_splats_transform(ctx.get(), &T.rec, n, s.num_coeffs(), s.transforms.data(), s.sh_coeffs.data(), s.min_scale ? s.min_scale->data() : nullptr,
                                  out.transforms.data(), out.sh_coeffs.data(), out.min_scale ? out.min_scale->data() : nullptr));
    ctx.sync();
    return out;
}

// keep [N] = 1 / 0 per splat (bh_splats_select_region); count (optional): the number kept, which makes the call blocking
inline DeviceBuffer<float> select_region(const Context& ctx, const Splats& s, const BhSceneRegion& region, uint32_t* count = nullptr) {
    static_assert(sizeof(BhSceneRegion) == 76 && BH_REGION_BOX == 0u && BH_REGION_ELLIPSOID == 1u, "BhSceneRegion layout");
    DeviceBuffer<float> keep(s.num_splats());
    ctx.check(bh_splats_select_region(ctx.get(), &region, s.transforms.data(), s.raw_opacities.data(), s.num_splats(), keep.data(), count));
    return keep;
}
// the kept rows in source order: select, count, decimate_to_count (ties keep ascending index)
inline Splats crop_splats(const Context& ctx, const Splats& s, const BhSceneRegion& region, std::vector<uint32_t>* keep_idx = nullptr) {
    uint32_t count = 0;
    const DeviceBuffer<float> keep = select_region(ctx, s, region, &count);
    return decimate_to_count(ctx, s, keep.data(), count, keep_idx);
}

// ---- mask lifting (include/brush_hip_lift.h; not in the reference) -----------------------------------------------
// The rows where keep [N] (device, 1 / 0: LiftAccumulator::select, select_region) is not 0, in source order: count (one readback of
// keep), then decimate_to_count, whose ties keep ascending index.  keep_idx serves FeatureField::gather.
inline Splats compact_splats(const Context& ctx, const Splats& s, const DeviceBuffer<float>& keep, std::vector<uint32_t>* keep_idx = nullptr) {
    if (keep.size() != s.num_splats()) throw Error(BH_ERR_INVALID_ARG, "compact_splats: one keep value per splat");
    ctx.sync();
    const std::vector<float> host = keep.download();
    const uint32_t count = (uint32_t)std::count_if(host.begin(), host.end(), [](float k) { return k != 0.0f; });
    return decimate_to_count(ctx, s, keep.data(), count, keep_idx);
}

// The tables of a mask lifting over any number of views: votes u64 [N,L] (votes[i, l] = the summed blend weight of splat i at the
// pixels of label l, in units of 2^-24) and, with stats, max_weight f32 [N] and pixel_count u32 [N].  Nothing is computed here.
class LiftAccumulator {
  public:
    LiftAccumulator(const Context& ctx, uint32_t n, uint32_t num_labels, bool stats = true) : ctx_(ctx), n_(n), num_labels_(num_labels), stats_(stats) {
        static_assert(sizeof(BhLiftSelect) == 24 && offsetof(BhLiftSelect, min_pixels) == 16 && BH_LIFT_MAX_LABELS == 256u && BH_LIFT_ANY_LABEL == 0xFFFFFFFFu,
                      "BhLiftSelect layout");
        if (num_labels == 0 || num_labels > BH_LIFT_MAX_LABELS) throw Error(BH_ERR_INVALID_ARG, "LiftAccumulator: num_labels must be 1 .. 256");
        votes.resize((size_t)n * num_labels);
        if (stats) {
            max_weight.resize(n);
            pixel_count.resize(n);
        }
        clear();
    }
    void clear() {
        votes.zero();
        max_weight.zero();
        pixel_count.zero();
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // the fills are ordered before the ctx stream's kernels
    }
    // one view's votes (bh_lift_accumulate): labels uint8 [H,W] on the device, or nullptr: label 0 everywhere
    void add(const RenderNode& node, const uint8_t* labels) {
        if (node.aux.num_splats != n_) throw Error(BH_ERR_INVALID_ARG, "LiftAccumulator::add: the node renders another number of splats");
        ctx_.check(bh_lift_accumulate(ctx_.get(), &node.aux.raw, labels, num_labels_, votes.data(), stats_ ? max_weight.data() : nullptr,
                                      stats_ ? pixel_count.data() : nullptr));
    }
    // the label with the most votes per splat, ties to the lowest; BH_LIFT_UNASSIGNED below min_weight (bh_lift_assign)
    DeviceBuffer<uint8_t> assign(float min_weight = 0.0f, DeviceBuffer<float>* share = nullptr) const {
        DeviceBuffer<uint8_t> out(n_);
        if (share) share->resize(n_);
        ctx_.check(bh_lift_assign(ctx_.get(), votes.data(), n_, num_labels_, min_weight, out.data(), share ? share->data() : nullptr));
        ctx_.sync();
        return out;
    }
    // keep [N] = 1 / 0 (bh_lift_select), what compact_splats takes
    DeviceBuffer<float> select(const BhLiftSelect& sel) const {
        DeviceBuffer<float> keep(n_);
        ctx_.check(bh_lift_select(ctx_.get(), votes.data(), stats_ ? max_weight.data() : nullptr, stats_ ? pixel_count.data() : nullptr, n_, num_labels_, &sel,
                                  keep.data()));
        ctx_.sync();
        return keep;
    }
    uint32_t num_splats() const { return n_; }
    uint32_t num_labels() const { return num_labels_; }

    DeviceBuffer<uint64_t> votes;
    DeviceBuffer<float> max_weight;
    DeviceBuffer<uint32_t> pixel_count;

  private:
    const Context& ctx_;
    uint32_t n_, num_labels_;
    bool stats_;
};

// ---- held-out evaluation (brush-train/src/eval.rs:23-63; run_eval of brush-process/src/train_stream.rs:506-566) ----------------
// eval_stats' metrics of a rendered [h,w,4] f32 image against gt_packed ([h,w] rgba8 device): metrics (device float[3]) = mse, psnr,
// ssim; rgb8 (device [h,w] or null) = the quantised RGB as rgba8.  Queued on the ctx stream (bh_eval_metrics).
inline void eval_metrics(const Context& ctx, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w, float* metrics,
                         uint32_t* rgb8 = nullptr) {
    ctx.check(bh_eval_metrics(ctx.get(), img_hwc4, gt_packed, h, w, metrics, rgb8));
}
struct EvalSample {  // eval.rs:14-20: the view's metrics, read back; image (keep_image): the quantised render as rgba8 [H,W]
    float mse = 0.0f, psnr = 0.0f, ssim = 0.0f;
    std::optional<DeviceBuffer<uint32_t>> image;
};
// eval_stats of one view (bh_eval_view): render on black with the floor folded in, quantise, score against gt_packed
inline EvalSample eval_stats(const Context& ctx, const Splats& splats, const Camera& camera, const uint32_t* gt_packed, uint32_t img_w, uint32_t img_h,
                             bool keep_image = false) {
    const BhCamera cam = camera.uniforms(img_w, img_h);
    DeviceBuffer<float> metrics(3);
    EvalSample out;
    if (keep_image) out.image.emplace((size_t)img_w * img_h);
    ctx.check(bh_eval_view(ctx.get(), &cam, splats.num_splats(), splats.sh_degree(), splats.transforms.data(), splats.sh_coeffs.data(),
                           splats.raw_opacities.data(), splats.min_scale ? splats.min_scale->data() : nullptr, splats.render_mip ? BH_FLAG_MIP : 0u,
                           gt_packed, metrics.data(), out.image ? out.image->data() : nullptr));
    ctx.sync();
    const std::vector<float> m = metrics.download();
    out.mse = m[0];
    out.psnr = m[1];
    out.ssim = m[2];
    return out;
}
struct EvalResult {  // train_stream.rs:559-560: per-view PSNR and SSIM averaged in f32; per_view rows (mse, psnr, ssim) in view order
    float avg_psnr = 0.0f, avg_ssim = 0.0f;
    std::vector<std::array<float, 3>> per_view;
    std::vector<DeviceBuffer<uint32_t>> images;   // keep_images: every view's rgba8 render
};
// run_eval over held-out views given as the loader's views (decoded into the uploader's pinned slots, packed like
// view_to_packed_data: premultiplied unless the alpha is a mask); the metrics stay on the device until one readback at the end
inline EvalResult run_eval(const Context& ctx, const Splats& splats, const std::vector<LoaderView>& views, bool keep_images = false) {
    EvalResult r;
    uint64_t max_pixels = 1;
    for (const LoaderView& v : views) max_pixels = std::max<uint64_t>(max_pixels, (uint64_t)v.w * v.h);
    DeviceBuffer<float> table(std::max<size_t>(views.size(), 1) * 3);
    {
        BatchUploader up(ctx, max_pixels, 2);
        for (size_t i = 0; i < views.size(); ++i) {
            const LoaderView& v = views[i];
            if (v.channels != 3 && v.channels != 4) throw Error(BH_ERR_INVALID_ARG, "run_eval: views must have 3 or 4 channels");
            auto [slot, dst] = up.map((uint64_t)v.w * v.h * v.channels);
            v.decode(dst);
            up.commit(slot, v.w, v.h, v.channels, v.channels == 4 && !v.alpha_is_mask);
            const BatchUploader::Packed gt = up.acquire(slot);
            const BhCamera cam = v.camera.uniforms(gt.w, gt.h);
            if (keep_images) r.images.emplace_back((size_t)gt.w * gt.h);
            ctx.check(bh_eval_view(ctx.get(), &cam, splats.num_splats(), splats.sh_degree(), splats.transforms.data(), splats.sh_coeffs.data(),
                                   splats.raw_opacities.data(), splats.min_scale ? splats.min_scale->data() : nullptr,
                                   splats.render_mip ? BH_FLAG_MIP : 0u, gt.img, table.data() + 3 * i, keep_images ? r.images.back().data() : nullptr));
            up.release(slot);
        }
        ctx.sync();   // (before the uploader's slots go)
    }
    const std::vector<float> t = table.download();
    float psnr = 0.0f, ssim = 0.0f;
    for (size_t i = 0; i < views.size(); ++i) {
        r.per_view.push_back({t[3 * i], t[3 * i + 1], t[3 * i + 2]});
        psnr += t[3 * i + 1];
        ssim += t[3 * i + 2];
    }
    r.avg_psnr = psnr / (float)views.size();
    r.avg_ssim = ssim / (float)views.size();
    return r;
}

// ---- LPIPS (crates/lpips/src/lib.rs; the lpips_loss_weight term of brush-train/src/train.rs:265-273) ------------------------------
// The VGG16 LpipsModel on the ctx's device (bh_lpips_create): params = BH_LPIPS_PARAM_COUNT floats in the canonical order of
// brush_hip_lpips.h.  Move-only; the model must outlive any ctx it is attached to (train_set_lpips).
class Lpips {
public:
    Lpips(const Context& ctx, const std::vector<float>& params) {
        h_ = bh_lpips_create(ctx.get(), params.data(), params.size());
        if (!h_) throw Error(BH_ERR_INVALID_ARG, bh_last_error(ctx.get()));
    }
    Lpips(const Lpips&) = delete;
    Lpips& operator=(const Lpips&) = delete;
    Lpips(Lpips&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Lpips& operator=(Lpips&& o) noexcept {
        if (this != &o) { bh_lpips_destroy(h_); h_ = o.h_; o.h_ = nullptr; }
        return *this;
    }
    ~Lpips() { bh_lpips_destroy(h_); }
    const bh_lpips* get() const { return h_; }

private:
    bh_lpips* h_ = nullptr;
};
// value (device float[1]) = LPIPS(img_hwc4 rgb, GT [+ (1 - a) bg when composite_bg]); queued on the ctx stream (bh_lpips_forward)
inline void lpips(const Context& ctx, const Lpips& model, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w, float* value,
                  const float* composite_bg = nullptr) {
    ctx.check(bh_lpips_forward(ctx.get(), model.get(), img_hwc4, gt_packed, h, w, composite_bg, value));
}
// ... and v_output [h,w,4] += weight * dLPIPS/dimg on rgb (bh_lpips_value_and_grad)
inline void lpips_value_and_grad(const Context& ctx, const Lpips& model, const float* img_hwc4, const uint32_t* gt_packed, uint32_t h, uint32_t w,
                                 float weight, float* value, float* v_output, const float* composite_bg = nullptr) {
    ctx.check(bh_lpips_value_and_grad(ctx.get(), model.get(), img_hwc4, gt_packed, h, w, composite_bg, weight, value, v_output));
}
// bh_train_step on this ctx adds weight * LPIPS (model == nullptr or weight 0: detached)
inline void train_set_lpips(const Context& ctx, const Lpips* model, float weight) {
    ctx.check(bh_train_set_lpips(ctx.get(), model ? model->get() : nullptr, weight));
}

// ---- camera pose gradients (brush_hip_pose.h; not in the reference) ---------------------------------------------------------------
// bh_train_step on this ctx writes the step's pose gradient into v_viewmat (device, 12 floats); nullptr detaches
inline void train_set_pose_grad(const Context& ctx, float* v_viewmat) { ctx.check(bh_train_set_pose_grad(ctx.get(), v_viewmat)); }
// (v_omega, v_tau) of a view-matrix gradient at the pose vm, in f64 on the host
inline std::array<double, 6> pose_twist(const float vm[12], const float v_viewmat[12]) {
    std::array<double, 6> t{};
    if (bh_pose_twist(vm, v_viewmat, t.data()) != 0) throw Error(BH_ERR_INVALID_ARG, "pose_twist: null argument");
    return t;
}
// W <- exp([omega]x) W, t <- exp([omega]x) t + tau on the uniforms, vm and cam_pos together
inline void camera_apply_twist(BhCamera& cam, const std::array<double, 6>& twist) {
    if (bh_camera_apply_twist(&cam, twist.data()) != 0) throw Error(BH_ERR_INVALID_ARG, "camera_apply_twist: null argument, a degenerate view matrix or a twist that is not finite");
}

// ---- camera intrinsics gradients (brush_hip_intrinsics.h; not in the reference) -------------------------------------
// bh_train_step on this ctx writes the step's intrinsics gradient into v_intrinsics (device, 4 floats); nullptr detaches
inline void train_set_intrinsics_grad(const Context& ctx, float* v_intrinsics) { ctx.check(bh_train_set_intrinsics_grad(ctx.get(), v_intrinsics)); }
// fx, fy, cx, cy into the uniforms, with the clamp limits and the cull angle that follow from them
inline void camera_set_intrinsics(BhCamera& cam, double fx, double fy, double cx, double cy) {
    if (bh_camera_set_intrinsics(&cam, fx, fy, cx, cy) != 0) throw Error(BH_ERR_INVALID_ARG, "camera_set_intrinsics: fx, fy must be positive, all four finite");
}

// ---- per-view exposure compensation (brush_hip_exposure.h; not in the reference) ---------------------------------------------------
// A device table of one affine colour transform m[12] (row-major 3x4, column 3 the offset) per training view, with Adam on the
// device (bh_exposure_*).  Views are numbered from 1.  Move-only; destroy it before its Context (a Context that dies first frees
// the table itself, and this handle must then not be used).  Only the getters read back.
class ExposureTable {
public:
    ExposureTable(const Context& ctx, uint32_t n_views, double lr = 1e-3, double beta1 = 0.9, double beta2 = 0.999, double eps = 1e-8)
        : ctx_(&ctx), n_(n_views), beta1_(beta1), beta2_(beta2), eps_(eps) {
        ctx.check(bh_exposure_create(ctx.get(), n_views, &h_));
        set_lr(lr);
    }
    ExposureTable(const ExposureTable&) = delete;
    ExposureTable& operator=(const ExposureTable&) = delete;
    ExposureTable(ExposureTable&& o) noexcept : ctx_(o.ctx_), h_(o.h_), n_(o.n_), beta1_(o.beta1_), beta2_(o.beta2_), eps_(o.eps_) { o.h_ = nullptr; }
    ~ExposureTable() { if (h_) (void)bh_exposure_destroy(ctx_->get(), h_); }
    bh_exposure* get() const { return h_; }
    uint32_t n_views() const { return n_; }
    void set_lr(double lr) { ctx_->check(bh_exposure_set_adam(ctx_->get(), h_, lr, beta1_, beta2_, eps_)); }
    // every row, [V,12] on the host (one synchronisation each)
    std::vector<float> params() const {
        std::vector<float> out((size_t)n_ * 12);
        ctx_->check(bh_exposure_get_params(ctx_->get(), h_, 1, n_, out.data()));
        return out;
    }
    std::vector<float> grads() const {
        std::vector<float> out((size_t)n_ * 12);
        ctx_->check(bh_exposure_get_grad(ctx_->get(), h_, 1, n_, out.data()));
        return out;
    }
    void set_params(const std::vector<float>& rows, uint32_t first_view = 1) {
        ctx_->check(bh_exposure_set_params(ctx_->get(), h_, first_view, (uint32_t)(rows.size() / 12), rows.data()));
    }
    struct State { std::array<double, 12> m1, m2; uint32_t t; };
    State state(uint32_t view) const {
        State s{};
        ctx_->check(bh_exposure_get_state(ctx_->get(), h_, view, s.m1.data(), s.m2.data(), &s.t));
        return s;
    }
    void set_state(uint32_t view, const State& s) { ctx_->check(bh_exposure_set_state(ctx_->get(), h_, view, s.m1.data(), s.m2.data(), s.t)); }
    // out = A x + b of img [h,w,4] (device) with the row of `view`; out may be img
    void apply(uint32_t view, const float* img_hwc4, uint32_t h, uint32_t w, float* out_hwc4) const {
        ctx_->check(bh_exposure_apply(ctx_->get(), h_, view, img_hwc4, h, w, out_hwc4));
    }
    // v_img = A^T v_exposed (may be in place), grads[view] = v_m, and with `update` one Adam step of the row
    void backward(uint32_t view, const float* img_hwc4, const float* v_exposed, uint32_t h, uint32_t w, float* v_img, bool update = false) {
        ctx_->check(bh_exposure_backward(ctx_->get(), h_, view, img_hwc4, v_exposed, h, w, v_img, update ? 1 : 0));
    }

private:
    const Context* ctx_;
    bh_exposure* h_ = nullptr;
    uint32_t n_;
    double beta1_, beta2_, eps_;
};
// bh_train_step on this ctx exposes its frame with the row of the batch's view_id and updates that row; nullptr detaches
inline void train_set_exposure(const Context& ctx, const ExposureTable* table) {
    ctx.check(bh_train_set_exposure(ctx.get(), table ? table->get() : nullptr));
}

// ---- environment maps (brush_hip_envmap.h; not in the reference) ------------------------------------------------------
// A device cubemap E[6][R][R][3] behind the splats with Adam on the device (bh_envmap_*): faces +X -X +Y -Y +Z -Z in world axes, pinhole
// cameras only, black when new.  Move-only; destroy it before its Context (a Context that dies first frees the map itself, and this
// handle must then not be used).  Only the getters read back, and backward (four bytes, to refuse a cotangent that is not finite).
class EnvironmentMap {
public:
    EnvironmentMap(const Context& ctx, uint32_t resolution = 64, double lr = 1e-3, double beta1 = 0.9, double beta2 = 0.999, double eps = 1e-15)
        : ctx_(&ctx), res_(resolution), beta1_(beta1), beta2_(beta2), eps_(eps) {
        ctx.check(bh_envmap_create(ctx.get(), resolution, &h_));
        set_lr(lr);
    }
    EnvironmentMap(const EnvironmentMap&) = delete;
    EnvironmentMap& operator=(const EnvironmentMap&) = delete;
    EnvironmentMap(EnvironmentMap&& o) noexcept : ctx_(o.ctx_), h_(o.h_), res_(o.res_), beta1_(o.beta1_), beta2_(o.beta2_), eps_(o.eps_) { o.h_ = nullptr; }
    ~EnvironmentMap() { if (h_) (void)bh_envmap_destroy(ctx_->get(), h_); }
    bh_envmap* get() const { return h_; }
    uint32_t resolution() const { return res_; }
    size_t floats() const { return (size_t)6 * res_ * res_ * 3; }
    void set_lr(double lr) { ctx_->check(bh_envmap_set_adam(ctx_->get(), h_, lr, beta1_, beta2_, eps_)); }
    // the table and its last gradient, [6,R,R,3] on the host (one synchronisation each)
    std::vector<float> params() const {
        std::vector<float> out(floats());
        ctx_->check(bh_envmap_get_params(ctx_->get(), h_, out.data()));
        return out;
    }
    std::vector<float> grads() const {
        std::vector<float> out(floats());
        ctx_->check(bh_envmap_get_grad(ctx_->get(), h_, out.data()));
        return out;
    }
    void set_params(const std::vector<float>& table) {
        if (table.size() != floats()) throw Error(BH_ERR_INVALID_ARG, "EnvironmentMap::set_params: the table must hold 6 R R 3 floats");
        ctx_->check(bh_envmap_set_params(ctx_->get(), h_, table.data()));
    }
    struct State { std::vector<float> m1, m2; uint32_t t = 0; };
    State state() const {
        State s;
        s.m1.resize(floats());
        s.m2.resize(floats());
        ctx_->check(bh_envmap_get_state(ctx_->get(), h_, s.m1.data(), s.m2.data(), &s.t));
        return s;
    }
    void set_state(const State& s) {
        if (s.m1.size() != floats() || s.m2.size() != floats()) throw Error(BH_ERR_INVALID_ARG, "EnvironmentMap::set_state: the moments must hold 6 R R 3 floats");
        ctx_->check(bh_envmap_set_state(ctx_->get(), h_, s.m1.data(), s.m2.data(), s.t));
    }
    // out = img [h,w,4] (device, rendered on black) over the map as `cam` sees it; out may be img
    void composite(const BhCamera& cam, const float* img_hwc4, uint32_t h, uint32_t w, float* out_hwc4) const {
        ctx_->check(bh_envmap_composite(ctx_->get(), h_, &cam, img_hwc4, h, w, out_hwc4));
    }
    // v_img = the gradient to the frame (may be in place), grads = v_E, and with `update` one Adam step of the table
    void backward(const BhCamera& cam, const float* img_hwc4, const float* v_out, uint32_t h, uint32_t w, float* v_img, bool update = false) {
        ctx_->check(bh_envmap_backward(ctx_->get(), h_, &cam, img_hwc4, v_out, h, w, v_img, update ? 1 : 0));
    }

private:
    const Context* ctx_;
    bh_envmap* h_ = nullptr;
    uint32_t res_;
    double beta1_, beta2_, eps_;
};
// bh_train_step on this ctx composites its frame over the map before the loss and updates the map; nullptr detaches
inline void train_set_envmap(const Context& ctx, const EnvironmentMap* map) {
    ctx.check(bh_train_set_envmap(ctx.get(), map ? map->get() : nullptr));
}

// ---- per-view bilateral grids (brush_hip_bilagrid.h; not in the reference) ----------------------------------------------------------
// A device table of one grid g[Hg][Wg][L][12] of row-major 3x4 colour matrices per training view, sliced by trilinear interpolation at
// (x, y, luminance), with Adam on the device (bh_bilagrid_*).  Views are numbered from 1.  Move-only; destroy it before its Context (a
// Context that dies first frees the table itself, and this handle must then not be used).  Only the getters read back.
class BilateralGridTable {
public:
    BilateralGridTable(const Context& ctx, uint32_t n_views, uint32_t grid_w = 16, uint32_t grid_h = 16, uint32_t grid_l = 8, double lr = 2e-3,
                       double beta1 = 0.9, double beta2 = 0.999, double eps = 1e-15)
        : ctx_(&ctx), n_(n_views), row_((size_t)grid_w * grid_h * grid_l * 12), beta1_(beta1), beta2_(beta2), eps_(eps) {
        ctx.check(bh_bilagrid_create(ctx.get(), n_views, grid_w, grid_h, grid_l, &h_));
        set_lr(lr);
    }
    BilateralGridTable(const BilateralGridTable&) = delete;
    BilateralGridTable& operator=(const BilateralGridTable&) = delete;
    BilateralGridTable(BilateralGridTable&& o) noexcept : ctx_(o.ctx_), h_(o.h_), n_(o.n_), row_(o.row_), beta1_(o.beta1_), beta2_(o.beta2_), eps_(o.eps_) {
        o.h_ = nullptr;
    }
    ~BilateralGridTable() { if (h_) (void)bh_bilagrid_destroy(ctx_->get(), h_); }
    bh_bilagrid* get() const { return h_; }
    uint32_t n_views() const { return n_; }
    size_t row_floats() const { return row_; }   // Hg Wg L 12
    std::array<uint32_t, 3> grid() const {        // (Wg, Hg, L)
        std::array<uint32_t, 3> g{};
        ctx_->check(bh_bilagrid_dims(ctx_->get(), h_, nullptr, &g[0], &g[1], &g[2]));
        return g;
    }
    void set_lr(double lr) { ctx_->check(bh_bilagrid_set_adam(ctx_->get(), h_, lr, beta1_, beta2_, eps_)); }
    // every grid, [V,Hg,Wg,L,12] on the host (one synchronisation each)
    std::vector<float> params() const {
        std::vector<float> out((size_t)n_ * row_);
        ctx_->check(bh_bilagrid_get_params(ctx_->get(), h_, 1, n_, out.data()));
        return out;
    }
    std::vector<float> grads() const {
        std::vector<float> out((size_t)n_ * row_);
        ctx_->check(bh_bilagrid_get_grad(ctx_->get(), h_, 1, n_, out.data()));
        return out;
    }
    void set_params(const std::vector<float>& rows, uint32_t first_view = 1) {
        ctx_->check(bh_bilagrid_set_params(ctx_->get(), h_, first_view, (uint32_t)(rows.size() / row_), rows.data()));
    }
    struct State { std::vector<float> m1, m2; uint32_t t; };
    State state(uint32_t view) const {
        State s{std::vector<float>(row_), std::vector<float>(row_), 0u};
        ctx_->check(bh_bilagrid_get_state(ctx_->get(), h_, view, s.m1.data(), s.m2.data(), &s.t));
        return s;
    }
    void set_state(uint32_t view, const State& s) {
        if (s.m1.size() != row_ || s.m2.size() != row_) throw Error(BH_ERR_INVALID_ARG, "BilateralGridTable::set_state: moments of another grid size");
        ctx_->check(bh_bilagrid_set_state(ctx_->get(), h_, view, s.m1.data(), s.m2.data(), s.t));
    }
    // out = the slice of img [h,w,4] (device) with the grid of `view`; out may be img
    void slice(uint32_t view, const float* img_hwc4, uint32_t h, uint32_t w, float* out_hwc4) const {
        ctx_->check(bh_bilagrid_slice(ctx_->get(), h_, view, img_hwc4, h, w, out_hwc4));
    }
    // v_img of v_sliced (may be in place), grads[view] = v_g + tv_weight dTV, and with `update` one Adam step of the grid
    void backward(uint32_t view, const float* img_hwc4, const float* v_sliced, uint32_t h, uint32_t w, float* v_img, float tv_weight = 0.0f,
                  bool update = false) {
        ctx_->check(bh_bilagrid_backward(ctx_->get(), h_, view, img_hwc4, v_sliced, h, w, v_img, tv_weight, update ? 1 : 0));
    }
    // value_dev[0] = the total variation of the grid of `view`; nothing is read back
    void tv(uint32_t view, float* value_dev) const { ctx_->check(bh_bilagrid_tv(ctx_->get(), h_, view, value_dev)); }

private:
    const Context* ctx_;
    bh_bilagrid* h_ = nullptr;
    uint32_t n_;
    size_t row_;
    double beta1_, beta2_, eps_;
};
// bh_train_step on this ctx slices its frame with the grid of the batch's view_id, adds tv_weight TV to the loss and updates that grid;
// nullptr detaches.  Not together with an exposure table.
inline void train_set_bilagrid(const Context& ctx, const BilateralGridTable* table, float tv_weight = 10.0f) {
    ctx.check(bh_train_set_bilagrid(ctx.get(), table ? table->get() : nullptr, tv_weight));
}

// ---- mesh extraction (brush_hip_mesh.h; not in the reference) -----------------------------------------------------------------------
static_assert(sizeof(BhTsdfGrid) == 56 && offsetof(BhTsdfGrid, voxel_size) == 12 && offsetof(BhTsdfGrid, nx) == 16 && offsetof(BhTsdfGrid, trunc) == 28 &&
                  offsetof(BhTsdfGrid, max_weight) == 32 && offsetof(BhTsdfGrid, tw) == 40 && offsetof(BhTsdfGrid, rgb) == 48,
              "BhTsdfGrid layout");
static_assert(sizeof(BhTsdfIntegrateConfig) == 16 && offsetof(BhTsdfIntegrateConfig, depth_max) == 4 && offsetof(BhTsdfIntegrateConfig, alpha_min) == 8,
              "BhTsdfIntegrateConfig layout");
// A triangle mesh on the device: vertices [V,3] f32, colours [V,3] f32 (empty: none), triangles [M,3] u32.
struct Mesh {
    DeviceBuffer<float> vertices, colours;
    DeviceBuffer<uint32_t> triangles;
    uint32_t n_vertices = 0, n_triangles = 0;
};
// bh_mesh_to_ply: the mesh as a binary little-endian PLY file (rows packed on the device, one copy)
inline std::vector<uint8_t> mesh_to_ply(const Context& ctx, const float* vertices, const float* colours /*or nullptr*/, uint32_t n_v, const uint32_t* triangles,
                                        uint32_t n_t) {
    uint64_t need = 0;
    ctx.check(bh_mesh_to_ply(ctx.get(), vertices, colours, n_v, triangles, n_t, nullptr, 0, &need));
    std::vector<uint8_t> out(need);
    ctx.check(bh_mesh_to_ply(ctx.get(), vertices, colours, n_v, triangles, n_t, out.data(), need, &need));
    return out;
}
namespace detail {
// what TsdfVolume and SparseTsdfVolume share: the fields of their structs, the view vectors' check, and extraction over the
// volume's struct, whose type picks the two C entry points
inline int tsdf_extract_count(bh_ctx* c, const BhTsdfGrid* v, uint32_t* nv, uint32_t* nt) { return bh_tsdf_extract_count(c, v, nv, nt); }
inline int tsdf_extract_count(bh_ctx* c, const BhSparseTsdf* v, uint32_t* nv, uint32_t* nt) { return bh_sptsdf_extract_count(c, v, nv, nt); }
inline int tsdf_extract(bh_ctx* c, const BhTsdfGrid* v, float* vertices, float* colours, uint32_t* triangles, uint32_t cap_v, uint32_t cap_t, uint32_t* nv, uint32_t* nt) {
    return bh_tsdf_extract(c, v, vertices, colours, triangles, cap_v, cap_t, nv, nt);
}
inline int tsdf_extract(bh_ctx* c, const BhSparseTsdf* v, float* vertices, float* colours, uint32_t* triangles, uint32_t cap_v, uint32_t cap_t, uint32_t* nv, uint32_t* nt) {
    return bh_sptsdf_extract(c, v, vertices, colours, triangles, cap_v, cap_t, nv, nt);
}
template <class V>
inline V tsdf_fields(const std::array<float, 3>& origin, float voxel_size, const std::array<uint32_t, 3>& dims, float trunc, float max_weight) {
    V v{};
    for (int a = 0; a < 3; ++a) v.origin[a] = origin[a];
    v.voxel_size = voxel_size;
    v.nx = dims[0]; v.ny = dims[1]; v.nz = dims[2];
    v.trunc = trunc > 0.0f ? trunc : 4.0f * voxel_size;
    v.max_weight = max_weight;
    return v;
}
inline void tsdf_check_views(const char* who, const std::vector<BhCamera>& cams, const std::vector<const float*>& depths, const std::vector<const float*>& images) {
    if (depths.size() != cams.size() || (!images.empty() && images.size() != cams.size()))
        throw Error(BH_ERR_INVALID_ARG, std::string(who) + ": as many depth maps (and images) as cameras");
}
template <class V>
inline std::pair<uint32_t, uint32_t> tsdf_count(const Context& ctx, const V& v) {
    uint32_t nv = 0, nt = 0;
    ctx.check(tsdf_extract_count(ctx.get(), &v, &nv, &nt));
    return {nv, nt};
}
template <class V>
inline Mesh tsdf_mesh(const Context& ctx, const V& v) {
    Mesh m;
    const auto [nv, nt] = tsdf_count(ctx, v);
    m.vertices.resize((size_t)nv * 3);
    if (v.rgb) m.colours.resize((size_t)nv * 3);
    m.triangles.resize((size_t)nt * 3);
    ctx.check(tsdf_extract(ctx.get(), &v, m.vertices.data(), v.rgb ? m.colours.data() : nullptr, m.triangles.data(), nv, nt, &m.n_vertices, &m.n_triangles));
    return m;
}
template <class V>
inline std::vector<uint8_t> tsdf_to_ply(const Context& ctx, const V& v) {
    const Mesh m = tsdf_mesh(ctx, v);
    return mesh_to_ply(ctx, m.vertices.data(), v.rgb ? m.colours.data() : nullptr, m.n_vertices, m.triangles.data(), m.n_triangles);
}
}  // namespace detail
// A dense TSDF volume that owns its device memory: nx x ny x nz samples at origin + voxel_size * (i, j, k), x fastest; tw holds
// { tsdf in units of trunc, weight }, rgb the mean colour.  integrate() fuses depth maps (KinectFusion's running mean, up to
// BH_TSDF_MAX_BATCH views per pass over the volume), extract() is marching tetrahedra at the zero level.  Move-only.
class TsdfVolume {
public:
    TsdfVolume(const Context& ctx, const std::array<float, 3>& origin, float voxel_size, const std::array<uint32_t, 3>& dims, float trunc = 0.0f /*0: 4 voxels*/,
               float max_weight = 64.0f, bool colour = true)
        : ctx_(&ctx), g_(detail::tsdf_fields<BhTsdfGrid>(origin, voxel_size, dims, trunc, max_weight)) {
        const uint64_t n = (uint64_t)dims[0] * dims[1] * dims[2];
        if (dims[0] < 2 || dims[1] < 2 || dims[2] < 2 || n > 0x7FFFFFFFull) throw Error(BH_ERR_INVALID_ARG, "TsdfVolume: dimensions of 2 or more, at most 2^31 - 1 samples");
        tw_.resize((size_t)n * 2);
        if (colour) rgb_.resize((size_t)n * 3);
        g_.tw = tw_.data();
        g_.rgb = colour ? rgb_.data() : nullptr;
        clear();
    }
    TsdfVolume(const TsdfVolume&) = delete;
    TsdfVolume& operator=(const TsdfVolume&) = delete;
    TsdfVolume(TsdfVolume&&) noexcept = default;
    const BhTsdfGrid& grid() const { return g_; }
    size_t samples() const { return (size_t)g_.nx * g_.ny * g_.nz; }
    std::vector<float> tw() const { ctx_->sync(); return tw_.download(); }     // [nz,ny,nx,2] on the host
    std::vector<float> rgb() const { ctx_->sync(); return rgb_.download(); }   // [nz,ny,nx,3] on the host (empty without colour)
    void set_tw(const std::vector<float>& host) {   // a field computed elsewhere, [nz,ny,nx,2]
        if (host.size() != samples() * 2) throw Error(BH_ERR_INVALID_ARG, "TsdfVolume::set_tw: a field of another size");
        ctx_->sync();
        hip_check(hipMemcpy(tw_.data(), host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy H2D");
    }
    void clear() { ctx_->check(bh_tsdf_clear(ctx_->get(), &g_)); }
    // depths[v] [H,W] and images[v] [H,W,4] (or an empty vector: no alpha test, no colour) are device pointers of cams[v]'s size
    void integrate(const std::vector<BhCamera>& cams, const std::vector<const float*>& depths, const std::vector<const float*>& images = {},
                   float depth_min = 0.0f, float depth_max = INFINITY, float alpha_min = 0.5f) {
        detail::tsdf_check_views("TsdfVolume::integrate", cams, depths, images);
        const BhTsdfIntegrateConfig cfg{depth_min, depth_max, alpha_min, 0u};
        ctx_->check(bh_tsdf_integrate(ctx_->get(), &g_, (uint32_t)cams.size(), cams.data(), depths.data(), images.empty() ? nullptr : images.data(), &cfg));
    }
    std::pair<uint32_t, uint32_t> count() const { return detail::tsdf_count(*ctx_, g_); }   // (vertices, triangles); blocking
    Mesh extract() const { return detail::tsdf_mesh(*ctx_, g_); }
    std::vector<uint8_t> to_ply() const { return detail::tsdf_to_ply(*ctx_, g_); }

private:
    const Context* ctx_;
    BhTsdfGrid g_;
    DeviceBuffer<float> tw_, rgb_;
};

// ---- sparse TSDF volumes (brush_hip_sparse_mesh.h; not in the reference) --------------------------------------------------------------
static_assert(sizeof(BhSparseTsdf) == 80 && offsetof(BhSparseTsdf, voxel_size) == 12 && offsetof(BhSparseTsdf, nx) == 16 && offsetof(BhSparseTsdf, trunc) == 28 &&
                  offsetof(BhSparseTsdf, n_blocks) == 36 && offsetof(BhSparseTsdf, bits) == 40 && offsetof(BhSparseTsdf, rank) == 48 &&
                  offsetof(BhSparseTsdf, keys) == 56 && offsetof(BhSparseTsdf, tw) == 64 && offsetof(BhSparseTsdf, rgb) == 72,
              "BhSparseTsdf layout");
// A sparse TSDF volume that owns its device memory: a virtual grid of up to 8192 samples per axis of which only the 8x8x8 blocks near
// the observed surfaces are held.  mark() the depth maps, commit() (counts the blocks, allocates and clears the pool), integrate(),
// extract() / to_ply(); mark_clear() starts over.  Move-only.
class SparseTsdfVolume {
public:
    SparseTsdfVolume(const Context& ctx, const std::array<float, 3>& origin, float voxel_size, const std::array<uint32_t, 3>& dims, float trunc = 0.0f /*0: 4 voxels*/,
                     float max_weight = 64.0f, bool colour = true)
        : ctx_(&ctx), colour_(colour), v_(detail::tsdf_fields<BhSparseTsdf>(origin, voxel_size, dims, trunc, max_weight)) {
        for (uint32_t d : dims)
            if (d < 2 || d > BH_SPTSDF_MAX_DIM) throw Error(BH_ERR_INVALID_ARG, "SparseTsdfVolume: dimensions of 2 .. 8192");
        const uint64_t total = (uint64_t)((dims[0] + 7) / 8) * ((dims[1] + 7) / 8) * ((dims[2] + 7) / 8);
        n_words_ = (size_t)((total + 31) / 32);
        bits_.resize(n_words_);
        rank_.resize(n_words_);
        v_.bits = bits_.data();
        v_.rank = rank_.data();
        mark_clear();
    }
    SparseTsdfVolume(const SparseTsdfVolume&) = delete;
    SparseTsdfVolume& operator=(const SparseTsdfVolume&) = delete;
    SparseTsdfVolume(SparseTsdfVolume&&) noexcept = default;
    const BhSparseTsdf& vol() const { return v_; }
    uint32_t n_blocks() const { return v_.n_blocks; }
    size_t n_words() const { return n_words_; }
    std::vector<uint32_t> bits() const { ctx_->sync(); return bits_.download(); }
    std::vector<uint32_t> rank() const { ctx_->sync(); return rank_.download(); }
    std::vector<uint32_t> keys() const { ctx_->sync(); return keys_.download(); }
    std::vector<float> tw() const { ctx_->sync(); return tw_.download(); }     // [n_blocks,8,8,8,2] on the host
    std::vector<float> rgb() const { ctx_->sync(); return rgb_.download(); }   // [n_blocks,8,8,8,3] on the host (empty without colour)
    void set_bits(const std::vector<uint32_t>& host) {   // a block set computed elsewhere; commit(0) allocates exactly it
        if (host.size() != n_words_ || v_.n_blocks) throw Error(BH_ERR_INVALID_ARG, "SparseTsdfVolume::set_bits: n_words words, before the commit");
        ctx_->sync();
        hip_check(hipMemcpy(bits_.data(), host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy H2D");
    }
    void set_tw(const std::vector<float>& host) {   // a field computed elsewhere, [n_blocks,8,8,8,2]
        if (host.size() != (size_t)v_.n_blocks * 1024) throw Error(BH_ERR_INVALID_ARG, "SparseTsdfVolume::set_tw: a pool of another size");
        ctx_->sync();
        hip_check(hipMemcpy(tw_.data(), host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy H2D");
    }
    // forgets the marks and the pool
    void mark_clear() {
        ctx_->sync();
        v_.n_blocks = 0;
        v_.keys = nullptr; v_.tw = nullptr; v_.rgb = nullptr;
        keys_ = DeviceBuffer<uint32_t>(); tw_ = DeviceBuffer<float>(); rgb_ = DeviceBuffer<float>();
        ctx_->check(bh_sptsdf_mark_clear(ctx_->get(), &v_));
    }
    // depths[v] [H,W] and images[v] [H,W,4] (or an empty vector: no alpha test) are device pointers of cams[v]'s size
    void mark(const std::vector<BhCamera>& cams, const std::vector<const float*>& depths, const std::vector<const float*>& images = {}, float depth_max = INFINITY,
              float alpha_min = 0.5f) {
        detail::tsdf_check_views("SparseTsdfVolume::mark", cams, depths, images);
        if (v_.n_blocks) throw Error(BH_ERR_INVALID_ARG, "SparseTsdfVolume::mark: after a commit: mark_clear() first");
        const BhTsdfIntegrateConfig cfg{0.0f, depth_max, alpha_min, 0u};
        ctx_->check(bh_sptsdf_mark(ctx_->get(), &v_, (uint32_t)cams.size(), cams.data(), depths.data(), images.empty() ? nullptr : images.data(), &cfg));
    }
    // -> the number of blocks (0: nothing marked, no pool); blocking
    uint32_t commit(uint32_t dilate = 1) {
        if (v_.n_blocks) throw Error(BH_ERR_INVALID_ARG, "SparseTsdfVolume::commit: already committed: mark_clear() starts over");
        uint32_t n = 0;
        ctx_->check(bh_sptsdf_commit(ctx_->get(), &v_, dilate, &n));
        if (n == 0) return 0;
        keys_.resize(n);
        tw_.resize((size_t)n * 1024);
        if (colour_) rgb_.resize((size_t)n * 1536);
        v_.keys = keys_.data();
        v_.tw = tw_.data();
        v_.rgb = colour_ ? rgb_.data() : nullptr;
        v_.n_blocks = n;
        clear();
        return n;
    }
    void clear() { ctx_->check(bh_sptsdf_clear(ctx_->get(), &v_)); }
    void integrate(const std::vector<BhCamera>& cams, const std::vector<const float*>& depths, const std::vector<const float*>& images = {},
                   float depth_min = 0.0f, float depth_max = INFINITY, float alpha_min = 0.5f) {
        detail::tsdf_check_views("SparseTsdfVolume::integrate", cams, depths, images);
        const BhTsdfIntegrateConfig cfg{depth_min, depth_max, alpha_min, 0u};
        ctx_->check(bh_sptsdf_integrate(ctx_->get(), &v_, (uint32_t)cams.size(), cams.data(), depths.data(), images.empty() ? nullptr : images.data(), &cfg));
    }
    std::pair<uint32_t, uint32_t> count() const { return detail::tsdf_count(*ctx_, v_); }   // (vertices, triangles); blocking
    Mesh extract() const { return detail::tsdf_mesh(*ctx_, v_); }
    std::vector<uint8_t> to_ply() const { return detail::tsdf_to_ply(*ctx_, v_); }
    // the window of the virtual grid from sample `start`, of dense's size, into `dense` (bh_sptsdf_to_dense)
    void to_dense(const std::array<uint32_t, 3>& start, TsdfVolume& dense) const {
        ctx_->check(bh_sptsdf_to_dense(ctx_->get(), &v_, start[0], start[1], start[2], &dense.grid()));
    }

private:
    const Context* ctx_;
    bool colour_;
    size_t n_words_ = 0;
    BhSparseTsdf v_;
    DeviceBuffer<uint32_t> bits_, rank_, keys_;
    DeviceBuffer<float> tw_, rgb_;
};

// ---- depth supervision (brush_hip_depth_loss.h; not in the reference) --------------------------------------------------------------
// A target: gt [H,W] f32 on the device holds depth (BH_DEPTH_LOSS_L1) or inverse depth (BH_DEPTH_LOSS_DISPARITY); t = fma(scale, gt, offset).
inline BhDepthTarget depth_target(const float* gt, uint32_t h, uint32_t w, uint32_t kind = BH_DEPTH_LOSS_L1, float weight = 1.0f, float scale = 1.0f,
                                  float offset = 0.0f) {
    static_assert(BH_DEPTH_LOSS_L1 == 0u && BH_DEPTH_LOSS_DISPARITY == 1u, "depth loss kinds");
    BhDepthTarget t{};
    t.gt = gt; t.h = h; t.w = w; t.kind = kind; t.weight = weight; t.scale = scale; t.offset = offset;
    return t;
}
// loss [2] (device) = (weight * sum |.| / (H W), valid pixels), v_depth [H,W] or nullptr = dloss / d depth; nothing is read back
inline void depth_loss_value_and_grad(const Context& ctx, const float* depth, const BhDepthTarget& target, float* loss, float* v_depth) {
    ctx.check(bh_depth_loss_value_and_grad(ctx.get(), depth, &target, loss, v_depth));
}
// metrics [4] (device) = (abs-rel, RMSE, share of valid pixels within a ratio of 1.25, valid pixels)
inline void eval_depth_metrics(const Context& ctx, const float* depth, const BhDepthTarget& target, float* metrics) {
    ctx.check(bh_eval_depth_metrics(ctx.get(), depth, &target, metrics));
}
// bh_train_step on this ctx adds the depth term of `target` (copied; its gt must outlive the steps); nullptr detaches
inline void train_set_depth(const Context& ctx, const BhDepthTarget* target) { ctx.check(bh_train_set_depth(ctx.get(), target)); }

// ---- feature maps (brush_hip_features.h; not in the reference) ------------------------------------------------------------------------
// A target of the fused feature losses: f32 [H,W,C] on the device (BH_FEATURE_LOSS_L1) or uint8 labels [H,W] (BH_FEATURE_LOSS_CROSS_ENTROPY)
inline BhFeatureTarget feature_target(const void* target, uint32_t h, uint32_t w, uint32_t channels, uint32_t kind = BH_FEATURE_LOSS_L1, float weight = 1.0f) {
    static_assert(BH_FEATURE_LOSS_L1 == 0u && BH_FEATURE_LOSS_CROSS_ENTROPY == 1u && BH_FEATURE_MAX_CHANNELS == 256u, "feature loss kinds");
    BhFeatureTarget t{};
    t.target = target; t.h = h; t.w = w; t.channels = channels; t.kind = kind; t.weight = weight;
    return t;
}
// loss [2] (device) = (weight * the mean, valid pixels), v_map [H,W,C] or nullptr = dloss / d map; nothing is read back
inline void feature_loss_value_and_grad(const Context& ctx, const float* map, const BhFeatureTarget& target, float* loss, float* v_map) {
    ctx.check(bh_feature_loss_value_and_grad(ctx.get(), map, &target, loss, v_map));
}

// ---- normal maps (brush_hip_normal.h; not in the reference) ---------------------------------------------------------------------------
// the camera-space normal [N,3] of every splat: the axis of the smallest scale of the rendered (folded) transforms, facing the camera
inline DeviceBuffer<float> splat_normals(const Context& ctx, const Splats& splats, const Camera& camera) {
    static_assert(BH_NORMAL_ACCUMULATED == 0u && BH_NORMAL_UNIT == 1u, "normal modes");
    const BhCamera cam = camera.uniforms(16, 16);   // (the normals read the view matrix only)
    const detail::Folded f = detail::fold(ctx, splats);
    DeviceBuffer<float> out;
    out.resize((size_t)splats.num_splats() * 3);
    ctx.check(bh_splat_normals(ctx.get(), &cam, f.t, splats.num_splats(), out.data()));
    ctx.sync();   // the folded temporaries die with this scope
    return out;
}
// camera-space normals [H,W,3] of a z-depth map [H,W] on the device (pinhole cameras only), and the gradient of <v_normal, normals>
inline DeviceBuffer<float> depth_to_normal(const Context& ctx, const Camera& camera, const float* depth, uint32_t h, uint32_t w) {
    const BhCamera cam = camera.uniforms(w, h);
    DeviceBuffer<float> out;
    out.resize((size_t)h * w * 3);
    ctx.check(bh_depth_to_normal(ctx.get(), &cam, depth, h, w, out.data()));
    ctx.sync();
    return out;
}
inline DeviceBuffer<float> depth_to_normal_backward(const Context& ctx, const Camera& camera, const float* depth, const float* v_normal, uint32_t h,
                                                    uint32_t w) {
    const BhCamera cam = camera.uniforms(w, h);
    DeviceBuffer<float> out;
    out.resize((size_t)h * w);
    ctx.check(bh_depth_to_normal_backward(ctx.get(), &cam, depth, v_normal, h, w, out.data()));
    ctx.sync();
    return out;
}

// ---- normal consistency (brush_hip_normal_loss.h; not in the reference) ---------------------------------------------------------------
// loss [2] (device) = (weight * sum A (1 - N . u) / (H W), valid pixels), v_normal [H,W,3], v_depth [H,W] (accumulate_v_depth: added
// to); normal = an accumulated normal map, depth = the expected depth, image = the frame [H,W,4] (its alpha, a constant); nothing is read back
inline void normal_consistency_value_and_grad(const Context& ctx, const Camera& camera, const float* normal, const float* depth, const float* image,
                                              uint32_t h, uint32_t w, float weight, bool accumulate_v_depth, float* loss, float* v_normal, float* v_depth) {
    static_assert(sizeof(BhNormalTermConfig) == 16, "BhNormalTermConfig layout");
    const BhCamera cam = camera.uniforms(w, h);
    ctx.check(bh_normal_consistency_value_and_grad(ctx.get(), &cam, normal, depth, image, h, w, weight, accumulate_v_depth ? 1u : 0u, loss, v_normal, v_depth));
}
// bh_train_step on this ctx adds the normal-consistency term at `weight` (<= 0: no term); nullptr detaches
inline void train_set_normal(const Context& ctx, const BhNormalTermConfig* cfg) { ctx.check(bh_train_set_normal(ctx.get(), cfg)); }
inline void train_set_normal(const Context& ctx, float weight) {
    BhNormalTermConfig cfg{};
    cfg.weight = weight;
    train_set_normal(ctx, &cfg);
}

// ---- distortion (brush_hip_distortion.h; not in the reference) -------------------------------------------------------------------------
// loss [2] (device) = (weight * sum(dist) / (H W), pixels) of a distortion map (channels 1) or a moment map (channels 4); nothing is read back
inline void distortion_loss(const Context& ctx, const float* map, uint32_t h, uint32_t w, uint32_t channels, float weight, float* loss) {
    ctx.check(bh_distortion_loss(ctx.get(), map, h, w, channels, weight, loss));
}
// bh_train_step on this ctx adds the distortion term (weight <= 0: no term); nullptr detaches
inline void train_set_distortion(const Context& ctx, const BhDistortionTermConfig* cfg) {
    static_assert(sizeof(BhDistortionTermConfig) == 16, "BhDistortionTermConfig layout");
    ctx.check(bh_train_set_distortion(ctx.get(), cfg));
}
inline void train_set_distortion(const Context& ctx, float weight, uint32_t kind = BH_DISTORTION_Z, float near_z = 0.2f, float far_z = 1000.0f) {
    BhDistortionTermConfig cfg{};
    cfg.weight = weight;
    cfg.kind = kind;
    cfg.near_z = near_z;
    cfg.far_z = far_z;
    train_set_distortion(ctx, &cfg);
}

// ---- point-cloud initialisation (brush-train/src/splat_init.rs:179-242; train_stream.rs:100-123) ---------------------------------
// compute_knn_scales in place: columns 7..9 of splats.transforms = ln(clamp((d1 + d2) / 4, 1e-3, 0.1 median_size)) (bh_knn_log_scales).
// nn_dist (optional): resized to [N,2], d1 and d2 per splat.  Returns the number of distance evaluations performed.
inline uint64_t knn_log_scales(const Context& ctx, Splats& splats, DeviceBuffer<float>* nn_dist = nullptr) {
    const uint32_t n = splats.num_splats();
    if (nn_dist) nn_dist->resize((size_t)n * 2);
    uint64_t pairs = 0;
    ctx.check(bh_knn_log_scales(ctx.get(), splats.transforms.data(), n, nn_dist ? nn_dist->data() : nullptr, &pairs));
    return pairs;
}
// to_init_splats (splat_init.rs:218-242) from host arrays: means [N,3]; every other argument may be empty and then takes the
// reference's default — rotation (1,0,0,0), log-scales by compute_knn_scales, SH one grey coefficient 0.5, raw opacity 0.
inline Splats to_init_splats(const Context& ctx, const std::vector<float>& means, const std::vector<float>& rotations = {},
                             const std::vector<float>& log_scales = {}, const std::vector<float>& sh_coeffs = {},
                             const std::vector<float>& raw_opacities = {}, bool render_mip = false) {
    const size_t n = means.size() / 3;
    if (means.size() != n * 3 || (!rotations.empty() && rotations.size() != n * 4) || (!log_scales.empty() && log_scales.size() != n * 3) ||
        (!raw_opacities.empty() && raw_opacities.size() != n) || (!sh_coeffs.empty() && (n == 0 || sh_coeffs.size() % (3 * n) != 0)))
        throw Error(BH_ERR_INVALID_ARG, "to_init_splats: means [N,3], rotations [N,4], log_scales [N,3], sh_coeffs [N,C,3], raw_opacities [N]");
    std::vector<float> tr(n * 10);
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) tr[i * 10 + k] = means[i * 3 + k];
        for (int k = 0; k < 4; ++k) tr[i * 10 + 3 + k] = rotations.empty() ? (k == 0 ? 1.0f : 0.0f) : rotations[i * 4 + k];
        for (int k = 0; k < 3; ++k) tr[i * 10 + 7 + k] = log_scales.empty() ? 0.0f : log_scales[i * 3 + k];
    }
    Splats s = Splats::from_host(tr, sh_coeffs.empty() ? std::vector<float>(n * 3, 0.5f) : sh_coeffs,
                                 raw_opacities.empty() ? std::vector<float>(n, 0.0f) : raw_opacities, render_mip);
    if (log_scales.empty()) knn_log_scales(ctx, s);
    return s;
}
// the init point cloud of the training stream (train_stream.rs:100-123): load_splat_from_ply with subsampling, then
// compute_knn_scales over the kept rows when the file has no scale_0 (import.rs:332)
inline std::pair<Splats, BhPlyInfo> load_init_splats(const Context& ctx, const std::vector<uint8_t>& bytes, uint32_t subsample_points = 1,
                                                     size_t max_splats = 0) {
    auto loaded = load_splat_from_ply(ctx, bytes, subsample_points, max_splats);
    const int has = bh_ply_vertex_has_property(bytes.data(), bytes.size(), "scale_0");
    if (has < 0) throw Error(has, "malformed PLY");
    if (has == 0) knn_log_scales(ctx, loaded.first);
    return loaded;
}

}  // namespace brush_hip
