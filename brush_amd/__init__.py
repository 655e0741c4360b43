"""brush_amd — host-side mirror (Python) of the Brush operator surface for the
splat-rasterizer hot path, above the C ABI of libbrush_hip.so.

Names and argument meaning follow the reference (paths under
/root/reference/crates/):
    Camera            brush-render/src/camera.rs:12-19 (camera_model: kernels/camera_model/mod.rs:31-38)
    fov_to_focal / focal_to_fov   brush-render/src/camera.rs:85-118
    Splats            brush-render/src/gaussian_splats.rs:62-74
    RasterPass        brush-render/src/gaussian_splats.rs:28-48
    render_splats     brush-render/src/gaussian_splats.rs:365-446 (forward / eval)
    render_splats_bwd brush-render/src/bwd/burn_glue.rs:223-311 (+ RenderBackwards::backward :121-182)
    render_splats_diff / RenderNode   the same as an autodiff node: forward now, backward later from its SAVED state (burn_glue.rs:336-371)
    render_depth / RenderNode.depth   accumulated, expected or median depth map of a node; RenderNode.backward(v_depth=) differentiates it
                                      (include/brush_hip_depth.h)
    radix_argsort     brush-sort/src/lib.rs:16
    tile_sort_offsets render.rs:228-243 + get_tile_offset.rs:11-58 (the forward's tile sort and offsets table, one operator)
    prefix_sum        brush-prefix-sum/src/lib.rs:11
    image_loss        brush-loss/src/lib.rs:1075-1104
    splat_to_ply / load_splat_from_ply   brush-serde/src/export.rs:179-204, import.rs:166-330 (plain PLY)
    splat_to_compressed_ply               the SuperSplat compressed.ply the reader of import.rs:407-600 takes
    BatchUploader / SceneLoader          brush-dataset/src/scene.rs:97-136, scene_loader.rs:59-174
    SplatTrainer      brush-train/src/train.rs:140-429 (step) and :431-893 (refine)
    compute_pup_scores / decimate_to_count   brush-train/src/lod.rs:13-142 (LOD boundary, brush-process/src/train_stream.rs:248-303)
    knn_log_scales / to_init_splats / load_init_splats   brush-train/src/splat_init.rs:179-242 (compute_knn_scales, to_init_splats),
                                         brush-process/src/train_stream.rs:100-123 (the init point cloud)
    eval_metrics / eval_stats / run_eval   brush-train/src/eval.rs:23-63 (PSNR / SSIM of held-out views),
                                         brush-process/src/train_stream.rs:506-566 (run_eval)
    Lpips / lpips / lpips_value_and_grad   crates/lpips/src/lib.rs (LpipsModel), brush-train/src/train.rs:265-273 (lpips_loss_weight)
    view_output_size / resize_image / BatchUploader.submit_view   brush-dataset/src/load_image.rs:60-131 (mask merge and
                                         image::imageops::resize of LoadImage::load)
    RenderNode.backward(pose=True) / pose_twist / Camera.apply_twist / PoseOptimizer   camera pose gradients and their host
                                         optimizer (not in the reference; gsplat's v_viewmats)
    RenderNode.backward(intrinsics=True) / Camera.with_intrinsics / IntrinsicsOptimizer   camera intrinsics gradients (focal,
                                         principal point) and their per-sensor host optimizer
    ExposureTable / SplatTrainer(exposure=)   per-view exposure compensation: an affine colour transform per training view with
                                         Adam on the device (not in the reference; the INRIA trainer's exposure)
    depth_loss_value_and_grad / eval_depth_metrics / SceneBatch(depth=) / TrainConfig.depth_loss_weight   depth supervision: a fused
                                         depth loss, a depth term in the step, held-out depth metrics (not in the reference; the INRIA
                                         trainer's depth regularisation, gsplat's depth_loss)
    splat_normals / render_normal / RenderNode.normal / RenderNode.backward(v_normal=) / depth_to_normal / depth_to_normal_backward
                                         rendered and depth-derived normal maps with their gradients (not in the reference; the maps
                                         2DGS / gsplat compare for normal consistency; include/brush_hip_normal.h)
    normal_consistency_value_and_grad / TrainConfig.normal_loss_weight   the normal-consistency regulariser those maps exist for: a
                                         fused loss with both gradients and a term in the step (not in the reference; 2DGS's
                                         normal loss; include/brush_hip_normal_loss.h)
    render_distortion / RenderNode.distortion / RenderNode.backward(v_distortion=) / distortion_loss / TrainConfig.distortion_loss_weight
                                         distortion maps with their gradient, the loss and a term in the step (not in the reference;
                                         2DGS's depth distortion; include/brush_hip_distortion.h)
    BilateralGridTable / SplatTrainer(bilagrid=)   per-view bilateral grids: a grid of affine colour transforms per training view, sliced
                                         at (x, y, luminance) before the loss, with a total-variation term and Adam on the device (not in
                                         the reference; gsplat's lib_bilagrid; include/brush_hip_bilagrid.h)
    TsdfVolume / fuse_views / mesh_to_ply    mesh extraction: rendered depth maps fused into a TSDF volume (8 views per pass over the
                                         volume), its zero level set by marching tetrahedra, a triangle-mesh PLY (not in the
                                         reference; include/brush_hip_mesh.h)
    SparseTsdfVolume                     the same fusion and mesh on 8x8x8 blocks allocated only near the observed surfaces: virtual
                                         grids of up to 8192 samples per axis (include/brush_hip_sparse_mesh.h)
    render_features / RenderNode.features / RenderNode.backward(v_features=, features=) / feature_loss_value_and_grad / FeatureField
                                         feature maps: caller-owned per-splat vectors of 1 .. 256 channels blended with the colour
                                         blend's weights, the gradient into them and the splats, fused L1 / cross-entropy losses (not
                                         in the reference; gsplat's colors [N, D]; include/brush_hip_features.h)
    SplatTrainer(feature_field=) / SceneBatch.features / TrainConfig.feature_loss_weight / FeatureField.carry / .gather
                                         feature fields trained jointly with the splats: the feature term inside the step, the
                                         field's Adam update on the device, its rows carried through refine (not in the reference;
                                         Feature-3DGS, Gaussian Grouping; include/brush_hip_feature_train.h)
    SceneTransform / Splats.transformed / .transform_ / Camera.transformed / SceneRegion / select_region / crop_splats
                                         scene editing: a similarity transform of a scene with the rotation of its SH bands, the
                                         same transform of a camera, a box / ellipsoid / opacity crop (not in the reference;
                                         include/brush_hip_scene.h)
    LiftAccumulator / lift_labels / compact_splats
                                         mask lifting: per-splat blend-weight votes from 2-D label maps over any number of views, the
                                         largest weight and the pixel count of each splat, argmax / threshold, compaction (not in
                                         the reference; SAGA, Gaussian Grouping, FlashSplat; include/brush_hip_lift.h)
    EnvironmentMap / SplatTrainer(envmap=) / run_eval(envmap=)
                                         environment maps: a learned cubemap behind the splats (sky, skyline, a bright window),
                                         composited behind the frame before the loss, with an exact integer gradient and Adam on the
                                         device (not in the reference; splatfacto-w's and Street Gaussians' sky, gsplat's
                                         backgrounds; include/brush_hip_envmap.h)

torch is used only for device memory, streams and torch.distributed; every
computation runs in the hand-written HIP kernels. No CPU fallback exists.
"""
from .host import (  # noqa: F401
    Camera, Context, RasterPass, RenderAux, SplatTrainer, Splats, TrainConfig, SceneBatch,
    get_context, image_loss, image_loss_backward, image_loss_value_and_grad, prefix_sum, radix_argsort, tile_sort_offsets, render_splats,
    render_splats_bwd, adam_step, gather_stats, RefineStats, splat_bounds, bounds_median_size, fov_to_focal, focal_to_fov,
    splat_to_ply, load_splat_from_ply, ply_parse_header, ParseMetadata, BatchUploader, SceneLoader, set_list_slicing, last_list_counts, set_view_id,
    render_splats_diff, RenderNode, compute_pup_scores, decimate_to_count, lod_target_count, pup_accumulate, pup_accumulate_view, pup_scores,
    knn_log_scales, to_init_splats, load_init_splats, ply_vertex_has_property, EvalSample, EvalResult, eval_metrics, eval_stats, run_eval,
    Lpips, lpips, lpips_value_and_grad, splat_to_compressed_ply, view_output_size, resize_image, render_depth,
    PoseOptimizer, pose_twist, IntrinsicsOptimizer, ExposureTable, depth_loss_value_and_grad, eval_depth_metrics,
    splat_normals, render_normal, depth_to_normal, depth_to_normal_backward, normal_consistency_value_and_grad,
    render_distortion, distortion_loss, BilateralGridTable,
    TsdfVolume, SparseTsdfVolume, mesh_to_ply, fuse_views,
    render_features, feature_loss_value_and_grad, FeatureField,
    SceneTransform, SceneRegion, select_region, crop_splats,
    LiftAccumulator, lift_labels, compact_splats,
    EnvironmentMap,
)
from ._ffi import BrushHipError  # noqa: F401
