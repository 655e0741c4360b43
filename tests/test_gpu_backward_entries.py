"""The refusal sequence of the six backward entry points, one table (include/brush_hip.h, brush_hip_pose.h, brush_hip_depth.h,
brush_hip_normal.h, brush_hip_distortion.h): return code and message of every refusal an entry makes, in the order it makes them.

Every step is called with the violations of all LATER steps present as well where they can coexist (a null pointer together with
bad modes, a bad mode on a forward-only frame, a forward-only or stale frame with null transforms), so a refusal that moved in
front of an earlier one would change the message this table expects.  The order, per entry:

    null ctx | null argument | distortion kind, normal mode, median depth, depth mode | not a BH_FLAG_BWD_INFO forward | stale forward
    | null transforms (normal and distortion entries only) | accepted

bh_render_backward is the odd one: it has no BhRenderOut, refuses a context without a BH_FLAG_BWD_INFO forward BEFORE its null
arguments, and cannot be stale.  The plain and pose entries answer BH_ERR_STATE for a forward-only frame, the three map entries
BH_ERR_INVALID_ARG.  A mode that belongs to an absent optional cotangent is not looked at.

32 x 32 pixels, 16 splats, SH degree 0."""
import ctypes as C
import math

import pytest
import torch

from brush_amd import synth

pytestmark = pytest.mark.gpu
INVALID_ARG, STATE = -1, -4
W = H = 32

# entry -> (the C arguments behind ctx in order, the ones that may not be NULL, the code of "not a BH_FLAG_BWD_INFO forward",
#           does it refuse null transforms)
OUTS = ("v_transforms", "v_sh_coeffs", "v_raw_opacities", "v_refine_weight")
PARAMS = ("transforms", "sh_coeffs", "raw_opacities")
ENTRIES = {
    "render_backward": (("v_output",) + PARAMS + OUTS, ("v_output",) + OUTS, STATE, False),
    "render_backward_saved": (("saved", "v_output") + PARAMS + OUTS, ("saved", "v_output") + OUTS, STATE, False),
    "render_backward_pose_saved": (("saved", "v_output") + PARAMS + OUTS + ("v_viewmat",), ("saved", "v_output") + OUTS + ("v_viewmat",), STATE, False),
    "render_backward_depth_saved": (("saved", "v_output", "v_depth", "depth_mode") + PARAMS + OUTS, ("saved", "v_depth") + OUTS, INVALID_ARG, False),
    "render_backward_normal_saved": (("saved", "v_output", "v_depth", "depth_mode", "v_normal", "normal_mode") + PARAMS + OUTS,
                                     ("saved", "v_normal") + OUTS, INVALID_ARG, True),
    "render_backward_distortion_saved": (("saved", "v_output", "v_depth", "depth_mode", "v_normal", "normal_mode", "v_distortion", "cfg") + PARAMS + OUTS,
                                         ("saved", "v_distortion", "cfg") + OUTS, INVALID_ARG, True),
}
MEDIAN, BAD = 2, 7   # BH_DEPTH_MEDIAN; no depth mode, normal mode or distortion kind


@pytest.mark.parametrize("who", list(ENTRIES))
def test_refusal_sequence(dev, who):
    import brush_amd as ba
    from brush_amd import _ffi, host
    names, required, not_bwd_code, refuses_null_transforms = ENTRIES[who]
    sc = synth.make_scene(16, 0xBE, sh_degree=0, log_scale_range=(math.log(0.05), math.log(0.4)), z_range=(2.0, 6.0))
    cp = synth.default_camera_params(W, H)
    cam = ba.Camera(position=cp["pos"], rotation=cp["rot_xyzw"], fov_x=cp["fov_x"], fov_y=cp["fov_y"], center_uv=cp["center_uv"])
    spl = ba.Splats(sc["transforms"], sc["sh"], sc["raw_opac"], device=dev)
    ctx = ba.Context(dev)
    try:
        lib, fn = ctx.lib, getattr(ctx.lib, "bh_" + who)
        node = ba.render_splats_diff(spl, cam, (W, H), ctx=ctx)
        r_t, r_o = node._folded
        keep = dict(v_output=torch.zeros((H, W, 4), device=dev), v_depth=torch.zeros((H, W), device=dev), v_normal=torch.zeros((H, W, 3), device=dev),
                    v_distortion=torch.zeros((H, W), device=dev), transforms=r_t, sh_coeffs=spl.sh_coeffs, raw_opacities=r_o,
                    v_transforms=torch.empty((16, 10), device=dev), v_sh_coeffs=torch.empty((16, 1, 3), device=dev),
                    v_raw_opacities=torch.empty((16,), device=dev), v_refine_weight=torch.empty((16,), device=dev), v_viewmat=torch.empty((12,), device=dev))
        good = {k: C.c_void_p(t.data_ptr()) for k, t in keep.items()}
        good.update(saved=C.byref(node.out), depth_mode=1, normal_mode=0, cfg=C.byref(_ffi.BhDistortionConfig(kind=0)))

        def call(handle=ctx._h, **over):
            assert set(over) <= set(good)
            args = dict(good, **over)
            return fn(handle, *[args[k] for k in names])

        def refused(rc, code, *texts):
            msg = lib.bh_last_error(ctx._h).decode()
            assert rc == code, (rc, msg)
            for t in texts:
                assert t in msg, msg

        has = lambda k: k in names   # noqa: E731
        bad_modes = {k: BAD for k in ("depth_mode", "normal_mode") if has(k)}
        if has("cfg"):
            bad_modes["cfg"] = C.byref(_ffi.BhDistortionConfig(kind=BAD))

        # ---- on the ctx's own BH_FLAG_BWD_INFO forward: null transforms (behind the lookup), then a call that is accepted
        if refuses_null_transforms:
            refused(call(transforms=None), INVALID_ARG, who + ": null transforms")
        # (a mode is looked at only with its cotangent: the optional ones are absent here)
        absent = {k: None for k in ("v_depth", "v_normal") if has(k) and k not in required}
        absent.update({m: BAD for k, m in (("v_depth", "depth_mode"), ("v_normal", "normal_mode")) if k in absent})
        assert call(**absent) == 0, lib.bh_last_error(ctx._h).decode()
        assert call() == 0, lib.bh_last_error(ctx._h).decode()
        ctx.sync()

        # ---- a forward-only frame is the ctx's forward now, and `node` is stale
        _, fwd_only, _ = host._forward(ctx, spl, cam, (W, H), (0, 0, 0), ba.RasterPass.Forward)
        later = dict(bad_modes, transforms=None)
        if has("saved"):
            later["saved"] = C.byref(fwd_only)

        assert call(handle=None) == INVALID_ARG
        if not has("saved"):   # bh_render_backward: the state of the ctx first, then its arguments (checked on a new BWD_INFO forward below)
            for over in ({}, {"v_output": None}):
                refused(call(**over), STATE, "render_backward needs a preceding BH_FLAG_BWD_INFO forward on this context")
        else:
            for k in required:
                refused(call(**dict(later, **{k: None})), INVALID_ARG, who + ": null argument")
            # distortion kind, normal mode, median depth, depth mode: each in front of the ones behind it
            if has("cfg"):
                refused(call(**later), INVALID_ARG, who + ": unknown distortion kind")
                for near, far in ((0.0, 10.0), (2.0, 2.0), (float("nan"), 10.0)):
                    ndc = C.byref(_ffi.BhDistortionConfig(kind=1, near_z=near, far_z=far))
                    refused(call(**dict(later, cfg=ndc)), INVALID_ARG, who + ": BH_DISTORTION_NDC needs 0 < near < far")
                later["cfg"] = good["cfg"]
            if has("normal_mode"):
                refused(call(**dict(later, depth_mode=MEDIAN)), INVALID_ARG, who + ": unknown normal mode")
                later["normal_mode"] = 0
            if has("depth_mode"):
                refused(call(**dict(later, depth_mode=MEDIAN)), INVALID_ARG, who + ": median depth has no gradient")
                refused(call(**later), INVALID_ARG, who + ": unknown depth mode")
                later["depth_mode"] = 1
            # every other pointer is valid-looking (then all but the transforms): refused before any of them is read
            for over in ({"saved": later["saved"]}, later):
                refused(call(**over), not_bwd_code, who + ": the saved forward was not a BH_FLAG_BWD_INFO forward")
            refused(call(**dict(later, saved=C.byref(node.out))), STATE, who + ": forward #%d is stale" % node.out.generation, "bh_render_retain")

        # ---- bh_render_backward's null arguments, behind its state check
        if not has("saved"):
            node = ba.render_splats_diff(spl, cam, (W, H), ctx=ctx)
            for k in required:
                refused(call(**{k: None, "transforms": None}), INVALID_ARG, who + ": null argument")
            assert call() == 0, lib.bh_last_error(ctx._h).decode()
        ctx.sync()
    finally:
        ctx.close()
