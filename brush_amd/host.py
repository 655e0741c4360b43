"""Host-side mirror of the Brush operator surface over libbrush_hip.so.

See brush_amd/__init__.py for the reference citations. Every function here is
plumbing around one C-ABI call; tensors are torch CUDA(HIP) tensors used purely
as device memory.
"""
import ctypes as C
import enum
import math
import os
from contextlib import contextmanager
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch

from . import _ffi
from ._ffi import BrushHipError
from .parallel import (DIRECT_ALLREDUCE_MIN_FLOATS, allreduce_direct, allreduce_exchange, allreduce_refine_maxima, allgather_strips, exchange_strip_halos, strip_spans_px,
                       strips_allow_halo_loss, tile_rows_for_rank)


# ---------------------------------------------------------------------------
# context
# ---------------------------------------------------------------------------
# The library reads no environment variable (bh_set_option is its one configuration entry point).  THIS harness — the test suite,
# bench.py, scripts/ab.sh — still lets a developer pick an A/B path from the shell: BH_OPTIONS="key=value,key=value", and the
# variable names earlier rounds' scripts use, translated here into options of every Context this process creates.
_LEGACY_ENV_OPTIONS = (   # (environment variable, option key, value or None = the variable's own value)
    ("BH_NO_LPT", "no_lpt", "1"), ("BH_GENERIC_DEPTH_SORT", "generic_depth_sort", "1"), ("BH_FORCE_PG", "force_exchange", "1"),
    ("BH_TRAIN_ZERO_GRADS", "zero_grads", "1"), ("BH_CUT_MIN_PAIRS", "cut_min_pairs", None), ("BH_CUT_SORT_ALL", "cut_sort_all", "1"),
    ("BH_NO_VIEW_HASH", "no_view_hash", "1"), ("BH_CUT_MARGIN_FIXED", "cut_margin_fixed", "1"), ("BH_CUT_CTRL", "cut_ctrl", None),
    ("BH_READBACK_COPY", "readback_copy", "1"), ("BH_EVENT_WAITS", "event_waits", "1"), ("BH_K16_ORDER", "k16_order", None),
    ("BH_CUT_MARGIN_PCT", "cut_margin_pct", None), ("BH_UPDATE_NO_DORMANT", "no_dormant", "1"),
    ("BH_K5_EXACT_SPW", "k5_exact_spw", None), ("BH_TILE_SORT_LSD", "tile_sort", "lsd"), ("BH_LOSS_BANDS", "loss_bands", None),
    ("BH_UPDATE_ROWS", "update_rows", None), ("BH_SORT_KPT", "sort_kpt", None),
)


def options_from_environment(env=None):
    """[(key, value)] a developer asked for through the shell (see above); applied by Context.__init__."""
    env = os.environ if env is None else env
    out = []
    for var, key, val in _LEGACY_ENV_OPTIONS:
        if var in env:
            out.append((key, env[var] if val is None else val))
    for item in filter(None, (x.strip() for x in env.get("BH_OPTIONS", "").split(","))):
        k, _, v = item.partition("=")
        out.append((k.strip(), v.strip()))
    return out


class Context:
    """One bh_ctx: a HIP stream + scratch arena. Single-threaded by contract
    (brush-async/src/lib.rs:1-17); make one per thread / per GPU."""

    def __init__(self, device=None, use_torch_stream=True, lib=None, options=None):
        # lib: tests only — the fault-injection build (_ffi.load_test_hooks()); everything a Context does goes through self.lib
        self.lib = lib if lib is not None else _ffi.load()
        if not torch.cuda.is_available():
            raise BrushHipError("no HIP device visible: brush_amd has no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0)
        # submit on torch's current stream (handle 0 = the default stream) so tensor ops
        # and brush_hip kernels are ordered without extra synchronisation
        stream = torch.cuda.current_stream(self.device).cuda_stream if use_torch_stream else 0
        # own stream (hipStreamNonBlocking): NOT ordered against torch's streams — the caller synchronises hand-overs
        # (what a viewer / trainer pair on separate threads wants, brush-async/src/lib.rs:4-17)
        self.uses_torch_stream = bool(use_torch_stream)
        self._h = self.lib.bh_create(self.device.index, C.c_void_p(stream), 0 if use_torch_stream else 1)
        if not self._h:
            raise BrushHipError("bh_create failed on %s" % self.device)
        self._h = C.c_void_p(self._h)
        for k, v in options_from_environment() + list((options or {}).items()):
            self.set_option(k, v)

    def set_option(self, key, value):
        """bh_set_option: select one of the library's alternative paths (same results; A/B measurements and their tests)."""
        self.check(self.lib.bh_set_option(self._h, str(key).encode(), str(value).encode()))

    def options(self):
        """{key: help} of every option this build knows (bh_option_name / bh_option_help)."""
        return {self.lib.bh_option_name(i).decode(): self.lib.bh_option_help(i).decode() for i in range(self.lib.bh_option_count())}

    def close(self):
        if getattr(self, "_h", None):
            self.lib.bh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != 0:
            raise BrushHipError("brush_hip error %d: %s" % (rc, self.lib.bh_last_error(self._h).decode()))

    def sync(self):
        self.check(self.lib.bh_sync(self._h))

    # ---- RCCL inside the library (bh_comm_*): for hosts without torch.distributed ----
    @staticmethod
    def comm_unique_id() -> bytes:
        """ncclGetUniqueId: call on rank 0, hand the 128 bytes to every rank (file, socket, TCPStore ...)."""
        buf = (C.c_char * 128)()
        rc = _ffi.load().bh_comm_unique_id(buf)
        if rc != 0:
            raise BrushHipError("bh_comm_unique_id failed (%d): RCCL not loadable" % rc)
        return bytes(buf)

    def comm_init(self, rank, world, unique_id: bytes):
        self.check(self.lib.bh_comm_init(self._h, int(rank), int(world), unique_id))

    def comm_destroy(self):
        self.check(self.lib.bh_comm_destroy(self._h))

    def comm_world(self):
        return int(self.lib.bh_comm_world(self._h))

    def comm_rank(self):
        return int(self.lib.bh_comm_rank(self._h))

    def comm_selftest(self):
        """bh_comm_selftest: every RCCL entry point the library binds, on rank-dependent patterns, checked on the host (collective)."""
        self.check(self.lib.bh_comm_selftest(self._h))

    def allreduce_sum(self, t: torch.Tensor):
        """In place, asynchronous on the ctx stream; t: contiguous float32 device tensor."""
        self.check(self.lib.bh_allreduce_sum_f32(self._h, _ptr(t), t.numel()))

    def allreduce_max(self, t: torch.Tensor):
        self.check(self.lib.bh_allreduce_max_f32(self._h, _ptr(t), t.numel()))

    def allgather_bytes(self, send: torch.Tensor, recv: torch.Tensor):
        """bh_allgather_bytes: every rank's `send` (contiguous, any dtype) lands in `recv` (world x the same bytes) in rank order."""
        nbytes = send.numel() * send.element_size()
        if recv.numel() * recv.element_size() != nbytes * self.comm_world():
            raise ValueError("recv must hold world x the bytes of send")
        self.check(self.lib.bh_allgather_bytes(self._h, _ptr(send), _ptr(recv), nbytes))

    def exchange_strip_halos(self, img_hwc4: torch.Tensor, row_begin_px: int, row_end_px: int):
        """bh_exchange_strip_halos: one frame split into strips of tile rows — fetch the 21 pixel rows above and below this rank's strip
        [row_begin_px, row_end_px) of the [H,W,4] f32 image from the neighbouring ranks, in place on the ctx stream."""
        h, w, c = img_hwc4.shape
        if c != 4:
            raise ValueError("img must be [H,W,4]")
        self.check(self.lib.bh_exchange_strip_halos(self._h, _ptr(img_hwc4), h, w, int(row_begin_px), int(row_end_px)))

    @staticmethod
    def strip_halo_plan(img_h, row_begin_px, row_end_px, rank, world):
        """The host arithmetic behind exchange_strip_halos (bh_strip_halo_plan): [(send, peer, first row, rows)], at most four."""
        ops = (_ffi.BhHaloOp * 4)()
        k = _ffi.load().bh_strip_halo_plan(int(img_h), int(row_begin_px), int(row_end_px), int(rank), int(world), ops)
        if k < 0:
            raise BrushHipError("strip_halo_plan: bad strip (%d)" % k)
        return [(bool(ops[i].send), int(ops[i].peer), int(ops[i].row_begin_px), int(ops[i].rows)) for i in range(k)]

    def set_list_cut_threshold(self, min_pairs: int):
        """bh_set_list_cut_threshold: frames with fewer intersections than this keep complete lists (default 1.5 M)."""
        self.check(self.lib.bh_set_list_cut_threshold(self._h, int(min_pairs)))

    def view_table_count(self):
        """bh_view_table_count: per-view tables the ctx holds (diagnostics)."""
        return int(self.lib.bh_view_table_count(self._h))

    def forget_views(self):
        """bh_forget_views: drop the per-view tile tables (after loading another scene)."""
        self.check(self.lib.bh_forget_views(self._h))

    def profile(self, on=True):
        """True/1: HIP events around every stage; 2: only around the dominant kernel; False/0: off."""
        self.check(self.lib.bh_profile_enable(self._h, int(on)))

    def profile_fetch(self):
        """{stage: (total_ms, calls)} accumulated since the last fetch."""
        cap = 32
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        calls = (C.c_uint32 * cap)()
        n = self.lib.bh_profile_fetch(self._h, names, ms, calls, cap)
        return {names[i].decode(): (ms[i], calls[i]) for i in range(n)}


_CONTEXTS = {}


def get_context(device=None) -> Context:
    if not torch.cuda.is_available():
        raise BrushHipError("no HIP device visible: brush_amd has no CPU path")
    idx = torch.cuda.current_device() if device is None else (torch.device(device).index or 0)
    if idx not in _CONTEXTS:
        _CONTEXTS[idx] = Context(torch.device("cuda", idx))
    return _CONTEXTS[idx]


class _DevArray:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def _view(ptr, shape, dtype, device):
    """Zero-copy torch view of ctx-owned device memory (valid until the next forward)."""
    n = 1
    for s in shape:
        n *= s
    if n == 0 or not ptr:
        return torch.empty(shape, dtype=dtype, device=device)
    typestr = {torch.float32: "<f4", torch.int32: "<i4", torch.uint8: "|u1"}[dtype]
    return torch.as_tensor(_DevArray(ptr, shape, typestr), device=device)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else C.c_void_p(t.data_ptr() if t is not None else 0)


def _f32c(t, device):
    t = torch.as_tensor(t, dtype=torch.float32, device=device)
    return t.contiguous()  # render.rs:57-59 into_contiguous


# ---------------------------------------------------------------------------
# Camera (brush-render/src/camera.rs)
# ---------------------------------------------------------------------------
def _model_and_dist(camera_model, dist):
    c = Camera(camera_model=camera_model, dist=tuple(dist or ()))
    return c.model_id(), c._dist8()


def fov_to_focal(fov, pixels, camera_model="pinhole", dist=None):
    """camera.rs:85-101 (f64): focal such that pixels/2 = focal * lens_law(fov/2)."""
    m, d = _model_and_dist(camera_model, dist)
    return _ffi.load().bh_fov_to_focal(float(fov), int(pixels), m, d)


def focal_to_fov(focal, pixels, camera_model="pinhole", dist=None):
    """camera.rs:104-118 (f64)."""
    m, d = _model_and_dist(camera_model, dist)
    return _ffi.load().bh_focal_to_fov(float(focal), int(pixels), m, d)


@dataclass
class Camera:
    position: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    rotation: Tuple[float, float, float, float] = (0.0, 0.0, 0.0, 1.0)  # glam order x, y, z, w
    fov_x: float = 1.0
    fov_y: float = 1.0
    center_uv: Tuple[float, float] = (0.5, 0.5)
    # CameraModel (kernels/camera_model/mod.rs:31-38): "pinhole" | "kb4" | "rt8" | "tpf" (or the BH_CAMERA_* id)
    # with its distortion parameters in the reference's struct order (see include/brush_hip.h)
    camera_model: object = "pinhole"
    dist: Tuple[float, ...] = ()

    def model_id(self):
        ids = {"pinhole": _ffi.CAMERA_PINHOLE, "kb4": _ffi.CAMERA_KANNALA_BRANDT_4, "rt8": _ffi.CAMERA_RADIAL_TANGENTIAL_8,
               "tpf": _ffi.CAMERA_THIN_PRISM_FISHEYE}
        return ids[self.camera_model] if isinstance(self.camera_model, str) else int(self.camera_model)

    def _dist8(self):
        d = (C.c_float * 8)()
        for i, v in enumerate(self.dist):
            d[i] = float(v)
        return d

    def is_valid(self):
        vals = list(self.position) + list(self.rotation) + [self.fov_x, self.fov_y] + list(self.center_uv)
        return all(math.isfinite(v) for v in vals)

    def uniforms(self, img_size, tile_rows=None) -> "_ffi.BhCamera":
        """Kernel uniforms for an (img_w, img_h) render: pinhole params, 3x4 view
        matrix, Jacobian clamp limits (camera.rs:63-101,200-254).  `tile_rows` = (begin, end)
        restricts the render to a strip of 16-px tile rows (one frame partitioned over GPUs)."""
        w, h = int(img_size[0]), int(img_size[1])
        cam = _ffi.BhCamera()
        pos = (C.c_float * 3)(*self.position)
        rot = (C.c_float * 4)(*self.rotation)
        rc = _ffi.load().bh_camera_setup_model(pos, rot, float(self.fov_x), float(self.fov_y), float(self.center_uv[0]),
                                               float(self.center_uv[1]), w, h, self.model_id(), self._dist8(), C.byref(cam))
        if rc != 0:
            raise BrushHipError("bh_camera_setup_model failed (%d): image size must be non-zero, camera model known" % rc)
        if tile_rows is not None:
            cam.tile_row_begin, cam.tile_row_end = int(tile_rows[0]), int(tile_rows[1])
        return cam

    def apply_twist(self, twist) -> "Camera":
        """The camera moved by the twist (omega, tau): W <- exp([omega]x) W, t <- exp([omega]x) t + tau on its world-to-camera
        pose, by bh_camera_apply_twist on its uniforms (include/brush_hip_pose.h); position and rotation are read back from the
        moved view matrix.  Returns a new Camera."""
        return self._with_pose_of(_uniforms_apply_twist(self.uniforms((16, 16)), twist))   # (vm and cam_pos do not depend on the image size)

    def with_intrinsics(self, fx, fy, cx, cy, img_size) -> "Camera":
        """This camera with the focal lengths and the principal point (pixels of an (img_w, img_h) frame) replaced: fov_x / fov_y by
        focal_to_fov for its lens, center_uv = (cx / W, cy / H).  Returns a new Camera (include/brush_hip_intrinsics.h)."""
        import dataclasses
        w, h = int(img_size[0]), int(img_size[1])
        if not (all(math.isfinite(float(v)) for v in (fx, fy, cx, cy)) and fx > 0 and fy > 0):
            raise ValueError("Camera.with_intrinsics: fx, fy must be positive, all four finite")
        return dataclasses.replace(self, fov_x=focal_to_fov(fx, w, self.camera_model, self.dist), fov_y=focal_to_fov(fy, h, self.camera_model, self.dist),
                                   center_uv=(float(cx) / w, float(cy) / h))

    def transformed(self, T: "SceneTransform") -> "Camera":
        """The camera that sees a scene moved by T (Splats.transformed) as this one saw the original: position s R p + t, orientation
        R times its own, by bh_camera_apply_scene_transform on its uniforms (include/brush_hip_scene.h).  Returns a new Camera."""
        cam = self.uniforms((16, 16))
        out = _ffi.BhCamera()
        if _ffi.load().bh_camera_apply_scene_transform(C.byref(cam), C.byref(T.as_struct()), C.byref(out)) != 0:
            raise BrushHipError("bh_camera_apply_scene_transform failed")
        return self._with_pose_of(out)

    def _with_pose_of(self, cam: "_ffi.BhCamera") -> "Camera":
        """This camera with the position and rotation read back from the view matrix of `cam`."""
        import dataclasses
        r = [[float(cam.vm[3 * i + j]) for j in range(3)] for i in range(3)]   # camera-to-world = W^T: r[i][j] = W[j][i] = vm[3 i + j]
        q = [1 + r[0][0] - r[1][1] - r[2][2], 1 - r[0][0] + r[1][1] - r[2][2], 1 - r[0][0] - r[1][1] + r[2][2], 1 + r[0][0] + r[1][1] + r[2][2]]
        k = q.index(max(q))   # the best-conditioned of the four quaternion extractions
        if k == 3:
            quat = (r[2][1] - r[1][2], r[0][2] - r[2][0], r[1][0] - r[0][1], q[3])
        elif k == 0:
            quat = (q[0], r[1][0] + r[0][1], r[0][2] + r[2][0], r[2][1] - r[1][2])
        elif k == 1:
            quat = (r[1][0] + r[0][1], q[1], r[2][1] + r[1][2], r[0][2] - r[2][0])
        else:
            quat = (r[0][2] + r[2][0], r[2][1] + r[1][2], q[2], r[1][0] - r[0][1])
        n = math.sqrt(sum(v * v for v in quat))
        return dataclasses.replace(self, position=tuple(float(v) for v in cam.cam_pos), rotation=tuple(v / n for v in quat))


# ---------------------------------------------------------------------------
# Splats (brush-render/src/gaussian_splats.rs:62-74)
# ---------------------------------------------------------------------------
class RasterPass(enum.Enum):
    Forward = 0
    Backward = 1
    BackwardSmoothCutoff = 2

    def bwd_info(self):
        return self is not RasterPass.Forward

    def smooth_cutoff(self):
        return self is RasterPass.BackwardSmoothCutoff


class Splats:
    """transforms [N,10] = means(3) quat wxyz(4) log-scales(3); sh_coeffs [N,C,3];
    raw_opacities [N] (logits)."""

    def __init__(self, transforms, sh_coeffs, raw_opacities, render_mip=False, device=None, min_scale=None):
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        # Splats::min_scale (gaussian_splats.rs:69-73): optional frozen per-splat world-space scale floor [N]
        self.min_scale = None if min_scale is None else _f32c(min_scale, device).reshape(-1)
        self.transforms = _f32c(transforms, device).reshape(-1, 10)
        n = self.transforms.shape[0]
        self.sh_coeffs = _f32c(sh_coeffs, device).reshape(n, -1, 3) if n else _f32c(sh_coeffs, device).reshape(0, 1, 3)
        self.raw_opacities = _f32c(raw_opacities, device).reshape(n)
        self.render_mip = bool(render_mip)
        c = self.sh_coeffs.shape[1]
        deg = int(round(math.sqrt(c))) - 1
        if (deg + 1) ** 2 != c or deg > 4:
            raise ValueError("sh_coeffs must have (d+1)^2 coefficients, d <= 4 (got %d)" % c)  # sh.rs sh_degree_from_coeffs
        self._sh_degree = deg

    @staticmethod
    def from_tensor_data(means, rotations_wxyz, log_scales, sh_coeffs, raw_opacities, render_mip=False, device=None):
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        tr = torch.cat([_f32c(means, device).reshape(-1, 3), _f32c(rotations_wxyz, device).reshape(-1, 4),
                        _f32c(log_scales, device).reshape(-1, 3)], dim=1)
        return Splats(tr, sh_coeffs, raw_opacities, render_mip, device)

    def num_splats(self):
        return self.transforms.shape[0]

    def sh_degree(self):
        return self._sh_degree

    @property
    def device(self):
        return self.transforms.device

    def clone(self):
        return Splats(self.transforms.clone(), self.sh_coeffs.clone(), self.raw_opacities.clone(), self.render_mip, self.device,
                      None if self.min_scale is None else self.min_scale.clone())

    # ---- scene editing (include/brush_hip_scene.h) ----
    def _transform(self, T, ctx, ot, osh, oms):
        ctx = ctx or get_context(self.device)
        ms = self.min_scale
        ctx.check(ctx.lib.bh_splats_transform(ctx._h, C.byref(T.as_struct()), self.num_splats(), self.sh_coeffs.shape[1], _ptr(self.transforms),
                                              _ptr(self.sh_coeffs), _ptr(ms) if ms is not None else None, _ptr(ot), _ptr(osh),
                                              _ptr(oms) if oms is not None else None))

    def transformed(self, T: "SceneTransform", ctx=None) -> "Splats":
        """New Splats moved by x' = s R x + t (bh_splats_transform): means, rotations, log-scales, the SH bands of degree >= 1 and
        min_scale; opacities do not change (a copy).  Render them from Camera.transformed(T) for the image of the original."""
        ot, osh = torch.empty_like(self.transforms), torch.empty_like(self.sh_coeffs)
        oms = None if self.min_scale is None else torch.empty_like(self.min_scale)
        self._transform(T, ctx, ot, osh, oms)
        return Splats(ot, osh, self.raw_opacities.clone(), self.render_mip, self.device, oms)

    def transform_(self, T: "SceneTransform", ctx=None) -> "Splats":
        """transformed(T) in place."""
        self._transform(T, ctx, self.transforms, self.sh_coeffs, self.min_scale)
        return self

    # ---- Mip-Splatting 3D filter (gaussian_splats.rs:188-256) ----
    def with_min_scale(self, f):
        """Attach a per-splat world-space scale floor [N] (Splats::with_min_scale)."""
        f = _f32c(f, self.device).reshape(-1)
        if f.numel() != self.num_splats():
            raise ValueError("min_scale must have one entry per splat")
        self.min_scale = f
        return self

    def folded(self, ctx=None):
        """(transforms, raw_opacities) the renderer sees: fold_min_scale(params) when a floor is set
        (gaussian_splats.rs:379-386), the raw parameters otherwise."""
        if self.min_scale is None:
            return self.transforms, self.raw_opacities
        ctx = ctx or get_context(self.device)
        ft, fo = torch.empty_like(self.transforms), torch.empty_like(self.raw_opacities)
        ctx.check(ctx.lib.bh_fold_min_scale(ctx._h, _ptr(self.transforms), _ptr(self.raw_opacities), _ptr(self.min_scale), self.num_splats(),
                                            _ptr(ft), _ptr(fo)))
        return ft, fo

    def opacities(self, ctx=None):
        """Post-activation opacity incl. the floor's energy compensation (Splats::opacities)."""
        return torch.sigmoid(self.folded(ctx)[1])

    def scales(self, ctx=None):
        """World-space scales sqrt(s^2 + f^2) (Splats::scales)."""
        return torch.exp(self.folded(ctx)[0][:, 7:10])

    def bake_min_scale(self, ctx=None):
        """Permanently fold the floor into the raw parameters and clear it (Splats::bake_min_scale): in place."""
        if self.min_scale is not None:
            ctx = ctx or get_context(self.device)
            ctx.check(ctx.lib.bh_fold_min_scale(ctx._h, _ptr(self.transforms), _ptr(self.raw_opacities), _ptr(self.min_scale), self.num_splats(),
                                                _ptr(self.transforms), _ptr(self.raw_opacities)))
            self.min_scale = None
        return self


@dataclass
class RenderAux:
    """RenderAux (brush-render/src/render_aux.rs:17-68) + the tensors saved for backward."""
    num_visible: int
    num_intersections: int
    img_size: Tuple[int, int]
    visible: Optional[torch.Tensor]
    max_radius: torch.Tensor
    tile_offsets: torch.Tensor
    projected_splats: torch.Tensor
    compact_gid_from_isect: torch.Tensor
    tile_id_from_isect: torch.Tensor
    global_from_compact_gid: torch.Tensor
    cum_tiles_hit: torch.Tensor
    intersect_counts: torch.Tensor
    depths_sorted: torch.Tensor
    # depth-sliced lists (render_splats(..., sliced=True), the train step's default): the far slice's [T,2] segment table, or
    # None when the lists are the exact ones; list_budget = pairs the near pass listed; num_listed_splats = entries of the compact
    # arrays (per-tile cuts sort and number only the splats that own a listed pair: a sub-sequence of the full depth order)
    tile_offsets_far: Optional[torch.Tensor] = None
    list_budget: int = 0
    num_listed_splats: int = 0

    def validate(self, num_splats):
        # render_aux.rs:30-45
        tiles = self.tile_offsets.shape[0]
        assert self.num_visible <= num_splats
        assert self.num_intersections <= max(self.num_visible, 1) * max(tiles, 1)


def set_list_slicing(near_share: float, ctx: Optional["Context"] = None, device=None):
    """Near slice's share of the pair list for sliced forwards on `ctx` (bh_set_list_slicing): (0, 1] fixed, <= 0 automatic."""
    ctx = ctx or get_context(device)
    ctx.check(ctx.lib.bh_set_list_slicing(ctx._h, float(near_share)))


def set_view_id(view_id: int, ctx: Optional["Context"] = None, device=None):
    """The view the following forwards on `ctx` render (bh_set_view_id; sticky, 0 = unknown): selects the per-tile depth-cut
    table that sliced forwards read and refresh."""
    ctx = ctx or get_context(device)
    ctx.check(ctx.lib.bh_set_view_id(ctx._h, int(view_id)))


def _forward(ctx, splats, camera, img_size, background, pass_, sliced=False):
    if img_size[0] <= 0 or img_size[1] <= 0:
        raise BrushHipError("Can't render images with 0 size.")  # render.rs:50-53
    cam = camera if isinstance(camera, _ffi.BhCamera) else camera.uniforms(img_size)
    flags = (_ffi.FLAG_MIP if splats.render_mip else 0)
    if pass_.bwd_info():
        flags |= _ffi.FLAG_BWD_INFO
    if pass_.smooth_cutoff():
        flags |= _ffi.FLAG_SMOOTH_CUTOFF
    if sliced:
        flags |= _ffi.FLAG_SLICED_LISTS
    out = _ffi.BhRenderOut()
    bg = (C.c_float * 3)(*[float(b) for b in background])
    n = splats.num_splats()
    r_t, r_o = splats.folded(ctx)  # gaussian_splats.rs:379-386: the 3D-filter floor is part of the splat
    ctx.check(ctx.lib.bh_render_forward(ctx._h, C.byref(cam), n, splats.sh_degree(), _ptr(r_t), _ptr(splats.sh_coeffs),
                                        _ptr(r_o), bg, flags, C.byref(out)))
    return cam, out, (r_t, r_o)


def last_list_counts(ctx: Optional["Context"] = None, device=None):
    """(near_pairs, far_pairs) the last forward on `ctx` actually listed (bh_last_list_counts; blocking): the pair lists of a
    depth-sliced forward hold that many defined entries, not num_intersections."""
    ctx = ctx or get_context(device)
    a, b = C.c_uint32(), C.c_uint32()
    ctx.check(ctx.lib.bh_last_list_counts(ctx._h, C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def _aux_from(out, n, w, h, device, copy, ctx=None):
    nv, ni, T = out.num_visible, out.num_intersections, out.num_tiles
    nl = out.num_listed_splats   # entries of the compact (depth-ordered) arrays: == nv unless per-tile cuts listed a subset of the splats
    i32, f32 = torch.int32, torch.float32
    listed = ni
    if out.tile_offsets_far and copy and ctx is not None:
        # depth-sliced lists: only the near slice's pairs and, behind them, the far slice's are defined (copies are trimmed to
        # them; copy=False views keep the arena's length and cost no readback)
        near, far = last_list_counts(ctx)
        listed = min(ni, near + far)

    def mk(ptr, shape, dt):
        v = _view(ptr, shape, dt, device)
        return v.clone() if copy else v
    return RenderAux(
        num_visible=nv, num_intersections=ni, img_size=(w, h),
        visible=mk(out.visible, (n,), f32) if out.visible else None,
        max_radius=mk(out.max_radius, (n,), f32),
        tile_offsets=mk(out.tile_offsets, (T, 2), i32),
        projected_splats=mk(out.projected, (nl, 9), f32),
        compact_gid_from_isect=mk(out.compact_gid_from_isect, (listed,), i32),
        tile_id_from_isect=mk(out.tile_id_from_isect, (listed,), i32),
        global_from_compact_gid=mk(out.global_from_compact_gid, (nl,), i32),
        cum_tiles_hit=mk(out.cum_tiles_hit, (nl,), i32),
        intersect_counts=mk(out.intersect_counts, (n,), i32),
        depths_sorted=mk(out.depths_sorted, (nl,), f32),
        tile_offsets_far=mk(out.tile_offsets_far, (T, 2), i32) if out.tile_offsets_far else None,
        list_budget=int(out.list_budget),
        num_listed_splats=int(nl),
    )


def render_splats(splats: Splats, camera, img_size, background=(0.0, 0.0, 0.0), pass_: RasterPass = RasterPass.Forward,
                  ctx: Optional[Context] = None, copy=True, tile_rows=None, sliced=False):
    """Forward render. RasterPass.Forward returns a packed rgba8 image [H,W] (int32
    bit pattern, r in bits 0-7); the Backward variants return f32 [H,W,4].
    Returns (image, RenderAux). With copy=False the tensors alias ctx scratch
    memory and are only valid until the next render on `ctx`.
    sliced=True: BH_FLAG_SLICED_LISTS (same image / visible / counts; the list outputs are truncated, see the header)."""
    ctx = ctx or get_context(splats.device)
    w, h = int(img_size[0]), int(img_size[1])
    if tile_rows is not None and not isinstance(camera, _ffi.BhCamera):
        camera = camera.uniforms((w, h), tile_rows)
    _, out, _ = _forward(ctx, splats, camera, (w, h), background, pass_, sliced)
    if pass_.bwd_info():
        img = _view(out.out_img, (h, w, 4), torch.float32, splats.device)
    else:
        img = _view(out.out_img_packed, (h, w), torch.int32, splats.device)
    if copy:
        img = img.clone()
    return img, _aux_from(out, splats.num_splats(), w, h, splats.device, copy, ctx)


def render_splats_bwd(splats: Splats, camera, img_size, background, v_output, pass_: RasterPass = RasterPass.Backward,
                      ctx: Optional[Context] = None, tile_rows=None, sliced=False):
    """Differentiable render: forward (Backward pass flags) + backward for a given
    dL/d(out_img) `v_output` [H,W,4] (a tensor, or a callable img -> v_output).
    Returns dict(img, aux, v_transforms, v_sh_coeffs, v_raw_opacities, v_refine_weight, v_combined)."""
    assert pass_.bwd_info(), "render_splats_bwd requires a Backward variant"  # bwd/burn_glue.rs:281-284
    ctx = ctx or get_context(splats.device)
    w, h = int(img_size[0]), int(img_size[1])
    dev = splats.device
    if tile_rows is not None and not isinstance(camera, _ffi.BhCamera):
        camera = camera.uniforms((w, h), tile_rows)
    _, out, (r_t, r_o) = _forward(ctx, splats, camera, (w, h), background, pass_, sliced)
    img = _view(out.out_img, (h, w, 4), torch.float32, dev).clone()
    aux = _aux_from(out, splats.num_splats(), w, h, dev, True, ctx)
    if callable(v_output):
        v_output = v_output(img)
    v_output = _f32c(v_output, dev).reshape(h, w, 4)
    n, c = splats.num_splats(), splats.sh_coeffs.shape[1]
    v_t = torch.empty((n, 10), dtype=torch.float32, device=dev)
    v_sh = torch.empty((n, c, 3), dtype=torch.float32, device=dev)
    v_op = torch.empty((n,), dtype=torch.float32, device=dev)
    v_rf = torch.empty((n,), dtype=torch.float32, device=dev)
    # the saved state goes in explicitly (SplatBwdOps::rasterize_bwd / project_bwd, bwd/burn_glue.rs:62-92)
    ctx.check(ctx.lib.bh_render_backward_saved(ctx._h, C.byref(out), _ptr(v_output), _ptr(r_t), _ptr(splats.sh_coeffs), _ptr(r_o),
                                               _ptr(v_t), _ptr(v_sh), _ptr(v_op), _ptr(v_rf)))
    if splats.min_scale is not None:  # chain through the fold (the autodiff of bwd/burn_glue.rs:260-270)
        ctx.check(ctx.lib.bh_fold_min_scale_backward(ctx._h, _ptr(splats.transforms), _ptr(splats.raw_opacities), _ptr(splats.min_scale), n,
                                                     _ptr(v_t), _ptr(v_op)))
    vc = _view(ctx.lib.bh_last_v_combined(ctx._h), (max(out.num_listed_splats, 1), 10), torch.float32, dev).clone()
    return dict(img=img, aux=aux, v_transforms=v_t, v_sh_coeffs=v_sh, v_raw_opacities=v_op, v_refine_weight=v_rf, v_combined=vc)


class RenderNode:
    """One differentiable render = the autodiff node `render_splats` registers in the reference (bwd/burn_glue.rs:223-311: the
    forward's outputs + the state RenderBackwards saves, :336-371).  `backward(v_output)` may be called after OTHER renders have
    run on the same ctx if the node was created with retain=True (bh_render_retain); without it a later forward makes the node
    stale and backward raises BrushHipError (BH_ERR_STATE) instead of returning another frame's gradients."""

    def __init__(self, ctx, splats, out, folded, img_size, retained):
        self.ctx, self.splats, self.out, self._folded, self.img_size, self.retained = ctx, splats, out, folded, img_size, retained
        w, h = img_size
        self.img = _view(out.out_img, (h, w, 4), torch.float32, splats.device)   # aliases ctx memory: valid while the node is (retained nodes: until release)

    def depth(self, mode="expected"):
        """The node's depth map [H,W] f32 (bh_render_depth): "accumulated" sum of w z, "expected" = accumulated / alpha, or
        "median" (z where the transmittance first falls to 1/2); a forward of a tile-row window writes its rows, the rest is 0."""
        return render_depth(self, mode)

    def normal(self, mode="accumulated"):
        """The node's normal map [H,W,3] f32 in camera space (bh_render_normal): "accumulated" sum of w n, or "unit" = accumulated /
        its length (0 where that is 0); a forward of a tile-row window writes its rows, the rest is 0."""
        return render_normal(self, mode)

    def distortion(self, kind="z", near=0.2, far=1000.0):
        """The node's distortion map [H,W] f32 (bh_render_distortion): sum over pairs of w_i w_j (m_i - m_j)^2 with m = z ("z") or
        2DGS's far (z - near) / ((far - near) z) ("ndc"); a forward of a tile-row window writes its rows, the rest is 0."""
        return render_distortion(self, kind, near, far)

    def features(self, features):
        """The node's feature map [H,W,C] f32 (bh_render_features): the blend of the caller's per-splat vectors `features` [N,C],
        1 <= C <= 256, with the colour blend's own weights; a forward of a tile-row window writes its rows, the rest is 0."""
        return render_features(self, features)

    def backward(self, v_output, v_depth=None, depth_mode="expected", pose=False, v_normal=None, normal_mode="accumulated", v_distortion=None,
                 distortion="z", distortion_near=0.2, distortion_far=1000.0, intrinsics=False, v_features=None, features=None):
        """Gradients of <v_output, img> [+ <v_depth, depth(depth_mode)>] [+ <v_normal, normal(normal_mode)>] [+ <v_distortion,
        distortion(kind `distortion`, distortion_near, distortion_far)>]; v_output may be None when another cotangent is given.
        pose=True (bh_render_backward_pose_saved): also "v_viewmat", the twelve f32 of the gradient with respect to the camera's
        view matrix in the layout of BhCamera.vm, on the device (no readback); the colour term only.
        intrinsics=True (bh_render_backward_intrinsics_saved, or bh_render_backward_camera_saved with v_depth / v_normal /
        v_distortion): also "v_intrinsics", the four f32 (v_fx, v_fy, v_cx, v_cy) of the gradient of the whole sum with respect to
        the camera's fx, fy, cx, cy, on the device (no readback); combinable with pose=True (include/brush_hip_intrinsics.h).
        v_features [H,W,C] with features [N,C] (bh_render_backward_features_saved): + <v_features, features(features)>, and
        "v_features" [N,C] in the result, the gradient with respect to `features`; not together with v_depth / v_normal /
        v_distortion / pose / intrinsics."""
        ctx, splats, dev = self.ctx, self.splats, self.splats.device
        w, h = self.img_size
        n, c = splats.num_splats(), splats.sh_coeffs.shape[1]
        if v_features is not None or features is not None:
            if v_depth is not None or v_normal is not None or v_distortion is not None or pose or intrinsics:
                raise BrushHipError("RenderNode.backward: the feature term does not combine with v_depth / v_normal / v_distortion / pose / intrinsics")
            return self._backward_features(v_output, v_features, features)
        if v_output is None and v_depth is None and v_normal is None and v_distortion is None:
            raise BrushHipError("RenderNode.backward: neither v_output nor v_depth")
        # the pose gradient is the colour term's: refused without v_output or with another cotangent (named: the one whose entry
        # point the call would have taken)
        other = "v_distortion" if v_distortion is not None else "v_normal" if v_normal is not None else "v_depth"
        if pose and (v_output is None or v_depth is not None or v_normal is not None or v_distortion is not None):
            raise BrushHipError("RenderNode.backward: the pose gradient is that of the colour term alone (v_output, no %s)" % other)

        def cot(t, *shape):
            return None if t is None else _f32c(t, dev).reshape(*shape)
        v_output, v_depth, v_normal, v_distortion = cot(v_output, h, w, 4), cot(v_depth, h, w), cot(v_normal, h, w, 3), cot(v_distortion, h, w)
        # (NULL for a cotangent that was not given)
        p_output, p_depth, p_normal, p_distortion = (None if t is None else _ptr(t) for t in (v_output, v_depth, v_normal, v_distortion))
        r_t, r_o = self._folded
        v_t = torch.empty((n, 10), dtype=torch.float32, device=dev)
        v_sh = torch.empty((n, c, 3), dtype=torch.float32, device=dev)
        v_op = torch.empty((n,), dtype=torch.float32, device=dev)
        v_rf = torch.empty((n,), dtype=torch.float32, device=dev)
        v_vm = torch.empty((12,), dtype=torch.float32, device=dev) if pose else None
        v_in = torch.empty((4,), dtype=torch.float32, device=dev) if intrinsics else None
        tail = (_ptr(r_t), _ptr(splats.sh_coeffs), _ptr(r_o), _ptr(v_t), _ptr(v_sh), _ptr(v_op), _ptr(v_rf))
        # the narrowest entry point that takes every cotangent given
        lib = ctx.lib
        if intrinsics:
            cams = (None if v_vm is None else _ptr(v_vm), _ptr(v_in))
            if p_depth is None and p_normal is None and p_distortion is None:
                entry, args = lib.bh_render_backward_intrinsics_saved, tail + cams
            else:   # the general entry: the optional term records
                addr = lambda p: None if p is None else p.value
                rec = _ffi.BhCameraGradTerms(v_depth=addr(p_depth), v_normal=addr(p_normal), v_distortion=addr(p_distortion), depth_mode=_depth_mode(depth_mode),
                                             normal_mode=_normal_mode(normal_mode),
                                             distortion=_distortion_config(distortion, distortion_near, distortion_far))
                entry, args = lib.bh_render_backward_camera_saved, (C.byref(rec),) + tail + cams
        elif p_distortion is not None or p_normal is not None:
            maps = (p_depth, _depth_mode(depth_mode), p_normal, _normal_mode(normal_mode))
            if p_distortion is not None:
                cfg = _distortion_config(distortion, distortion_near, distortion_far)
                entry, args = lib.bh_render_backward_distortion_saved, maps + (p_distortion, C.byref(cfg)) + tail
            else:
                entry, args = lib.bh_render_backward_normal_saved, maps + tail
        elif pose:
            entry, args = lib.bh_render_backward_pose_saved, tail + (_ptr(v_vm),)
        elif p_depth is not None:
            entry, args = lib.bh_render_backward_depth_saved, (p_depth, _depth_mode(depth_mode)) + tail
        else:
            entry, args = lib.bh_render_backward_saved, tail
        ctx.check(entry(ctx._h, C.byref(self.out), p_output, *args))
        if splats.min_scale is not None:
            ctx.check(ctx.lib.bh_fold_min_scale_backward(ctx._h, _ptr(splats.transforms), _ptr(splats.raw_opacities), _ptr(splats.min_scale), n,
                                                         _ptr(v_t), _ptr(v_op)))
        res = dict(v_transforms=v_t, v_sh_coeffs=v_sh, v_raw_opacities=v_op, v_refine_weight=v_rf)
        if v_vm is not None:
            res["v_viewmat"] = v_vm
        if v_in is not None:
            res["v_intrinsics"] = v_in
        return res

    def _backward_features(self, v_output, v_map, features):
        ctx, splats, dev = self.ctx, self.splats, self.splats.device
        w, h = self.img_size
        n, c = splats.num_splats(), splats.sh_coeffs.shape[1]
        if v_map is None or features is None:
            raise BrushHipError("RenderNode.backward: v_features and features go together")
        features = _feature_rows(features, n, dev, "RenderNode.backward")
        ch = int(features.shape[1])
        v_map = _f32c(v_map, dev)
        if tuple(v_map.shape) != (h, w, ch):
            raise BrushHipError("RenderNode.backward: v_features must be [%d, %d, %d]" % (h, w, ch))
        v_output = None if v_output is None else _f32c(v_output, dev).reshape(h, w, 4)
        r_t, r_o = self._folded
        v_t = torch.empty((n, 10), dtype=torch.float32, device=dev)
        v_sh = torch.empty((n, c, 3), dtype=torch.float32, device=dev)
        v_op = torch.empty((n,), dtype=torch.float32, device=dev)
        v_rf = torch.empty((n,), dtype=torch.float32, device=dev)
        v_f = torch.empty((n, ch), dtype=torch.float32, device=dev)
        ctx.check(ctx.lib.bh_render_backward_features_saved(ctx._h, C.byref(self.out), None if v_output is None else _ptr(v_output), _ptr(features), ch,
                                                            _ptr(v_map), _ptr(r_t), _ptr(splats.sh_coeffs), _ptr(r_o), _ptr(v_t), _ptr(v_sh), _ptr(v_op),
                                                            _ptr(v_rf), _ptr(v_f)))
        if splats.min_scale is not None:
            ctx.check(ctx.lib.bh_fold_min_scale_backward(ctx._h, _ptr(splats.transforms), _ptr(splats.raw_opacities), _ptr(splats.min_scale), n,
                                                         _ptr(v_t), _ptr(v_op)))
        return dict(v_transforms=v_t, v_sh_coeffs=v_sh, v_raw_opacities=v_op, v_refine_weight=v_rf, v_features=v_f)

    def release(self):
        if self.retained:
            self.ctx.check(self.ctx.lib.bh_render_release(self.ctx._h, C.byref(self.out)))
            self.retained = False


DEPTH_MODES = {"accumulated": _ffi.DEPTH_ACCUMULATED, "expected": _ffi.DEPTH_EXPECTED, "median": _ffi.DEPTH_MEDIAN}


def _depth_mode(mode):
    return int(DEPTH_MODES[mode]) if isinstance(mode, str) else int(mode)


def render_depth(saved: "RenderNode", mode="expected", out=None):
    """Depth map [H,W] f32 of a differentiable render's saved state (bh_render_depth; include/brush_hip_depth.h): the node must be
    the ctx's most recent forward or a retained one.  `out`: a contiguous f32 [H,W] tensor to write into (rows outside a tile-row
    window are left as they are); otherwise a zero-filled one is returned."""
    ctx, dev = saved.ctx, saved.splats.device
    w, h = saved.img_size
    if out is None:
        out = torch.zeros((h, w), dtype=torch.float32, device=dev)
    if not (torch.is_tensor(out) and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (h, w)
            and out.device == torch.device(dev)):
        raise BrushHipError("render_depth: `out` must be a contiguous float32 [%d, %d] tensor on %s" % (h, w, dev))
    ctx.check(ctx.lib.bh_render_depth(ctx._h, C.byref(saved.out), _depth_mode(mode), _ptr(out)))
    return out


NORMAL_MODES = {"accumulated": _ffi.NORMAL_ACCUMULATED, "unit": _ffi.NORMAL_UNIT}


def _normal_mode(mode):
    return int(NORMAL_MODES[mode]) if isinstance(mode, str) else int(mode)


def _camera_of(camera, shape_hw):
    h, w = shape_hw
    return camera if isinstance(camera, _ffi.BhCamera) else camera.uniforms((int(w), int(h)))


def splat_normals(splats: Splats, camera, ctx: Optional[Context] = None):
    """The camera-space normal [N,3] f32 of every splat (bh_splat_normals; include/brush_hip_normal.h): the axis of the smallest
    scale of the rendered (folded) transforms, turned to face the camera.  `camera`: a BhCamera, or a Camera (any image size)."""
    ctx = ctx or get_context(splats.device)
    cam = camera if isinstance(camera, _ffi.BhCamera) else camera.uniforms((16, 16))
    n = splats.num_splats()
    r_t, _ = splats.folded(ctx)
    out = torch.empty((n, 3), dtype=torch.float32, device=splats.device)
    ctx.check(ctx.lib.bh_splat_normals(ctx._h, C.byref(cam), _ptr(r_t), n, _ptr(out)))
    if splats.min_scale is not None:
        ctx.sync()   # the folded temporary dies with this scope
    return out


def render_normal(saved: "RenderNode", mode="accumulated", out=None):
    """Normal map [H,W,3] f32 of a differentiable render's saved state (bh_render_normal; include/brush_hip_normal.h): the node must
    be the ctx's most recent forward or a retained one.  `out`: a contiguous f32 [H,W,3] tensor to write into (rows outside a
    tile-row window are left as they are); otherwise a zero-filled one is returned."""
    ctx, dev = saved.ctx, saved.splats.device
    w, h = saved.img_size
    if out is None:
        out = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    if not (torch.is_tensor(out) and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (h, w, 3)
            and out.device == torch.device(dev)):
        raise BrushHipError("render_normal: `out` must be a contiguous float32 [%d, %d, 3] tensor on %s" % (h, w, dev))
    ctx.check(ctx.lib.bh_render_normal(ctx._h, C.byref(saved.out), _ptr(saved._folded[0]), _normal_mode(mode), _ptr(out)))
    return out


FEATURE_MAX_CHANNELS = _ffi.FEATURE_MAX_CHANNELS
FEATURE_LOSS_KINDS = {"l1": _ffi.FEATURE_LOSS_L1, "cross_entropy": _ffi.FEATURE_LOSS_CROSS_ENTROPY}


def _feature_rows(features, n, dev, who):
    features = _f32c(features, dev)
    if features.dim() != 2 or features.shape[0] != n:
        raise BrushHipError("%s: features must be [%d, C]" % (who, n))
    return features


def render_features(saved: "RenderNode", features, out=None):
    """Feature map [H,W,C] f32 of a differentiable render's saved state (bh_render_features; include/brush_hip_features.h): the
    blend of `features` [N,C] (one row per splat, 1 <= C <= 256) with the colour blend's own weights, nothing clamped, no
    background.  The node must be the ctx's most recent forward or a retained one.  `out`: a contiguous f32 [H,W,C] tensor to write
    into (rows outside a tile-row window are left as they are); otherwise a zero-filled one is returned."""
    ctx, dev = saved.ctx, saved.splats.device
    w, h = saved.img_size
    features = _feature_rows(features, saved.splats.num_splats(), dev, "render_features")
    ch = int(features.shape[1])
    if out is None:
        out = torch.zeros((h, w, ch), dtype=torch.float32, device=dev)
    if not (torch.is_tensor(out) and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (h, w, ch)
            and out.device == torch.device(dev)):
        raise BrushHipError("render_features: `out` must be a contiguous float32 [%d, %d, %d] tensor on %s" % (h, w, ch, dev))
    ctx.check(ctx.lib.bh_render_features(ctx._h, C.byref(saved.out), _ptr(features), ch, _ptr(out)))
    return out


def feature_loss_value_and_grad(map, target, kind="l1", weight=1.0, want_grad=True, ctx: Optional[Context] = None):
    """The fused feature losses (bh_feature_loss_value_and_grad; include/brush_hip_features.h) of a feature map [H,W,C]: "l1"
    against an f32 target [H,W,C] (a pixel counts when all its target values are finite; the mean over H W C), or "cross_entropy"
    against uint8 labels [H,W] (a pixel counts when label < C, 255 = ignore; the mean over H W) -> (loss [2] device f32 = (weight *
    the mean, valid pixels), v_map [H,W,C] or None).  Queued on the ctx stream: nothing is read back."""
    dev = map.device
    ctx = ctx or get_context(dev)
    map = _f32c(map, dev)
    if map.dim() != 3:
        raise ValueError("the feature map must be [H, W, C]")
    h, w, ch = (int(s) for s in map.shape)
    k = int(FEATURE_LOSS_KINDS[kind]) if isinstance(kind, str) else int(kind)
    if k == _ffi.FEATURE_LOSS_CROSS_ENTROPY:
        target = torch.as_tensor(target, dtype=torch.uint8, device=dev).contiguous()
        want = (h, w)
    else:
        target = _f32c(target, dev)
        want = (h, w, ch)
    if tuple(target.shape) != want:
        raise ValueError("the feature target must be %s" % (want,))
    t = _ffi.BhFeatureTarget()
    t.target, t.h, t.w, t.channels, t.kind, t.weight = target.data_ptr(), h, w, ch, k, float(weight)
    loss = torch.empty((2,), dtype=torch.float32, device=dev)
    v_map = torch.empty_like(map) if want_grad else None
    ctx.check(ctx.lib.bh_feature_loss_value_and_grad(ctx._h, _ptr(map), C.byref(t), _ptr(loss), _ptr(v_map) if want_grad else None))
    return loss, v_map


class FeatureField:
    """Caller-owned per-splat feature vectors [N,C] with their Adam state.  On a fixed set of splats (the second stage of LangSplat
    and Gaussian Grouping): zero-initialised features, `render(node)` the map, `backward(node, v_map)` the gradients,
    `step(v_features)` one Adam step (adam_step with row_len = C).  Jointly with the splats (Feature-3DGS, gsplat's colors [N, D]):
    SplatTrainer(..., feature_field=field) trains it inside the step against SceneBatch.features and carries it through refine
    (`carry`); `gather` follows a decimation.  `t` counts the Adam updates applied so far, whoever applied them."""

    def __init__(self, n, channels, lr=1e-2, device=None, ctx: Optional[Context] = None, beta1=0.9, beta2=0.999, eps=1e-15):
        if not 1 <= int(channels) <= FEATURE_MAX_CHANNELS:
            raise BrushHipError("FeatureField: channels must be 1 .. %d" % FEATURE_MAX_CHANNELS)
        self.ctx = ctx or get_context(device)
        dev = device if device is not None else "cuda:%d" % torch.cuda.current_device()
        self.lr, self.beta1, self.beta2, self.eps = float(lr), beta1, beta2, eps
        self.features = torch.zeros((int(n), int(channels)), dtype=torch.float32, device=dev)
        self.m1 = torch.zeros_like(self.features)
        self.m2 = torch.zeros_like(self.features)
        self.t = 0

    def render(self, node: "RenderNode"):
        return render_features(node, self.features)

    def backward(self, node: "RenderNode", v_map, v_output=None):
        return node.backward(v_output, v_features=v_map, features=self.features)

    def step(self, v_features):
        self.t += 1
        adam_step(self.features, _f32c(v_features, self.features.device), self.m1, self.m2, self.lr, self.t, beta1=self.beta1, beta2=self.beta2,
                  eps=self.eps, ctx=self.ctx)

    def as_struct(self) -> "_ffi.BhFeatureField":
        """The field as bh_train_set_features takes it (include/brush_hip_feature_train.h): the three tensors, the counters and the
        Adam constants; `step` = the updates applied so far (self.t)."""
        f = _ffi.BhFeatureField()
        f.features, f.m1, f.m2 = self.features.data_ptr(), self.m1.data_ptr(), self.m2.data_ptr()
        f.n, f.channels, f.step = int(self.features.shape[0]), int(self.features.shape[1]), int(self.t)
        f.lr, f.beta1, f.beta2, f.eps = float(self.lr), float(self.beta1), float(self.beta2), float(self.eps)
        return f

    def carry(self, ctx: Optional[Context] = None, total_splats: Optional[int] = None):
        """Takes the field through the ctx's pending refine plan (bh_refine_carry_rows; valid between bh_refine_plan and
        bh_refine_apply — SplatTrainer.refine calls it there): the features follow their splats, a split parent's row goes to both
        halves; the moments of both halves of a split start at zero, as refine leaves the splats' own.  Replaces the three tensors.
        total_splats: the plan's BhRefineStats.total_splats if the caller has it (refine does); None reads it from the plan's flags (one
        synchronising readback)."""
        ctx = ctx or self.ctx
        dev = self.features.device
        n, ch = (int(v) for v in self.features.shape)
        flags = ctx.lib.bh_refine_plan_flags(ctx._h, 0)
        if not flags:
            raise BrushHipError("FeatureField.carry: no refine plan is pending (call it between bh_refine_plan and bh_refine_apply)")
        if total_splats is None:
            ctx.sync()
            total_splats = int(_view(flags, (n,), torch.int32, dev).sum().item()) + int(_view(ctx.lib.bh_refine_plan_flags(ctx._h, 2), (n,), torch.int32, dev).sum().item())
        new = [torch.empty((int(total_splats), ch), dtype=torch.float32, device=dev) for _ in range(3)]
        if not ctx.uses_torch_stream:
            torch.cuda.current_stream(dev).synchronize()
        for src, dst, mode in ((self.features, new[0], _ffi.CARRY_COPY), (self.m1, new[1], _ffi.CARRY_ZERO_SPLIT), (self.m2, new[2], _ffi.CARRY_ZERO_SPLIT)):
            ctx.check(ctx.lib.bh_refine_carry_rows(ctx._h, _ptr(src), _ptr(dst), ch, mode))
        if not ctx.uses_torch_stream:
            ctx.sync()   # the old tables are released below: on torch's own stream its allocator orders that, on the ctx's nothing does
        self.features, self.m1, self.m2 = new

    def gather(self, indices):
        """Keeps the rows `indices` (what decimate_to_count(..., return_indices=True) returns), in that order: plain indexing of the
        three tensors."""
        idx = torch.as_tensor(indices, device=self.features.device).long()
        self.features, self.m1, self.m2 = (t[idx].contiguous() for t in (self.features, self.m1, self.m2))


DISTORTION_KINDS = {"z": _ffi.DISTORTION_Z, "ndc": _ffi.DISTORTION_NDC}


def _distortion_kind(kind):
    return int(DISTORTION_KINDS[kind]) if isinstance(kind, str) else int(kind)


def _distortion_config(kind, near, far):
    return _ffi.BhDistortionConfig(kind=_distortion_kind(kind), near_z=float(near), far_z=float(far))


def render_distortion(saved: "RenderNode", kind="z", near=0.2, far=1000.0, out=None, moments=False):
    """Distortion map [H,W] f32 of a differentiable render's saved state (bh_render_distortion; include/brush_hip_distortion.h), or —
    moments=True — its moment map [H,W,4] = (A, M1', M2', r) (bh_render_distortion_moments; what distortion_loss and the backward
    read).  The node must be the ctx's most recent forward or a retained one.  `out`: a contiguous f32 tensor of that shape to write
    into (rows outside a tile-row window are left as they are); otherwise a zero-filled one is returned."""
    ctx, dev = saved.ctx, saved.splats.device
    w, h = saved.img_size
    shape = (h, w, 4) if moments else (h, w)
    if out is None:
        out = torch.zeros(shape, dtype=torch.float32, device=dev)
    if not (torch.is_tensor(out) and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape
            and out.device == torch.device(dev)):
        raise BrushHipError("render_distortion: `out` must be a contiguous float32 %s tensor on %s" % (list(shape), dev))
    cfg = _distortion_config(kind, near, far)
    fn = ctx.lib.bh_render_distortion_moments if moments else ctx.lib.bh_render_distortion
    ctx.check(fn(ctx._h, C.byref(saved.out), C.byref(cfg), _ptr(out)))
    return out


def distortion_loss(dist_or_moments, weight=1.0, ctx: Optional[Context] = None):
    """weight * sum(dist) / (H W) of a distortion map [H,W] or a moment map [H,W,4] (bh_distortion_loss): -> loss [2] device f32 =
    (the loss, the number of pixels).  f64 sums in a fixed order: two calls give the same bits.  The gradient with respect to the
    distortion map is the constant weight / (H W).  Queued on the ctx stream: nothing is read back."""
    dev = dist_or_moments.device
    ctx = ctx or get_context(dev)
    m = _f32c(dist_or_moments, dev)
    if m.dim() == 2:
        channels = 1
    elif m.dim() == 3 and m.shape[2] == 4:
        channels = 4
    else:
        raise ValueError("distortion_loss: a distortion map [H, W] or a moment map [H, W, 4]")
    h, w = m.shape[0], m.shape[1]
    loss = torch.empty((2,), dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.bh_distortion_loss(ctx._h, _ptr(m), h, w, channels, float(weight), _ptr(loss)))
    return loss


def depth_to_normal(depth, camera, ctx: Optional[Context] = None):
    """Camera-space normals [H,W,3] f32 of a z-depth map [H,W] (bh_depth_to_normal): central differences of the back-projected
    points, 0 on the border and wherever the pixel or one of its four neighbours holds no finite depth > 0.  Pinhole cameras only."""
    dev = depth.device
    ctx = ctx or get_context(dev)
    depth = _f32c(depth, dev)
    if depth.dim() != 2:
        raise ValueError("depth_to_normal: the depth map must be [H, W]")
    h, w = depth.shape
    cam = _camera_of(camera, (h, w))
    out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.bh_depth_to_normal(ctx._h, C.byref(cam), _ptr(depth), h, w, _ptr(out)))
    return out


def depth_to_normal_backward(depth, v_normal, camera, ctx: Optional[Context] = None):
    """v_depth [H,W] f32 = the gradient of <v_normal, depth_to_normal(depth)> (bh_depth_to_normal_backward): a gather without
    atomics, the same bits on every call."""
    dev = depth.device
    ctx = ctx or get_context(dev)
    depth = _f32c(depth, dev)
    if depth.dim() != 2:
        raise ValueError("depth_to_normal_backward: the depth map must be [H, W]")
    h, w = depth.shape
    v_normal = _f32c(v_normal, dev).reshape(h, w, 3)
    cam = _camera_of(camera, (h, w))
    out = torch.empty((h, w), dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.bh_depth_to_normal_backward(ctx._h, C.byref(cam), _ptr(depth), _ptr(v_normal), h, w, _ptr(out)))
    return out


DEPTH_LOSS_KINDS = {"l1": _ffi.DEPTH_LOSS_L1, "disparity": _ffi.DEPTH_LOSS_DISPARITY}


def _depth_target(gt, dev, kind="l1", weight=1.0, scale=1.0, offset=0.0, shape=None):
    """(BhDepthTarget, the tensor its gt points into).  `kind`: "l1" (gt holds depth) or "disparity" (gt holds inverse depth)."""
    gt = _f32c(gt, dev)
    if gt.dim() != 2 or (shape is not None and tuple(gt.shape) != tuple(shape)):
        raise ValueError("the depth target must be [H, W]%s" % ("" if shape is None else " = %s" % (tuple(shape),)))
    t = _ffi.BhDepthTarget()
    t.gt, t.h, t.w = gt.data_ptr(), int(gt.shape[0]), int(gt.shape[1])
    t.kind = int(DEPTH_LOSS_KINDS[kind]) if isinstance(kind, str) else int(kind)
    t.weight, t.scale, t.offset = float(weight), float(scale), float(offset)
    return t, gt


def depth_loss_value_and_grad(depth, gt, kind="l1", weight=1.0, scale=1.0, offset=0.0, ctx: Optional[Context] = None, want_grad=True):
    """The fused depth loss (bh_depth_loss_value_and_grad; include/brush_hip_depth_loss.h) of an expected-depth map [H,W] against
    the target t = fma(scale, gt, offset): -> (loss [2] device f32 = (weight * sum |.| / (H W), valid pixels), v_depth [H,W] or
    None).  A pixel counts when gt is finite, t > 0 and depth > 0.  Queued on the ctx stream: nothing is read back."""
    dev = depth.device
    ctx = ctx or get_context(dev)
    depth = _f32c(depth, dev)
    t, keep = _depth_target(gt, dev, kind, weight, scale, offset, shape=depth.shape)
    loss = torch.empty((2,), dtype=torch.float32, device=dev)
    v_depth = torch.empty_like(depth) if want_grad else None
    ctx.check(ctx.lib.bh_depth_loss_value_and_grad(ctx._h, _ptr(depth), C.byref(t), _ptr(loss), _ptr(v_depth) if want_grad else None))
    return loss, v_depth


def normal_consistency_value_and_grad(normal, depth, image, camera, weight=1.0, v_depth=None, ctx: Optional[Context] = None):
    """The fused normal-consistency operator (bh_normal_consistency_value_and_grad; include/brush_hip_normal_loss.h) between an
    accumulated normal map [H,W,3] and the normals of the expected-depth map [H,W] of the same frame, weighted by the alpha of `image`
    [H,W,4] (a constant): -> (loss [2] device f32 = (weight * sum A (1 - N . u) / (H W), valid pixels), v_normal [H,W,3], v_depth
    [H,W]).  `v_depth`: a contiguous f32 [H,W] tensor the depth gradient is ADDED to in place (and returned); None: a fresh one.
    Pinhole cameras only.  Queued on the ctx stream: nothing is read back."""
    dev = depth.device
    ctx = ctx or get_context(dev)
    depth = _f32c(depth, dev)
    if depth.dim() != 2:
        raise ValueError("normal_consistency_value_and_grad: the depth map must be [H, W]")
    h, w = depth.shape
    normal = _f32c(normal, dev).reshape(h, w, 3)
    image = _f32c(image, dev).reshape(h, w, 4)
    accumulate = v_depth is not None
    if accumulate and (v_depth.dtype != torch.float32 or tuple(v_depth.shape) != (h, w) or not v_depth.is_contiguous() or v_depth.device != dev):
        raise BrushHipError("normal_consistency_value_and_grad: `v_depth` must be a contiguous float32 [%d, %d] tensor on %s" % (h, w, dev))
    cam = camera.uniforms((w, h))
    loss = torch.empty((2,), dtype=torch.float32, device=dev)
    v_normal = torch.empty_like(normal)
    if not accumulate:
        v_depth = torch.empty_like(depth)
    ctx.check(ctx.lib.bh_normal_consistency_value_and_grad(ctx._h, C.byref(cam), _ptr(normal), _ptr(depth), _ptr(image), h, w, float(weight),
                                                           1 if accumulate else 0, _ptr(loss), _ptr(v_normal), _ptr(v_depth)))
    return loss, v_normal, v_depth


def eval_depth_metrics(depth, gt, kind="l1", scale=1.0, offset=0.0, ctx: Optional[Context] = None, out=None):
    """Held-out depth metrics (bh_eval_depth_metrics) of an expected-depth map against a target: -> device f32 [4] = (abs-rel, RMSE,
    share of pixels with max(E / z, z / E) < 1.25, valid pixels); validity as in depth_loss_value_and_grad.  Nothing is read back."""
    dev = depth.device
    ctx = ctx or get_context(dev)
    depth = _f32c(depth, dev)
    t, keep = _depth_target(gt, dev, kind, 1.0, scale, offset, shape=depth.shape)
    metrics = out if out is not None else torch.empty((4,), dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.bh_eval_depth_metrics(ctx._h, _ptr(depth), C.byref(t), _ptr(metrics)))
    return metrics


def render_splats_diff(splats: Splats, camera, img_size, background=(0.0, 0.0, 0.0), pass_: RasterPass = RasterPass.Backward,
                       ctx: Optional[Context] = None, retain=False, sliced=False, tile_rows=None) -> RenderNode:
    """Forward of a differentiable render; gradients later through RenderNode.backward (bwd/burn_glue.rs:223-311)."""
    assert pass_.bwd_info()
    ctx = ctx or get_context(splats.device)
    w, h = int(img_size[0]), int(img_size[1])
    if tile_rows is not None and not isinstance(camera, _ffi.BhCamera):
        camera = camera.uniforms((w, h), tile_rows)
    _, out, folded = _forward(ctx, splats, camera, (w, h), background, pass_, sliced)
    if retain:
        ctx.check(ctx.lib.bh_render_retain(ctx._h, C.byref(out)))
    return RenderNode(ctx, splats, out, folded, (w, h), bool(retain))


# ---------------------------------------------------------------------------
# Camera pose refinement (include/brush_hip_pose.h)
# ---------------------------------------------------------------------------
def pose_twist(vm, v_viewmat):
    """(v_omega, v_tau) [6] f64 of a view-matrix gradient (bh_pose_twist): the derivative of the loss along
    W <- exp([omega]x) W, t <- exp([omega]x) t + tau at zero.  `vm`, `v_viewmat`: twelve floats, column-major 3x4."""
    import numpy as np
    a = (C.c_float * 12)(*[float(v) for v in vm])
    b = (C.c_float * 12)(*[float(v) for v in v_viewmat])
    out = (C.c_double * 6)()
    if _ffi.load().bh_pose_twist(a, b, out) != 0:
        raise BrushHipError("bh_pose_twist failed")
    return np.array(list(out), np.float64)


def _uniforms_apply_twist(cam: "_ffi.BhCamera", twist) -> "_ffi.BhCamera":
    """A copy of the uniforms `cam` moved by the twist (bh_camera_apply_twist rewrites vm and cam_pos together)."""
    out = _ffi.BhCamera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(out))
    tw = (C.c_double * 6)(*[float(v) for v in twist])
    if _ffi.load().bh_camera_apply_twist(C.byref(out), tw) != 0:
        raise BrushHipError("bh_camera_apply_twist failed")
    return out


class PoseOptimizer:
    """Adam on a 6-vector (omega, tau) per view id, on the host in f64: the view's camera is its dataset camera moved by that
    twist (Camera.apply_twist / bh_camera_apply_twist).  The gradient is the twist of v_viewmat at the current pose (pose_twist),
    which is the gradient with respect to the 6-vector to first order in it.

    One step of a view: `camera(view_id, base, img_size)` gives the uniforms to render, `update(view_id, vm, v_viewmat)` takes the
    twelve floats read back after the backward (48 bytes, one synchronisation of the stream the backward ran on: `step` does it).  A camera
    that moves every step must not key the per-view tile-cut tables by its hash, which would mint a table per step: `bind`
    names the view with bh_set_view_id, and SplatTrainer passes the batch's view_id."""

    def __init__(self, lr_rotation=1e-3, lr_translation=1e-3, beta1=0.9, beta2=0.999, eps=1e-12):
        self.lr_rotation, self.lr_translation = float(lr_rotation), float(lr_translation)
        self.beta1, self.beta2, self.eps = float(beta1), float(beta2), float(eps)
        self.views = {}   # view id -> dict(twist [6], m1 [6], m2 [6], t)

    def _state(self, view_id):
        import numpy as np
        view_id = int(view_id)
        if view_id <= 0:
            raise ValueError("PoseOptimizer: a view id > 0 names the view (0 = unknown)")
        if view_id not in self.views:
            self.views[view_id] = dict(twist=np.zeros(6), m1=np.zeros(6), m2=np.zeros(6), t=0)
        return self.views[view_id]

    def twist(self, view_id):
        return self._state(view_id)["twist"].copy()

    def camera(self, view_id, base, img_size=None) -> "_ffi.BhCamera":
        """The uniforms of view `view_id` at its current correction; `base`: its dataset Camera (with img_size) or BhCamera."""
        if not isinstance(base, _ffi.BhCamera):
            base = base.uniforms(img_size)
        return _uniforms_apply_twist(base, self._state(view_id)["twist"])

    def bind(self, ctx, view_id, base, img_size=None) -> "_ffi.BhCamera":
        """camera(), and names the view on `ctx` for the forwards that follow (bh_set_view_id)."""
        ctx.check(ctx.lib.bh_set_view_id(ctx._h, int(view_id)))
        return self.camera(view_id, base, img_size)

    def update(self, view_id, vm, v_viewmat):
        """One Adam step of the view's 6-vector on the twist of `v_viewmat` [12] at the rendered pose `vm` [12]."""
        import numpy as np
        s = self._state(view_id)
        g = pose_twist(vm, v_viewmat)
        s["t"] += 1
        s["m1"] = self.beta1 * s["m1"] + (1.0 - self.beta1) * g
        s["m2"] = self.beta2 * s["m2"] + (1.0 - self.beta2) * g * g
        m1 = s["m1"] / (1.0 - self.beta1 ** s["t"])
        m2 = s["m2"] / (1.0 - self.beta2 ** s["t"])
        lr = np.array([self.lr_rotation] * 3 + [self.lr_translation] * 3)
        s["twist"] = s["twist"] - lr * m1 / (np.sqrt(m2) + self.eps)
        return g

    def step(self, view_id, vm, v_viewmat_dev, ctx: Optional["Context"] = None):
        """update() on a device tensor of twelve floats the backward on `ctx` wrote: the 48-byte readback waits for the stream that
        wrote them — torch's current stream, which the copy synchronises, or the ctx's own (Context(use_torch_stream=False)),
        which is synchronised first.  Pass the ctx the backward ran on (None = the device's default context)."""
        ctx = ctx or get_context(v_viewmat_dev.device)
        if not ctx.uses_torch_stream:
            ctx.sync()
        return self.update(view_id, vm, v_viewmat_dev.detach().cpu().numpy().astype("float64"))


# ---------------------------------------------------------------------------
# Camera intrinsics refinement (include/brush_hip_intrinsics.h)
# ---------------------------------------------------------------------------
def _uniforms_set_intrinsics(cam: "_ffi.BhCamera", fx, fy, cx, cy) -> "_ffi.BhCamera":
    """A copy of the uniforms `cam` with these intrinsics (bh_camera_set_intrinsics rewrites the clamp limits and the cull angle with them)."""
    out = _ffi.BhCamera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(_ffi.BhCamera))
    if _ffi.load().bh_camera_set_intrinsics(C.byref(out), float(fx), float(fy), float(cx), float(cy)) != 0:
        raise BrushHipError("bh_camera_set_intrinsics failed: fx, fy must be positive, all four finite")
    return out


class IntrinsicsOptimizer:
    """Adam on a 4-vector (s_x, s_y, du, dv) per SENSOR, on the host in f64: a view of that sensor is rendered with
    fx = fx0 exp(s_x), fy = fy0 exp(s_y), center_uv + (du, dv) of its dataset camera — free of the resolution, so the image scales of
    one sensor share the vector.  `sensor_of`: view id -> sensor id (a view it does not name, and every view without it, belongs to
    sensor 0).  The gradient of a step's v_intrinsics (v_fx, v_fy, v_cx, v_cy) is (v_fx fx, v_fy fy, v_cx W, v_cy H); share_focal ties
    s_x = s_y and sums the two.

    One step of a view, as PoseOptimizer's: `camera(view_id, base, img_size)` gives the uniforms to render, `update(view_id, cam,
    v_intrinsics)` takes the rendered uniforms and the four floats read back after the backward (`step` does the readback), `bind`
    also names the view on the ctx (a camera that changes every step must not key the per-view tables by its hash)."""

    def __init__(self, lr_focal=1e-3, lr_center=1e-4, sensor_of=None, share_focal=False, beta1=0.9, beta2=0.999, eps=1e-12):
        self.lr_focal, self.lr_center = float(lr_focal), float(lr_center)
        self.sensor_of = dict(sensor_of or {})
        self.share_focal = bool(share_focal)
        self.beta1, self.beta2, self.eps = float(beta1), float(beta2), float(eps)
        self.sensors = {}   # sensor id -> dict(params [4], m1 [4], m2 [4], t)

    def _state(self, view_id):
        import numpy as np
        view_id = int(view_id)
        if view_id <= 0:
            raise ValueError("IntrinsicsOptimizer: a view id > 0 names the view (0 = unknown)")
        sensor = self.sensor_of.get(view_id, 0)
        if sensor not in self.sensors:
            self.sensors[sensor] = dict(params=np.zeros(4), m1=np.zeros(4), m2=np.zeros(4), t=0)
        return self.sensors[sensor]

    def params(self, view_id):
        return self._state(view_id)["params"].copy()

    def camera(self, view_id, base, img_size=None) -> "_ffi.BhCamera":
        """The uniforms of view `view_id` at its sensor's current correction; `base`: its dataset Camera (with img_size) or BhCamera."""
        if not isinstance(base, _ffi.BhCamera):
            base = base.uniforms(img_size)
        sx, sy, du, dv = self._state(view_id)["params"]
        if sx == 0.0 and sy == 0.0 and du == 0.0 and dv == 0.0:   # the identity, to the bit
            out = _ffi.BhCamera()
            C.memmove(C.byref(out), C.byref(base), C.sizeof(_ffi.BhCamera))
            return out
        return _uniforms_set_intrinsics(base, float(base.fx) * math.exp(sx), float(base.fy) * math.exp(sy), float(base.cx) + du * base.img_w,
                                        float(base.cy) + dv * base.img_h)

    def bind(self, ctx, view_id, base, img_size=None) -> "_ffi.BhCamera":
        """camera(), and names the view on `ctx` for the forwards that follow (bh_set_view_id)."""
        ctx.check(ctx.lib.bh_set_view_id(ctx._h, int(view_id)))
        return self.camera(view_id, base, img_size)

    def update(self, view_id, cam, v_intrinsics):
        """One Adam step of the sensor's 4-vector on `v_intrinsics` [4] of a frame rendered with the uniforms `cam`."""
        import numpy as np
        s = self._state(view_id)
        v = np.asarray(v_intrinsics, np.float64).reshape(4)
        g = np.array([v[0] * float(cam.fx), v[1] * float(cam.fy), v[2] * float(cam.img_w), v[3] * float(cam.img_h)])
        if self.share_focal:
            g[0] = g[1] = g[0] + g[1]
        s["t"] += 1
        s["m1"] = self.beta1 * s["m1"] + (1.0 - self.beta1) * g
        s["m2"] = self.beta2 * s["m2"] + (1.0 - self.beta2) * g * g
        m1 = s["m1"] / (1.0 - self.beta1 ** s["t"])
        m2 = s["m2"] / (1.0 - self.beta2 ** s["t"])
        lr = np.array([self.lr_focal] * 2 + [self.lr_center] * 2)
        s["params"] = s["params"] - lr * m1 / (np.sqrt(m2) + self.eps)
        return g

    def step(self, view_id, cam, v_intrinsics_dev, ctx: Optional["Context"] = None):
        """update() on a device tensor of four floats the backward on `ctx` wrote; the 16-byte readback waits as PoseOptimizer.step's."""
        ctx = ctx or get_context(v_intrinsics_dev.device)
        if not ctx.uses_torch_stream:
            ctx.sync()
        return self.update(view_id, cam, v_intrinsics_dev.detach().cpu().numpy().astype("float64"))


# ---------------------------------------------------------------------------
# Learned device tables: per-view exposure compensation (include/brush_hip_exposure.h) and bilateral grids
# (include/brush_hip_bilagrid.h), and the environment map (include/brush_hip_envmap.h)
# ---------------------------------------------------------------------------
def _hwc4_out(img, out):
    """The result tensor of an [H,W,4] operator on `img`: a new one, or the caller's `out` once it fits."""
    if out is None:
        return torch.empty_like(img)
    if out.shape != img.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.data_ptr() % 16:
        raise ValueError("out must be a contiguous, 16-byte aligned f32 [H,W,4]")
    return out


class _ParamTable:
    """What the learned device tables share (csrc/param_table.h): rows of `shape` f32 parameters, each with its gradient, its Adam
    moments (of the kind's dtype) and its step count.  A per-view kind has `n_views` rows, numbered from 1, and its arrays a leading
    [V] axis; a kind without views (`_per_view` = False) is its one row, and its C entry points take no row arguments.  A subclass
    names the C symbols' prefix and the moment type, opens the table with `_open`, checks the moments it is handed in `_moment` and
    words its shape in `_params_shape_text`."""
    _prefix = None                      # "bh_exposure" | "bh_bilagrid" | "bh_envmap"
    _moment_np, _moment_c = None, None  # the moments' numpy dtype and ctypes type
    _per_view = True

    def _fn(self, name):
        return getattr(self.lib, "%s_%s" % (self._prefix, name))

    def _rows(self, *rows):
        """The row arguments of a C call."""
        return tuple(int(r) for r in rows) if self._per_view else ()

    def _open(self, ctx, n_views, shape, create_args, lr, beta1, beta2, eps):
        ctx = ctx or get_context()
        self.ctx, self.lib, self.n_views, self.shape = ctx, ctx.lib, int(n_views), tuple(shape)   # shape: one row
        self._all = ((self.n_views,) if self._per_view else ()) + self.shape                      # ... and every row
        h = C.c_void_p()
        ctx.check(self._fn("create")(ctx._h, *self._rows(n_views), *create_args, C.byref(h)))
        self._h = h
        self.lr, self.beta1, self.beta2, self.eps = float(lr), float(beta1), float(beta2), float(eps)
        self.set_lr(lr)

    def set_lr(self, lr):
        """The learning rate of every following update (bh_*_set_adam); 0 freezes the rows while their moments still move."""
        self.ctx.check(self._fn("set_adam")(self.ctx._h, self._h, float(lr), self.beta1, self.beta2, self.eps))
        self.lr = float(lr)

    def _get(self, fn):
        import numpy as np
        out = np.empty(self._all, np.float32)
        self.ctx.check(fn(self.ctx._h, self._h, *self._rows(1, self.n_views), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def _set_rows(self, first, count, a):
        self.ctx.check(self._fn("set_params")(self.ctx._h, self._h, *self._rows(first, count), a.ctypes.data_as(C.POINTER(C.c_float))))

    @property
    def params(self):
        """f32 numpy copy of the whole table (one synchronisation): [V, *shape], or [*shape] for a kind without views; assign an array of
        the same shape to set it."""
        return self._get(self._fn("get_params"))

    @params.setter
    def params(self, value):
        import numpy as np
        a = np.ascontiguousarray(np.asarray(value, np.float32))
        if a.shape != self._all:
            raise ValueError("params must be " + self._params_shape_text())
        self._set_rows(1, self.n_views, a)

    @property
    def grads(self):
        """f32, shaped like `params`: the last gradient written for each row, a TV term's included (zeros for a row no backward or train
        step has touched)."""
        return self._get(self._fn("get_grad"))

    def state(self, view):
        """(m1, m2 [*shape] of the moments' dtype, t) of row `view`: its Adam moments and step count."""
        import numpy as np
        m1, m2, t = np.empty(self.shape, self._moment_np), np.empty(self.shape, self._moment_np), C.c_uint32()
        p = C.POINTER(self._moment_c)
        self.ctx.check(self._fn("get_state")(self.ctx._h, self._h, *self._rows(view), m1.ctypes.data_as(p), m2.ctypes.data_as(p), C.byref(t)))
        return m1, m2, int(t.value)

    def set_state(self, view, m1, m2, t):
        """Puts a row's Adam state back (resuming from a checkpoint)."""
        a, b = self._moment(m1, "m1"), self._moment(m2, "m2")
        p = C.POINTER(self._moment_c)
        self.ctx.check(self._fn("set_state")(self.ctx._h, self._h, *self._rows(view), a.ctypes.data_as(p), b.ctypes.data_as(p), int(t)))

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):   # (a closed context has freed its tables)
                self._fn("destroy")(self.ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ExposureTable(_ParamTable):
    """A device table of one affine colour transform m[12] (row-major 3x4, column 3 the offset) per training view, with its Adam
    moments (f64) and update on the device (bh_exposure_*): y = A x + b on the rasterizer's image before the loss.  Views are numbered
    from 1 (row i is view id i + 1, as SceneLoader numbers them).  Nothing here reads back except the getters (`params`, `grads`
    [V,12] f32, `state` (m1 [12] f64, m2 [12] f64, t)).  SplatTrainer(exposure=table) attaches it to the train step.  Data parallel
    over cameras: the table is per process, nothing is all-reduced, a view must stay with one rank."""
    _prefix, _moment_np, _moment_c = "bh_exposure", "float64", C.c_double

    def __init__(self, n_views, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, ctx: Optional[Context] = None):
        self._open(ctx, n_views, (12,), (), lr, beta1, beta2, eps)

    def _params_shape_text(self):
        return "[%d, 12]" % self.n_views

    def _moment(self, m, what):
        import numpy as np
        return np.ascontiguousarray(m, np.float64).reshape(12)

    def set_view(self, view, m):
        """Row `view` (from 1) = the twelve floats m."""
        a = (C.c_float * 12)(*[float(v) for v in m])
        self.ctx.check(self.lib.bh_exposure_set_params(self.ctx._h, self._h, int(view), 1, a))

    def apply(self, view, img, out=None):
        """y = A x + b of `img` [H,W,4] f32 with row `view`; `out` may be `img` (in place)."""
        img = _aligned_hwc4(img, img.device)
        out = _hwc4_out(img, out)
        h, w = int(img.shape[0]), int(img.shape[1])
        self.ctx.check(self.lib.bh_exposure_apply(self.ctx._h, self._h, int(view), _ptr(img), h, w, _ptr(out)))
        return out

    def backward(self, view, img, v_exposed, update=False, out=None):
        """v_img = A^T v_exposed (`out` may be `v_exposed`), grads[view] = v_m of (img, v_exposed), and with `update` one Adam
        step of row `view` on it."""
        img = _aligned_hwc4(img, img.device)
        v = _aligned_hwc4(v_exposed, img.device)
        if v.shape != img.shape:
            raise ValueError("v_exposed must have the shape of img")
        out = _hwc4_out(img, out)
        h, w = int(img.shape[0]), int(img.shape[1])
        self.ctx.check(self.lib.bh_exposure_backward(self.ctx._h, self._h, int(view), _ptr(img), _ptr(v), h, w, _ptr(out), 1 if update else 0))
        return out


class EnvironmentMap(_ParamTable):
    """A learned cubemap E[6,R,R,3] f32 behind the splats (include/brush_hip_envmap.h): what the splats leave
    uncovered shows the map along the pixel's world ray, out = img + (1 - alpha) E(d), with the exact integer gradient to the table, its
    Adam moments (f32) and the update on the device.  Faces are +X, -X, +Y, -Y, +Z, -Z in world axes, the library's own table (no
    OpenGL flips); pinhole cameras only.  A new map is black.  Nothing here reads back except the getters (`params`, `grads`
    [6,R,R,3] f32, `state` (m1, m2 [6,R,R,3] f32, t)) and `backward`, which fetches four bytes to refuse a cotangent that is not
    finite.  SplatTrainer(envmap=map) attaches it to the train step."""
    _prefix, _moment_np, _moment_c, _per_view = "bh_envmap", "float32", C.c_float, False

    def __init__(self, resolution=64, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15, ctx: Optional[Context] = None):
        self.resolution = int(resolution)
        self._open(ctx, 1, (6, self.resolution, self.resolution, 3), (self.resolution,), lr, beta1, beta2, eps)

    def _params_shape_text(self):
        return "[6, %d, %d, 3]" % (self.resolution, self.resolution)

    def _moment(self, m, what):
        import numpy as np
        a = np.ascontiguousarray(np.asarray(m, np.float32))
        if a.shape != self.shape:
            raise ValueError("%s must be %s" % (what, self._params_shape_text()))
        return a

    def state(self):
        """(m1, m2 [6,R,R,3] f32, t): the Adam moments and the step count."""
        return super().state(1)

    def set_state(self, m1, m2, t):
        """Puts the Adam state back (resuming from a checkpoint)."""
        super().set_state(1, m1, m2, t)

    @staticmethod
    def _camera(camera, img):
        return camera if isinstance(camera, _ffi.BhCamera) else camera.uniforms((int(img.shape[1]), int(img.shape[0])))

    def composite(self, img, camera, out=None):
        """`img` [H,W,4] f32 (rendered on black) over the map as `camera` (a Camera or a BhCamera) sees it; `out` may be `img`."""
        img = _aligned_hwc4(img, img.device)
        out = _hwc4_out(img, out)
        cam = self._camera(camera, img)
        self.ctx.check(self.lib.bh_envmap_composite(self.ctx._h, self._h, C.byref(cam), _ptr(img), int(img.shape[0]), int(img.shape[1]), _ptr(out)))
        return out

    def backward(self, img, camera, v, update=False, out=None):
        """The gradient to the frame of the cotangent `v` on composite(img, camera) (`out` may be `v`), grads = v_E, and with
        `update` one Adam step of the table on it.  A `v` whose rgb holds a NaN or an infinity is refused and nothing is written."""
        img = _aligned_hwc4(img, img.device)
        v = _aligned_hwc4(v, img.device)
        if v.shape != img.shape:
            raise ValueError("v must have the shape of img")
        out = _hwc4_out(img, out)
        cam = self._camera(camera, img)
        self.ctx.check(self.lib.bh_envmap_backward(self.ctx._h, self._h, C.byref(cam), _ptr(img), _ptr(v), int(img.shape[0]), int(img.shape[1]), _ptr(out),
                                                   1 if update else 0))
        return out


class BilateralGridTable(_ParamTable):
    """A device table of one bilateral grid per training view: g[Hg,Wg,L,12] f32, a grid of row-major 3x4 colour matrices looked up
    by trilinear interpolation at (x, y, luminance) and applied to the rasterizer's image before the loss, with its Adam moments
    (f32) and update on the device (bh_bilagrid_*; gsplat's lib_bilagrid).  `grid` is (Wg, Hg, L), gsplat's (grid_X, grid_Y, grid_W).
    Views are numbered from 1.  Nothing here reads back except the getters (`params`, `grads` [V,Hg,Wg,L,12] f32, `state` (m1, m2
    [Hg,Wg,L,12] f32, t), and `tv` on request).  SplatTrainer(bilagrid=table) attaches it to the train step.  Data parallel over
    cameras: the table is per process, nothing is all-reduced, a view must stay with one rank."""
    _prefix, _moment_np, _moment_c = "bh_bilagrid", "float32", C.c_float

    def __init__(self, n_views, grid=(16, 16, 8), lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-15, ctx: Optional[Context] = None):
        self.grid_w, self.grid_h, self.grid_l = (int(v) for v in grid)
        self._open(ctx, n_views, (self.grid_h, self.grid_w, self.grid_l, 12), (self.grid_w, self.grid_h, self.grid_l), lr, beta1, beta2, eps)

    def _params_shape_text(self):
        return "%r" % ((self.n_views,) + self.shape,)

    def _moment(self, m, what):
        import numpy as np
        a = np.ascontiguousarray(m, np.float32)
        if a.shape != self.shape:
            raise ValueError("moments must be %r" % (self.shape,))
        return a

    def set_view(self, view, g):
        """The grid of `view` (from 1) = g [Hg,Wg,L,12]."""
        import numpy as np
        a = np.ascontiguousarray(np.asarray(g, np.float32))
        if a.shape != self.shape:
            raise ValueError("a view's grid must be %r" % (self.shape,))
        self._set_rows(view, 1, a)

    def slice(self, view, img, out=None):
        """y = A(x, y, luminance) x of `img` [H,W,4] f32 with the grid of `view`; `out` may be `img` (in place)."""
        img = _aligned_hwc4(img, img.device)
        out = _hwc4_out(img, out)
        h, w = int(img.shape[0]), int(img.shape[1])
        self.ctx.check(self.lib.bh_bilagrid_slice(self.ctx._h, self._h, int(view), _ptr(img), h, w, _ptr(out)))
        return out

    def backward(self, view, img, v_sliced, tv_weight=0.0, update=False, out=None):
        """v_img of the cotangent `v_sliced` (`out` may be `v_sliced`), grads[view] = v_g of (img, v_sliced) + tv_weight dTV/dg, and
        with `update` one Adam step of the grid of `view` on it."""
        img = _aligned_hwc4(img, img.device)
        v = _aligned_hwc4(v_sliced, img.device)
        if v.shape != img.shape:
            raise ValueError("v_sliced must have the shape of img")
        out = _hwc4_out(img, out)
        h, w = int(img.shape[0]), int(img.shape[1])
        self.ctx.check(self.lib.bh_bilagrid_backward(self.ctx._h, self._h, int(view), _ptr(img), _ptr(v), h, w, _ptr(out), float(tv_weight),
                                                     1 if update else 0))
        return out

    def tv(self, view, out=None):
        """The total variation of the grid of `view` as a device tensor of one f32 (`out`, or a new one on the ctx's device)."""
        if out is None:
            out = torch.empty(1, dtype=torch.float32, device=self.ctx.device)
        self.ctx.check(self.lib.bh_bilagrid_tv(self.ctx._h, self._h, int(view), _ptr(out)))
        return out

    def to_gsplat(self):
        """Every grid in gsplat's layout: grids[v, k, l, j, i] = g[v][j][i][l][k], a [V,12,L,Hg,Wg] f32 numpy array."""
        import numpy as np
        return np.ascontiguousarray(self.params.transpose(0, 4, 3, 1, 2))

    def from_gsplat(self, grids):
        """Sets every grid from gsplat's BilateralGrid.grids [V,12,L,Hg,Wg] (a numpy array or a tensor)."""
        import numpy as np
        a = np.asarray(grids.detach().cpu().numpy() if hasattr(grids, "detach") else grids, np.float32)
        if a.shape != (self.n_views, 12, self.grid_l, self.grid_h, self.grid_w):
            raise ValueError("grids must be [%d, 12, %d, %d, %d]" % (self.n_views, self.grid_l, self.grid_h, self.grid_w))
        self.params = a.transpose(0, 3, 4, 2, 1)


# ---------------------------------------------------------------------------
# PLY at the edges (brush-serde)
# ---------------------------------------------------------------------------
def splat_to_ply(splats: Splats, up_axis=None, ctx: Optional[Context] = None) -> bytes:
    """splat_to_ply (brush-serde/src/export.rs:179-204): the INRIA-layout binary PLY, rows packed on the
    device (3D-filter floor baked, quaternions normalised, SH permuted to [channel][coeff])."""
    ctx = ctx or get_context(splats.device)
    n = splats.num_splats()
    up = (C.c_float * 3)(*[float(v) for v in up_axis]) if up_axis is not None else None
    need = C.c_uint64(0)
    args = (_ptr(splats.transforms), _ptr(splats.sh_coeffs), _ptr(splats.raw_opacities),
            _ptr(splats.min_scale) if splats.min_scale is not None else None, n, splats.sh_degree(), int(splats.render_mip), up)
    ctx.check(ctx.lib.bh_splat_to_ply(ctx._h, *args, None, 0, C.byref(need)))
    buf = (C.c_char * need.value)()
    ctx.check(ctx.lib.bh_splat_to_ply(ctx._h, *args, buf, need.value, C.byref(need)))
    return bytes(buf)


def splat_to_compressed_ply(splats: Splats, up_axis=None, ctx: Optional[Context] = None, return_order=False):
    """The splats as a SuperSplat / PlayCanvas compressed.ply (include/brush_hip_compressed_ply.h), the format
    load_splat_from_ply reads back: Morton-ordered rows, per-256-row chunk ranges, 16 B per splat + 3K bytes of SH.  The 3D-filter
    floor is baked first, as in splat_to_ply.  return_order: also the file row -> input row map (int32 [N] device)."""
    ctx = ctx or get_context(splats.device)
    n = splats.num_splats()
    up = (C.c_float * 3)(*[float(v) for v in up_axis]) if up_axis is not None else None
    order = torch.empty((n,), dtype=torch.int32, device=splats.device) if return_order else None
    need = C.c_uint64(0)
    args = (_ptr(splats.transforms), _ptr(splats.sh_coeffs), _ptr(splats.raw_opacities),
            _ptr(splats.min_scale) if splats.min_scale is not None else None, n, splats.sh_degree(), int(splats.render_mip), up,
            _ptr(order) if order is not None and n else None)
    ctx.check(ctx.lib.bh_splat_to_compressed_ply(ctx._h, *args, None, 0, C.byref(need)))
    buf = (C.c_char * need.value)()
    ctx.check(ctx.lib.bh_splat_to_compressed_ply(ctx._h, *args, buf, need.value, C.byref(need)))
    return (bytes(buf), order) if return_order else bytes(buf)


@dataclass
class ParseMetadata:
    """brush-serde/src/import.rs:19-24"""
    up_axis: Optional[Tuple[float, float, float]]
    render_mode: Optional[str]
    total_splats: int
    sh_degree: int
    compressed: bool = False   # a SuperSplat-compressed file (import.rs:244-250, 407-600)


def ply_parse_header(data: bytes) -> ParseMetadata:
    """Header of a splat PLY (host only; no GPU needed)."""
    info = _ffi.BhPlyInfo()
    rc = _ffi.load().bh_ply_parse_header(data, len(data), C.byref(info))
    if rc != 0:
        raise BrushHipError("unsupported PLY (%d): only binary_little_endian float vertex rows (or SuperSplat-compressed chunks) are read" % rc
                            if rc == -5 else "malformed PLY (%d)" % rc)
    return ParseMetadata(tuple(info.up_axis) if info.has_up_axis else None, {0: "default", 1: "mip"}.get(info.render_mode), int(info.num_splats),
                         int(info.sh_degree), bool(info.compressed))


def load_splat_from_ply(data: bytes, device=None, render_mip=None, ctx: Optional[Context] = None, subsample_points: Optional[int] = None,
                        max_splats: Optional[int] = None):
    """load_splat_from_ply + SplatData::into_splats (import.rs:166-181, 77-97) -> (Splats, ParseMetadata).
    render_mip None = take the file's SplatRenderMode comment (default mode when absent).
    subsample_points = s keeps every s-th row (rows s-1, 2s-1, ...: import.rs:346-349); max_splats then applies
    SplatData::subsample (import.rs:49-74: rows 0, step, 2 step, ... with step = ceil(n / max_splats); 0 / None = no cap), as
    the training stream does (brush-process/src/train_stream.rs:111).  meta.total_splats is the number of rows kept."""
    meta = ply_parse_header(data)
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    ctx = ctx or get_context(device)
    s = int(subsample_points or 1)
    if s < 1:
        raise BrushHipError("subsample_points must be >= 1")
    first, step, n = s - 1, s, meta.total_splats // s
    if max_splats and n > max_splats:
        step2 = -(-n // int(max_splats))
        n, step = -(-n // step2), step * step2
    c = (meta.sh_degree + 1) ** 2
    tr = torch.empty((n, 10), dtype=torch.float32, device=device)
    sh = torch.empty((n, c, 3), dtype=torch.float32, device=device)
    op = torch.empty((n,), dtype=torch.float32, device=device)
    ctx.check(ctx.lib.bh_splats_from_ply_strided(ctx._h, data, len(data), first, step, n, _ptr(tr), _ptr(sh), _ptr(op)))
    mip = (meta.render_mode == "mip") if render_mip is None else bool(render_mip)
    meta.total_splats = n
    return Splats(tr, sh, op, mip, device), meta


# ---------------------------------------------------------------------------
# primitives
# ---------------------------------------------------------------------------
def _as_u32(t, device):
    t = torch.as_tensor(t, device=device)
    if t.dtype not in (torch.int32, torch.uint32):
        t = t.to(torch.int64).to(torch.int32) if t.dtype != torch.int64 else (t & 0xFFFFFFFF).to(torch.int32)
    return t.contiguous()


def radix_argsort(keys, values=None, sorting_bits=32, ctx: Optional[Context] = None):
    """Stable argsort of u32 keys (int32 bit patterns) on their low `sorting_bits`
    bits; returns (sorted_keys, sorted_values). brush-sort/src/lib.rs:16-33 asserts."""
    dev = keys.device if isinstance(keys, torch.Tensor) and keys.is_cuda else torch.device("cuda", torch.cuda.current_device())
    ctx = ctx or get_context(dev)
    k = _as_u32(keys, dev)
    if k.dim() != 1:
        raise BrushHipError("radix_argsort: keys must be 1-D")
    v = None
    if values is not None:
        v = _as_u32(values, dev)
        if v.shape != k.shape:
            raise BrushHipError("radix_argsort: input keys and values must have the same number of elements")
    if sorting_bits > 32:
        raise BrushHipError("radix_argsort: can only sort up to 32 bits")
    ok, ov = torch.empty_like(k), torch.empty_like(k)
    ctx.check(ctx.lib.bh_radix_argsort(ctx._h, _ptr(k), _ptr(v) if v is not None else None, k.numel(), int(sorting_bits), _ptr(ok), _ptr(ov)))
    return ok, ov


def tile_sort_offsets(tile_ids, compact_gids, num_tiles: int, ctx: Optional[Context] = None):
    """The forward's tile sort + offsets table as one operator (render.rs:228-243 + get_tile_offset.rs:11-58): (tile id, compact
    splat id) pairs in depth order -> (tile_ids_sorted, compact_gids_sorted, tile_offsets [num_tiles, 2]); stable."""
    dev = tile_ids.device if isinstance(tile_ids, torch.Tensor) and tile_ids.is_cuda else torch.device("cuda", torch.cuda.current_device())
    ctx = ctx or get_context(dev)
    k, v = _as_u32(tile_ids, dev), _as_u32(compact_gids, dev)
    if k.dim() != 1 or v.shape != k.shape:
        raise BrushHipError("tile_sort_offsets: tile ids and splat ids must be 1-D and of the same length")
    ok, ov = torch.empty_like(k), torch.empty_like(k)
    offs = torch.empty((int(num_tiles), 2), dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.bh_tile_sort_offsets(ctx._h, _ptr(k), _ptr(v), k.numel(), int(num_tiles), _ptr(ok), _ptr(ov), _ptr(offs)))
    return ok, ov, offs


def prefix_sum(x, ctx: Optional[Context] = None):
    """Inclusive u32 prefix sum (brush-prefix-sum/src/lib.rs:11)."""
    dev = x.device if isinstance(x, torch.Tensor) and x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    ctx = ctx or get_context(dev)
    a = _as_u32(x, dev)
    o = torch.empty_like(a)
    ctx.check(ctx.lib.bh_prefix_sum(ctx._h, _ptr(a), a.numel(), _ptr(o)))
    return o


def _loss_cfg(l1_weight, ssim_weight, composite_bg, mask):
    cfg = _ffi.BhLossConfig()
    cfg.l1_weight, cfg.ssim_weight = float(l1_weight), float(ssim_weight)
    bg = composite_bg if composite_bg is not None else (0.0, 0.0, 0.0)
    cfg.bg[0], cfg.bg[1], cfg.bg[2] = [float(b) for b in bg]
    cfg.composite_bg = 1 if composite_bg is not None else 0
    cfg.mask = 1 if mask else 0
    return cfg


def image_loss(pred_hwc, gt_packed, l1_weight=0.8, ssim_weight=-0.2, composite_bg=None, mask=False, ctx: Optional[Context] = None):
    """Per-pixel l1_w*|pred-gt| + ssim_w*SSIM loss map [H,W,C] (C=3, or 4 with the
    alpha-match plane); gt_packed [H,W] rgba8 as int32. brush-loss/src/lib.rs:1075-1104."""
    dev = pred_hwc.device
    ctx = ctx or get_context(dev)
    h, w, c = pred_hwc.shape
    pred_chw = pred_hwc.permute(2, 0, 1).contiguous().float()  # lib.rs:1076
    gt = _as_u32(gt_packed, dev).reshape(h, w)
    out = torch.empty_like(pred_chw)
    cfg = _loss_cfg(l1_weight, ssim_weight, composite_bg, mask)
    ctx.check(ctx.lib.bh_image_loss_forward(ctx._h, _ptr(pred_chw), _ptr(gt), c, h, w, C.byref(cfg), _ptr(out)))
    return out.permute(1, 2, 0).contiguous()


def image_loss_backward(pred_hwc, gt_packed, dl_dmap_hwc, l1_weight=0.8, ssim_weight=-0.2, composite_bg=None, mask=False,
                        ctx: Optional[Context] = None):
    dev = pred_hwc.device
    ctx = ctx or get_context(dev)
    h, w, c = pred_hwc.shape
    pred_chw = pred_hwc.permute(2, 0, 1).contiguous().float()
    dl = dl_dmap_hwc.permute(2, 0, 1).contiguous().float()
    gt = _as_u32(gt_packed, dev).reshape(h, w)
    out = torch.empty_like(pred_chw)
    cfg = _loss_cfg(l1_weight, ssim_weight, composite_bg, mask)
    ctx.check(ctx.lib.bh_image_loss_backward(ctx._h, _ptr(pred_chw), _ptr(gt), _ptr(dl), c, h, w, C.byref(cfg), _ptr(out)))
    return out.permute(1, 2, 0).contiguous()


def image_loss_value_and_grad(img_hwc4, gt_packed, l1_weight=0.8, ssim_weight=-0.2, composite_bg=None, mask=False,
                              alpha_weight=0.0, ctx: Optional[Context] = None):
    """Fused train-step loss: returns (loss [1] device tensor, dloss/dimg [H,W,4]).  Equivalent to
    mean(image_loss(...)) (+ alpha term) and its gradient (train.rs:227-260), in two kernels."""
    dev = img_hwc4.device
    ctx = ctx or get_context(dev)
    h, w, c = img_hwc4.shape
    if c != 4:
        raise ValueError("img must be [H,W,4]")
    img = img_hwc4.contiguous().float()
    gt = _as_u32(gt_packed, dev).reshape(h, w)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    v_out = torch.empty_like(img)
    cfg = _loss_cfg(l1_weight, ssim_weight, composite_bg, mask)
    ctx.check(ctx.lib.bh_image_loss_value_and_grad(ctx._h, _ptr(img), _ptr(gt), h, w, C.byref(cfg), float(alpha_weight), _ptr(loss), _ptr(v_out)))
    return loss, v_out


def gather_stats(refine_weight_norm, vis_weight, max_screen_size, refine_weight, visible, screen_radius, ctx: Optional[Context] = None):
    """RefineRecord::gather_stats (brush-train/src/stats.rs:40-50), in place on the three running [N] tensors: maxima of the refine
    weight and the screen radius, sum of the visibility flags."""
    ctx = ctx or get_context(refine_weight.device)
    n = refine_weight.numel()
    ctx.check(ctx.lib.bh_gather_stats(ctx._h, _ptr(refine_weight_norm), _ptr(vis_weight), _ptr(max_screen_size), _ptr(refine_weight), _ptr(visible),
                                      _ptr(screen_radius), n))


def adam_step(param, grad, m1, m2, lr, t, col_scale=None, reduce_m2=False, beta1=0.9, beta2=0.999, eps=1e-15, ctx: Optional[Context] = None):
    """In-place AdamScaled step on a [rows, ...] parameter (adam_scaled.rs:75-147)."""
    ctx = ctx or get_context(param.device)
    rows = param.shape[0]
    row_len = param.numel() // rows if rows else 1
    ctx.check(ctx.lib.bh_adam_step(ctx._h, _ptr(param), _ptr(grad), _ptr(m1), _ptr(m2), rows, row_len,
                                   _ptr(col_scale) if col_scale is not None else None, float(lr), int(t), int(bool(reduce_m2)),
                                   float(beta1), float(beta2), float(eps)))


# ---------------------------------------------------------------------------
# training (brush-train)
# ---------------------------------------------------------------------------
@dataclass
class TrainConfig:
    """Subset of brush-train/src/config.rs:7-132 that defines step(); same defaults."""
    total_train_iters: int = 30000
    lr_mean: float = 2e-5
    lr_mean_end: float = 2e-7
    lr_coeffs_dc: float = 2e-3
    lr_coeffs_sh_scale: float = 10.0
    lr_opac: float = 0.012
    lr_scale: float = 5e-3
    lr_rotation: float = 2e-3
    ssim_weight: float = 0.2
    match_alpha_weight: float = 0.1
    mean_noise_weight: float = 50.0
    background_color: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    background_noise_strength: float = 0.1
    render_mip: bool = False
    # not in the reference: False = the step's forward builds depth-sliced per-tile lists (BH_FLAG_SLICED_LISTS, same results);
    # True = the reference's full lists
    exact_lists: bool = False
    # refine options (config.rs:47-86)
    max_splats: int = 10_000_000
    refine_every: int = 200
    growth_grad_threshold: float = 0.0025
    growth_select_fraction: float = 0.25
    growth_stop_iter: int = 15000
    split_at_screen_size: float = 0.5
    opac_decay: float = 0.004
    # config.rs:92: > 0 adds lpips_loss_weight * LPIPS(pred, GT) to the loss; needs SplatTrainer(..., lpips=Lpips)
    lpips_loss_weight: float = 0.0
    # not in the reference: > 0 adds the depth term (brush_hip_depth_loss.h) for batches that carry a depth map; the weight goes
    # from depth_loss_weight to depth_loss_weight_end (None: constant) over total_train_iters on lr_mean's exponential curve
    depth_loss_weight: float = 0.0
    depth_loss_weight_end: Optional[float] = None
    depth_loss_kind: str = "l1"   # "l1": SceneBatch.depth holds depth; "disparity": it holds inverse depth
    # not in the reference: > 0 adds the normal-consistency term (brush_hip_normal_loss.h; 2DGS's regulariser) from step
    # normal_loss_from_iter on (2DGS starts it at 7000); pinhole cameras, whole frames
    normal_loss_weight: float = 0.0
    normal_loss_from_iter: int = 0
    # not in the reference: > 0 adds the distortion term (brush_hip_distortion.h; 2DGS's depth distortion, its companion regulariser)
    # from step distortion_loss_from_iter on (2DGS starts it at 3000); kind "z", or "ndc" with distortion_near / distortion_far
    distortion_loss_weight: float = 0.0
    distortion_loss_from_iter: int = 0
    distortion_kind: str = "z"
    distortion_near: float = 0.2
    distortion_far: float = 1000.0
    # not in the reference: > 0 adds the feature term (brush_hip_feature_train.h) from step feature_loss_from_iter on, for batches that
    # carry a feature target; needs SplatTrainer(..., feature_field=FeatureField); kind "l1" or "cross_entropy"
    feature_loss_weight: float = 0.0
    feature_loss_kind: str = "l1"
    feature_loss_from_iter: int = 0

    def depth_weight_at(self, step: int) -> float:
        """The depth term's weight at step `step` (from 1): w0 * (w1 / w0) ** ((step - 1) / total_train_iters)."""
        w0 = float(self.depth_loss_weight)
        w1 = w0 if self.depth_loss_weight_end is None else float(self.depth_loss_weight_end)
        if w0 <= 0.0 or w1 <= 0.0 or w1 == w0:
            return w0
        return w0 * (w1 / w0) ** ((int(step) - 1) / float(self.total_train_iters))


@dataclass
class RefineStats:
    """brush-train/src/msg.rs RefineStats (+ the number of splits drawn to refill the pruned budget)."""
    num_added: int
    num_split_oversized: int
    num_split_high_grad: int
    num_pruned: int
    num_pruned_non_finite: int
    total_splats: int
    num_resampled: int = 0


BOUND_PERCENTILE = 0.8  # train.rs:30


def splat_bounds(splats, percentile=BOUND_PERCENTILE, ctx=None):
    """get_splat_bounds (train.rs:124-133, splat_init.rs:130-160): (center[3], extent[3]) of the
    per-axis percentile box of the means."""
    ctx = ctx or get_context(splats.device)
    c, e = (C.c_float * 3)(), (C.c_float * 3)()
    ctx.check(ctx.lib.bh_splat_bounds(ctx._h, _ptr(splats.transforms), splats.num_splats(), float(percentile), c, e))
    return tuple(c), tuple(e)


def bounds_median_size(extent):
    """BoundingBox::median_size (bounding_box.rs:23-29)."""
    return sorted(float(x) for x in extent)[1] * 2.0


# ---------------------------------------------------------------------------
# Mesh extraction: TSDF fusion of depth maps, marching tetrahedra, mesh PLY (include/brush_hip_mesh.h)
# ---------------------------------------------------------------------------
def mesh_to_ply(vertices, triangles, colours=None, ctx: Optional[Context] = None) -> bytes:
    """A triangle mesh (vertices [V,3] f32, triangles [M,3] indices, colours [V,3] f32 in [0,1] or None) as a binary little-endian
    PLY (bh_mesh_to_ply): rows packed on the device, one device-to-host copy."""
    dev = vertices.device
    ctx = ctx or get_context(dev)
    vertices = _f32c(vertices, dev).reshape(-1, 3)
    n_v = vertices.shape[0]
    if colours is not None:
        colours = _f32c(colours, dev).reshape(-1, 3)
        if colours.shape[0] != n_v:
            raise ValueError("mesh_to_ply: %d colours for %d vertices" % (colours.shape[0], n_v))
    triangles = torch.as_tensor(triangles, device=dev)
    if triangles.dtype != torch.int32:
        triangles = triangles.to(torch.int32)
    triangles = triangles.contiguous().reshape(-1, 3)
    args = (_ptr(vertices), _ptr(colours) if colours is not None else None, n_v, _ptr(triangles), triangles.shape[0])
    need = C.c_uint64(0)
    ctx.check(ctx.lib.bh_mesh_to_ply(ctx._h, *args, None, 0, C.byref(need)))
    buf = (C.c_char * need.value)()
    ctx.check(ctx.lib.bh_mesh_to_ply(ctx._h, *args, buf, need.value, C.byref(need)))
    return bytes(buf)


class _TsdfVolumeBase:
    """What TsdfVolume and SparseTsdfVolume share: the fields and their refusals, from_bounds, the packing of views, and clear /
    integrate / count / extract_mesh / to_ply over the subclass's struct (`_struct()`) and the prefix of its entry points (`_ENTRY`).
    A subclass adds its size limit (`_check_size`) and its buffers."""

    def __init__(self, origin, voxel_size, dims, trunc, max_weight, device, ctx):
        name = type(self).__name__
        self.origin = tuple(float(v) for v in origin)
        self.voxel_size = float(voxel_size)
        self.dims = tuple(int(v) for v in dims)
        self.trunc = 4.0 * self.voxel_size if trunc is None else float(trunc)
        self.max_weight = float(max_weight)
        # refused here, before the device is touched (the library refuses the same)
        if len(self.origin) != 3 or len(self.dims) != 3:
            raise ValueError("%s: origin and dims have three entries" % name)
        if min(self.dims) < 2:
            raise ValueError("%s: every dimension must be at least 2" % name)
        self._check_size(name)
        if not (math.isfinite(self.voxel_size) and self.voxel_size > 0.0):
            raise ValueError("%s: voxel_size must be a finite number > 0" % name)
        if not (math.isfinite(self.trunc) and self.trunc > 0.0):
            raise ValueError("%s: trunc must be a finite number > 0" % name)
        if not self.max_weight >= 1.0:
            raise ValueError("%s: max_weight must be at least 1" % name)
        self.ctx = ctx or get_context(device)
        self.device = self.ctx.device

    @classmethod
    def from_bounds(cls, bounds, resolution, **kw):
        """A volume over the box bounds = (center[3], extent[3]) (half sizes, as splat_bounds returns them) with `resolution`
        samples along its longest side and cubic voxels."""
        center, extent = bounds
        resolution = int(resolution)
        if resolution < 2:
            raise ValueError("TsdfVolume.from_bounds: resolution must be at least 2")
        voxel = 2.0 * max(float(e) for e in extent) / (resolution - 1)
        if not voxel > 0.0:
            raise ValueError("TsdfVolume.from_bounds: an empty box")
        dims = tuple(max(2, int(math.ceil(2.0 * float(e) / voxel)) + 1) for e in extent)
        origin = tuple(float(c) - 0.5 * voxel * (d - 1) for c, d in zip(center, dims))
        return cls(origin, voxel, dims, **kw)

    def _committed(self, who):
        """Raises where the volume cannot take the call `who` yet (a sparse volume before its commit)."""

    def _call(self, entry, *args):
        s = self._struct()
        self.ctx.check(getattr(self.ctx.lib, self._ENTRY + entry)(self.ctx._h, C.byref(s), *args))

    def _views(self, depths, cameras, images, who):
        depths, cameras = list(depths), list(cameras)
        if len(depths) != len(cameras) or (images is not None and len(images) != len(depths)):
            raise ValueError("%s.%s: as many cameras (and images) as depth maps" % (type(self).__name__, who))
        n = len(depths)
        cams = TsdfVolume.check_views(cameras, [tuple(d.shape) for d in depths])
        dev = self.device
        depths = [_f32c(d, dev) for d in depths]
        dptr = (C.c_void_p * max(n, 1))(*[d.data_ptr() for d in depths])
        iptr = None
        if images is not None:
            images = [_f32c(im, dev).reshape(d.shape[0], d.shape[1], 4) for im, d in zip(images, depths)]
            iptr = (C.c_void_p * max(n, 1))(*[im.data_ptr() for im in images])
        return n, cams, dptr, iptr, (depths, images)   # (the last entry keeps the converted tensors alive across the call)

    def clear(self):
        """T = 1, W = 0, rgb = 0 in every sample held (a sparse volume: and keys from the index)."""
        self._committed("clear")
        self._call("clear")

    def integrate(self, depths, cameras, images=None, depth_min=0.0, depth_max=math.inf, alpha_min=0.5):
        """Fuses depths[v] [H,W] f32 (z-depth, 0 = none) seen by cameras[v] (Camera or BhCamera, pinhole) into the volume, in order;
        images[v] [H,W,4] f32 gives the alpha test and, with colour, the colour.  Queued: nothing is read back.  A sparse volume fuses
        into its allocated blocks: every allocated sample ends with the bits the dense volume would hold."""
        self._committed("integrate")
        n, cams, dptr, iptr, keep = self._views(depths, cameras, images, "integrate")
        if n == 0:
            return
        cfg = _ffi.BhTsdfIntegrateConfig(float(depth_min), float(depth_max), float(alpha_min), 0)
        self._call("integrate", n, cams, dptr, iptr, C.byref(cfg))

    def count(self):
        """(n_vertices, n_triangles) of the zero level set (bh_tsdf_extract_count / bh_sptsdf_extract_count; blocking)."""
        self._committed("count")
        nv, nt = C.c_uint32(), C.c_uint32()
        self._call("extract_count", C.byref(nv), C.byref(nt))
        return int(nv.value), int(nt.value)

    def extract_mesh(self):
        """(vertices [V,3] f32, colours [V,3] f32 or None, triangles [M,3] int32) on the device: marching tetrahedra at the zero level
        over the cubes whose eight corners were observed; counter-clockwise seen from outside, deterministic.  A sparse volume's
        vertices come in pool order (by block key, then by the sample's index in its block)."""
        n_v, n_t = self.count()
        dev = self.device
        vertices = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
        colours = torch.empty((n_v, 3), dtype=torch.float32, device=dev) if self.rgb is not None else None
        triangles = torch.empty((n_t, 3), dtype=torch.int32, device=dev)
        nv, nt = C.c_uint32(), C.c_uint32()
        self._call("extract", _ptr(vertices), _ptr(colours) if colours is not None else None, _ptr(triangles), n_v, n_t, C.byref(nv), C.byref(nt))
        return vertices, colours, triangles

    def to_ply(self) -> bytes:
        vertices, colours, triangles = self.extract_mesh()
        return mesh_to_ply(vertices, triangles, colours, ctx=self.ctx)


class TsdfVolume(_TsdfVolumeBase):
    """A dense truncated signed distance volume on the device (include/brush_hip_mesh.h): `dims` = (nx, ny, nz) samples at
    origin + voxel_size * (i, j, k), x fastest.  `tw` [nz,ny,nx,2] f32 holds {tsdf in units of trunc, weight}, `rgb` [nz,ny,nx,3] the
    mean colour (None with colour=False).  integrate() fuses depth maps (KinectFusion's running mean, up to 8 views per launch),
    extract_mesh() is marching tetrahedra at the zero level, to_ply() the mesh as a PLY file."""
    _ENTRY = "bh_tsdf_"

    def __init__(self, origin, voxel_size, dims, trunc=None, max_weight=64.0, colour=True, device=None, ctx: Optional[Context] = None):
        super().__init__(origin, voxel_size, dims, trunc, max_weight, device, ctx)
        nx, ny, nz = self.dims
        self.tw = torch.empty((nz, ny, nx, 2), dtype=torch.float32, device=self.device)
        self.rgb = torch.empty((nz, ny, nx, 3), dtype=torch.float32, device=self.device) if colour else None
        self.clear()

    def _check_size(self, name):
        if self.dims[0] * self.dims[1] * self.dims[2] > 2 ** 31 - 1:
            raise ValueError("%s: more than 2^31 - 1 samples" % name)

    def grid(self) -> "_ffi.BhTsdfGrid":
        g = _ffi.BhTsdfGrid()
        g.origin = (C.c_float * 3)(*self.origin)
        g.voxel_size = self.voxel_size
        g.nx, g.ny, g.nz = self.dims
        g.trunc, g.max_weight, g.reserved = self.trunc, self.max_weight, 0
        g.tw = self.tw.data_ptr()
        g.rgb = self.rgb.data_ptr() if self.rgb is not None else None
        return g

    _struct = grid

    @staticmethod
    def check_views(cameras, shapes):
        """The BhCamera array of `cameras` for depth maps of `shapes` [(H, W), ...]; ValueError for what bh_tsdf_integrate refuses
        (a lens model other than the pinhole, a tile-row window, a camera of another size), before the device is touched."""
        cams = (_ffi.BhCamera * len(cameras))()
        for v, (cam, shape) in enumerate(zip(cameras, shapes)):
            if len(shape) != 2:
                raise ValueError("TsdfVolume.integrate: a depth map must be [H, W]")
            cams[v] = _camera_of(cam, shape)
            if cams[v].model != _ffi.CAMERA_PINHOLE:
                raise ValueError("TsdfVolume.integrate: pinhole cameras only")
            if cams[v].tile_row_begin != 0 or cams[v].tile_row_end != 0:
                raise ValueError("TsdfVolume.integrate: a camera with a tile-row window")
            if (cams[v].img_h, cams[v].img_w) != tuple(shape):
                raise ValueError("TsdfVolume.integrate: camera %d is %dx%d, its depth map %dx%d" % (v, cams[v].img_w, cams[v].img_h, shape[1], shape[0]))
        return cams


class SparseTsdfVolume(_TsdfVolumeBase):
    """A sparse truncated signed distance volume on the device (include/brush_hip_sparse_mesh.h): a virtual grid of
    `dims` = (nx, ny, nz) samples (each 2 .. 8192) at origin + voxel_size * (i, j, k), of which only the 8x8x8 blocks near the observed
    surfaces are held.  mark() sets the blocks the depth maps' rays cross inside the truncation band, commit() dilates them, counts
    them and allocates the pool (`keys` [n_blocks], `tw` [n_blocks,8,8,8,2], `rgb` [n_blocks,8,8,8,3] or None), integrate() fuses depth
    maps by TsdfVolume's rule, extract_mesh() / to_ply() are TsdfVolume's, to_dense() writes a window into a TsdfVolume."""
    _ENTRY = "bh_sptsdf_"

    def __init__(self, origin, voxel_size, dims, trunc=None, max_weight=64.0, colour=True, device=None, ctx: Optional[Context] = None):
        super().__init__(origin, voxel_size, dims, trunc, max_weight, device, ctx)
        self.colour = bool(colour)
        self.n_words = (self.block_dims[0] * self.block_dims[1] * self.block_dims[2] + 31) // 32
        self.bits = torch.zeros(self.n_words, dtype=torch.int32, device=self.device)
        self.rank = torch.zeros(self.n_words, dtype=torch.int32, device=self.device)
        self.n_blocks = 0
        self.keys = self.tw = self.rgb = None

    def _check_size(self, name):
        if max(self.dims) > _ffi.SPTSDF_MAX_DIM:
            raise ValueError("%s: a dimension above %d" % (name, _ffi.SPTSDF_MAX_DIM))
        self.block_dims = tuple((d + _ffi.SPTSDF_BLOCK - 1) // _ffi.SPTSDF_BLOCK for d in self.dims)
        if self.block_dims[0] * self.block_dims[1] * self.block_dims[2] > 2 ** 30:
            raise ValueError("%s: more than 2^30 virtual blocks" % name)

    def mark_steps(self) -> int:
        """M of bh_sptsdf_mark: the smallest integer with (float)M * (4 voxel_size) >= 2 trunc, in f32."""
        import numpy as np
        step, band = np.float32(4.0) * np.float32(self.voxel_size), np.float32(2.0) * np.float32(self.trunc)
        m = 0
        while m <= _ffi.SPTSDF_MAX_STEPS and not np.float32(m) * step >= band:
            m += 1
        return m

    def vol(self) -> "_ffi.BhSparseTsdf":
        v = _ffi.BhSparseTsdf()
        v.origin = (C.c_float * 3)(*self.origin)
        v.voxel_size = self.voxel_size
        v.nx, v.ny, v.nz = self.dims
        v.trunc, v.max_weight, v.n_blocks = self.trunc, self.max_weight, self.n_blocks
        v.bits, v.rank = self.bits.data_ptr(), self.rank.data_ptr()
        v.keys = self.keys.data_ptr() if self.keys is not None else None
        v.tw = self.tw.data_ptr() if self.tw is not None else None
        v.rgb = self.rgb.data_ptr() if self.rgb is not None else None
        return v

    _struct = vol

    def _committed(self, who):
        if self.n_blocks == 0:
            raise ValueError("SparseTsdfVolume.%s: the volume has no blocks: mark() and commit() first" % who)

    def mark_clear(self):
        """Forgets every mark and the committed pool: the volume is as new."""
        self.n_blocks = 0
        self.keys = self.tw = self.rgb = None
        self._call("mark_clear")

    def mark(self, depths, cameras, images=None, depth_max=math.inf, alpha_min=0.5):
        """Marks the blocks that the rays of depths[v] [H,W] cross within trunc of the depth (bh_sptsdf_mark); any number of calls
        before commit().  Queued: nothing is read back."""
        if self.n_blocks:
            raise ValueError("SparseTsdfVolume.mark: after a commit: mark_clear() first")
        if self.mark_steps() > _ffi.SPTSDF_MAX_STEPS:
            raise ValueError("SparseTsdfVolume.mark: trunc is more than %d steps of 4 voxels" % _ffi.SPTSDF_MAX_STEPS)
        n, cams, dptr, iptr, keep = self._views(depths, cameras, images, "mark")
        if n == 0:
            return
        cfg = _ffi.BhTsdfIntegrateConfig(0.0, float(depth_max), float(alpha_min), 0)
        self._call("mark", n, cams, dptr, iptr, C.byref(cfg))

    def commit(self, dilate=1) -> int:
        """Allocates every block within `dilate` (0, 1 or 2) blocks of a marked one, and clears the pool; -> the number of blocks
        (0: nothing was marked, and the volume stays without a pool).  Blocking (one readback)."""
        if isinstance(dilate, bool) or int(dilate) != dilate or not 0 <= int(dilate) <= 2:
            raise ValueError("SparseTsdfVolume.commit: dilate must be 0, 1 or 2")
        if self.n_blocks:
            raise ValueError("SparseTsdfVolume.commit: already committed: mark_clear() starts over")
        n = C.c_uint32()
        self._call("commit", int(dilate), C.byref(n))
        n = int(n.value)
        if n:
            self.keys = torch.empty(n, dtype=torch.int32, device=self.device)
            self.tw = torch.empty((n, 8, 8, 8, 2), dtype=torch.float32, device=self.device)
            self.rgb = torch.empty((n, 8, 8, 8, 3), dtype=torch.float32, device=self.device) if self.colour else None
            self.n_blocks = n
            self.clear()
        return n

    def to_dense(self, start=(0, 0, 0), dims=None, colour=None) -> TsdfVolume:
        """The window of the virtual grid from sample `start`, `dims` samples wide (default: to the end of the grid), as a TsdfVolume:
        allocated samples bit for bit, T = 1, W = 0, rgb = 0 elsewhere (bh_sptsdf_to_dense).  The dense volume's origin is
        origin + voxel_size * start, so only a window from (0, 0, 0) is guaranteed to place its samples on the same f32 positions."""
        self._committed("to_dense")
        start = tuple(int(v) for v in start)
        if len(start) != 3 or min(start) < 0 or any(s >= d for s, d in zip(start, self.dims)):
            raise ValueError("SparseTsdfVolume.to_dense: start must lie inside the grid")
        dims = tuple(d - s for s, d in zip(start, self.dims)) if dims is None else tuple(int(v) for v in dims)
        origin = tuple(o + self.voxel_size * s for o, s in zip(self.origin, start))
        dense = TsdfVolume(origin, self.voxel_size, dims, trunc=self.trunc, max_weight=self.max_weight, colour=self.colour if colour is None else bool(colour),
                           ctx=self.ctx)
        g = dense.grid()
        self._call("to_dense", start[0], start[1], start[2], C.byref(g))
        return dense


def _fuse_render(splats, camera, size, depth_mode, pass_, ctx):
    node = render_splats_diff(splats, camera, size, (0.0, 0.0, 0.0), pass_, ctx=ctx)
    # (the node's image aliases ctx memory the next forward overwrites)
    return node.depth(depth_mode), node.img.clone(), camera if isinstance(camera, _ffi.BhCamera) else camera.uniforms(size)


def fuse_views(splats: "Splats", cameras, img_size, volume, depth_mode="expected", pass_: "RasterPass" = None, depth_min=0.0,
               depth_max=math.inf, alpha_min=0.5, dilate=1):
    """Renders `splats` from every camera (a BH_FLAG_BWD_INFO forward on black), takes the depth map RenderNode.depth(depth_mode)
    and the forward's image, and fuses them into `volume` in batches of 8 views (one pass over the volume per batch).
    A SparseTsdfVolume takes two passes over the cameras: render and mark(); commit(dilate); render again and integrate in batches of
    8 — a forward more per view, and no depth map is kept alive between the passes."""
    pass_ = RasterPass.Backward if pass_ is None else pass_
    ctx = volume.ctx
    w, h = int(img_size[0]), int(img_size[1])
    cameras = list(cameras)
    if isinstance(volume, SparseTsdfVolume):
        for camera in cameras:
            depth, image, cam = _fuse_render(splats, camera, (w, h), depth_mode, pass_, ctx)
            volume.mark([depth], [cam], [image], depth_max=depth_max, alpha_min=alpha_min)
        if volume.commit(dilate) == 0:
            return volume
    for first in range(0, len(cameras), _ffi.TSDF_MAX_BATCH):
        cams, depths, images = [], [], []
        for camera in cameras[first:first + _ffi.TSDF_MAX_BATCH]:
            depth, image, cam = _fuse_render(splats, camera, (w, h), depth_mode, pass_, ctx)
            depths.append(depth); images.append(image); cams.append(cam)
        volume.integrate(depths, cams, images, depth_min=depth_min, depth_max=depth_max, alpha_min=alpha_min)
    return volume


@dataclass
class SceneBatch:
    """brush-dataset/src/scene.rs:139-147: packed rgba8 GT [H,W] + camera."""
    img_packed: torch.Tensor
    camera: Camera
    has_alpha: bool = False
    alpha_is_mask: bool = False
    view_id: int = 0   # which view of the dataset this is (index + 1; 0 = unknown): keys the per-tile depth cuts (BhTrainBatch.view_id)
    # depth supervision (TrainConfig.depth_loss_weight): the view's depth (or inverse depth) map [H,W] f32, and the per-view
    # alignment t = depth_scale * depth + depth_offset of a monocular prior (1, 0 for metric depth).  None: no depth term this step
    depth: Optional[torch.Tensor] = None
    depth_scale: float = 1.0
    depth_offset: float = 0.0
    # feature supervision (TrainConfig.feature_loss_weight, SplatTrainer(feature_field=)): the view's target, f32 [H,W,C] for
    # feature_loss_kind "l1" or uint8 labels [H,W] (255 = ignore) for "cross_entropy".  None: no feature term this step
    features: Optional[torch.Tensor] = None

    def img_size(self):
        return tuple(self.img_packed.shape)  # (h, w)


@dataclass
class TrainStepStats:
    num_visible: int
    num_intersections: int
    lr_mean: float
    loss: float
    exchange_rows: int = 0  # mask-keyed exchange: gradient rows sent this step (0 = the dense block)


def view_output_size(w: int, h: int, max_resolution: int = 1920, scale: float = 1.0):
    """-> (width, height) LoadImage::load resizes a w x h view to (load_image.rs output_scale: the long edge capped to
    max_resolution, times the LOD image scale, never enlarged).  max_resolution 0 or None: no cap.  Host only."""
    lib = _ffi.load()
    ow, oh = C.c_uint32(), C.c_uint32()
    rc = lib.bh_view_output_size(int(w), int(h), int(max_resolution or 0), float(scale), C.byref(ow), C.byref(oh))
    if rc < 0:
        raise ValueError("view_output_size: w, h > 0 and a finite scale > 0")
    return int(ow.value), int(oh.value)


_FILTERS = {"lanczos3": _ffi.FILTER_LANCZOS3, "triangle": _ffi.FILTER_TRIANGLE}


def resize_image(t, size, filter="lanczos3", ctx: Optional[Context] = None):
    """image::imageops::resize(t, width, height, filter) of the image crate 0.25, bit for bit: t uint8 [H,W]
    or [H,W,C] (C = 1, 3, 4) on the device, size = (width, height); -> uint8 tensor [height, width(, C)] on t's device.  Alpha is
    filtered like any other channel.  The same size is a copy."""
    if filter not in _FILTERS:
        raise ValueError("filter must be 'lanczos3' or 'triangle'")
    if t.dtype != torch.uint8 or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] not in (1, 3, 4)):
        raise ValueError("resize_image: a uint8 [H,W] or [H,W,1|3|4] tensor")
    if t.device.type != "cuda":
        raise ValueError("resize_image: the image must be on the device")
    ctx = ctx or get_context(t.device)
    nw, nh = int(size[0]), int(size[1])
    c = 1 if t.dim() == 2 else int(t.shape[2])
    src = t.contiguous()
    out = torch.empty((nh, nw) + tuple(t.shape[2:]), dtype=torch.uint8, device=t.device)
    ctx.check(ctx.lib.bh_resize_u8(ctx._h, _ptr(src), int(t.shape[1]), int(t.shape[0]), c, _ptr(out), nw, nh, _FILTERS[filter]))
    return out


class BatchUploader:
    """Ring of pinned staging slots + a copy stream that turns decoded host images into packed rgba8
    device batches while the previous batch trains (bh_uploader_*: view_to_packed_data of
    brush-dataset/src/scene.rs:97-136 on the device, the hand-off of scene_loader.rs:59-174)."""

    def __init__(self, max_pixels, slots=3, ctx: Optional[Context] = None):
        self.ctx = ctx or get_context()
        self.lib = self.ctx.lib
        self._h = C.c_void_p(self.lib.bh_uploader_create(self.ctx._h, int(max_pixels), int(slots)))
        if not self._h:
            raise BrushHipError("bh_uploader_create failed (max_pixels > 0, 2 <= slots <= 16, enough pinned memory)")
        self.max_pixels, self.slots = int(max_pixels), int(slots)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.bh_uploader_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise BrushHipError("uploader error %d: %s" % (rc, self.lib.bh_uploader_last_error(self._h).decode()))
        return rc

    def map(self, nbytes):
        """-> (slot, writable uint8 numpy view of the slot's pinned buffer): decode straight into it, then commit()."""
        import numpy as np
        p = C.c_void_p()
        slot = self._check(self.lib.bh_uploader_begin(self._h, int(nbytes), C.byref(p)))
        buf = (C.c_uint8 * int(nbytes)).from_address(p.value)
        return slot, np.frombuffer(buf, dtype=np.uint8)

    def commit(self, slot, w, h, channels, premultiply):
        self._check(self.lib.bh_uploader_commit(self._h, int(slot), int(w), int(h), int(channels), int(bool(premultiply))))

    def submit(self, img_u8, premultiply=True):
        """img_u8: C-contiguous uint8 [H,W,3] or [H,W,4] host array.  `premultiply` applies to RGBA views
        (AlphaMode::Transparent); returns the slot index."""
        import numpy as np
        a = np.ascontiguousarray(img_u8, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] not in (3, 4):
            raise ValueError("image must be [H,W,3] or [H,W,4] uint8")
        h, w, c = a.shape
        return self._check(self.lib.bh_uploader_submit(self._h, a.ctypes.data_as(C.c_void_p), w, h, c, int(bool(premultiply) and c == 4)))

    def submit_view(self, img_u8, mask=None, invert_mask=False, max_resolution=1920, scale=1.0, premultiply=None):
        """LoadImage::load (load_image.rs:60-131) of a decoded view, on the device: img_u8 uint8 [H,W,3|4]; mask (optional) uint8
        [h,w] of one channel (an RGBA mask reduced to its alpha, a colour mask to luma, by the caller), Triangle-resized to the
        image when its size differs, becomes the alpha channel (255 - mask with invert_mask); then Lanczos3 down to
        view_output_size(W, H, max_resolution, scale); then view_to_packed_data.  premultiply: AlphaMode::Transparent (default:
        True without a mask, False with one, as LoadImage::new picks).  Returns the slot; acquire() gives the output size."""
        import numpy as np
        a = np.ascontiguousarray(img_u8, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] not in (3, 4):
            raise ValueError("image must be [H,W,3] or [H,W,4] uint8")
        h, w, c = a.shape
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            if m.ndim == 3 and m.shape[2] == 1:
                m = m[:, :, 0]
            if m.ndim != 2 or m.size == 0:
                raise ValueError("mask must be a one-channel uint8 [h,w] array")
        if premultiply is None:
            premultiply = m is None
        img_bytes = a.size
        total = img_bytes + (m.size if m is not None else 0)
        slot, buf = self.map(total)
        try:
            buf[:img_bytes] = a.reshape(-1)
            if m is not None:
                buf[img_bytes:total] = m.reshape(-1)
        except Exception:
            # a mapped slot must be committed or the ring stalls: commit a view the library refuses, which frees it
            self.lib.bh_uploader_commit_view(self._h, int(slot), C.byref(_ffi.BhViewLoad()))
            raise
        d = _ffi.BhViewLoad(w=w, h=h, channels=c, mask_w=m.shape[1] if m is not None else 0, mask_h=m.shape[0] if m is not None else 0,
                            invert_mask=int(bool(invert_mask)), mask_offset=img_bytes if m is not None else 0,
                            max_resolution=int(max_resolution or 0), scale=float(scale), premultiply=int(bool(premultiply)))
        self._check(self.lib.bh_uploader_commit_view(self._h, int(slot), C.byref(d)))
        return slot

    def acquire(self, slot):
        """-> (packed int32 [H,W] device tensor aliasing the slot, has_alpha).  Work queued on the ctx stream
        afterwards is ordered behind the upload; call release(slot) once the step that reads it is queued."""
        p, w, h, ha = C.c_void_p(), C.c_uint32(), C.c_uint32(), C.c_int()
        self._check(self.lib.bh_uploader_acquire(self._h, int(slot), C.byref(p), C.byref(w), C.byref(h), C.byref(ha)))
        return _view(p.value, (int(h.value), int(w.value)), torch.int32, self.ctx.device), bool(ha.value)

    def release(self, slot):
        self._check(self.lib.bh_uploader_release(self._h, int(slot)))


class SceneLoader:
    """SceneLoader (brush-dataset/src/scene_loader.rs:59-174): an endless shuffled stream of SceneBatch over
    a list of views, prefetched by a loader thread through a BatchUploader so the H2D copy + packing of the
    next views overlap the current train step.

    views: sequence of (image, Camera[, alpha_is_mask[, mask]]) with image a uint8 [H,W,3|4] array or a callable
    returning one (the decode), and mask an optional one-channel uint8 [h,w] array or callable (load_image.rs:69-112: it
    becomes the view's alpha; alpha_is_mask None then means True, AlphaMode::Masked).  max_resolution / image_scale: the
    views are resampled on the device as LoadImage::load does (BatchUploader.submit_view; LoadImage::with_scale for a LOD
    level), invert_masks as LoadDatasetConfig's.  With the defaults (None, 1.0) and no masks the views go through
    BatchUploader.submit unchanged.  Shuffling: every epoch is a seeded Fisher-Yates permutation (SplitMix64) of
    this rank's views — the reference's order comes from rand::StdRng inside racing loader tasks and is not
    reproducible, so only the "every view once per epoch" property is kept.  `rank`/`world` shard the view
    list for data-parallel training (view i belongs to rank i % world)."""

    def __init__(self, views, seed=0, uploader: Optional[BatchUploader] = None, slots=3, rank=0, world=1, ctx: Optional[Context] = None,
                 max_resolution: Optional[int] = None, image_scale: float = 1.0, invert_masks: bool = False):
        import queue
        import threading
        self.views = [v for i, v in enumerate(views) if i % world == rank]
        self.view_ids = [i + 1 for i in range(len(views)) if i % world == rank]   # dataset index + 1 (0 = "unknown view")
        if not self.views:
            raise ValueError("Need at least one view in dataset")  # scene_loader.rs:130
        self.max_resolution, self.image_scale, self.invert_masks = max_resolution, float(image_scale), bool(invert_masks)
        if not (self.image_scale > 0.0 and math.isfinite(self.image_scale)):
            raise ValueError("image_scale must be finite and > 0")
        self._own_uploader = uploader is None
        if uploader is None:
            mp = 0
            for v in self.views:
                img = v[0]() if callable(v[0]) else v[0]
                mask = self._view_mask(v)
                px = img.shape[0] * img.shape[1]
                staged = img.size + (mask.size if mask is not None else 0)   # image + mask bytes in one pinned slot
                mp = max(mp, px, (staged + 3) // 4)
            uploader = BatchUploader(mp, slots, ctx)
        self.up = uploader
        self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._q = queue.Queue(maxsize=max(1, self.up.slots - 1))  # slots in flight = queued + the one being trained on
        self._stop = threading.Event()
        self._held = None
        self._thread = threading.Thread(target=self._run, name="brush-hip-loader", daemon=True)
        self._thread.start()

    @staticmethod
    def _view_mask(view):
        m = view[3] if len(view) > 3 else None
        return m() if callable(m) else m

    @staticmethod
    def _splitmix(state):
        state = (state + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return state, z ^ (z >> 31)

    def epoch_order(self, epoch):
        """The view order of `epoch` (deterministic in seed, epoch and the shard)."""
        n = len(self.views)
        order = list(range(n))
        st = (self._seed ^ (0xD1B54A32D192ED03 * (epoch + 1))) & 0xFFFFFFFFFFFFFFFF
        for i in range(n - 1, 0, -1):
            st, r = self._splitmix(st)
            j = r % (i + 1)
            order[i], order[j] = order[j], order[i]
        return order

    def _run(self):
        import queue
        epoch = 0
        try:
            while not self._stop.is_set():
                for idx in self.epoch_order(epoch):
                    view = self.views[idx]
                    img = view[0]() if callable(view[0]) else view[0]
                    mask_img = self._view_mask(view)
                    flag = view[2] if len(view) > 2 else None
                    mask = bool(flag) if flag is not None else mask_img is not None   # alpha_is_mask (AlphaMode::Masked)
                    # wait for a free place in the queue BEFORE mapping a slot, so a mapped slot is never parked
                    while not self._stop.is_set() and self._q.full():
                        self._stop.wait(0.0005)
                    if self._stop.is_set():
                        return
                    if mask_img is None and self.max_resolution is None and self.image_scale == 1.0:
                        slot = self.up.submit(img, premultiply=not mask)
                    else:
                        slot = self.up.submit_view(img, mask=mask_img, invert_mask=self.invert_masks, max_resolution=self.max_resolution or 0,
                                                   scale=self.image_scale, premultiply=not mask)
                    self._q.put((slot, idx, view[1], mask))
                epoch += 1
        except Exception as e:  # surface loader failures to the consumer ("Scene loader failed to load an image")
            try:
                self._q.put(e, timeout=1.0)
            except queue.Full:
                pass

    def next_batch(self):
        """-> SceneBatch (its img_packed aliases an uploader slot that stays valid until the NEXT next_batch call).
        Call after queuing the train step of the previous batch: that is what releases its slot."""
        if self._held is not None:
            self.up.release(self._held)
            self._held = None
        item = self._q.get()
        if isinstance(item, Exception):
            raise BrushHipError("Scene loader failed to load an image: %r" % (item,))
        slot, idx, cam, mask = item
        packed, has_alpha = self.up.acquire(slot)
        self._held = slot
        b = SceneBatch(packed, cam, has_alpha=has_alpha, alpha_is_mask=mask, view_id=self.view_ids[idx])
        b.view_index = idx
        return b

    def close(self):
        self._stop.set()
        try:
            while True:
                self._q.get_nowait()
        except Exception:
            pass
        self._thread.join(timeout=5.0)
        if self._own_uploader:
            self.up.close()


class SplatTrainer:
    """SplatTrainer::{new, step} (brush-train/src/train.rs:140-429). Owns the three
    Adam states and the RefineRecord; `step` runs forward, L1+SSIM loss, backward,
    statistics, Adam and the optional mean noise inside one C-ABI call.

    Data parallel (not in the reference): pass `process_group` and the
    per-rank gradients + visible flags are summed with ONE torch.distributed all_reduce
    (RCCL over xGMI) between backward and Adam, the gradients scaled by 1/world inside the
    update; every rank applies the identical update.  The RefineRecord's running maxima stay
    rank-local until `sync_refine_stats()` (called by `refine`) MAX-reduces them."""

    def __init__(self, config: TrainConfig, median_scene_scale: float = 1.0, process_group=None, ctx: Optional[Context] = None,
                 partition: str = "cameras", native_comm: bool = False, sparse_exchange: bool = True, seed: Optional[int] = None,
                 allreduce: str = "ring", lpips: Optional["Lpips"] = None, pose_optimizer: Optional["PoseOptimizer"] = None,
                 exposure: Optional["ExposureTable"] = None, exposure_lr=None, bilagrid: Optional["BilateralGridTable"] = None, bilagrid_lr=None,
                 bilagrid_tv_weight: float = 10.0, envmap: Optional["EnvironmentMap"] = None, envmap_lr=None,
                 intrinsics_optimizer: Optional["IntrinsicsOptimizer"] = None, feature_field: Optional["FeatureField"] = None):
        """seed: an int turns on the two stochastic terms of the reference's step — the visibility-gated noise on the
        means (train.rs:389-416) and the background jitter (train.rs:896-908) — drawn by the library's counter-based
        generator as pure functions of (seed, step[, splat]); data-parallel ranks must pass the same seed.  None (the
        default of this mirror, which the parity tests rely on): the terms appear only when injected through
        step(background=..., noise_samples=...).

        partition (only with a process_group): "cameras" = data parallel, every rank its own view,
        mean gradient; "tiles" = every rank renders a strip of tile rows of the SAME view, strips are
        all-gathered before the loss and the partial gradients summed.

        lpips: the LpipsModel the step uses when config.lpips_loss_weight > 0 (train.rs:153, 265-273; bh_train_set_lpips).
        Not with partition "tiles".

        pose_optimizer: a PoseOptimizer that refines the batches' cameras beside the splats (bh_train_set_pose_grad): every step
        renders the batch's view at its current correction, reads the step's twelve pose-gradient floats back (48 bytes, one
        synchronisation per step) and updates that view's 6-vector.  Batches must carry a view_id > 0.  Not with partition
        "tiles".

        exposure: an ExposureTable (bh_train_set_exposure): every step exposes its frame with the row of the batch's view_id
        (1 .. n_views) before the loss and updates that row on the device: no readback, no synchronisation.  exposure_lr: an
        optional callable of the step number (from 1) giving the table's learning rate for that step.  Not with partition
        "tiles".

        bilagrid: a BilateralGridTable (bh_train_set_bilagrid), the alternative to `exposure` for photometric effects that vary over
        the frame or with brightness: every step slices its frame with the grid of the batch's view_id before the loss, adds
        bilagrid_tv_weight times the grid's total variation to the loss (10 is gsplat's weight) and updates that grid on the
        device.  bilagrid_lr: an optional callable of the step number (from 1), as exposure_lr.  Not with partition "tiles" and
        not together with `exposure`.

        feature_field: a FeatureField (bh_train_set_features) trained beside the splats: a step whose batch carries a feature target
        (SceneBatch.features), at config.feature_loss_weight > 0 and from config.feature_loss_from_iter on, blends the field's
        map, adds the fused feature loss, backpropagates it into the field AND the splats and updates the field on the device
        (no readback); `refine` carries the field's rows through the plan.  Not with partition "tiles" and not together with
        `pose_optimizer`.

        envmap: an EnvironmentMap (bh_train_set_envmap): every step composites its frame over the map before the loss (an exposure
        table or a bilateral grid then act on the composited frame) and updates the map on the device.  The frame is rendered on
        black: config.background_color must be (0, 0, 0) and the background jitter is not drawn.  envmap_lr: an optional callable of
        the step number (from 1), as exposure_lr.  Not with partition "tiles" and not together with `pose_optimizer`.

        intrinsics_optimizer: an IntrinsicsOptimizer that refines the sensors' focal lengths and principal points beside the splats
        (bh_train_set_intrinsics_grad): every step renders the batch's view with its sensor's current intrinsics, reads the step's
        four gradient floats back and updates that sensor's 4-vector.  May be combined with `pose_optimizer`: the two readbacks
        (48 + 16 bytes) are one copy behind one synchronisation.  Batches must carry a view_id > 0.  Not with partition "tiles", not
        with `envmap` (the ray directions depend on the intrinsics) and not with config.normal_loss_weight > 0 (the depth-to-normal
        stencil uses fx, fy)."""
        if partition not in ("cameras", "tiles"):
            raise ValueError("partition must be 'cameras' or 'tiles'")
        if pose_optimizer is not None and partition == "tiles":
            raise ValueError("pose_optimizer is not available with partition 'tiles'")
        if exposure is not None and partition == "tiles":
            raise ValueError("exposure is not available with partition 'tiles'")
        if feature_field is not None and partition == "tiles":
            raise ValueError("feature_field is not available with partition 'tiles'")
        if feature_field is not None and pose_optimizer is not None:
            raise ValueError("feature_field and pose_optimizer cannot be combined (the pose pass does not carry the feature term's gradient)")
        if envmap is not None and partition == "tiles":
            raise ValueError("envmap is not available with partition 'tiles'")
        if envmap is not None and any(float(b) != 0.0 for b in config.background_color):
            raise ValueError("envmap needs background_color (0, 0, 0): the map is what lies behind the splats")
        if envmap is not None and pose_optimizer is not None:
            raise ValueError("envmap and pose_optimizer cannot be combined (the pose pass does not carry the lookup's dependence on the rotation)")
        if intrinsics_optimizer is not None and partition == "tiles":
            raise ValueError("intrinsics_optimizer is not available with partition 'tiles'")
        if intrinsics_optimizer is not None and envmap is not None:
            raise ValueError("envmap and intrinsics_optimizer cannot be combined (the ray directions depend on the intrinsics)")
        if intrinsics_optimizer is not None and float(config.normal_loss_weight) > 0.0:
            raise ValueError("normal_loss_weight > 0 and intrinsics_optimizer cannot be combined (the depth-to-normal stencil uses fx, fy)")
        self.envmap, self.envmap_lr = envmap, envmap_lr
        self.feature_field = feature_field
        self.pose_optimizer = pose_optimizer
        self.intrinsics_optimizer = intrinsics_optimizer
        self._cam_buf = None    # [16] f32 on the device: the step's v_viewmat [12] | v_intrinsics [4], read back as one
        self._pose_buf = None   # ... and the two views of it the step's buffers are attached as
        self._intr_buf = None
        self.exposure, self.exposure_lr = exposure, exposure_lr
        if bilagrid is not None and partition == "tiles":
            raise ValueError("bilagrid is not available with partition 'tiles'")
        if bilagrid is not None and exposure is not None:
            raise ValueError("bilagrid and exposure are alternatives: pass one of them")
        self.bilagrid, self.bilagrid_lr, self.bilagrid_tv_weight = bilagrid, bilagrid_lr, float(bilagrid_tv_weight)
        if allreduce not in ("ring", "direct"):
            raise ValueError("allreduce must be 'ring' (all_reduce / ncclAllReduce) or 'direct' (reduce-scatter + all-gather over point-to-point messages)")
        # how long messages of the gradient exchange are summed: the collective library's all-reduce, or the direct algorithm for a
        # fully connected node (comm.hip comm_allreduce_direct; here, for the hook path, parallel.allreduce_direct).  With
        # native_comm the caller selects it on the context: ctx.set_option("grad_allreduce", "direct")
        self.allreduce = allreduce
        # native_comm: the ctx carries an RCCL communicator (Context.comm_init) and bh_train_step all-reduces the
        # exchange buffer itself — no torch.distributed, no callback (data parallel over cameras only)
        # (partition "tiles": the library also moves the strips' 21-px halos itself — bh_exchange_strip_halos, strip-wise loss only)
        if native_comm and process_group is not None:
            raise ValueError("native_comm excludes process_group")
        self.native_comm = bool(native_comm)
        self.seed = None if seed is None else (int(seed) & 0xFFFFFFFFFFFFFFFF)
        # exchange only the gradient rows of splats some rank (view or strip) saw (BhTrainBatch.exchange_mode 1,
        # brush_amd/csrc/exchange.hip); False = one dense all-reduce of the whole exchange buffer
        self.sparse_exchange = bool(sparse_exchange)
        self.partition = partition
        self._img_hook = None
        self.bounds = None  # (center, extent); None = unit box scaled by median_scene_scale (set by refine / set_bounds)
        self.config = config
        self.median_scene_scale = float(median_scene_scale)
        self.step_count = 0
        self.state = None
        self.ctx = ctx
        self.pg = process_group
        self._hook = None
        self.generator = None
        self.view_cams = []  # [(centre xyz, focal px)] of the train views: enables the Mip-Splatting 3D filter
        # partition == "tiles": strips are re-cut every `rebalance_every` steps so that every rank gets the same number of
        # blended intersections (the backward's work), measured on the previous frame ("balance by
        # intersection count, not rows"); 0 keeps equal-height strips
        self.rebalance_every = 8
        self._row_weights = None
        # partition == "tiles": evaluate the loss strip-wise (each rank on its own rows, 21-px halos from the neighbours)
        # instead of all-gathering the frame and computing the whole loss everywhere; TrainStepStats.loss is then this
        # rank's share of the frame's loss (reduce_loss() sums the shares)
        self.strip_loss = True
        self._strip_loss_now = False
        self.batch_patch = None   # optional callable(BhTrainBatch): edits the C struct right before bh_train_step
        self.lpips = lpips

    MIN_SCALE_FACTOR = 0.1       # train.rs:44
    MIN_SCALE_FREEZE_FRAC = 0.9  # train.rs:37

    def set_view_cams(self, view_cams):
        """SplatTrainer::set_view_cams (train.rs:170-174): per train view (world centre (x,y,z), focal in px at
        native resolution).  Empty disables the 3D filter."""
        self.view_cams = [(tuple(float(v) for v in c), float(f)) for c, f in view_cams]

    def compute_min_scale(self, splats, ctx=None):
        """compute_min_scale (train.rs:102-125) -> [N] tensor, or None when there are no view cameras."""
        if not self.view_cams or self.MIN_SCALE_FACTOR <= 0.0:
            return None
        ctx = ctx or self.ctx or get_context(splats.device)
        k = len(self.view_cams)
        vc = (C.c_float * (4 * k))()
        for i, (c, f) in enumerate(self.view_cams):
            vc[4 * i], vc[4 * i + 1], vc[4 * i + 2], vc[4 * i + 3] = c[0], c[1], c[2], f
        out = torch.empty(splats.num_splats(), dtype=torch.float32, device=splats.device)
        ctx.check(ctx.lib.bh_compute_min_scale(ctx._h, _ptr(splats.transforms), splats.num_splats(), vc, k, float(self.MIN_SCALE_FACTOR), _ptr(out)))
        return out

    def _init_state(self, splats: Splats):
        dev = splats.device
        n = splats.num_splats()
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        self.state = dict(m1_t=z(n, 10), m2_t=z(n, 10), m1_sh=z(*splats.sh_coeffs.shape), m2_sh=z(n), m1_o=z(n), m2_o=z(n),
                          refine_weight_norm=z(n), vis_weight=z(n), max_screen_size=z(n))
        if self.ctx is not None and not self.ctx.uses_torch_stream:
            torch.cuda.current_stream(dev).synchronize()   # the zero-fills ran on torch's stream, the step runs on the ctx's own

    def sample_background(self, rng=None, step=None):
        """train.rs:896-908: base + U(-s, s)^3, clamped to [0,1].  With the trainer's seed: the library's generator at
        (seed, step); else from `rng` (a random.Random) if given; else the base colour."""
        s = self.config.background_noise_strength
        base = self.config.background_color
        if self.seed is not None and rng is None:
            out = (C.c_float * 3)()
            _ffi.load().bh_sample_background(self.seed, int(self.step_count + 1 if step is None else step), (C.c_float * 3)(*[float(b) for b in base]), float(s), out)
            return tuple(out)
        if s <= 0.0 or rng is None:
            return tuple(base)
        return tuple(min(1.0, max(0.0, b + (rng.random() * 2.0 - 1.0) * s)) for b in base)

    def normal_samples(self, n, step, device, ctx=None):
        """The [n,3] N(0,1) samples the seeded step number `step` draws (bh_normal_samples)."""
        ctx = ctx or self.ctx or get_context(device)
        out = torch.empty((int(n), 3), dtype=torch.float32, device=device)
        ctx.check(ctx.lib.bh_normal_samples(ctx._h, int(self.seed or 0), int(step), int(n), _ptr(out)))
        return out

    def _make_hook(self, dev):
        import torch.distributed as dist
        pg = self.pg
        world = dist.get_world_size(pg)

        views = {}  # device pointer -> flat float32 view of the longest range summed there so far (only [:count] is touched)

        def hook(_user, exch_ptr, sum_count):
            try:
                cnt = int(sum_count)
                t = views.get(exch_ptr)
                if t is None or t.numel() < cnt:
                    t = views[exch_ptr] = _view(exch_ptr, (cnt,), torch.float32, dev)
                if self.allreduce == "direct" and cnt >= DIRECT_ALLREDUCE_MIN_FLOATS:
                    allreduce_direct(t, cnt, pg)
                else:
                    allreduce_exchange(t, cnt, pg)
                return 0
            except Exception:  # never unwind across the C boundary
                return 1
        self._world = world
        return _ffi.GRAD_HOOK(hook)

    def _make_image_hook(self, dev):
        pg = self.pg

        def hook(_user, img_ptr, h, w, r0, r1):
            try:
                img = _view(img_ptr, (int(h), int(w), 4), torch.float32, dev)
                import torch.distributed as dist
                spans = strip_spans_px(int(h), dist.get_world_size(pg), self._row_weights)
                if self._strip_loss_now:
                    exchange_strip_halos(img, spans, dist.get_rank(pg), pg)
                else:
                    allgather_strips(img, int(r0), int(r1), pg, spans=spans)
                return 0
            except Exception:  # never unwind across the C boundary
                return 1
        return _ffi.IMAGE_HOOK(hook)

    def _train_config(self, splats):
        c, cfg = self.config, _ffi.BhTrainConfig()
        cfg.lr_mean, cfg.lr_mean_end, cfg.total_train_iters = c.lr_mean, c.lr_mean_end, c.total_train_iters
        cfg.lr_coeffs_dc, cfg.lr_coeffs_sh_scale, cfg.lr_opac = c.lr_coeffs_dc, c.lr_coeffs_sh_scale, c.lr_opac
        cfg.lr_scale, cfg.lr_rotation, cfg.ssim_weight = c.lr_scale, c.lr_rotation, c.ssim_weight
        cfg.match_alpha_weight, cfg.mean_noise_weight = c.match_alpha_weight, c.mean_noise_weight
        cfg.background[0], cfg.background[1], cfg.background[2] = c.background_color
        cfg.median_scene_scale = self.median_scene_scale
        cfg.render_mip = 1 if (c.render_mip or splats.render_mip) else 0
        cfg.exact_lists = 1 if c.exact_lists else 0
        cfg.growth_stop_iter = int(c.growth_stop_iter)   # from that step on nobody reads the refine weight (train.rs:589-614): the step stops computing it
        return cfg

    def _tile_window(self, ctx, b, h, dev):
        """partition "tiles": this rank's strip of tile rows goes into b.camera, with the image hook that moves the strips or — native_comm —
        the library's own halo exchange, and the strip-wise loss where the strips allow it.  -> whether the frame is split at all."""
        native_tiles = self.native_comm and self.partition == "tiles" and ctx.comm_world() > 1
        if not ((self.pg is not None and self.partition == "tiles") or native_tiles):
            return False
        if native_tiles:
            t_rank, t_world = ctx.comm_rank(), ctx.comm_world()
        else:
            import torch.distributed as dist
            t_rank, t_world = dist.get_rank(self.pg), dist.get_world_size(self.pg)
        rows = tile_rows_for_rank((h + 15) // 16, t_rank, t_world, self._row_weights)
        cam = _ffi.BhCamera()
        C.memmove(C.byref(cam), C.byref(b.camera), C.sizeof(cam))
        cam.tile_row_begin, cam.tile_row_end = rows
        b.camera = cam
        halo_ok = strips_allow_halo_loss(strip_spans_px(h, t_world, self._row_weights))
        if native_tiles:
            # no hook: the library exchanges the halos over its own communicator (strip-wise loss is the only native mode)
            if not halo_ok:
                raise BrushHipError("native tile partition needs every strip to be at least 21 pixel rows tall")
            self._strip_loss_now = True
        else:
            if self._img_hook is None:
                self._img_hook = self._make_image_hook(dev)
            b.image_hook = C.cast(self._img_hook, C.c_void_p)
            self._strip_loss_now = bool(self.strip_loss) and halo_ok
        b.strip_loss = int(self._strip_loss_now)
        return True

    def _feature_target(self, ctx, batch, dev):
        """The feature target of this batch (TrainConfig.feature_loss_weight, from feature_loss_from_iter on), checked and converted
        -> (BhFeatureTarget, the tensor it points into), or (None, None): no feature term this step."""
        c, ff, ftarget = self.config, self.feature_field, batch.features
        fw = float(c.feature_loss_weight) if ftarget is not None else 0.0
        if ff is None:
            if fw > 0.0:
                raise ValueError("feature_loss_weight > 0 and a batch with a feature target need SplatTrainer(..., feature_field=FeatureField(...))")
            return None, None
        if not (fw > 0.0 and self.step_count + 1 >= int(c.feature_loss_from_iter)):
            return None, None
        fk = c.feature_loss_kind
        fk = int(FEATURE_LOSS_KINDS[fk]) if isinstance(fk, str) else int(fk)
        ch = int(ff.features.shape[1])
        if fk == _ffi.FEATURE_LOSS_CROSS_ENTROPY:
            ftgt = torch.as_tensor(ftarget, dtype=torch.uint8, device=dev).contiguous()
            if ftgt.dim() != 2:
                raise ValueError("SceneBatch.features: cross-entropy labels must be uint8 [H, W]")
        else:
            ftgt = _f32c(ftarget, dev)
            if ftgt.dim() != 3 or int(ftgt.shape[2]) != ch:
                raise ValueError("SceneBatch.features: an l1 target must be float32 [H, W, %d]" % ch)
        if ftgt is not ftarget and not ctx.uses_torch_stream:
            torch.cuda.current_stream(dev).synchronize()   # the conversion ran on torch's stream, the step runs on the ctx's own
        ft = _ffi.BhFeatureTarget()
        ft.target, ft.h, ft.w, ft.channels, ft.kind, ft.weight = ftgt.data_ptr(), int(ftgt.shape[0]), int(ftgt.shape[1]), ch, fk, fw
        return ft, ftgt

    def _step_terms(self, ctx, batch, b, dev):
        """What this step attaches to the ctx, in attach order, for `_attached`: (setter, the arguments that attach this step's term — or
        say that there is none —, the arguments that detach it behind the step, or None: the term stays as set), or a plain callable that
        has its turn at that place.  What the step cannot do is said here, before anything is attached.
        -> (terms, (depth tensor, feature tensor) the terms point into, the BhFeatureTarget or None)."""
        c, lib, step = self.config, ctx.lib, self.step_count + 1
        lw = float(c.lpips_loss_weight)
        if lw > 0.0 and self.lpips is None:
            raise ValueError("lpips_loss_weight > 0 needs SplatTrainer(..., lpips=Lpips.from_state_dict(...))")
        ff = self.feature_field
        ft, ftgt = self._feature_target(ctx, batch, dev)
        off = (None,)
        terms = []
        # the terms of the batch.  Depth: for a batch that has a depth map, at this step's weight (a weight of 0 is no term)
        dgt = None
        if batch.depth is not None:
            dt, dgt = _depth_target(batch.depth, dev, c.depth_loss_kind, c.depth_weight_at(step), batch.depth_scale, batch.depth_offset, shape=batch.img_size())
            terms.append((lib.bh_train_set_depth, (C.byref(dt),), off))
        else:
            terms.append((lib.bh_train_set_depth, off, off))
        # normal consistency and distortion: from their *_from_iter on
        nw = float(c.normal_loss_weight)
        if nw > 0.0 and step >= int(c.normal_loss_from_iter):
            terms.append((lib.bh_train_set_normal, (C.byref(_ffi.BhNormalTermConfig(weight=nw)),), off))
        else:
            terms.append((lib.bh_train_set_normal, off, off))
        xw = float(c.distortion_loss_weight)
        if xw > 0.0 and step >= int(c.distortion_loss_from_iter):
            xt = _ffi.BhDistortionTermConfig(weight=xw, kind=_distortion_kind(c.distortion_kind), near_z=float(c.distortion_near), far_z=float(c.distortion_far))
            terms.append((lib.bh_train_set_distortion, (C.byref(xt),), off))
        else:
            terms.append((lib.bh_train_set_distortion, off, off))
        # features: the field and this batch's target, or none for a batch without one or while the weight is off.  (A trainer without a
        # field makes neither call: there is nothing of another trainer's to clear.)
        if ff is not None:
            terms.append((lib.bh_train_set_features, (C.byref(ff.as_struct()), C.byref(ft)) if ft is not None else (None, None), (None, None)))
        if self.batch_patch is not None:   # last word on the BhTrainBatch (callers that partition a frame themselves; tests)
            terms.append(lambda: self.batch_patch(b))
        # the terms of the trainer.  LPIPS is set for THIS trainer's step, whatever another trainer on the ctx left, and stays
        terms.append((lib.bh_train_set_lpips, (self.lpips._h if lw > 0.0 else None, lw if lw > 0.0 else 0.0), None))
        if self.pose_optimizer is not None:
            terms.append((lib.bh_train_set_pose_grad, (_ptr(self._pose_buf),), off))
        if self.intrinsics_optimizer is not None:
            terms.append((lib.bh_train_set_intrinsics_grad, (_ptr(self._intr_buf),), off))
        ex, grid = self.exposure, self.bilagrid
        if ex is not None:
            if self.exposure_lr is not None:
                terms.append(lambda: ex.set_lr(self.exposure_lr(step)))
            terms.append((lib.bh_train_set_exposure, (ex._h,), off))
        if grid is not None:
            if self.bilagrid_lr is not None:
                terms.append(lambda: grid.set_lr(self.bilagrid_lr(step)))
            terms.append((lib.bh_train_set_bilagrid, (grid._h, self.bilagrid_tv_weight), (None, 0.0)))
        env = self.envmap
        if env is not None:
            if self.envmap_lr is not None:
                terms.append(lambda: env.set_lr(self.envmap_lr(step)))
            terms.append((lib.bh_train_set_envmap, (env._h,), off))
        return terms, (dgt, ftgt), ft

    @staticmethod
    @contextmanager
    def _attached(ctx, terms):
        """The terms of a step are ctx state (bh_train_set_*) and a ctx may serve several trainers: every trainer attaches what its own
        step needs right before the step, in `terms`' order, and detaches it behind the step in the same order, whether or not the step
        succeeded."""
        try:
            for t in terms:
                if callable(t):
                    t()
                else:
                    ctx.check(t[0](ctx._h, *t[1]))
            yield
        finally:
            for t in terms:
                if not callable(t) and t[2] is not None:
                    t[0](ctx._h, *t[2])

    def step(self, batch: SceneBatch, splats: Splats, background=None, noise_samples=None) -> Tuple[Splats, TrainStepStats]:
        """One optimisation step, in place on `splats`. `background` / `noise_samples`
        [N,3] inject the two stochastic terms; None = base colour / no noise."""
        ctx = self.ctx or get_context(splats.device)
        dev = splats.device
        if self.state is None:
            self._init_state(splats)
        cfg, st = self._train_config(splats), self._train_state(splats, self.state)
        st.min_scale = splats.min_scale.data_ptr() if splats.min_scale is not None else None
        h, w = batch.img_size()
        b = _ffi.BhTrainBatch()
        b.camera = batch.camera if isinstance(batch.camera, _ffi.BhCamera) else batch.camera.uniforms((w, h))
        tiles = self._tile_window(ctx, b, h, dev)
        gt = _as_u32(batch.img_packed, dev)
        b.gt_packed = gt.data_ptr()
        b.has_alpha, b.alpha_is_mask = int(batch.has_alpha), int(batch.alpha_is_mask)
        # (an environment map is what lies behind the splats: its trainer's base colour is black and the jitter is not drawn)
        jitter = self.seed is not None and self.envmap is None
        bg = background if background is not None else (self.sample_background() if jitter else self.config.background_color)
        b.background[0], b.background[1], b.background[2] = [float(v) for v in bg]
        ns = None
        if noise_samples is not None:
            ns = _f32c(noise_samples, dev).reshape(-1, 3)
            b.noise_samples = ns.data_ptr()
        elif self.seed is not None:
            b.device_noise, b.noise_seed = 1, self.seed
        stats = _ffi.BhTrainStats()
        b.exchange_mode = 1 if (self.sparse_exchange and (self.pg is not None or self.native_comm)) else 0
        b.view_id = int(batch.view_id) & 0xFFFFFFFF
        po, io = self.pose_optimizer, self.intrinsics_optimizer
        if io is not None:   # the view with its sensor's current intrinsics ...
            b.camera = io.camera(b.view_id, b.camera)
        if po is not None:   # ... at its current correction, named by its id (a moving camera's hash would mint a view table per step)
            b.camera = po.camera(b.view_id, b.camera)
        if (po is not None or io is not None) and self._cam_buf is None:
            self._cam_buf = torch.zeros((16,), dtype=torch.float32, device=dev)
            self._pose_buf, self._intr_buf = self._cam_buf[:12], self._cam_buf[12:]
            if not ctx.uses_torch_stream:
                torch.cuda.current_stream(dev).synchronize()   # the zero-fill ran on torch's stream, the step runs on the ctx's own
        hook, scale = None, 1.0
        if self.native_comm:
            scale = 1.0 if tiles else 1.0 / ctx.comm_world()
        if self.pg is not None:
            if self._hook is None:
                self._hook = self._make_hook(dev)
            hook, scale = self._hook, (1.0 if tiles else 1.0 / self._world)
        terms, kept, ft = self._step_terms(ctx, batch, b, dev)
        with self._attached(ctx, terms):
            ctx.check(ctx.lib.bh_train_step(ctx._h, C.byref(cfg), C.byref(st), C.byref(b), C.cast(hook, C.c_void_p) if hook else None, None,
                                            float(scale), C.byref(stats)))
        if po is not None or io is not None:   # one readback (48 + 16 bytes) behind one synchronisation
            if not ctx.uses_torch_stream:
                ctx.sync()
            cam_grads = self._cam_buf.detach().cpu().numpy().astype("float64")
            if po is not None:
                po.update(b.view_id, list(b.camera.vm), cam_grads[:12])
            if io is not None:
                io.update(b.view_id, b.camera, cam_grads[12:])
        if ft is not None:   # the step succeeded with the term: the library applied one Adam update to the field
            self.feature_field.t += 1
        self.step_count = st.step_count
        self._last_stats = stats
        self._keep = (gt, ns) + kept
        if tiles and self.rebalance_every > 0:
            if self.step_count % self.rebalance_every == 0:
                self._measure_row_weights(ctx, (h + 15) // 16, (w + 15) // 16, dev)
            elif self.step_count == 1:
                self._warm_rebalance((h + 15) // 16, (w + 15) // 16, dev)
        return splats, stats

    def _measure_row_weights(self, ctx, tile_bh, tile_bw, dev):
        """Per tile row: intersections this frame actually blended (the lists' shrunk ends), summed over the ranks'
        strips -> the weights of the next cut.  One small readback + one [tile_bh] all-reduce every rebalance_every steps."""
        out = _ffi.BhRenderOut()
        ctx.check(ctx.lib.bh_last_render_out(ctx._h, C.byref(out)))
        per_row = self._rows_blended(_view(out.tile_offsets, (tile_bh * tile_bw, 2), torch.int32, dev), tile_bh, tile_bw)
        if out.tile_offsets_far:   # depth-sliced lists: a tile's blended splats = its near segment + its far segment
            per_row = per_row + self._rows_blended(_view(out.tile_offsets_far, (tile_bh * tile_bw, 2), torch.int32, dev), tile_bh, tile_bw)
        if self.native_comm:
            per_row = per_row.contiguous()
            if not ctx.uses_torch_stream:
                torch.cuda.current_stream(dev).synchronize()
            ctx.allreduce_sum(per_row)
            ctx.sync()
        else:
            import torch.distributed as dist
            dist.all_reduce(per_row, op=dist.ReduceOp.SUM, group=self.pg)
        self._row_weights = [float(x) + 1.0 for x in per_row.tolist()]  # +1: empty rows still cost a launch slot

    @staticmethod
    def _rows_blended(tile_offsets, tile_bh, tile_bw):
        to = tile_offsets.to(torch.int64)
        return (to[:, 1] - to[:, 0]).clamp(min=0).view(tile_bh, tile_bw).sum(1).to(torch.float32)

    def _warm_rebalance(self, tile_bh, tile_bw, dev):
        """The first use of each torch kernel above loads its code object (~200 ms in total on ROCm): pay that in the
        first step, not in the middle of training when the first re-cut happens."""
        per_row = self._rows_blended(torch.zeros((tile_bh * tile_bw, 2), dtype=torch.int32, device=dev), tile_bh, tile_bw)
        if not self.native_comm:
            import torch.distributed as dist
            dist.all_reduce(per_row, op=dist.ReduceOp.SUM, group=self.pg)
        per_row.tolist()

    def _train_state(self, splats, s):
        st = _ffi.BhTrainState()
        st.n, st.sh_degree = splats.num_splats(), splats.sh_degree()
        st.transforms, st.sh_coeffs, st.raw_opacities = splats.transforms.data_ptr(), splats.sh_coeffs.data_ptr(), splats.raw_opacities.data_ptr()
        st.m1_transforms, st.m2_transforms = s["m1_t"].data_ptr(), s["m2_t"].data_ptr()
        st.m1_sh, st.m2_sh = s["m1_sh"].data_ptr(), s["m2_sh"].data_ptr()
        st.m1_opac, st.m2_opac = s["m1_o"].data_ptr(), s["m2_o"].data_ptr()
        st.refine_weight_norm, st.vis_weight, st.max_screen_size = s["refine_weight_norm"].data_ptr(), s["vis_weight"].data_ptr(), s["max_screen_size"].data_ptr()
        st.step_count = self.step_count
        return st

    def sync_refine_stats(self):
        """Multi-GPU: MAX-reduce the RefineRecord's running maxima (refine_weight_norm,
        max_screen_size) over the ranks; afterwards every replica's RefineRecord is identical.
        Needed once before refine, not per step (brush_amd/parallel.py)."""
        if self.pg is not None and self.state is not None:
            allreduce_refine_maxima(self.state["refine_weight_norm"], self.state["max_screen_size"], self.pg)
        elif self.native_comm and self.state is not None:
            ctx = self.ctx or get_context(self.state["refine_weight_norm"].device)
            ctx.allreduce_max(self.state["refine_weight_norm"])
            ctx.allreduce_max(self.state["max_screen_size"])

    def set_bounds(self, center, extent):
        self.bounds = (tuple(float(x) for x in center), tuple(float(x) for x in extent))
        self.median_scene_scale = bounds_median_size(self.bounds[1])

    def refine(self, iter: int, splats: Splats, seed: Optional[int] = None):
        """SplatTrainer::refine (train.rs:431-663): prune dead / oversized / out-of-bounds / non-finite
        splats, refill the pruned budget by opacity x visibility sampling, split splats that are too big
        on screen or have a high positional gradient, reset their Adam moments, decay opacities and
        recompute the scene bounds.  Returns (new Splats, RefineStats); the trainer's optimizer state
        and RefineRecord are replaced.  `seed` (default: derived from iter) drives every random choice, so
        data-parallel ranks stay identical."""
        ctx = self.ctx or get_context(splats.device)
        dev = splats.device
        if self.state is None:
            raise BrushHipError("Can only refine if refine stats are initialized")  # train.rs:445
        splats.bake_min_scale(ctx)  # train.rs:433-437: refine manipulates the canonical (un-floored) params
        self.sync_refine_stats()
        if self.bounds is None:
            self.set_bounds(*splat_bounds(splats, ctx=ctx))
        c = self.config
        cfg = _ffi.BhRefineConfig()
        cfg.iter, cfg.total_train_iters = int(iter), max(int(c.total_train_iters), 1)
        cfg.growth_stop_iter = min(int(c.growth_stop_iter), int(c.total_train_iters))  # train.rs:150
        cfg.max_splats = int(c.max_splats)
        cfg.growth_grad_threshold, cfg.growth_select_fraction = c.growth_grad_threshold, c.growth_select_fraction
        cfg.split_at_screen_size, cfg.opac_decay = c.split_at_screen_size, c.opac_decay
        for k in range(3):
            cfg.bounds_center[k], cfg.bounds_extent[k] = self.bounds[0][k], self.bounds[1][k]
        cfg.seed = int(seed) if seed is not None else (0x5EED0000 + int(iter))
        st_in = self._train_state(splats, self.state)
        ff = self.feature_field
        if ff is not None and int(ff.features.shape[0]) != st_in.n:
            raise BrushHipError("refine: the feature field has %d rows, the splats %d" % (int(ff.features.shape[0]), st_in.n))
        rs = _ffi.BhRefineStats()
        ctx.check(ctx.lib.bh_refine_plan(ctx._h, C.byref(cfg), C.byref(st_in), C.byref(rs)))
        n2 = rs.total_splats
        z = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        coeffs = splats.sh_coeffs.shape[1]
        new = Splats(z(n2, 10), z(n2, coeffs, 3), z(n2), splats.render_mip, dev)
        ns = dict(m1_t=z(n2, 10), m2_t=z(n2, 10), m1_sh=z(n2, coeffs, 3), m2_sh=z(n2), m1_o=z(n2), m2_o=z(n2),
                  refine_weight_norm=z(n2), vis_weight=z(n2), max_screen_size=z(n2))
        st_out = self._train_state(new, ns)
        self.last_refine_plan = {k: _view(ctx.lib.bh_refine_plan_flags(ctx._h, i), (st_in.n,), torch.int32, dev).clone()
                                 for i, k in enumerate(("keep", "new_row", "split", "child_slot"))}
        if ff is not None:   # between plan and apply: the field's rows follow the plan (bh_refine_carry_rows)
            ff.carry(ctx, total_splats=n2)
        ctx.check(ctx.lib.bh_refine_apply(ctx._h, C.byref(cfg), C.byref(st_in), C.byref(st_out)))
        self.state = ns
        self.set_bounds(*splat_bounds(new, ctx=ctx))  # train.rs:634
        # train.rs:636-648: recompute the 3D-filter floor for the new positions / count unless frozen
        if float(iter) / float(max(int(c.total_train_iters), 1)) < self.MIN_SCALE_FREEZE_FRAC:
            f = self.compute_min_scale(new, ctx)
            if f is not None:
                new.with_min_scale(f)
        stats = RefineStats(rs.num_added, rs.num_split_oversized, rs.num_split_high_grad, rs.num_pruned, rs.num_pruned_non_finite,
                            rs.total_splats, rs.num_resampled)
        return new, stats

    def reduce_loss(self, stats: "TrainStepStats") -> float:
        """Tile-partitioned frame with the strip-wise loss: every rank holds its strip's share of the frame's loss;
        this sums the shares (a collective: call it on every rank).  Otherwise returns stats.loss."""
        if self.pg is not None and self.partition == "tiles" and self._strip_loss_now:
            import torch.distributed as dist
            t = torch.tensor([stats.loss], dtype=torch.float64, device=self.state["m2_o"].device)
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.pg)
            return float(t.item())
        if self.native_comm and self.partition == "tiles" and self._strip_loss_now:
            ctx = self.ctx or get_context(self.state["m2_o"].device)
            t = torch.tensor([stats.loss], dtype=torch.float32, device=self.state["m2_o"].device)
            if not ctx.uses_torch_stream:
                torch.cuda.current_stream(t.device).synchronize()
            ctx.allreduce_sum(t)
            ctx.sync()
            return float(t.item())
        return stats.loss

    def stats(self, ctx=None) -> TrainStepStats:
        """Resolve the stats of the last step (synchronises)."""
        (ctx or self.ctx or get_context()).sync()
        s = self._last_stats
        return TrainStepStats(s.num_visible, s.num_intersections, s.lr_mean, s.loss, s.exchange_rows)


# ---------------------------------------------------------------------------
# LOD decimation (brush-train/src/lod.rs; called at every LOD boundary, brush-process/src/train_stream.rs:248-303)
# ---------------------------------------------------------------------------
PUP_PLANES = 21   # lower-triangle entries of the 6x6 H: entry (i, k), i >= k, lives in plane i (i + 1) / 2 + k of the [21, N] accumulator


def lod_target_count(n: int, keep_pct: int) -> int:
    """`(before as f32 * lod_keep_pct as f32 / 100.0).max(1.0) as u32` (train_stream.rs:261), in f32 like the reference."""
    import numpy as np
    v = max(np.float32(n) * np.float32(keep_pct) / np.float32(100.0), np.float32(1.0))
    if v != v:   # `as u32` saturates: NaN -> 0, +inf / huge -> u32::MAX
        return 0
    return int(min(float(v), 4294967295.0))


def pup_accumulate(v_transforms, hessian=None, rows=None, ctx: Optional[Context] = None):
    """hessian [21, N] += J Jᵀ of the rows of v_transforms [N, 10] (J = columns 0..2 and 7..9), lod.rs:120-126; rows: optional
    device list of row ids (only those rows are added).  A new zero accumulator when hessian is None.  Returns the accumulator."""
    dev = v_transforms.device
    ctx = ctx or get_context(dev)
    v = _f32c(v_transforms, dev).reshape(-1, 10)
    n = v.shape[0]
    if hessian is None:
        hessian = torch.zeros((PUP_PLANES, n), dtype=torch.float32, device=dev)
    if tuple(hessian.shape) != (PUP_PLANES, n) or hessian.dtype != torch.float32 or not hessian.is_contiguous():
        raise ValueError("hessian must be a contiguous f32 [21, N] tensor")
    r = None if rows is None else _as_u32(rows, dev).reshape(-1)
    ctx.check(ctx.lib.bh_pup_accumulate(ctx._h, _ptr(v), n, _ptr(r) if r is not None else None, 0 if r is None else r.numel(), _ptr(hessian)))
    return hessian


def pup_scores(hessian, ctx: Optional[Context] = None):
    """log_det_6x6 (lod.rs:44-70) of every splat's accumulated H ([21, N]) -> scores [N] f32 (-inf: not positive definite)."""
    dev = hessian.device
    ctx = ctx or get_context(dev)
    h = _f32c(hessian, dev)
    if h.dim() != 2 or h.shape[0] != PUP_PLANES:
        raise ValueError("hessian must be [21, N]")
    n = h.shape[1]
    scores = torch.empty((n,), dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.bh_pup_scores(ctx._h, _ptr(h), n, _ptr(scores)))
    return scores


def pup_accumulate_view(splats: "Splats", camera, gt_packed, hessian, ctx: Optional[Context] = None):
    """One view of compute_pup_scores (bh_pup_accumulate_view): forward, L1 loss against gt_packed ([H, W] rgba8 as int32),
    backward, hessian += J Jᵀ over the visible splats.  Makes the ctx's last unretained forward stale."""
    dev = splats.device
    ctx = ctx or get_context(dev)
    gt = _as_u32(gt_packed, dev)
    h, w = gt.shape
    cam = camera if isinstance(camera, _ffi.BhCamera) else camera.uniforms((w, h))
    n = splats.num_splats()
    if tuple(hessian.shape) != (PUP_PLANES, n) or hessian.dtype != torch.float32 or not hessian.is_contiguous():
        raise ValueError("hessian must be a contiguous f32 [21, N] tensor")
    ms = splats.min_scale
    ctx.check(ctx.lib.bh_pup_accumulate_view(ctx._h, C.byref(cam), n, splats.sh_degree(), _ptr(splats.transforms), _ptr(splats.sh_coeffs),
                                             _ptr(splats.raw_opacities), _ptr(ms) if ms is not None else None,
                                             _ffi.FLAG_MIP if splats.render_mip else 0, _ptr(gt), _ptr(hessian)))
    return hessian


def compute_pup_scores(splats: "Splats", views, ctx: Optional[Context] = None, return_hessian=False):
    """compute_pup_scores (lod.rs:78-142): PUP sensitivity score of every splat over the training views -> scores [N] f32 on the
    device (and the [21, N] accumulator with return_hessian).  `views` has SceneLoader's shape: (image uint8 [H,W,3|4] or a
    callable returning one, Camera[, alpha_is_mask]); the GT is packed like view_to_packed_data (premultiplied unless the alpha is a
    mask) through a BatchUploader.  One bh_pup_accumulate_view per view, in list order, then bh_pup_scores."""
    import numpy as np
    dev = splats.device
    ctx = ctx or get_context(dev)
    n = splats.num_splats()
    hessian = torch.zeros((PUP_PLANES, n), dtype=torch.float32, device=dev)
    up = None
    try:
        for view in views:
            img = view[0]() if callable(view[0]) else view[0]
            img = np.ascontiguousarray(img, dtype=np.uint8)
            mask = bool(view[2]) if len(view) > 2 else False
            pixels = img.shape[0] * img.shape[1]
            if up is None or up.max_pixels < pixels:
                if up is not None:
                    ctx.sync()   # (the slots of the old ring may still be read by queued views)
                    up.close()
                up = BatchUploader(pixels, 2, ctx)
            slot = up.submit(img, premultiply=not mask)
            gt, _ = up.acquire(slot)
            pup_accumulate_view(splats, view[1], gt, hessian, ctx)
            up.release(slot)
        scores = pup_scores(hessian, ctx)
    finally:
        if up is not None:
            ctx.sync()
            up.close()
    return (scores, hessian) if return_hessian else scores


def decimate_to_count(splats: "Splats", scores, target_count: int, ctx: Optional[Context] = None, return_indices=False):
    """decimate_to_count (lod.rs:13-38): new Splats of the target_count highest-scored splats in score-descending order (ties:
    ascending index; NaN after -inf).  min_scale, when set, is gathered too.  target_count >= N returns `splats` itself.
    return_indices: also the kept source rows (int32 [K] device)."""
    dev = splats.device
    ctx = ctx or get_context(dev)
    n = splats.num_splats()
    s = _f32c(scores, dev).reshape(-1)
    if s.numel() != n:
        raise ValueError("one score per splat")
    target_count = int(target_count)
    if target_count >= n:
        return (splats, torch.arange(n, dtype=torch.int32, device=dev)) if return_indices else splats
    k = max(target_count, 0)
    c = splats.sh_coeffs.shape[1]
    ot = torch.empty((k, 10), dtype=torch.float32, device=dev)
    osh = torch.empty((k, c, 3), dtype=torch.float32, device=dev)
    oo = torch.empty((k,), dtype=torch.float32, device=dev)
    oms = None if splats.min_scale is None else torch.empty((k,), dtype=torch.float32, device=dev)
    idx = torch.empty((k,), dtype=torch.int32, device=dev)
    ms = splats.min_scale
    ctx.check(ctx.lib.bh_decimate_to_count(ctx._h, _ptr(s), n, k, c, _ptr(splats.transforms), _ptr(splats.sh_coeffs), _ptr(splats.raw_opacities),
                                           _ptr(ms) if ms is not None else None, _ptr(ot), _ptr(osh), _ptr(oo),
                                           _ptr(oms) if oms is not None else None, _ptr(idx)))
    out = Splats(ot, osh, oo, splats.render_mip, dev, oms)
    return (out, idx) if return_indices else out


# ---------------------------------------------------------------------------
# scene editing: similarity transform with SH rotation, region crop (include/brush_hip_scene.h)
# ---------------------------------------------------------------------------
class SceneTransform:
    """The similarity x' = s R x + t (R a proper rotation, s > 0) as the library's record: f64 (q, t, s) and everything the kernel reads,
    the rotation matrices of the SH bands 1..4 included.  Every operation is one of the C functions of include/brush_hip_scene.h."""

    def __init__(self, record: Optional["_ffi.BhSceneTransform"] = None):
        if record is None:
            record = SceneTransform.from_quat()._rec
        self._rec = record

    @staticmethod
    def from_quat(q_wxyz=(1.0, 0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0), s=1.0) -> "SceneTransform":
        """R from the quaternion (w, x, y, z) — normalised by the library — translation t, scale s."""
        rec = _ffi.BhSceneTransform()
        q = (C.c_double * 4)(*[float(v) for v in q_wxyz])
        tt = (C.c_double * 3)(*[float(v) for v in t])
        if _ffi.load().bh_scene_transform_make(q, tt, float(s), C.byref(rec)) != 0:
            raise BrushHipError("bh_scene_transform_make: the quaternion must be finite and not zero, the translation finite, the scale a finite number > 0")
        return SceneTransform(rec)

    @staticmethod
    def from_matrix(m, tol=1e-6) -> "SceneTransform":
        """From a 4x4 matrix [[s R, t], [0, 0, 0, 1]].  Refused (ValueError): a last row that differs from (0, 0, 0, 1) by more than
        `tol`; a 3x3 block A whose determinant is not > 0 (a reflection); shear or non-uniform scale, i.e. an entry of
        A^T A / s^2 - I above `tol` with s = det(A)^(1/3).  The default 1e-6 admits a matrix that was stored in f32."""
        import numpy as np
        m = np.asarray(m.detach().cpu().numpy() if torch.is_tensor(m) else m, np.float64)
        if m.shape != (4, 4) or not np.isfinite(m).all():
            raise ValueError("from_matrix: a finite 4x4 matrix")
        if np.abs(m[3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > tol:
            raise ValueError("from_matrix: the last row must be (0, 0, 0, 1)")
        a = m[:3, :3]
        det = float(np.linalg.det(a))
        if not det > 0.0:
            raise ValueError("from_matrix: the determinant must be > 0 (no reflections)")
        s = det ** (1.0 / 3.0)
        r = a / s
        if np.abs(r.T @ r - np.eye(3)).max() > tol:
            raise ValueError("from_matrix: shear or non-uniform scale (A^T A / s^2 differs from I by more than %g)" % tol)
        q = [1 + r[0, 0] + r[1, 1] + r[2, 2], 1 + r[0, 0] - r[1, 1] - r[2, 2], 1 - r[0, 0] + r[1, 1] - r[2, 2], 1 - r[0, 0] - r[1, 1] + r[2, 2]]
        k = q.index(max(q))   # the best-conditioned of the four quaternion extractions, (w, x, y, z)
        if k == 0:
            quat = (q[0], r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1])
        elif k == 1:
            quat = (r[2, 1] - r[1, 2], q[1], r[1, 0] + r[0, 1], r[0, 2] + r[2, 0])
        elif k == 2:
            quat = (r[0, 2] - r[2, 0], r[1, 0] + r[0, 1], q[2], r[2, 1] + r[1, 2])
        else:
            quat = (r[1, 0] - r[0, 1], r[0, 2] + r[2, 0], r[2, 1] + r[1, 2], q[3])
        return SceneTransform.from_quat(quat, m[:3, 3], s)

    def as_struct(self) -> "_ffi.BhSceneTransform":
        return self._rec

    @property
    def quat(self):
        return tuple(self._rec.q)

    @property
    def translation(self):
        return tuple(self._rec.t)

    @property
    def scale(self):
        return float(self._rec.s)

    def inverse(self) -> "SceneTransform":
        rec = _ffi.BhSceneTransform()
        if _ffi.load().bh_scene_transform_invert(C.byref(self._rec), C.byref(rec)) != 0:
            raise BrushHipError("bh_scene_transform_invert failed")
        return SceneTransform(rec)

    def __matmul__(self, other: "SceneTransform") -> "SceneTransform":
        """self @ other applies `other` first."""
        rec = _ffi.BhSceneTransform()
        if _ffi.load().bh_scene_transform_compose(C.byref(self._rec), C.byref(other._rec), C.byref(rec)) != 0:
            raise BrushHipError("bh_scene_transform_compose failed: the product is no transform (scale out of range?)")
        return SceneTransform(rec)

    def matrix(self):
        """[[s R, t], [0, 0, 0, 1]] as a 4x4 float64 numpy array, from the record's f64 fields."""
        import numpy as np
        w, x, y, z = self._rec.q
        r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)
        m = np.eye(4)
        m[:3, :3] = self._rec.s * r
        m[:3, 3] = list(self._rec.t)
        return m

    def sh_rotation(self, l: int):
        """D_l, the (2l+1) x (2l+1) float32 matrix that turns the SH coefficients of band l (1..4) with the scene."""
        import numpy as np
        l = int(l)
        if not 1 <= l <= 4:
            raise ValueError("sh_rotation: band 1..4")
        first = (0, 0, 9, 34, 83)[l]
        m = 2 * l + 1
        return np.array(self._rec.sh_rot[first:first + m * m], np.float32).reshape(m, m)


@dataclass
class SceneRegion:
    """An oriented box or an ellipsoid, and an opacity floor (BhSceneRegion): `rotation` is 3x3 row-major with the region's axes in
    world coordinates as its columns; invert keeps the outside; min_raw_opacity drops splats whose raw opacity (logit) is below it."""
    kind: str = "box"   # "box" | "ellipsoid"
    center: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    half_extent: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    rotation: Tuple[float, ...] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    invert: bool = False
    min_raw_opacity: float = -math.inf

    def as_struct(self) -> "_ffi.BhSceneRegion":
        kinds = {"box": _ffi.REGION_BOX, "ellipsoid": _ffi.REGION_ELLIPSOID}
        if self.kind not in kinds:
            raise ValueError("SceneRegion.kind: 'box' or 'ellipsoid'")
        rot = [float(v) for row in self.rotation for v in (row if hasattr(row, "__len__") else (row,))]
        if len(rot) != 9 or len(self.center) != 3 or len(self.half_extent) != 3:
            raise ValueError("SceneRegion: center [3], half_extent [3], rotation 3x3")
        g = _ffi.BhSceneRegion(kind=kinds[self.kind], invert=int(bool(self.invert)), min_raw_opacity=float(self.min_raw_opacity))
        g.center[:] = [float(v) for v in self.center]
        g.half_extent[:] = [float(v) for v in self.half_extent]
        g.rot[:] = rot
        return g


def select_region(splats: "Splats", region: SceneRegion, ctx: Optional[Context] = None, return_count=False):
    """keep [N] f32 device: 1.0 where the splat's mean lies in the region (outside with invert) and its raw opacity is not below the
    floor, 0.0 elsewhere (bh_splats_select_region).  return_count: also the number kept (one blocking readback)."""
    dev = splats.device
    ctx = ctx or get_context(dev)
    n = splats.num_splats()
    keep = torch.empty((n,), dtype=torch.float32, device=dev)
    count = C.c_uint32(0)
    ctx.check(ctx.lib.bh_splats_select_region(ctx._h, C.byref(region.as_struct()), _ptr(splats.transforms), _ptr(splats.raw_opacities), n, _ptr(keep),
                                              C.byref(count) if return_count else None))
    return (keep, int(count.value)) if return_count else keep


def crop_splats(splats: "Splats", region: SceneRegion, return_indices=False, ctx: Optional[Context] = None):
    """New Splats of the rows select_region keeps, in source order: select, count, decimate_to_count (whose ties keep ascending
    index).  return_indices: also the kept source rows (int32 [K] device)."""
    ctx = ctx or get_context(splats.device)
    keep, count = select_region(splats, region, ctx=ctx, return_count=True)
    return decimate_to_count(splats, keep, count, ctx=ctx, return_indices=return_indices)


# ---------------------------------------------------------------------------
# mask lifting: per-splat blend-weight votes from 2-D label maps (include/brush_hip_lift.h)
# ---------------------------------------------------------------------------
class LiftAccumulator:
    """The tables of a mask lifting over any number of views (include/brush_hip_lift.h): `votes` int64 [N,L] — the library's u64,
    the same bits while below 2^63 — with votes[i, l] = the sum over views and pixels of label l of the blend weight of splat i in
    units of 2^-24, and with stats=True `max_weight` f32 [N] (the largest weight the splat had at a pixel) and `pixel_count` int32 [N]
    (the number of pixels it reached).  Integer sums: the same bits whatever the order of views, tiles or calls."""

    def __init__(self, n, num_labels, device=None, stats=True, ctx: Optional[Context] = None):
        n, num_labels = int(n), int(num_labels)
        if not 1 <= num_labels <= _ffi.LIFT_MAX_LABELS:
            raise BrushHipError("LiftAccumulator: num_labels must be 1 .. %d" % _ffi.LIFT_MAX_LABELS)
        self.ctx = ctx or get_context(device)
        self.device = self.ctx.device if device is None else device
        self.n, self.num_labels = n, num_labels
        self.votes = torch.zeros((n, num_labels), dtype=torch.int64, device=self.device)
        self.max_weight = torch.zeros((n,), dtype=torch.float32, device=self.device) if stats else None
        self.pixel_count = torch.zeros((n,), dtype=torch.int32, device=self.device) if stats else None

    def clear(self):
        for t in (self.votes, self.max_weight, self.pixel_count):
            if t is not None:
                t.zero_()
        return self

    def add(self, node: "RenderNode", labels=None):
        """One view's votes (bh_lift_accumulate): `node` a BH_FLAG_BWD_INFO forward of the accumulator's splats, the ctx's most recent or
        a retained one; `labels` uint8 [H,W] (a value >= num_labels, 255 by convention, votes nowhere) or None: label 0 everywhere."""
        if node.splats.num_splats() != self.n:
            raise BrushHipError("LiftAccumulator.add: the node renders %d splats, the tables hold %d" % (node.splats.num_splats(), self.n))
        w, h = node.img_size
        if labels is not None:
            labels = torch.as_tensor(labels, device=self.device)
            if labels.dtype != torch.uint8 or tuple(labels.shape) != (h, w):
                raise BrushHipError("LiftAccumulator.add: labels must be uint8 [%d, %d]" % (h, w))
            labels = labels.contiguous()
        ctx = node.ctx
        ctx.check(ctx.lib.bh_lift_accumulate(ctx._h, C.byref(node.out), _ptr(labels) if labels is not None else None, self.num_labels,
                                             _ptr(self.votes), _ptr(self.max_weight) if self.max_weight is not None else None,
                                             _ptr(self.pixel_count) if self.pixel_count is not None else None))
        return self

    def weights(self):
        """f32 [N,L] = votes / 2^24: the summed blend weights (exact in f64 below 2^53 raw units, then rounded once)."""
        return (self.votes.to(torch.float64) * (1.0 / _ffi.LIFT_VOTE_ONE)).to(torch.float32)

    def assign(self, min_weight=0.0, return_share=False):
        """uint8 [N]: the label with the most votes per splat, ties to the lowest (bh_lift_assign); 255 where the splat's summed weight is
        0 or below min_weight.  return_share: also f32 [N], the winning label's share of the row's total (+0 where unassigned)."""
        out = torch.empty((self.n,), dtype=torch.uint8, device=self.device)
        share = torch.empty((self.n,), dtype=torch.float32, device=self.device) if return_share else None
        self.ctx.check(self.ctx.lib.bh_lift_assign(self.ctx._h, _ptr(self.votes), self.n, self.num_labels, float(min_weight), _ptr(out),
                                                   _ptr(share) if share is not None else None))
        return (out, share) if return_share else out

    def select(self, label=None, min_share=0.5, min_weight=0.0, min_max_weight=0.0, min_pixels=0, invert=False):
        """keep f32 [N], 1.0 / 0.0 (bh_lift_select), what compact_splats and decimate_to_count take: the splat got a vote and at least
        min_weight in all; with a `label`, that label holds at least min_share of the splat's votes; min_max_weight / min_pixels > 0
        test the two statistics (stats=True).  Every test asked for must pass; invert flips the result."""
        sel = _ffi.BhLiftSelect(label=_ffi.LIFT_ANY_LABEL if label is None else int(label), min_share=float(min_share), min_weight=float(min_weight),
                                min_max_weight=float(min_max_weight), min_pixels=int(min_pixels), invert=1 if invert else 0)
        keep = torch.empty((self.n,), dtype=torch.float32, device=self.device)
        self.ctx.check(self.ctx.lib.bh_lift_select(self.ctx._h, _ptr(self.votes), _ptr(self.max_weight) if self.max_weight is not None else None,
                                                   _ptr(self.pixel_count) if self.pixel_count is not None else None, self.n, self.num_labels,
                                                   C.byref(sel), _ptr(keep)))
        return keep


def lift_labels(splats: "Splats", views, num_labels, img_size, pass_: "RasterPass" = None, ctx: Optional[Context] = None, stats=True):
    """Lifts 2-D label maps onto `splats`: `views` yields (camera, labels uint8 [H,W] or None); each view is a BH_FLAG_BWD_INFO
    forward on black (as fuse_views renders its views) whose votes join one LiftAccumulator, which is returned."""
    pass_ = RasterPass.Backward if pass_ is None else pass_
    ctx = ctx or get_context(splats.device)
    w, h = int(img_size[0]), int(img_size[1])
    acc = LiftAccumulator(splats.num_splats(), num_labels, splats.device, stats=stats, ctx=ctx)
    for camera, labels in views:
        acc.add(render_splats_diff(splats, camera, (w, h), (0.0, 0.0, 0.0), pass_, ctx=ctx), labels)
    return acc


def compact_splats(splats: "Splats", keep, return_indices=False, ctx: Optional[Context] = None):
    """New Splats of the rows where keep [N] (1.0 / 0.0: LiftAccumulator.select, select_region) is not 0, in source order: count
    (one blocking readback of keep), then decimate_to_count, whose ties keep ascending index.  return_indices: also the kept source
    rows (int32 [K] device), which serve FeatureField.gather."""
    ctx = ctx or get_context(splats.device)
    keep = _f32c(keep, splats.device).reshape(-1)
    if keep.numel() != splats.num_splats():
        raise ValueError("one keep value per splat")
    count = int(torch.count_nonzero(keep).item())
    return decimate_to_count(splats, keep, count, ctx=ctx, return_indices=return_indices)


# ---------------------------------------------------------------------------
# held-out evaluation (brush-train/src/eval.rs:23-63, run_eval of brush-process/src/train_stream.rs:506-566)
# ---------------------------------------------------------------------------
@dataclass
class EvalSample:
    """EvalSample (eval.rs:14-20) of one view: mse, psnr and ssim read back from `metrics`, the device [3] f32 tensor (mse, psnr,
    ssim) bh_eval_view wrote; `image` (keep_image) is the quantised render as rgba8 [H, W] (int32 bit pattern, alpha 255)."""
    mse: float
    psnr: float
    ssim: float
    metrics: torch.Tensor
    image: Optional[torch.Tensor] = None


@dataclass
class EvalResult:
    """What run_eval reports (train_stream.rs:559-560): the per-view PSNRs and SSIMs averaged in f32, and the per-view table
    [V, 3] (mse, psnr, ssim) on the host; `images` (keep_images) the views' rgba8 renders, in view order."""
    avg_psnr: float
    avg_ssim: float
    per_view: torch.Tensor
    images: Optional[list] = None
    # views that carry depth (run_eval): [V, 4] (abs-rel, RMSE, share within 1.25, valid pixels) on the host, NaN rows for views
    # without depth, and the mean abs-rel over the views that have one; None when no view carries depth
    depth_per_view: Optional[torch.Tensor] = None
    avg_depth_abs_rel: Optional[float] = None


def _aligned_hwc4(img_hwc4, dev):
    img = _f32c(img_hwc4, dev)
    if img.dim() != 3 or img.shape[2] != 4:
        raise ValueError("img must be [H,W,4]")
    return img if img.data_ptr() % 16 == 0 else img.clone()   # (float4 loads: a sliced view may start off a 16-byte boundary)


def eval_metrics(img_hwc4, gt_packed, ctx: Optional[Context] = None, keep_image=False, out=None):
    """eval_stats' metrics (eval.rs:38-55) of a rendered [H, W, 4] f32 image against gt_packed ([H, W] rgba8 as int32), in one fused
    kernel (bh_eval_metrics): -> device f32 [3] = (mse, psnr, ssim), written into `out` when given; with keep_image also the
    quantised RGB as rgba8 [H, W].  Queued on the ctx stream: nothing is read back."""
    dev = img_hwc4.device
    ctx = ctx or get_context(dev)
    img = _aligned_hwc4(img_hwc4, dev)
    h, w = int(img.shape[0]), int(img.shape[1])
    gt = _as_u32(gt_packed, dev).reshape(h, w)
    metrics = out if out is not None else torch.empty((3,), dtype=torch.float32, device=dev)
    rgb8 = torch.empty((h, w), dtype=torch.int32, device=dev) if keep_image else None
    ctx.check(ctx.lib.bh_eval_metrics(ctx._h, _ptr(img), _ptr(gt), h, w, _ptr(metrics), _ptr(rgb8) if rgb8 is not None else None))
    return (metrics, rgb8) if keep_image else metrics


def _eval_view(ctx, splats, camera, gt, metrics, rgb8):
    h, w = int(gt.shape[0]), int(gt.shape[1])
    cam = camera if isinstance(camera, _ffi.BhCamera) else camera.uniforms((w, h))
    ms = splats.min_scale
    ctx.check(ctx.lib.bh_eval_view(ctx._h, C.byref(cam), splats.num_splats(), splats.sh_degree(), _ptr(splats.transforms), _ptr(splats.sh_coeffs),
                                   _ptr(splats.raw_opacities), _ptr(ms) if ms is not None else None, _ffi.FLAG_MIP if splats.render_mip else 0,
                                   _ptr(gt), _ptr(metrics), _ptr(rgb8) if rgb8 is not None else None))


def eval_stats(splats: "Splats", camera, gt_packed, ctx: Optional[Context] = None, keep_image=False) -> EvalSample:
    """eval_stats (eval.rs:23-63) of one view through bh_eval_view: render (background 0, f32, the 3D-filter floor folded in) and
    score against gt_packed ([H, W] rgba8 as int32, packed like view_to_packed_data).  Reads the three metrics back.  Makes the
    ctx's last unretained forward stale."""
    dev = splats.device
    ctx = ctx or get_context(dev)
    gt = _as_u32(gt_packed, dev)
    if gt.dim() != 2:
        raise ValueError("gt_packed must be [H, W]")
    metrics = torch.empty((3,), dtype=torch.float32, device=dev)
    rgb8 = torch.empty(tuple(gt.shape), dtype=torch.int32, device=dev) if keep_image else None
    _eval_view(ctx, splats, camera, gt, metrics, rgb8)
    ctx.sync()
    mse, psnr, ssim = (float(v) for v in metrics.cpu())
    return EvalSample(mse=mse, psnr=psnr, ssim=ssim, metrics=metrics, image=rgb8)


def run_eval(splats: "Splats", views, ctx: Optional[Context] = None, keep_images=False, envmap: Optional["EnvironmentMap"] = None) -> EvalResult:
    """run_eval (train_stream.rs:506-566): eval_stats of every held-out view, the per-view PSNR and SSIM averaged in f32 (not the
    PSNR of a mean MSE).  `views` has compute_pup_scores' shape: (image uint8 [H,W,3|4] or a callable returning one, Camera[,
    alpha_is_mask[, depth]]), packed through a BatchUploader.  Every view's metrics go to its row of one device table; one readback at
    the end.  `depth`: the view's depth map [H,W] f32, or a dict(depth=, kind="l1", scale=1.0, offset=0.0): such a view is also
    rendered differentiably for its expected depth and scored by eval_depth_metrics (EvalResult.depth_per_view).  `envmap`: the scene's
    EnvironmentMap: every view is then rendered on black (render_splats), composited over the map and scored by eval_metrics; the
    3D-filter floor bh_eval_view folds in is not applied on that path."""
    import numpy as np
    dev = splats.device
    ctx = ctx or get_context(dev)
    views = list(views)
    table = torch.empty((len(views), 3), dtype=torch.float32, device=dev)
    depth_table = None
    images = [] if keep_images else None
    up = None
    try:
        for i, view in enumerate(views):
            img = view[0]() if callable(view[0]) else view[0]
            img = np.ascontiguousarray(img, dtype=np.uint8)
            mask = bool(view[2]) if len(view) > 2 else False
            pixels = img.shape[0] * img.shape[1]
            if up is None or up.max_pixels < pixels:
                if up is not None:
                    ctx.sync()   # (the slots of the old ring may still be read by queued views)
                    up.close()
                up = BatchUploader(pixels, 2, ctx)
            slot = up.submit(img, premultiply=not mask)
            gt, _ = up.acquire(slot)
            rgb8 = torch.empty(tuple(gt.shape), dtype=torch.int32, device=dev) if keep_images else None
            if envmap is None:
                _eval_view(ctx, splats, view[1], gt, table[i], rgb8)
            else:
                frame, _ = render_splats(splats, view[1], (img.shape[1], img.shape[0]), (0.0, 0.0, 0.0), RasterPass.Backward, ctx=ctx)
                scored = eval_metrics(envmap.composite(frame, view[1], out=frame), gt, ctx=ctx, keep_image=keep_images, out=table[i])
                rgb8 = scored[1] if keep_images else None
            up.release(slot)
            if keep_images:
                images.append(rgb8)
            dv = view[3] if len(view) > 3 else None
            if dv is not None:
                dv = dv if isinstance(dv, dict) else dict(depth=dv)
                if depth_table is None:
                    depth_table = torch.full((len(views), 4), float("nan"), dtype=torch.float32, device=dev)
                    if not ctx.uses_torch_stream:
                        torch.cuda.current_stream(dev).synchronize()   # the fill ran on torch's stream, the metrics on the ctx's own
                node = render_splats_diff(splats, view[1], (img.shape[1], img.shape[0]), ctx=ctx)
                eval_depth_metrics(node.depth("expected"), torch.as_tensor(dv["depth"]).to(dev), dv.get("kind", "l1"), dv.get("scale", 1.0),
                                   dv.get("offset", 0.0), ctx=ctx, out=depth_table[i])
    finally:
        if up is not None:
            ctx.sync()
            up.close()
    per_view = table.cpu()
    psnr, ssim = np.float32(0.0), np.float32(0.0)
    for r in per_view.numpy():   # train_stream.rs:540-541: psnr += the view's psnr (f32), in view order
        psnr = np.float32(psnr + r[1])
        ssim = np.float32(ssim + r[2])
    with np.errstate(invalid="ignore", divide="ignore"):
        psnr = np.float32(psnr / np.float32(len(views)))   # :559-560 (no views: 0 / 0 = NaN, as in the reference)
        ssim = np.float32(ssim / np.float32(len(views)))
    res = EvalResult(avg_psnr=float(psnr), avg_ssim=float(ssim), per_view=per_view, images=images)
    if depth_table is not None:
        res.depth_per_view = depth_table.cpu()
        rows = res.depth_per_view.numpy()
        res.avg_depth_abs_rel = float(np.mean(rows[~np.isnan(rows[:, 0]), 0], dtype=np.float64))
    return res


# ---------------------------------------------------------------------------
# LPIPS (crates/lpips/src/lib.rs; the lpips_loss_weight term of brush-train/src/train.rs:153, 265-273)
# ---------------------------------------------------------------------------
LPIPS_CONVS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
               (512, 512), (512, 512), (512, 512))   # (Cin, Cout) in forward order
LPIPS_BLOCK_CONVS = (2, 2, 3, 3, 3)
LPIPS_HEAD_CHANNELS = (64, 128, 256, 512, 512)
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
# the torch `lpips` package's VGG: conv i of block b sits at features index _LPIPS_TORCH_IDX[b][i] of net.slice{b+1}
_LPIPS_TORCH_IDX = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))


def _np32(t):
    import numpy as np
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu()
    return np.asarray(t, dtype=np.float32)


class Lpips:
    """LpipsModel (crates/lpips/src/lib.rs) on one device: the 13 VGG16 convs and 5 heads, uploaded and repacked once
    (bh_lpips_create).  Parameters in canonical order (`flat`, LPIPS_PARAM_COUNT f32): per conv weight [Cout,Cin,3,3] then bias
    [Cout], then the heads [C].  No weights ship with the library: load them with from_state_dict, or Lpips.random for tests."""

    def __init__(self, flat, ctx: Optional[Context] = None):
        import numpy as np
        flat = np.ascontiguousarray(_np32(flat).reshape(-1))
        ctx = ctx or get_context()
        self.ctx = ctx
        self.device = ctx.device
        self.lib = ctx.lib
        h = ctx.lib.bh_lpips_create(ctx._h, flat.ctypes.data_as(C.POINTER(C.c_float)), int(flat.size))
        if not h:
            raise BrushHipError("bh_lpips_create: %s" % ctx.lib.bh_last_error(ctx._h).decode())
        self._h = C.c_void_p(h)

    @classmethod
    def from_params(cls, flat, ctx: Optional[Context] = None) -> "Lpips":
        return cls(flat, ctx)

    @classmethod
    def from_state_dict(cls, sd, ctx: Optional[Context] = None) -> "Lpips":
        """From the reference's burn field names (blocks.{b}.convs.{j}.{weight,bias}, heads.{b}.weight) or the torch `lpips`
        package's (net.slice{s}.{idx}.{weight,bias}, lin{b}.model.1.weight; scaling_layer.shift / scale, if present, must be the
        constants this model hard-codes)."""
        return cls(cls.flat_from_state_dict(sd), ctx)

    @staticmethod
    def flat_from_state_dict(sd):
        import numpy as np
        burn = any(k.startswith("blocks.") for k in sd)
        if not burn:
            for name, want in (("scaling_layer.shift", LPIPS_SHIFT), ("scaling_layer.scale", LPIPS_SCALE)):
                if name in sd and not np.allclose(_np32(sd[name]).reshape(-1), np.asarray(want, np.float32), rtol=0, atol=1e-6):
                    raise ValueError("%s is %s, this model hard-codes %s" % (name, _np32(sd[name]).reshape(-1), want))
        parts = []
        L = 0
        for b, n in enumerate(LPIPS_BLOCK_CONVS):
            for j in range(n):
                ci, co = LPIPS_CONVS[L]
                key = "blocks.%d.convs.%d" % (b, j) if burn else "net.slice%d.%d" % (b + 1, _LPIPS_TORCH_IDX[b][j])
                w, bias = _np32(sd[key + ".weight"]), _np32(sd[key + ".bias"])
                if w.shape != (co, ci, 3, 3) or bias.shape != (co,):
                    raise ValueError("%s: shape %s / %s, expected (%d, %d, 3, 3) / (%d,)" % (key, w.shape, bias.shape, co, ci, co))
                parts += [w.reshape(-1), bias]
                L += 1
        for b, c in enumerate(LPIPS_HEAD_CHANNELS):
            key = "heads.%d.weight" % b if burn else "lin%d.model.1.weight" % b
            h = _np32(sd[key])
            if h.size != c:
                raise ValueError("%s: %d values, expected %d" % (key, h.size, c))
            parts.append(h.reshape(-1))
        flat = np.concatenate(parts)
        assert flat.size == _ffi.LPIPS_PARAM_COUNT
        return flat

    @staticmethod
    def random_params(seed=0):
        """Test weights (not a trained model): He-normal convs, small biases, non-negative heads, so that activations stay O(1)."""
        import numpy as np
        rng = np.random.default_rng(seed)
        parts = []
        for ci, co in LPIPS_CONVS:
            parts.append((rng.standard_normal(co * ci * 9) * math.sqrt(2.0 / (9 * ci))).astype(np.float32))
            parts.append((rng.uniform(-0.05, 0.05, co)).astype(np.float32))
        for c in LPIPS_HEAD_CHANNELS:
            parts.append((np.abs(rng.standard_normal(c)) * 0.1).astype(np.float32))
        return np.concatenate(parts)

    @classmethod
    def random(cls, seed=0, ctx: Optional[Context] = None) -> "Lpips":
        return cls(cls.random_params(seed), ctx)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.bh_lpips_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _lpips_args(img_hwc4, gt_packed, composite_bg, dev):
    img = _aligned_hwc4(img_hwc4, dev)
    h, w = int(img.shape[0]), int(img.shape[1])
    gt = _as_u32(gt_packed, dev).reshape(h, w)
    bg = (C.c_float * 3)(*[float(v) for v in composite_bg]) if composite_bg is not None else None
    return img, gt, h, w, bg


def lpips(img_hwc4, gt_packed, model: Lpips, composite_bg=None, ctx: Optional[Context] = None):
    """LpipsModel::lpips(img rgb, unpack_gt_rgb(gt_packed, composite_bg)) -> device f32 [1] (bh_lpips_forward).  img_hwc4 [H,W,4]
    f32 (alpha ignored), gt_packed [H,W] rgba8 as int32; H, W >= 16.  Queued on the ctx stream: nothing is read back."""
    dev = img_hwc4.device
    ctx = ctx or get_context(dev)
    img, gt, h, w, bg = _lpips_args(img_hwc4, gt_packed, composite_bg, dev)
    value = torch.empty((1,), dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.bh_lpips_forward(ctx._h, model._h, _ptr(img), _ptr(gt), h, w, bg, _ptr(value)))
    return value


def lpips_value_and_grad(img_hwc4, gt_packed, model: Lpips, composite_bg=None, weight=1.0, v_output=None, ctx: Optional[Context] = None):
    """(LPIPS [1], v_output [H,W,4]) with v_output.rgb += weight * dLPIPS/dimg (bh_lpips_value_and_grad); v_output defaults to
    zeros and is updated in place when given."""
    dev = img_hwc4.device
    ctx = ctx or get_context(dev)
    img, gt, h, w, bg = _lpips_args(img_hwc4, gt_packed, composite_bg, dev)
    value = torch.empty((1,), dtype=torch.float32, device=dev)
    if v_output is None:
        v_output = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    if v_output.shape != (h, w, 4) or v_output.dtype != torch.float32 or not v_output.is_contiguous():
        raise ValueError("v_output must be a contiguous f32 [H,W,4]")
    ctx.check(ctx.lib.bh_lpips_value_and_grad(ctx._h, model._h, _ptr(img), _ptr(gt), h, w, bg, float(weight), _ptr(value), _ptr(v_output)))
    return value, v_output


# ---------------------------------------------------------------------------
# point-cloud initialisation (brush-train/src/splat_init.rs:179-242, brush-process/src/train_stream.rs:100-123)
# ---------------------------------------------------------------------------
def ply_vertex_has_property(data: bytes, name: str) -> bool:
    """Whether the PLY's vertex element has property `name` (host only).  has_property("scale_0") is how import.rs:332 decides
    that SplatData::log_scales is None; a SuperSplat-compressed file always has scales."""
    rc = _ffi.load().bh_ply_vertex_has_property(data, len(data), name.encode())
    if rc < 0:
        raise BrushHipError("malformed or unsupported PLY (%d)" % rc)
    return rc == 1


def knn_log_scales(splats_or_transforms, ctx: Optional[Context] = None, return_distances=False, return_stats=False):
    """compute_knn_scales (splat_init.rs:179-216) on the device: per row ln(clamp((d1 + d2) / 4, 1e-3, 0.1 median_size)), d1 <= d2
    the f32 distances to the two nearest other rows, median_size from the 0.75-percentile box; n < 3 gives 0.  A non-finite row is
    nobody's neighbour and a missing neighbour is at +inf (such rows get the upper clamp).
    A Splats is updated in place (transforms columns 7..9); a tensor ([N,10] transforms or [N,3] means) is not modified.
    Returns log_scales [N,3] f32 (the three columns are equal), then nn_dist [N,2] (d1, d2) with return_distances, then
    {"pairs_tested": distance evaluations performed} with return_stats."""
    if isinstance(splats_or_transforms, Splats):
        dev = splats_or_transforms.device
        tr = splats_or_transforms.transforms
    else:
        t = splats_or_transforms
        dev = t.device if isinstance(t, torch.Tensor) and t.is_cuda else torch.device("cuda", torch.cuda.current_device())
        t = _f32c(t, dev)
        if t.dim() != 2 or t.shape[1] not in (3, 10):
            raise ValueError("expected Splats, transforms [N,10] or means [N,3]")
        tr = torch.zeros((t.shape[0], 10), dtype=torch.float32, device=dev)
        tr[:, : t.shape[1]] = t
    ctx = ctx or get_context(dev)
    n = tr.shape[0]
    nn = torch.empty((n, 2), dtype=torch.float32, device=dev) if return_distances else None
    pairs = C.c_uint64(0)
    ctx.check(ctx.lib.bh_knn_log_scales(ctx._h, _ptr(tr), n, _ptr(nn) if nn is not None else None, C.byref(pairs)))
    out = [tr[:, 7:10].clone()]
    if return_distances:
        out.append(nn)
    if return_stats:
        out.append({"pairs_tested": int(pairs.value)})
    return out[0] if len(out) == 1 else tuple(out)


def to_init_splats(means, rotations=None, log_scales=None, sh_coeffs=None, raw_opacities=None, render_mip=False, device=None,
                   ctx: Optional[Context] = None) -> Splats:
    """to_init_splats (splat_init.rs:218-242): Splats from a point cloud's SplatData, with the reference's defaults for what is
    absent — log-scales by compute_knn_scales (knn_log_scales, only when log_scales is None), rotation (1, 0, 0, 0) (w x y z),
    raw opacity inverse_sigmoid(0.5) = 0, SH a single grey coefficient 0.5 per channel."""
    device = torch.device(device) if device is not None else (means.device if isinstance(means, torch.Tensor) and means.is_cuda
                                                               else torch.device("cuda", torch.cuda.current_device()))
    m = _f32c(means, device).reshape(-1, 3)
    n = m.shape[0]
    rot = (_f32c(rotations, device).reshape(n, 4) if rotations is not None
           else torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=device).repeat(n, 1))
    ls = _f32c(log_scales, device).reshape(n, 3) if log_scales is not None else torch.zeros((n, 3), dtype=torch.float32, device=device)
    sh = _f32c(sh_coeffs, device).reshape(n, -1, 3) if sh_coeffs is not None else torch.full((n, 1, 3), 0.5, dtype=torch.float32, device=device)
    op = _f32c(raw_opacities, device).reshape(n) if raw_opacities is not None else torch.zeros((n,), dtype=torch.float32, device=device)
    splats = Splats(torch.cat([m, rot, ls], dim=1), sh, op, render_mip, device)
    if log_scales is None:
        knn_log_scales(splats, ctx)
    return splats


def load_init_splats(data: bytes, max_splats: Optional[int] = None, subsample_points: Optional[int] = None, device=None, render_mip=None,
                     ctx: Optional[Context] = None):
    """What the training stream does with an init PLY (train_stream.rs:100-123): load_splat_from_ply with subsampling
    (subsample_points, then SplatData::subsample(max_splats)), then to_init_splats — compute_knn_scales over the KEPT rows when the
    file has no scale_0 (import.rs:332), the file's scales otherwise.  Rotation / opacity / SH defaults are the loader's, which
    are to_init_splats' own.  -> (Splats, ParseMetadata)."""
    splats, meta = load_splat_from_ply(data, device=device, render_mip=render_mip, ctx=ctx, subsample_points=subsample_points, max_splats=max_splats)
    if not ply_vertex_has_property(data, "scale_0"):
        knn_log_scales(splats, ctx)
    return splats, meta
