"""Mip-Splatting's 3D smoothing filter on the GPU: the per-Gaussian filter size from the training cameras, and its fused
application to scales and opacity with the backward (the mathematics is stated at the gsr_filter3d_*
entry points of include/gsr.h, the kernels are csrc/gsr_filter3d.hip).  Together with `set_antialiasing(True)`, the 2D
half, it renders a scene trained with Mip-Splatting or any trainer that copied its `filter_3D`.

    packed = pack_cameras(train_cameras, device)                      # once per camera set
    filter_3D = compute_3d_filter(gaussians._xyz.detach(), packed)     # after densify / MCMC refine / transform, every 100 steps
    scales, opacity = apply_3d_filter(gaussians._scaling, gaussians._opacity, filter_3D, from_raw=True)   # every step

  * `compute_3d_filter(means3D, cameras, return_valid=False)` -> (P,1): Mip-Splatting's `compute_3D_filter`, one launch
    over all cameras.  For every row the smallest view-space depth over the cameras that see it (beyond the 0.2 near plane,
    inside the image widened by 15 % on every side); a row no camera sees takes the largest depth of the seen rows;
    filter_3D = depth / (the largest focal length in pixels) * sqrt(0.2).  Where Mip-Splatting raises -- no camera sees any
    row -- every row takes the depth 100000: nothing here waits for the device in order to raise.
  * `apply_3d_filter(scales, opacity, filter_3D, from_raw=False)` -> (scales_eff (P,3), opacity_eff (P,1)):
    `get_scaling_with_3D_filter` and `get_opacity_with_3D_filter` in one launch each way.  s_eff = sqrt(s^2 + f^2),
    o_eff = o sqrt(prod s^2 / prod (s^2 + f^2)).  Differentiable by scales and opacity, not by filter_3D.
  * `bake_3d_filter(raw_scales, raw_opacity, filter_3D)` -> raw parameters with the filter folded in: `save_fused_ply`.

`filter_3D` is not a row of the parameter arena: it is a function of positions and cameras and is simply recomputed.  Every
result is the same bits on every run.  There is no CPU fallback and no torch-operator fallback.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native
from .normals import _check, _check_devices, _ptr, _stream

__all__ = ["PackedCameras", "pack_cameras", "compute_3d_filter", "apply_3d_filter", "bake_3d_filter", "CAMERAS_PER_CHUNK",
           "ROWS_PER_BLOCK", "CAMERA_DOUBLES"]

#: cameras one LDS stage of the sweep holds and rows one block owns (gsr_filter3d.hip: F3_CHUNK, F3_ROWS); the tests size
#: their cases around them
CAMERAS_PER_CHUNK = 32
ROWS_PER_BLOCK = 256
#: binary64 values per packed camera (include/gsr.h: GSR_FILTER3D_CAMERA_DOUBLES)
CAMERA_DOUBLES = 20
_SQRT_0_2 = math.sqrt(0.2)


class PackedCameras:
    """A camera set as the sweep reads it: `records` (V, CAMERA_DOUBLES) float64 on the device, `f_max` the largest
    horizontal focal length in pixels of all of them.  Built by `pack_cameras`."""

    def __init__(self, records: torch.Tensor, f_max: float):
        self.records, self.f_max = records, float(f_max)

    def __len__(self) -> int:
        return int(self.records.shape[0])

    @property
    def device(self) -> torch.device:
        return self.records.device


def camera_records(cameras: Sequence, what: str = "pack_cameras") -> Tuple[np.ndarray, float]:
    """((V, CAMERA_DOUBLES) float64 numpy, f_max): the host half of `pack_cameras`, layout as include/gsr.h states it."""
    cams = list(cameras)
    if len(cams) == 0:
        raise ValueError(f"{what}: cameras is empty")
    views = []
    rec = np.empty((len(cams), CAMERA_DOUBLES), dtype=np.float64)
    for i, c in enumerate(cams):
        W, H = int(c.image_width), int(c.image_height)
        fovx, fovy = float(c.FoVx), float(c.FoVy)
        if W < 1 or H < 1:
            raise ValueError(f"{what}: camera {i} has image size {W} x {H} (W x H), expected positive")
        if not (0.0 < fovx < math.pi and 0.0 < fovy < math.pi):
            raise ValueError(f"{what}: camera {i} has FoVx {fovx}, FoVy {fovy}, expected inside (0, pi)")
        V = c.world_view_transform
        if not isinstance(V, torch.Tensor) or tuple(V.shape) != (4, 4):
            raise ValueError(f"{what}: camera {i} has no (4, 4) world_view_transform tensor")
        views.append(V.detach().to(torch.float32))
        w, h = float(W), float(H)
        rec[i, 12:] = (w / (2.0 * math.tan(fovx / 2.0)), h / (2.0 * math.tan(fovy / 2.0)), 0.5 * w, 0.5 * h,
                       -0.15 * w, 1.15 * w, -0.15 * h, 1.15 * h)
    if len({v.device for v in views}) > 1:
        views = [v.cpu() for v in views]
    rec[:, :12] = torch.stack(views).cpu().numpy().astype(np.float64)[:, :, :3].reshape(len(cams), 12)  # (one transfer)
    if not np.isfinite(rec).all():
        raise ValueError(f"{what}: a camera has a value that is not finite")
    return rec, float(rec[:, 12].max())


def pack_cameras(cameras: Sequence, device="cuda") -> PackedCameras:
    """Packs a list of cameras (`world_view_transform`, `FoVx`, `FoVy`, `image_width`, `image_height`: `synth.Camera`, the
    reference's `Simple_Camera`) once on the host, so that recomputing the filter costs no per-camera host work."""
    rec, f_max = camera_records(cameras)
    return PackedCameras(torch.from_numpy(rec).to(device).contiguous(), f_max)


def compute_3d_filter(means3D: torch.Tensor, cameras: Union[PackedCameras, Sequence], return_valid: bool = False):
    """filter_3D (P,1) float32 [, valid (P,) bool: rows at least one camera sees].  means3D (P,3) float32, contiguous, on the
    GPU; `cameras`: a `PackedCameras`, or a list of cameras (packed here, on every call).  No gradient."""
    what = "compute_3d_filter"
    _check(what, "means3D", means3D, (None, 3))
    _check_devices(what, means3D=means3D)
    dev = means3D.device
    packed = cameras if isinstance(cameras, PackedCameras) else PackedCameras(*_to_device(camera_records(cameras, what), dev))
    rec = packed.records
    if (not isinstance(rec, torch.Tensor) or rec.dtype != torch.float64 or rec.ndimension() != 2 or rec.shape[0] < 1
            or rec.shape[1] != CAMERA_DOUBLES or not rec.is_contiguous()):
        raise RuntimeError(f"{what}: cameras.records must be a contiguous (V, {CAMERA_DOUBLES}) float64 tensor with V >= 1")
    if rec.device != dev:
        raise RuntimeError(f"{what}: cameras is on {rec.device}, expected {dev}")
    if not (math.isfinite(packed.f_max) and packed.f_max > 0.0):
        raise ValueError(f"{what}: cameras.f_max must be finite and positive, got {packed.f_max}")
    P = int(means3D.shape[0])
    L = _native.lib()
    nbytes = ctypes.c_size_t(0)
    _native.check("gsr_filter3d_workspace_size", L.gsr_filter3d_workspace_size(P, ctypes.byref(nbytes)))
    work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    out = torch.empty((P, 1), dtype=torch.float32, device=dev)
    valid = torch.empty((P,), dtype=torch.bool, device=dev)
    with torch.cuda.device(dev):
        _native.check("gsr_filter3d_sweep", L.gsr_filter3d_sweep(
            _stream(dev), P, int(rec.shape[0]), _ptr(means3D.detach()), _ptr(rec), packed.f_max, _SQRT_0_2, _ptr(work),
            _ptr(out), _ptr(valid)))
    return (out, valid) if return_valid else out


def _to_device(rec_fmax, dev):
    rec, f_max = rec_fmax
    return torch.from_numpy(rec).to(dev).contiguous(), f_max


class _Apply3DFilter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scales, opacity, filter_3D, from_raw):
        dev = scales.device
        s, o, f = scales.detach(), opacity.detach(), filter_3D.detach()
        P = int(s.shape[0])
        s_eff = torch.empty((P, 3), dtype=torch.float32, device=dev)
        o_eff = torch.empty((P, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _native.check("gsr_filter3d_apply_forward", _native.lib().gsr_filter3d_apply_forward(
                _stream(dev), P, int(from_raw), _ptr(s), _ptr(o), _ptr(f), _ptr(s_eff), _ptr(o_eff)))
        ctx.set_materialize_grads(False)
        ctx.gsr_from_raw = int(from_raw)
        ctx.save_for_backward(s, o, f)
        return s_eff, o_eff

    @staticmethod
    @once_differentiable
    def backward(ctx, dL_ds_eff, dL_do_eff):
        want_s, want_o = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        # the opacity's gradient comes from dL_do_eff alone; the scales' from both
        want_o = want_o and dL_do_eff is not None
        want_s = want_s and (dL_ds_eff is not None or dL_do_eff is not None)
        if not (want_s or want_o):
            return None, None, None, None
        s, o, f = ctx.saved_tensors
        dev = s.device
        up = lambda g: None if g is None else g.detach().to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
        up_s, up_o = up(dL_ds_eff), up(dL_do_eff)
        g_s = torch.empty_like(s) if want_s else None
        g_o = torch.empty_like(o) if want_o else None
        with torch.cuda.device(dev):
            _native.check("gsr_filter3d_apply_backward", _native.lib().gsr_filter3d_apply_backward(
                _stream(dev), int(s.shape[0]), ctx.gsr_from_raw, _ptr(s), _ptr(o), _ptr(f), _ptr(up_s), _ptr(up_o), _ptr(g_s),
                _ptr(g_o)))
        return g_s, g_o, None, None


def apply_3d_filter(scales: torch.Tensor, opacity: torch.Tensor, filter_3D: torch.Tensor,
                    from_raw: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scales_eff (P,3), opacity_eff (P,1)): s_eff_k = sqrt(s_k^2 + f^2), o_eff = o sqrt(prod s_k^2 / prod (s_k^2 + f^2))
    with f = filter_3D of the row.  scales (P,3), opacity (P,1), filter_3D (P,1): float32, contiguous, on the GPU.

    from_raw=False: the inputs are the activated values (`get_scaling`, `get_opacity`).  from_raw=True: they are the raw
    parameters, the kernel applies s = exp(raw) and o = sigmoid(raw) itself and the backward returns the gradients of the
    raw parameters.  Differentiable by scales and opacity; filter_3D gets no gradient.  At f = 0 the result is the input."""
    what = "apply_3d_filter"
    _check(what, "scales", scales, (None, 3))
    P = int(scales.shape[0])
    _check(what, "opacity", opacity, (P, 1))
    _check(what, "filter_3D", filter_3D, (P, 1))
    _check_devices(what, scales=scales, opacity=opacity, filter_3D=filter_3D)
    return _Apply3DFilter.apply(scales, opacity, filter_3D, bool(from_raw))


def bake_3d_filter(raw_scales: torch.Tensor, raw_opacity: torch.Tensor,
                   filter_3D: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(log s_eff (P,3), logit o_eff (P,1)): raw parameters with the filter folded in, what Mip-Splatting's `save_fused_ply`
    writes -- a file any 3DGS viewer renders without knowing about the filter."""
    s_eff, o_eff = apply_3d_filter(raw_scales, raw_opacity, filter_3D, from_raw=True)
    return torch.log(s_eff), torch.logit(o_eff)
