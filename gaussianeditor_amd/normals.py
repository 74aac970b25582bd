"""Surface normals on the GPU: the normal of every Gaussian, the normal of the rendered depth image, and the depth-normal
consistency loss of 2DGS / PGSR / RaDe-GS / dn-splatter that ties them together (the mathematics is
stated at the gsr_gaussian_normals_*, gsr_depth_normals_* and gsr_normal_loss_* entry points of include/gsr.h, the kernels
are csrc/gsr_normals.hip).

    pkg = render(cam, gaussians, pipe, bg, return_alpha=True, return_normals=True)
    loss = normal_consistency_loss(pkg["normals"], pkg["depth_3dgs"], pkg["alpha"], cam)

  * `gaussian_normals(rotations, scales, means3D, viewmatrix)` -> (P,3): the shortest axis of every Gaussian in camera
    space, turned towards the camera.  `render(..., return_normals=True)` composites it with the view's alpha into
    `out["normals"]` (3,H,W).
  * `depth_to_normals(depth, alpha, camera)` -> (3,H,W): central differences of the back-projected depth image, exactly
    zero at invalid pixels (border, a tap with alpha <= alpha_min or z <= 0).
  * `normal_consistency_loss(normals, depth, alpha, camera)` -> scalar: (1 / (H W)) sum over valid pixels of A - <N, n_d>,
    fused: the depth-normal image is never written.

All normals are in camera space (COLMAP axes, z forward) and point towards the camera; rotate with `V[:3,:3].T` for world
space.  Every result and every gradient is the same bits on every run (no atomics, fixed summation order).  The rendered
depth only carries a gradient under `gaussianeditor_amd.set_depth_grad(True)`; without it the loss still reaches the
rotations (through the normal image) and everything the alpha image depends on.  There is no CPU fallback and no
torch-operator fallback.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _native

__all__ = ["gaussian_normals", "depth_to_normals", "normal_consistency_loss", "camera_intrinsics", "TILE", "ROWS_PER_BLOCK"]

#: pixels (x, y) one block of the image kernels owns, and rows one block of the per-Gaussian kernels owns
#: (gsr_normals.hip: NR_TX, NR_TY, NR_ROWS); the tests size their cases around them
TILE = (32, 8)
ROWS_PER_BLOCK = 256


def _check(what: str, name: str, t, shape: Tuple[Optional[int], ...]) -> None:
    """dtype, shape (None: any size) and contiguity of `t`, by name (then `_check_devices` for all of a call's tensors)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what}: {name} has dtype {t.dtype}, expected torch.float32")
    if t.ndimension() != len(shape) or any(s is not None and int(d) != s for d, s in zip(t.shape, shape)):
        want = "(" + ", ".join("*" if s is None else str(s) for s in shape) + ")"
        raise RuntimeError(f"{what}: {name} has shape {tuple(t.shape)}, expected {want}")
    if not t.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be contiguous")


def _check_devices(what: str, **tensors) -> None:
    """Every tensor on the ROCm GPU, and on the device of the first."""
    ref = None
    for name, t in tensors.items():
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{what}: {name} must live on the ROCm GPU (device 'cuda'); there is no CPU fallback")
        ref = t if ref is None else ref
        if t.device != ref.device:
            raise RuntimeError(f"{what}: {name} is on {t.device}, expected {ref.device}")


def camera_intrinsics(cam_or_settings) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) in pixels as the rasterizer's ndc2Pix implies them: fx = W / (2 tanfovx), fy = H / (2 tanfovy),
    cx = (W - 1) / 2, cy = (H - 1) / 2.  Takes a camera (`image_width`, `image_height`, `FoVx`, `FoVy`) or a
    `GaussianRasterizationSettings` (`tanfovx`, `tanfovy`)."""
    c = cam_or_settings
    W, H = int(c.image_width), int(c.image_height)
    if hasattr(c, "tanfovx"):
        tx, ty = float(c.tanfovx), float(c.tanfovy)
    else:
        tx, ty = math.tan(float(c.FoVx) * 0.5), math.tan(float(c.FoVy) * 0.5)
    return W / (2.0 * tx), H / (2.0 * ty), (W - 1) / 2.0, (H - 1) / 2.0


def _intrinsics(what: str, camera, fx, fy, cx, cy, H: int, W: int) -> Tuple[float, float, float, float]:
    if camera is None and (fx is None or fy is None or cx is None or cy is None):
        raise ValueError(f"{what}: give a camera (or rasterization settings), or all four of fx, fy, cx, cy")
    if camera is not None:
        if (int(camera.image_height), int(camera.image_width)) != (H, W):
            raise ValueError(f"{what}: the camera is {int(camera.image_height)} x {int(camera.image_width)} (H x W) but the "
                             f"image is {H} x {W}")
        d = camera_intrinsics(camera)
    else:
        d = (None,) * 4
    k = tuple(float(o) if o is not None else v for o, v in zip((fx, fy, cx, cy), d))
    if not (all(math.isfinite(v) for v in k) and k[0] > 0.0 and k[1] > 0.0):
        raise ValueError(f"{what}: fx and fy must be positive and all four intrinsics finite, got {k}")
    return k


def _alpha_min(what: str, alpha_min) -> float:
    a = float(alpha_min)
    if not math.isfinite(a):
        raise ValueError(f"{what}: alpha_min must be finite, got {a}")
    return a


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rotations, scales, means3D, viewmatrix):
        dev = rotations.device
        q, s, p, v = (t.detach() for t in (rotations, scales, means3D, viewmatrix))
        P = int(q.shape[0])
        out = torch.empty((P, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _native.check("gsr_gaussian_normals_forward", _native.lib().gsr_gaussian_normals_forward(
                _stream(dev), P, _ptr(q), _ptr(s), _ptr(p), _ptr(v), _ptr(out)))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, s, p, v)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dL_dout):
        if dL_dout is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        q, s, p, v = ctx.saved_tensors
        dev = q.device
        up = dL_dout.detach().to(device=dev, dtype=torch.float32).contiguous()
        grad = torch.empty_like(q)
        with torch.cuda.device(dev):
            _native.check("gsr_gaussian_normals_backward", _native.lib().gsr_gaussian_normals_backward(
                _stream(dev), int(q.shape[0]), _ptr(q), _ptr(s), _ptr(p), _ptr(v), _ptr(up), _ptr(grad)))
        return grad, None, None, None


def gaussian_normals(rotations: torch.Tensor, scales: torch.Tensor, means3D: torch.Tensor,
                     viewmatrix: torch.Tensor) -> torch.Tensor:
    """(P,3): per Gaussian the column of R(q / |q|) that belongs to its smallest scale (on a tie the lowest index), in
    camera space, with the sign that faces the camera (n . p_c <= 0).  rotations (P,4) w,x,y,z, need not be normalised;
    scales (P,3); means3D (P,3); viewmatrix (4,4): the transposed view matrix the rasterizer takes
    (`cam.world_view_transform`).  All float32, contiguous, on the GPU.

    The gradient goes to `rotations` only (it passes through the normalisation, so it is orthogonal to q).  `scales`,
    `means3D` and the camera get none: they only choose the axis and the sign, and the output is piecewise constant in
    them.  A precomputed covariance is not supported."""
    what = "gaussian_normals"
    _check(what, "rotations", rotations, (None, 4))
    P = int(rotations.shape[0])
    _check(what, "scales", scales, (P, 3))
    _check(what, "means3D", means3D, (P, 3))
    _check(what, "viewmatrix", viewmatrix, (4, 4))
    _check_devices(what, rotations=rotations, scales=scales, means3D=means3D, viewmatrix=viewmatrix)
    return _GaussianNormals.apply(rotations, scales, means3D, viewmatrix)


class _DepthNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, k, alpha_min):
        dev = depth.device
        H, W = int(depth.shape[-2]), int(depth.shape[-1])
        d, a = depth.detach(), None if alpha is None else alpha.detach()
        out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _native.check("gsr_depth_normals_forward", _native.lib().gsr_depth_normals_forward(
                _stream(dev), H, W, *k, alpha_min, _ptr(d), _ptr(a), _ptr(out)))
        ctx.set_materialize_grads(False)
        ctx.gsr_args = (H, W, k, alpha_min, a is not None)
        ctx.save_for_backward(*((d,) if a is None else (d, a)))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dL_dout):
        H, W, k, alpha_min, has_alpha = ctx.gsr_args
        want_d, want_a = ctx.needs_input_grad[0], has_alpha and ctx.needs_input_grad[1]
        if dL_dout is None or not (want_d or want_a):
            return None, None, None, None
        d = ctx.saved_tensors[0]
        a = ctx.saved_tensors[1] if has_alpha else None
        dev = d.device
        up = dL_dout.detach().to(device=dev, dtype=torch.float32).contiguous()
        g_d = torch.empty_like(d) if want_d else None
        g_a = torch.empty_like(a) if want_a else None
        with torch.cuda.device(dev):
            _native.check("gsr_depth_normals_backward", _native.lib().gsr_depth_normals_backward(
                _stream(dev), H, W, *k, alpha_min, _ptr(d), _ptr(a), _ptr(up), _ptr(g_d), _ptr(g_a)))
        return g_d, g_a, None, None


def depth_to_normals(depth: torch.Tensor, alpha: Optional[torch.Tensor] = None, camera=None, *, fx=None, fy=None, cx=None,
                     cy=None, alpha_min: float = 0.5) -> torch.Tensor:
    """(3,H,W): the camera-space normal of the depth image at every pixel, from the central differences of the
    back-projected points p(x,y) = z(x,y) ((x - cx) / fx, (y - cy) / fy, 1); exact on a plane under perspective.

    depth (1,H,W) float32.  With `alpha` (1,H,W) the depth is the rasterizer's unnormalised `depth_3dgs` and
    z = depth / max(alpha, 1e-8); without, z = depth.  `camera`: a camera or rasterization settings, for the intrinsics
    `camera_intrinsics` gives; explicit fx, fy, cx, cy override them one by one.  The result is exactly (0,0,0) at invalid
    pixels: the image border, and wherever the pixel or one of its four neighbours has alpha <= alpha_min or z <= 0.

    Differentiable by depth and alpha (through z; the validity mask carries no gradient).  A depth that came out of
    `render()` only passes the gradient on under `set_depth_grad(True)`."""
    what = "depth_to_normals"
    _check(what, "depth", depth, (1, None, None))
    H, W = int(depth.shape[1]), int(depth.shape[2])
    if H < 1 or W < 1:
        raise RuntimeError(f"{what}: depth has shape {tuple(depth.shape)}, expected a non-empty (1, H, W)")
    if alpha is not None:
        _check(what, "alpha", alpha, (1, H, W))
    _check_devices(what, depth=depth, alpha=alpha)
    k = _intrinsics(what, camera, fx, fy, cx, cy, H, W)
    return _DepthNormals.apply(depth, alpha, k, _alpha_min(what, alpha_min))


class _NormalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normals, depth, alpha, k, alpha_min):
        dev = normals.device
        H, W = int(depth.shape[-2]), int(depth.shape[-1])
        n, d, a = normals.detach(), depth.detach(), alpha.detach()
        L = _native.lib()
        nbytes = ctypes.c_size_t(0)
        _native.check("gsr_normal_loss_workspace_size", L.gsr_normal_loss_workspace_size(H, W, ctypes.byref(nbytes)))
        work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _native.check("gsr_normal_loss_forward", L.gsr_normal_loss_forward(
                _stream(dev), H, W, *k, alpha_min, _ptr(n), _ptr(d), _ptr(a), _ptr(work), _ptr(out)))
        ctx.set_materialize_grads(False)
        ctx.gsr_args = (H, W, k, alpha_min)
        ctx.save_for_backward(n, d, a)
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, dL_dloss):
        want = ctx.needs_input_grad[:3]
        if dL_dloss is None or not any(want):
            return None, None, None, None, None
        H, W, k, alpha_min = ctx.gsr_args
        n, d, a = ctx.saved_tensors
        dev = n.device
        up = dL_dloss.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        g_n = torch.empty_like(n) if want[0] else None
        g_d = torch.empty_like(d) if want[1] else None
        g_a = torch.empty_like(a) if want[2] else None
        with torch.cuda.device(dev):
            _native.check("gsr_normal_loss_backward", _native.lib().gsr_normal_loss_backward(
                _stream(dev), H, W, *k, alpha_min, _ptr(n), _ptr(d), _ptr(a), _ptr(up), _ptr(g_n), _ptr(g_d), _ptr(g_a)))
        return g_n, g_d, g_a, None, None


def normal_consistency_loss(normals: torch.Tensor, depth: torch.Tensor, alpha: torch.Tensor, camera=None, *, fx=None,
                            fy=None, cx=None, cy=None, alpha_min: float = 0.5) -> torch.Tensor:
    """The depth-normal consistency term, a device scalar:

        L = (1 / (H W)) sum over valid pixels of (A - <N, n_d>)

    normals N (3,H,W): the alpha-composited normal image, `render(..., return_normals=True)["normals"]`; depth, alpha
    (1,H,W): `depth_3dgs` and `alpha` of the same render; n_d = `depth_to_normals(depth, alpha, ...)`, never written to
    memory; A = alpha, a constant weight.  With |N| <= A every term is >= 0 and equals 2DGS's A (1 - <N / A, n_d>).  The
    sum is divided by H W, not by the number of valid pixels: the loss does not jump when a pixel changes validity.

    The gradient goes to N (-n_d / (H W) at valid pixels, 0 elsewhere) and to depth and alpha through n_d; the explicit A
    term gives none (2DGS detaches it).  The depth of `render()` only passes its gradient on under `set_depth_grad(True)`."""
    what = "normal_consistency_loss"
    _check(what, "normals", normals, (3, None, None))
    H, W = int(normals.shape[1]), int(normals.shape[2])
    if H < 1 or W < 1:
        raise RuntimeError(f"{what}: normals has shape {tuple(normals.shape)}, expected a non-empty (3, H, W)")
    _check(what, "depth", depth, (1, H, W))
    _check(what, "alpha", alpha, (1, H, W))
    _check_devices(what, normals=normals, depth=depth, alpha=alpha)
    k = _intrinsics(what, camera, fx, fy, cx, cy, H, W)
    return _NormalLoss.apply(normals, depth, alpha, k, _alpha_min(what, alpha_min))
