"""Per-image appearance compensation on the GPU: a small learnable bilateral grid per training image, looked up by pixel
position and luminance, gives every rendered pixel its own affine 3 x 4 colour transform ("slice"); a total-variation
regulariser keeps the grids smooth.  What gsplat's trainer calls use_bilateral_grid, between render() and the loss:

    grid = BilateralGrid(num_images=len(cameras)).cuda()                 # identity: the image passes unchanged
    image = grid(render(cam, gaussians, pipe, bg)["render"], cam.uid)      # (3,H,W) -> (3,H,W)
    loss = photometric_loss(image, gt) + 10.0 * grid.tv_loss()

The grids are (N,12,GZ,GY,GX), gsplat's layout (k = 4 c + m: row c, column m of the 3 x 4 matrix), so checkpoints interchange.
The mathematics is stated at the gsr_bilagrid_* entry points of include/gsr.h; the kernels are csrc/loss/gsr_bilagrid.hip
(DESIGN.md section 23): the forward never materialises the (12,H,W) affine field of the grid_sample route, the backward uses
no atomics -- both gradients, the TV value and its gradient are the same bits on every run.  There is no CPU fallback and no
torch-operator fallback.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _native

MAX_GRID_XY, MAX_GRID_Z = 32, 16


def _check_grids(name: str, grids: torch.Tensor):
    if not isinstance(grids, torch.Tensor):
        raise TypeError(f"{name}: grids must be a tensor")
    if grids.dtype != torch.float32:
        raise RuntimeError(f"{name}: grids must be float32, not {grids.dtype}")
    if grids.ndimension() != 5 or grids.shape[1] != 12 or grids.shape[0] < 1:
        raise RuntimeError(f"{name}: expected grids of shape (N,12,GZ,GY,GX) with N >= 1, got {tuple(grids.shape)}")
    gz, gy, gx = (int(s) for s in grids.shape[2:])
    if not (2 <= gx <= MAX_GRID_XY and 2 <= gy <= MAX_GRID_XY and 2 <= gz <= MAX_GRID_Z):
        raise ValueError(f"{name}: grid size (GX,GY,GZ) = ({gx},{gy},{gz}) is outside 2..{MAX_GRID_XY} x 2..{MAX_GRID_XY} x "
                         f"2..{MAX_GRID_Z}")
    if not grids.is_cuda:
        raise RuntimeError(f"{name}: grids must be on the ROCm GPU (device 'cuda'); there is no CPU fallback")


def _check(name: str, grids: torch.Tensor, image: torch.Tensor, idx):
    """Every refusal happens here, before any launch; returns the batch size B."""
    if not isinstance(image, torch.Tensor):
        raise TypeError(f"{name}: the image must be a tensor")
    if image.dtype != torch.float32:
        raise RuntimeError(f"{name}: the image must be float32, not {image.dtype}")
    if image.ndimension() not in (3, 4) or image.shape[-3] != 3 or image.numel() == 0:
        raise RuntimeError(f"{name}: expected a non-empty (3,H,W) or (B,3,H,W) image, got {tuple(image.shape)}")
    if not isinstance(grids, torch.Tensor):
        raise TypeError(f"{name}: grids must be a tensor")
    B, N = (1 if image.ndimension() == 3 else int(image.shape[0])), (int(grids.shape[0]) if grids.ndimension() else 0)
    if isinstance(idx, torch.Tensor):
        if idx.dtype != torch.int64:
            raise RuntimeError(f"{name}: a tensor idx must be int64, not {idx.dtype}")
        if idx.ndimension() > 1 or (idx.ndimension() == 1 and idx.shape[0] != B):
            raise RuntimeError(f"{name}: idx must have shape () or ({B},), one grid index per image, got {tuple(idx.shape)}")
    elif isinstance(idx, int) and not isinstance(idx, bool):
        if not 0 <= idx < N:
            raise IndexError(f"{name}: idx {idx} is out of range for {N} grids")
    else:
        raise TypeError(f"{name}: idx must be an int or an int64 tensor on the device, not {type(idx).__name__}")
    _check_grids(name, grids)
    if not image.is_cuda:
        raise RuntimeError(f"{name}: the image must be on the ROCm GPU (device 'cuda'); there is no CPU fallback")
    if image.device != grids.device or (isinstance(idx, torch.Tensor) and idx.device != grids.device):
        raise RuntimeError(f"{name}: grids, the image and a tensor idx must be on the same device (idx is read by the kernel)")
    return B


class _SliceImage(torch.autograd.Function):
    """out = slice(grids, image, idx), differentiable by grids and image.  idx: (B,) int64 on the device.  need_grad: a
    backward will follow (decided by the caller, as in losses._PhotometricLoss) -- only then is anything saved."""

    @staticmethod
    def forward(ctx, grids, image, idx, need_grad):
        dev = image.device
        H, W = int(image.shape[-2]), int(image.shape[-1])
        B = idx.shape[0]
        N, _, GZ, GY, GX = (int(s) for s in grids.shape)
        g, img = grids.detach().contiguous(), image.detach().contiguous()
        out = torch.empty_like(img)
        with torch.cuda.device(dev):
            _native.check("gsr_bilagrid_slice_forward", _native.lib().gsr_bilagrid_slice_forward(
                torch.cuda.current_stream(dev).cuda_stream, B, H, W, N, GX, GY, GZ, g.data_ptr(), idx.data_ptr(), img.data_ptr(),
                out.data_ptr()))
        ctx.set_materialize_grads(False)
        if need_grad:
            ctx.save_for_backward(g, img, idx)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dL_dout):
        want_grids, want_image = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if dL_dout is None or not (want_grids or want_image):
            return None, None, None, None
        g, img, idx = ctx.saved_tensors
        dev = img.device
        H, W = int(img.shape[-2]), int(img.shape[-1])
        B = idx.shape[0]
        N, _, GZ, GY, GX = (int(s) for s in g.shape)
        up = dL_dout.detach().to(device=dev, dtype=torch.float32).contiguous()
        L = _native.lib()
        d_img = torch.empty_like(img) if want_image else None
        d_grids = work = None
        if want_grids:
            nbytes = ctypes.c_size_t(0)
            _native.check("gsr_bilagrid_workspace_size", L.gsr_bilagrid_workspace_size(B, H, W, GX, GY, GZ, ctypes.byref(nbytes)))
            work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
            d_grids = torch.empty_like(g)
        with torch.cuda.device(dev):
            _native.check("gsr_bilagrid_slice_backward", L.gsr_bilagrid_slice_backward(
                torch.cuda.current_stream(dev).cuda_stream, B, H, W, N, GX, GY, GZ, g.data_ptr(), idx.data_ptr(), img.data_ptr(),
                up.data_ptr(), None if work is None else work.data_ptr(), None if d_img is None else d_img.data_ptr(),
                None if d_grids is None else d_grids.data_ptr()))
        return d_grids, d_img, None, None


def slice_image(grids: torch.Tensor, image: torch.Tensor, idx) -> torch.Tensor:
    """The image with every pixel's colour passed through the 3 x 4 affine transform its grid holds at (luminance, y, x).
    grids (N,12,GZ,GY,GX) float32; image (3,H,W) or (B,3,H,W) float32, planar; idx: which grid each image uses -- a Python
    int (checked here) or an int64 tensor of shape () or (B,) ON THE DEVICE, which the kernel reads: the host neither waits
    for it nor reads it back, so a device-side index out of range cannot be refused; the kernel clamps it to [0, N - 1].
    Differentiable by grids and by the image; what autograd does not need is not computed."""
    B = _check("slice_image", grids, image, idx)
    if isinstance(idx, torch.Tensor):
        index = idx.detach().reshape(-1).expand(B).contiguous()
    else:
        index = torch.full((B,), idx, dtype=torch.int64, device=grids.device)
    need_grad = bool((grids.requires_grad or image.requires_grad) and torch.is_grad_enabled())
    return _SliceImage.apply(grids, image, index, need_grad)


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, need_grad):
        dev = grids.device
        N, _, GZ, GY, GX = (int(s) for s in grids.shape)
        g = grids.detach().contiguous()
        L = _native.lib()
        nbytes = ctypes.c_size_t(0)
        _native.check("gsr_bilagrid_tv_workspace_size", L.gsr_bilagrid_tv_workspace_size(N, GX, GY, GZ, ctypes.byref(nbytes)))
        work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _native.check("gsr_bilagrid_tv_forward", L.gsr_bilagrid_tv_forward(
                torch.cuda.current_stream(dev).cuda_stream, N, GX, GY, GZ, g.data_ptr(), work.data_ptr(), out.data_ptr()))
        ctx.set_materialize_grads(False)
        if need_grad:
            ctx.save_for_backward(g)
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, dL_dtv):
        if dL_dtv is None or not ctx.needs_input_grad[0]:
            return None, None
        g, = ctx.saved_tensors
        dev = g.device
        N, _, GZ, GY, GX = (int(s) for s in g.shape)
        up = dL_dtv.detach().to(device=dev, dtype=torch.float32).contiguous()
        grad = torch.empty_like(g)
        with torch.cuda.device(dev):
            _native.check("gsr_bilagrid_tv_backward", _native.lib().gsr_bilagrid_tv_backward(
                torch.cuda.current_stream(dev).cuda_stream, N, GX, GY, GZ, g.data_ptr(), up.data_ptr(), grad.data_ptr()))
        return grad, None


def total_variation_loss(grids: torch.Tensor) -> torch.Tensor:
    """(1 / N) sum over d in {z, y, x} of mean((forward difference of the grids along d)^2): gsplat's total_variation_loss.
    grids (N,12,GZ,GY,GX) float32 on the GPU; a device scalar, differentiable by grids."""
    _check_grids("total_variation_loss", grids)
    return _TotalVariation.apply(grids, bool(grids.requires_grad and torch.is_grad_enabled()))


class BilateralGrid(torch.nn.Module):
    """num_images learnable grids of grid_x x grid_y x grid_w (x, y, luminance) affine colour transforms, initialised to the
    identity (A = [I | 0] at every vertex).  Give its parameter an optimizer group of its own (gsplat: Adam, lr 2e-3)."""

    def __init__(self, num_images: int, grid_x: int = 16, grid_y: int = 16, grid_w: int = 8):
        super().__init__()
        if not (isinstance(num_images, int) and num_images >= 1):
            raise ValueError(f"BilateralGrid: num_images must be a positive int, not {num_images!r}")
        if not (2 <= grid_x <= MAX_GRID_XY and 2 <= grid_y <= MAX_GRID_XY and 2 <= grid_w <= MAX_GRID_Z):
            raise ValueError(f"BilateralGrid: grid size (grid_x,grid_y,grid_w) = ({grid_x},{grid_y},{grid_w}) is outside "
                             f"2..{MAX_GRID_XY} x 2..{MAX_GRID_XY} x 2..{MAX_GRID_Z}")
        eye = torch.eye(3, 4, dtype=torch.float32).reshape(1, 12, 1, 1, 1)
        self.grids = torch.nn.Parameter(eye.repeat(num_images, 1, grid_w, grid_y, grid_x))

    def forward(self, image: torch.Tensor, idx) -> torch.Tensor:
        return slice_image(self.grids, image, idx)

    def tv_loss(self) -> torch.Tensor:
        return total_variation_loss(self.grids)
