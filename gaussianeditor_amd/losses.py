"""The training loss on the GPU: L1, SSIM and their combination in ONE forward kernel and ONE backward kernel.

Reference: gaussiansplatting/utils/loss_utils.py (l1_loss :17-18, ssim :33-63) and the loss line of its two trainers,
`(1 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt))` (gaussiansplatting/train.py:89,
train_from_mesh.py:136).  There the SSIM is five grouped 11 x 11 conv2d calls and some fifteen elementwise kernels, and
autograd runs all of them backward; here it is gsr_photometric_loss_forward / _backward of the C ABI (include/gsr.h,
csrc/loss/gsr_loss.hip): the forward leaves three per-pixel maps, the backward convolves them.  No float
atomics: loss and gradient are the same bits on every run.  There is no CPU fallback and no torch-operator fallback.

    from gaussianeditor_amd.losses import l1_loss, ssim          # the reference's two functions
    loss = photometric_loss(image, gt, lambda_dssim=0.2)          # the trainers' loss line in one call
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _native

def _check(name: str, image: torch.Tensor, gt: torch.Tensor):
    for what, t in (("the image", image), ("gt", gt)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: {what} must be a tensor")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name}: {what} must be float32, not {t.dtype}")
    if image.shape != gt.shape:
        raise RuntimeError(f"{name}: shapes differ: {tuple(image.shape)} and {tuple(gt.shape)}")
    if image.ndimension() not in (3, 4) or image.numel() == 0:
        raise RuntimeError(f"{name}: expected non-empty (C,H,W) or (N,C,H,W) images, got {tuple(image.shape)}")
    if gt.requires_grad:
        raise RuntimeError(f"{name}: gt requires a gradient; the loss is differentiated by the image only")
    for what, t in (("the image", image), ("gt", gt)):
        if not t.is_cuda:
            raise RuntimeError(f"{name}: {what} must be on the ROCm GPU (device 'cuda'); there is no CPU fallback")
    if image.device != gt.device:
        raise RuntimeError(f"{name}: the image and gt must be on the same device")


class _PhotometricLoss(torch.autograd.Function):
    """(loss, l1, ssim) = w_l1 * L1 + w_ssim * SSIM + c and its two terms; only `loss` is differentiable, by `image`.
    need_grad: a backward will follow (decided by the caller: grad mode is always off inside forward, and
    ctx.needs_input_grad is True under torch.no_grad() too) -- only then are the maps allocated, written and saved."""

    @staticmethod
    def forward(ctx, image, gt, w_l1, w_ssim, c, need_grad):
        dev = image.device
        H, W = int(image.shape[-2]), int(image.shape[-1])
        planes = image.numel() // (H * W)
        img, ref = image.detach().contiguous(), gt.detach().contiguous()
        L = _native.lib()
        nbytes = ctypes.c_size_t(0)
        _native.check("gsr_loss_workspace_size", L.gsr_loss_workspace_size(planes, H, W, ctypes.byref(nbytes)))
        work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        maps = None
        if need_grad and ctypes.c_float(w_ssim).value != 0.0:  # (the library's own test: w_ssim as binary32)
            maps = torch.empty((3,) + tuple(img.shape), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _native.check("gsr_photometric_loss_forward", L.gsr_photometric_loss_forward(
                torch.cuda.current_stream(dev).cuda_stream, planes, H, W, img.data_ptr(), ref.data_ptr(),
                ctypes.c_float(w_l1), ctypes.c_float(w_ssim), ctypes.c_float(c),
                None if maps is None else maps.data_ptr(), work.data_ptr(), out3.data_ptr()))
        loss, l1, ssim_ = out3.unbind(0)
        ctx.mark_non_differentiable(l1, ssim_)
        ctx.set_materialize_grads(False)
        if need_grad:
            ctx.geometry = (planes, H, W, w_l1, w_ssim)
            ctx.save_for_backward(*((img, ref) if maps is None else (img, ref, maps)))
        return loss, l1, ssim_

    @staticmethod
    @once_differentiable
    def backward(ctx, dL_dloss, _dl1, _dssim):
        if dL_dloss is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        planes, H, W, w_l1, w_ssim = ctx.geometry
        img, ref, *rest = ctx.saved_tensors
        dev = img.device
        g = dL_dloss.detach().to(device=dev, dtype=torch.float32).contiguous()
        grad = torch.empty_like(img)
        # (with w_ssim == 0 the kernel reads no maps; the ABI still wants a pointer)
        maps = rest[0] if rest else img
        L = _native.lib()
        with torch.cuda.device(dev):
            _native.check("gsr_photometric_loss_backward", L.gsr_photometric_loss_backward(
                torch.cuda.current_stream(dev).cuda_stream, planes, H, W, img.data_ptr(), ref.data_ptr(), maps.data_ptr(),
                ctypes.c_float(w_l1), ctypes.c_float(w_ssim), g.data_ptr(), grad.data_ptr()))
        return grad, None, None, None, None, None


def _apply(image, gt, w_l1, w_ssim, c):
    return _PhotometricLoss.apply(image, gt, w_l1, w_ssim, c, bool(image.requires_grad and torch.is_grad_enabled()))


def l1_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """mean |network_output - gt| (loss_utils.py:17-18); the gradient is sign(network_output - gt) / N, 0 where they are equal."""
    _check("l1_loss", network_output, gt)
    return _apply(network_output, gt, 1.0, 0.0, 0.0)[0]


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """The reference's ssim(img1, img2) (loss_utils.py:33-63): mean SSIM map, 11-tap Gaussian window of sigma 1.5, zero
    padding.  Differentiable by img1.  Other window sizes and size_average=False are refused, not emulated."""
    if window_size != 11:
        raise ValueError(f"ssim: window_size must be 11 (the fused kernel's window), not {window_size}")
    if not size_average:
        raise ValueError("ssim: size_average=False is not supported (the kernel reduces to the mean)")
    _check("ssim", img1, img2)
    return _apply(img1, img2, 0.0, 1.0, 0.0)[0]


def photometric_loss(image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2, return_terms: bool = False):
    """(1 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt)): the loss line of the reference's
    trainers.  return_terms: (loss, l1, ssim), the last two detached device scalars for logging (no readback happens here).
    With lambda_dssim == 0 the SSIM is not evaluated and its term is NaN."""
    _check("photometric_loss", image, gt)
    lam = float(lambda_dssim)
    loss, l1, ssim_ = _apply(image, gt, 1.0 - lam, -lam, lam)
    return (loss, l1, ssim_) if return_terms else loss
