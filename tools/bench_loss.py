#!/usr/bin/env python3
"""Cost of the training loss (1 - 0.2) * L1 + 0.2 * (1 - SSIM), forward + backward, on two routes that take turns in one
process:

    fused   gaussianeditor_amd.losses.photometric_loss   (loss_forward_kernel + loss_finish_kernel, loss_backward_kernel)
    torch   the same loss from torch operators in float32, as 3DGS trainers write it: five grouped 11 x 11 conv2d calls,
            the elementwise SSIM map, mean, abs().mean(), and autograd's backward through all of it

at 3 x 1080 x 1920 (the headline view) and 3 x 512 x 512 (the edit loop's view).

    python tools/bench_loss.py [--iters 50] [--windows 3] [--out profiles/r07_loss.json]

Timing: HIP events around windows of `iters` forward + backward iterations (nothing is read back inside a window); the
routes alternate window by window after a warm-up of both, and the median window is reported, per iteration.  The two
fused kernels are also timed on their own through the C ABI (windows of `iters` launches, no Python between the launches
beyond ctypes), and their achieved bytes per second are stated against the COMPULSORY traffic: with N = planes * H * W
values of 4 bytes, kernel A reads 2 planes (image, ground truth) and writes 3 (the maps), kernel B reads 5 (image, ground
truth, three maps) and writes 1 -- 11 passes of 4 N bytes (274 MB at 1080p).  Halo re-reads come out of the caches and are
not in the model.  One JSON line per size."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gaussianeditor_amd import _native  # noqa: E402
from gaussianeditor_amd.losses import photometric_loss  # noqa: E402

SIZES = ((3, 1080, 1920), (3, 512, 512))
LAMBDA = 0.2
#: the train steps the loss is set against (ms): 10^6 Gaussians at 1080p, and the 512 x 512 edit loop view
STEPS_MS = {(3, 1080, 1920): 0.55, (3, 512, 512): 0.64}


def torch_window(channels, dev):
    g = torch.exp(-(torch.arange(11, dtype=torch.float32) - 5) ** 2 / (2 * 1.5 ** 2))
    g = g / g.sum()
    return (g[:, None] * g[None, :]).expand(channels, 1, 11, 11).contiguous().to(dev)


def torch_loss(x, y, window):
    c = x.shape[-3]
    blur = lambda t: F.conv2d(t, window, padding=5, groups=c)  # noqa: E731
    mu1, mu2 = blur(x), blur(y)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = blur(x * x) - mu1_sq, blur(y * y) - mu2_sq, blur(x * y) - mu12
    ssim = (((2 * mu12 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1_sq + mu2_sq + 1e-4) * (s1 + s2 + 9e-4))).mean()
    return (1.0 - LAMBDA) * (x - y).abs().mean() + LAMBDA * (1.0 - ssim)


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def median(v):
    return sorted(v)[len(v) // 2]


def run(shape, iters, windows, dev):
    planes, H, W = shape
    g = torch.Generator().manual_seed(0)
    base = F.interpolate(torch.rand(1, planes, H // 8 + 2, W // 8 + 2, generator=g), size=(H, W), mode="bicubic")[0]
    x = (base + 0.05 * torch.randn(planes, H, W, generator=g)).clamp(0, 1).to(dev).requires_grad_(True)
    y = (base + 0.10 * torch.randn(planes, H, W, generator=g)).clamp(0, 1).to(dev)
    win = torch_window(planes, dev)

    def fused():
        x.grad = None
        photometric_loss(x, y, LAMBDA).backward()

    def eager():
        x.grad = None
        torch_loss(x[None], y[None], win).backward()

    # the kernels alone, through the C ABI
    L = _native.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    nbytes = ctypes.c_size_t(0)
    _native.check("gsr_loss_workspace_size", L.gsr_loss_workspace_size(planes, H, W, ctypes.byref(nbytes)))
    work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    maps, out3 = torch.empty((3, planes, H, W), device=dev), torch.empty(3, device=dev)
    one, grad = torch.ones((), device=dev), torch.empty((planes, H, W), device=dev)
    xd = x.detach()
    f = ctypes.c_float

    def kernel_a():
        _native.check("fwd", L.gsr_photometric_loss_forward(s, planes, H, W, xd.data_ptr(), y.data_ptr(), f(1 - LAMBDA), f(-LAMBDA),
                                                          f(LAMBDA), maps.data_ptr(), work.data_ptr(), out3.data_ptr()))

    def kernel_b():
        _native.check("bwd", L.gsr_photometric_loss_backward(s, planes, H, W, xd.data_ptr(), y.data_ptr(), maps.data_ptr(),
                                                           f(1 - LAMBDA), f(-LAMBDA), one.data_ptr(), grad.data_ptr()))

    routes = (("fused", fused), ("torch", eager), ("kernel_a", kernel_a), ("kernel_b", kernel_b))
    for _, fn in routes:  # warm-up: code objects, conv algorithm selection, the allocator's blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    # both routes compute the same thing: compare before timing
    fused()
    g_fused, l_fused = x.grad.clone(), photometric_loss(x, y, LAMBDA).detach().item()
    eager()
    l_torch = torch_loss(x[None], y[None], win).detach().item()
    g_err = float((g_fused - x.grad).abs().max() / x.grad.abs().max())
    t = {name: [] for name, _ in routes}
    for _ in range(windows):
        for name, fn in routes:  # the routes take turns window by window
            t[name].append(window_ms(fn, iters))
    n_bytes = 4.0 * planes * H * W
    res = dict(planes=planes, H=H, W=W, iters=iters, windows=windows,
               fused_ms=round(median(t["fused"]), 4), torch_ms=round(median(t["torch"]), 4),
               fused_ms_windows=[round(v, 4) for v in t["fused"]], torch_ms_windows=[round(v, 4) for v in t["torch"]],
               speedup=round(median(t["torch"]) / median(t["fused"]), 2),
               kernel_a_ms=round(median(t["kernel_a"]), 4), kernel_b_ms=round(median(t["kernel_b"]), 4),
               kernel_a_model_GBps=round(5 * n_bytes / (median(t["kernel_a"]) * 1e-3) / 1e9, 1),
               kernel_b_model_GBps=round(6 * n_bytes / (median(t["kernel_b"]) * 1e-3) / 1e9, 1),
               model_MB=round(11 * n_bytes / 1e6, 1), step_ms=STEPS_MS[shape],
               fused_over_step=round(median(t["fused"]) / STEPS_MS[shape], 3),
               torch_over_step=round(median(t["torch"]) / STEPS_MS[shape], 3),
               loss_fused=l_fused, loss_torch=l_torch, grad_max_rel_diff=g_err)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda:0")
    res = [run(shape, a.iters, a.windows, dev) for shape in SIZES]
    if a.out:
        with open(a.out, "w") as fh:
            for r in res:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
