#!/usr/bin/env python3
"""Cost of the bilateral-grid colour correction (gaussianeditor_amd.bilagrid), forward + backward, on two routes that take
turns STEP BY STEP in one process, so that clock and cache drift fall on both alike:

    fused   slice_image / total_variation_loss  (csrc/loss/gsr_bilagrid.hip: bila_slice_forward_kernel,
            bila_slice_backward_kernel + bila_reduce_kernel; bila_tv_forward_kernel + bila_tv_finish_kernel, bila_tv_backward_kernel)
    torch   the same mathematics from torch operators in float32, as trainers write it: F.grid_sample on the 5-D grid (which
            materialises the (12,H,W) affine field), the per-pixel 3 x 4 product, and autograd's backward through both; the TV
            term as three sliced differences, squares and means

for one image (B = 1) at 1920 x 1080 and at 512 x 512, grid 16 x 16 x 8 of N = 4 grids; both the grids and the image take a
gradient, as in a training step.

    python tools/bench_bilagrid.py [--steps 30] [--warmup 5] [--only 1080p|512]

Timing: HIP events on the current stream around each step (forward + backward, nothing read back inside); the median of
`steps` steps and the interquartile range, in ms.  One JSON line per (size, what, route).  The kernels' own times come from
running this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gaussianeditor_amd.bilagrid import slice_image, total_variation_loss  # noqa: E402

SIZES = {"1080p": (1080, 1920), "512": (512, 512)}
GRID = (16, 16, 8)  # GX, GY, GZ
N_GRIDS = 4


def torch_slice(grids, image, idx):
    """image (1,3,H,W) -> (1,3,H,W)"""
    _, _, H, W = image.shape
    u = (torch.arange(W, dtype=image.dtype, device=image.device) + 0.5) / W
    v = (torch.arange(H, dtype=image.dtype, device=image.device) + 0.5) / H
    gray = (0.299 * image[:, 0] + 0.587 * image[:, 1] + 0.114 * image[:, 2]).clamp(0.0, 1.0)
    vv, uu = torch.meshgrid(v, u, indexing="ij")
    coords = torch.stack([uu.expand_as(gray), vv.expand_as(gray), gray], dim=-1) * 2.0 - 1.0
    field = F.grid_sample(grids[idx:idx + 1], coords[:, None], mode="bilinear", padding_mode="border", align_corners=True)
    A = field[:, :, 0].reshape(1, 3, 4, H, W)
    return (A[:, :, :3] * image[:, None]).sum(2) + A[:, :, 3]


def torch_tv(grids):
    return ((grids[:, :, 1:] - grids[:, :, :-1]).pow(2).mean() + (grids[:, :, :, 1:] - grids[:, :, :, :-1]).pow(2).mean() +
            (grids[..., 1:] - grids[..., :-1]).pow(2).mean())


def quartiles(t):
    t = sorted(t)
    q = lambda f: t[min(len(t) - 1, int(f * len(t)))]  # noqa: E731
    return q(0.5), q(0.75) - q(0.25)


def run(name, steps, warmup, dev):
    H, W = SIZES[name]
    GX, GY, GZ = GRID
    g = torch.Generator().manual_seed(0)
    eye = torch.eye(3, 4).reshape(1, 12, 1, 1, 1)
    grids = (eye + 0.1 * torch.randn(N_GRIDS, 12, GZ, GY, GX, generator=g)).to(dev).requires_grad_(True)
    base = F.interpolate(torch.rand(1, 3, H // 8 + 2, W // 8 + 2, generator=g), size=(H, W), mode="bicubic")[0]
    image = (base + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1).to(dev).requires_grad_(True)
    dout = (torch.randn(3, H, W, generator=g) / (H * W)).to(dev)

    def fused_slice():
        slice_image(grids, image, 1).backward(dout)

    def torch_slice_step():
        torch_slice(grids, image[None], 1).backward(dout[None])

    def fused_tv():
        total_variation_loss(grids).backward()

    def torch_tv_step():
        torch_tv(grids).backward()

    routes = (("slice", "fused", fused_slice), ("slice", "torch", torch_slice_step), ("tv", "fused", fused_tv),
              ("tv", "torch", torch_tv_step))
    # the routes compute the same thing: compare before timing
    got = {}
    for what, route, fn in routes:
        grids.grad = image.grad = None
        fn()
        got[what, route] = (grids.grad.clone(), None if image.grad is None else image.grad.clone())
    # (dL/dimage: a pixel whose luminance coordinate lies within float32 rounding of a z-cell face falls into the other cell
    #  on the torch route, and its guidance term jumps: the count of such values is reported next to the maximum)
    diff = {}
    for what in ("slice", "tv"):
        (ga, ia), (gb, ib) = got[what, "fused"], got[what, "torch"]
        diff[what] = dict(grids_max_rel_diff=float((ga - gb).abs().max() / gb.abs().max()))
        if ia is not None:
            rel = (ia - ib).abs() / ib.abs().max()
            diff[what].update(image_max_rel_diff=float(rel.max()), image_values_beyond_1e_4=int((rel > 1e-4).sum()))
    times = {(what, route): [] for what, route, _ in routes}
    for i in range(warmup + steps):
        for what, route, fn in routes:  # the routes take turns step by step
            grids.grad = image.grad = None
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[what, route].append(a.elapsed_time(b))
    out = []
    for (what, route), t in times.items():
        med, iqr = quartiles(t)
        out.append(dict(size=name, H=H, W=W, grid=list(GRID), grids=N_GRIDS, what=what, route=route, steps=steps,
                        ms_median=round(med, 4), ms_iqr=round(iqr, 4), ms_min=round(min(t), 4),
                        gradients_fused_against_torch=diff[what]))
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=sorted(SIZES), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bilagrid.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda:0")
    for name in ([a.only] if a.only else list(SIZES)):
        run(name, a.steps, a.warmup, dev)


if __name__ == "__main__":
    main()
