#!/usr/bin/env python3
"""Cost of the feature image (`features=`: C per-Gaussian channels composited in one walk per 16-channel block) against the
only route there was before it -- one three-channel render per slice -- in one process, the modes taking turns step by step,
on the headline view (synth-v1 10^6 Gaussians, 1920 x 1080) and the 512 x 512 edit loop view, C = 16:

  forward (on the state of one rendered view, under no_grad)
    features       gsr_blend_forward_features, all 16 channels                      (feature_forward_kernel)
    aux x6         six rasterize_gaussians_aux launches, three channels each        (the former route)
  train step (render, loss, backward)
    plain          colour loss only
    features       colour loss + a loss on the C = 16 feature image                 (feature_forward / feature_backward_kernel)
    override x6    the plain step + six render(override_color = slice) with a loss and a backward each (the former route)
  zero fill
    zero_features  torch.zeros((P, 16)): the fill of dL_dfeatures every feature backward starts from (64 MB at 10^6 x 16)

    python tools/bench_features.py [--steps 30] [--warmup 5] [--only headline|edit512] [--channels 16]

Prints one JSON line per (view, part, mode): the median over the steps in ms (CUDA events around each step) and the
interquartile range.  Per-kernel times (feature_forward_kernel, feature_backward_kernel next to K7 = blend_backward_kernel,
the fill) come from running this under `rocprofv3 --kernel-trace --stats`: the kernels are told apart by name."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gaussianeditor_amd.diff_gaussian_rasterization import _C, GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from gaussianeditor_amd.synth import ring_cameras, seed_gradient, synth_scene  # noqa: E402

VIEWS = {"headline": (1_000_000, 1920, 1080, 0.01), "edit512": (1_000_000, 512, 512, 0.01)}


def _stats(view, part, mode, times, **more):
    t = sorted(times)
    n = len(t)
    q = lambda f: t[min(n - 1, int(f * n))]  # noqa: E731
    rec = dict(view=view, part=part, mode=mode, steps=n, ms_median=round(q(0.5), 4), ms_iqr=round(q(0.75) - q(0.25), 4),
               ms_min=round(t[0], 4), ms_max=round(t[-1], 4), **more)
    print(json.dumps(rec), flush=True)
    return rec


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def run(name, steps, warmup, C, dev):
    P, W, H, s0 = VIEWS[name]
    sc = synth_scene(P, seed=0, s0=s0)
    cam = ring_cameras(8, W, H)[0]
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), sc["bg"].to(dev), 1.0,
                                       cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), 3,
                                       cam.camera_center.to(dev), False, False)
    rs0 = rs._replace(bg=torch.zeros(3, device=dev))
    leaves = [sc[k].to(dev).requires_grad_(True) for k in ("xyz", "opacity", "features", "scaling", "rotation")]
    feats = (torch.rand(P, C, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev).requires_grad_(True)
    nsl = (C + 2) // 3
    pad = torch.zeros(P, 3 * nsl - C, device=dev)
    G = seed_gradient(H, W, 0).to(dev)
    GF = torch.cat([seed_gradient(H, W, 7 + k) for k in range(nsl)], dim=0)[:C].contiguous().to(dev)
    GFs = torch.cat([GF, torch.zeros(3 * nsl - C, H, W, device=dev)], dim=0)
    out = []

    # ---- forward, on one view's state
    xyz, op, sh, scl, rot = (t.detach() for t in leaves)
    e = torch.empty(0, device=dev)
    R, _, _, _, geom, binning, img = _C.rasterize_gaussians(rs.bg, xyz, e, op, scl, rot, 1.0, e, rs.viewmatrix, rs.projmatrix,
                                                            rs.tanfovx, rs.tanfovy, H, W, sh, 3, rs.campos, False, False)
    fd = feats.detach()
    cols = [c.contiguous() for c in torch.cat([fd, pad], dim=1).split(3, dim=1)]
    bg0 = torch.zeros(3, device=dev)
    fwd = {"features": lambda: _C.rasterize_features(fd, R, geom, binning, img, H, W),
           f"aux x{nsl}": lambda: [_C.rasterize_gaussians_aux(bg0, c, R, geom, binning, img, H, W) for c in cols],
           "zero_features": lambda: torch.zeros((P, C), dtype=torch.float32, device=dev)}
    times = {k: [] for k in fwd}
    for i in range(warmup + steps):
        for k, fn in fwd.items():
            t = _timed(fn)
            if i >= warmup:
                times[k].append(t)
    for k in fwd:
        out.append(_stats(name, "zero fill" if k == "zero_features" else "forward", k, times[k], C=C, R=R))
    del geom, binning, img

    # ---- train step
    def clear():
        for t in leaves + [feats]:
            t.grad = None

    def render(**kw):
        xyz, op, sh, scl, rot = leaves
        m2d = torch.zeros_like(xyz, requires_grad=True)
        return xyz, m2d, op, scl, rot, GaussianRasterizer(kw.pop("rs", rs))(xyz, m2d, op, scales=scl, rotations=rot, **kw)

    def step_plain():
        clear()
        *_, outs = render(shs=leaves[2])
        (outs[0] * G).sum().backward()

    def step_features():
        clear()
        *_, outs = render(shs=leaves[2], features=feats)
        ((outs[0] * G).sum() + (outs[3] * GF).sum()).backward()

    def step_override():
        step_plain()
        padded = torch.cat([feats, pad], dim=1)
        for k in range(nsl):
            *_, outs = render(colors_precomp=padded[:, 3 * k:3 * k + 3], rs=rs0)
            (outs[0] * GFs[3 * k:3 * k + 3]).sum().backward()

    modes = {"plain": step_plain, "features": step_features, f"override x{nsl}": step_override}
    times = {k: [] for k in modes}
    for i in range(warmup + steps):
        for k, fn in modes.items():  # the modes take turns: drift of the clocks hits all alike
            t = _timed(fn)
            if i >= warmup:
                times[k].append(t)
    for k in modes:
        out.append(_stats(name, "train step", k, times[k], C=C))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--only", choices=sorted(VIEWS), default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in ([a.only] if a.only else list(VIEWS)):
        run(name, a.steps, a.warmup, a.channels, dev)


if __name__ == "__main__":
    main()
