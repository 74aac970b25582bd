#!/usr/bin/env python3
"""Cost of the depth-distortion image (`return_distortion`: one dedicated walk, three scalars of state per lane) against the
only route there was before it -- the composition through `features=[z, z^2]` + `return_alpha`, D = A M2 - M1^2 formed in
torch -- in one process, the routes taking turns step by step, on the headline view (synth-v1 10^6 Gaussians, 1920 x 1080) and
the 512 x 512 edit loop view:

  forward (on the state of one rendered view, under no_grad)
    distortion     gsr_blend_forward_distortion, image + moments                    (distortion_forward_kernel)
    composition    gsr_blend_forward_features with C = 2, gsr_alpha_image, the three torch ops of A M2 - M1^2
  train step (render, loss, backward)
    plain          colour loss only
    distortion     colour loss + the mean of the distortion image                   (distortion_forward / _backward_kernel)
    composition    colour loss + the mean of A M2 - M1^2 of the feature / alpha images (feature_forward / _backward_kernel)

    python tools/bench_distortion.py [--steps 30] [--warmup 5] [--only headline|edit512]

Prints one JSON line per (view, part, mode): the median over the steps in ms (CUDA events around each step) and the
interquartile range.  Per-kernel times (distortion_forward_kernel, distortion_backward_kernel next to K6 =
blend_forward_kernel, K7 = blend_backward_kernel and the feature kernels) come from running this under
`rocprofv3 --kernel-trace --stats`: the kernels are told apart by name."""
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


def run(name, steps, warmup, dev):
    P, W, H, s0 = VIEWS[name]
    sc = synth_scene(P, seed=0, s0=s0)
    cam = ring_cameras(8, W, H)[0]
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), sc["bg"].to(dev), 1.0,
                                       cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), 3,
                                       cam.camera_center.to(dev), False, False)
    leaves = [sc[k].to(dev).requires_grad_(True) for k in ("xyz", "opacity", "features", "scaling", "rotation")]
    G = seed_gradient(H, W, 0).to(dev)
    out = []

    # ---- forward, on one view's state
    xyz, op, sh, scl, rot = (t.detach() for t in leaves)
    e = torch.empty(0, device=dev)
    R, _, _, _, geom, binning, img = _C.rasterize_gaussians(rs.bg, xyz, e, op, scl, rot, 1.0, e, rs.viewmatrix, rs.projmatrix,
                                                            rs.tanfovx, rs.tanfovy, H, W, sh, 3, rs.campos, False, False)
    # the composition's features: the view-space depth and its square (the depth is data here, as in a training loop that
    # computes it from means3D in torch)
    V = rs.viewmatrix.reshape(4, 4)
    z = (xyz @ V[:3, 2] + V[3, 2]).detach()
    zz = torch.stack([z, z * z], dim=1).contiguous()

    def compose_forward():
        F = _C.rasterize_features(zz, R, geom, binning, img, H, W)
        A = _C.alpha_image(img, H, W)
        return A[0] * F[1] - F[0] * F[0]

    fwd = {"distortion": lambda: _C.rasterize_distortion(P, R, geom, binning, img, H, W), "composition": compose_forward}
    times = {k: [] for k in fwd}
    for i in range(warmup + steps):
        for k, fn in fwd.items():
            t = _timed(fn)
            if i >= warmup:
                times[k].append(t)
    for k in fwd:
        out.append(_stats(name, "forward", k, times[k], R=R))
    del geom, binning, img

    # ---- train step
    def clear():
        for t in leaves:
            t.grad = None

    def render(**kw):
        xyz, op, sh, scl, rot = leaves
        m2d = torch.zeros_like(xyz, requires_grad=True)
        return GaussianRasterizer(rs)(xyz, m2d, op, shs=sh, scales=scl, rotations=rot, **kw)

    def step_plain():
        clear()
        outs = render()
        (outs[0] * G).sum().backward()

    def step_distortion():
        clear()
        outs = render(return_distortion=True)
        ((outs[0] * G).sum() + outs[-1].mean()).backward()

    def step_composition():
        clear()
        zl = leaves[0] @ V[:3, 2] + V[3, 2]
        outs = render(return_alpha=True, features=torch.stack([zl, zl * zl], dim=1))
        A, F = outs[-2][0], outs[-1]
        ((outs[0] * G).sum() + (A * F[1] - F[0] * F[0]).mean()).backward()

    modes = {"plain": step_plain, "distortion": step_distortion, "composition": step_composition}
    times = {k: [] for k in modes}
    for i in range(warmup + steps):
        for k, fn in modes.items():  # the modes take turns: drift of the clocks hits all alike
            t = _timed(fn)
            if i >= warmup:
                times[k].append(t)
    for k in modes:
        out.append(_stats(name, "train step", k, times[k]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=sorted(VIEWS), default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in ([a.only] if a.only else list(VIEWS)):
        run(name, a.steps, a.warmup, dev)


if __name__ == "__main__":
    main()
