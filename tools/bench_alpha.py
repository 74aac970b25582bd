#!/usr/bin/env python3
"""Cost of the alpha image (`return_alpha=True`, gaussianeditor_amd.set_alpha_output): one train step -- render, loss,
backward -- in four modes that take turns step by step in one process, on the headline view (synth-v1 10^6 Gaussians,
1920 x 1080) and the 512 x 512 edit loop view:

    plain          colour loss only (today's step)
    alpha          + the alpha image and a loss on it        (alpha_image_kernel, the ALPHA K7, the backward as its two halves)
    depth          + a loss on the depth image               (the DEPTH K7: no list segments)
    depth+alpha    both                                      (DEPTH + ALPHA)

    python tools/bench_alpha.py [--steps 30] [--warmup 5] [--only headline|edit512]

Prints one JSON line per (view, mode) with the median step time in ms (CUDA events around each step).  `alpha` against
`plain` is the price of the feature; `alpha` against `depth` shows that an alpha backward keeps the list segments a depth
backward gives up.  Per-kernel times (K7 = blend_backward_kernel, alpha_image_kernel) come from running this under
`rocprofv3 --kernel-trace --stats`: the alpha steps launch the ALPHA instantiations (fifth template argument = true), so the
modes are told apart by the kernel names."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gaussianeditor_amd import options  # noqa: E402
from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from gaussianeditor_amd.synth import ring_cameras, seed_gradient, synth_scene  # noqa: E402

VIEWS = {"headline": (1_000_000, 1920, 1080, 0.01), "edit512": (1_000_000, 512, 512, 0.01)}
MODES = (("plain", False, False), ("alpha", True, False), ("depth", False, True), ("depth+alpha", True, True))


def run(name, steps, warmup, dev):
    P, W, H, s0 = VIEWS[name]
    sc = synth_scene(P, seed=0, s0=s0)
    cam = ring_cameras(8, W, H)[0]
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), sc["bg"].to(dev), 1.0,
                                       cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), 3,
                                       cam.camera_center.to(dev), False, False)
    leaves = [sc[k].to(dev).requires_grad_(True) for k in ("xyz", "opacity", "features", "scaling", "rotation")]
    G = seed_gradient(H, W, 0).to(dev)
    GA, GD = seed_gradient(H, W, 5)[:1].to(dev), seed_gradient(H, W, 7)[:1].to(dev)
    times = {mode: [] for mode, _, _ in MODES}
    for i in range(warmup + steps):
        for mode, alpha, depth in MODES:  # the modes take turns: drift of the clocks hits all alike
            for t in leaves:
                t.grad = None
            xyz, op, sh, scl, rot = leaves
            m2d = torch.zeros_like(xyz, requires_grad=True)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            with options.override(options.FLAG_DEPTH_GRAD if depth else 0):
                outs = GaussianRasterizer(rs)(xyz, m2d, op, shs=sh, scales=scl, rotations=rot, **({"return_alpha": True} if alpha else {}))
            loss = (outs[0] * G).sum()
            if alpha:
                loss = loss + (outs[3] * GA).sum()
            if depth:
                loss = loss + (outs[2] * GD).sum()
            loss.backward()
            b.record()
            torch.cuda.synchronize()
            assert len(outs) == (4 if alpha else 3)
            if i >= warmup:
                times[mode].append(a.elapsed_time(b))
    out = []
    for mode, _, _ in MODES:
        t = sorted(times[mode])
        out.append(dict(view=name, P=P, W=W, H=H, mode=mode, steps=steps, step_ms_median=round(t[len(t) // 2], 4),
                        step_ms_min=round(t[0], 4), step_ms_max=round(t[-1], 4)))
        print(json.dumps(out[-1]), flush=True)
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
