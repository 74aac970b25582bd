#!/usr/bin/env python3
"""Cost of absolute screen-space gradients (gaussianeditor_amd.set_abs_grad): one train step -- render, loss, backward -- with
the flag off and on, ALTERNATING step by step in one process, on the headline view (synth-v1 10^6 Gaussians, 1920 x 1080) and
the 512 x 512 edit loop view.

    python tools/bench_abs_grad.py [--steps 30] [--warmup 5] [--only headline|edit512]

Prints one JSON line per (view, mode) with the median step time in ms (CUDA events around each step).  Per-kernel times
(K7 = blend_backward_kernel, the take kernel = abs_grad_take_kernel, K8+K9 = preprocess_backward_kernel) come from running
this under `rocprofv3 --kernel-trace --stats`: the flagged steps launch the ABS instantiations (fourth template argument =
true), so the two modes are told apart by the kernel names."""
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
MODES = (("plain", 0), ("absgrad", options.FLAG_ABS_GRAD))


def run(name, steps, warmup, dev):
    P, W, H, s0 = VIEWS[name]
    sc = synth_scene(P, seed=0, s0=s0)
    cam = ring_cameras(8, W, H)[0]
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), sc["bg"].to(dev), 1.0,
                                       cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), 3,
                                       cam.camera_center.to(dev), False, False)
    leaves = [sc[k].to(dev).requires_grad_(True) for k in ("xyz", "opacity", "features", "scaling", "rotation")]
    G = seed_gradient(H, W, 0).to(dev)
    times = {mode: [] for mode, _ in MODES}
    for i in range(warmup + steps):
        for mode, flags in MODES:  # the two modes take turns: drift of the clocks hits both alike
            for t in leaves:
                t.grad = None
            xyz, op, sh, scl, rot = leaves
            m2d = torch.zeros_like(xyz, requires_grad=True)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            with options.override(flags):
                color, radii, d = GaussianRasterizer(rs)(xyz, m2d, op, shs=sh, scales=scl, rotations=rot)
            (color * G).sum().backward()
            b.record()
            torch.cuda.synchronize()
            assert hasattr(m2d, "absgrad") == bool(flags)
            if i >= warmup:
                times[mode].append(a.elapsed_time(b))
    out = []
    for mode, _ in MODES:
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
