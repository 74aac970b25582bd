#!/usr/bin/env python3
"""Cost of camera pose gradients (gaussianeditor_amd.set_pose_grad): the BACKWARD of one train step with the flag off and on,
ALTERNATING step by step in one process, on the headline view (synth-v1 10^6 Gaussians, 1920 x 1080) and the 512 x 512 edit
loop view.  The camera tensors require a gradient in both modes; only the flag differs.

    python tools/bench_pose_grad.py [--steps 30] [--warmup 5] [--reps 3] [--only headline|edit512]

Prints one JSON line per (view, repetition, mode) with the median backward time in ms (CUDA events around the backward)."""
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
MODES = (("plain", 0), ("pose_grad", options.FLAG_POSE_GRAD))


def run(name, steps, warmup, reps, dev):
    P, W, H, s0 = VIEWS[name]
    sc = synth_scene(P, seed=0, s0=s0)
    cam = ring_cameras(8, W, H)[0]
    cams = [t.to(dev).clone().requires_grad_(True) for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), sc["bg"].to(dev), 1.0,
                                       cams[0], cams[1], 3, cams[2], False, False)
    leaves = [sc[k].to(dev).requires_grad_(True) for k in ("xyz", "opacity", "features", "scaling", "rotation")]
    G = seed_gradient(H, W, 0).to(dev)
    for rep in range(reps):
        times = {mode: [] for mode, _ in MODES}
        for i in range(warmup + steps):
            for mode, flags in MODES:  # the two modes take turns: drift of the clocks hits both alike
                for t in leaves + cams:
                    t.grad = None
                xyz, op, sh, scl, rot = leaves
                m2d = torch.zeros_like(xyz, requires_grad=True)
                with options.override(flags):
                    color, radii, d = GaussianRasterizer(rs)(xyz, m2d, op, shs=sh, scales=scl, rotations=rot)
                loss = (color * G).sum()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                loss.backward()
                b.record()
                torch.cuda.synchronize()
                assert (cams[0].grad is not None) == bool(flags)
                if i >= warmup:
                    times[mode].append(a.elapsed_time(b))
        for mode, _ in MODES:
            t = sorted(times[mode])
            print(json.dumps(dict(view=name, P=P, W=W, H=H, rep=rep, mode=mode, steps=steps,
                                  backward_ms_median=round(t[len(t) // 2], 4), backward_ms_min=round(t[0], 4),
                                  backward_ms_max=round(t[-1], 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=sorted(VIEWS), default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in ([a.only] if a.only else list(VIEWS)):
        run(name, a.steps, a.warmup, a.reps, dev)


if __name__ == "__main__":
    main()
