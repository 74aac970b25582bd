#!/usr/bin/env python3
"""Cost of the contribution statistics (gsr_trace_contributions: sum / max of the blending weight per Gaussian, the
contribution-weighted mask sums, the per-pixel pick buffer) against the nearest existing kernel and against the only route
to sum w there was before it, in one process, the modes taking turns step by step, on synth-v1 10^6 Gaussians at 512 x 512
(the edit loop's view) and 1920 x 1080 (the headline view):

  kernel (on the state of one binned view: one launch each)
    contrib C=0            gsr_trace_contributions, no mask, no pixel images       (trace_contributions_kernel<0>)
    contrib C=1 +pixels    one mask channel, top_id and top_weight written         (trace_contributions_kernel<1>)
    apply_weights C=1      gsr_trace_weights on the same state                     (trace_weights_kernel<1>, K12)
  call (preprocess without colours + bin + the kernel, as the public functions run them; the trick: a whole train step)
    contrib C=0            GaussianRasterizer.trace_contributions
    contrib C=1 +pixels
    apply_weights C=1      GaussianRasterizer.apply_weights
    backward-trick         render with colours 1, backward with dL/dpixel = 1: dL_dcolors[:, 0] = sum w (K1 .. K6, K7, K8+K9)
  zero fill
    zero_stats             torch.zeros((P, 4), int64): the table a series of views starts from (32 MB at 10^6)

    python tools/bench_contrib.py [--steps 30] [--warmup 5] [--only edit512|headline]

Prints one JSON line per (view, part, mode): the median over the steps in ms (CUDA events around each step) and the
interquartile range, and per view the ratios contrib : apply_weights (kernel) and contrib : backward-trick (call)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gaussianeditor_amd import _native  # noqa: E402
from gaussianeditor_amd.diff_gaussian_rasterization import _C, GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from gaussianeditor_amd.synth import ring_cameras, synth_scene  # noqa: E402

VIEWS = {"edit512": (1_000_000, 512, 512, 0.01), "headline": (1_000_000, 1920, 1080, 0.01)}


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


def _turns(modes, steps, warmup):
    times = {k: [] for k in modes}
    for i in range(warmup + steps):
        for k, fn in modes.items():  # the modes take turns: drift of the clocks hits all alike
            t = _timed(fn)
            if i >= warmup:
                times[k].append(t)
    return times


def run(name, steps, warmup, dev):
    P, W, H, s0 = VIEWS[name]
    sc = synth_scene(P, seed=0, s0=s0)
    cam = ring_cameras(8, W, H)[0]
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), torch.zeros(3, device=dev), 1.0,
                                       cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), 3,
                                       cam.camera_center.to(dev), False, False)
    xyz, op, sh, scl, rot = (sc[k].to(dev) for k in ("xyz", "opacity", "features", "scaling", "rotation"))
    mask = (torch.rand(1, H, W, generator=torch.Generator().manual_seed(2)) > 0.5).float().to(dev)
    stats0 = torch.zeros((P, 3), dtype=torch.int64, device=dev)
    stats1 = torch.zeros((P, 4), dtype=torch.int64, device=dev)
    w = torch.zeros((P, 1), dtype=torch.float32, device=dev)
    cnt = torch.zeros((P, 1), dtype=torch.int32, device=dev)
    e = torch.empty(0, device=dev)
    R, _, _, _, geom, binning, img = _C.rasterize_gaussians(rs.bg, xyz, e, op, scl, rot, 1.0, e, rs.viewmatrix, rs.projmatrix,
                                                            rs.tanfovx, rs.tanfovy, H, W, sh, 3, rs.campos, False, False)
    L = _native.lib()

    def k12():
        _native.check("gsr_trace_weights", L.gsr_trace_weights(
            torch.cuda.current_stream(dev).cuda_stream, P, R, W, H, 1, geom.data_ptr(), binning.data_ptr(), img.data_ptr(),
            mask.data_ptr(), w.data_ptr(), cnt.data_ptr(), 0))

    kernel = {"contrib C=0": lambda: _C.trace_contributions_state(stats0, R, geom, binning, img, H, W),
              "contrib C=1 +pixels": lambda: _C.trace_contributions_state(stats1, R, geom, binning, img, H, W, image_weights=mask,
                                                                          return_pixels=True),
              "apply_weights C=1": k12,
              "zero_stats": lambda: torch.zeros((P, 4), dtype=torch.int64, device=dev)}
    times = _turns(kernel, steps, warmup)
    recs = {k: _stats(name, "zero fill" if k == "zero_stats" else "kernel", k, times[k], R=R) for k in kernel}
    del geom, binning, img

    rast = GaussianRasterizer(rs)
    ones = torch.ones(P, 3, device=dev, requires_grad=True)
    leaves = [t.clone().requires_grad_(True) for t in (xyz, op, scl, rot)]
    Gone = torch.ones(3, H, W, device=dev)

    def trick():
        ones.grad = None
        for t in leaves:
            t.grad = None
        x, o, s, r = leaves
        m2d = torch.zeros_like(x, requires_grad=True)
        outs = rast(x, m2d, o, colors_precomp=ones, scales=s, rotations=r)
        outs[0].backward(Gone)

    call = {"contrib C=0": lambda: rast.trace_contributions(xyz, op, scales=scl, rotations=rot, stats=stats0),
            "contrib C=1 +pixels": lambda: rast.trace_contributions(xyz, op, scales=scl, rotations=rot, stats=stats1,
                                                                    image_weights=mask, return_pixels=True),
            "apply_weights C=1": lambda: rast.apply_weights(xyz, None, op, None, w, scl, rot, None, cnt, mask),
            "backward-trick": trick}
    times = _turns(call, steps, warmup)
    crecs = {k: _stats(name, "call", k, times[k]) for k in call}
    print(json.dumps(dict(
        view=name, part="ratios",
        kernel_contrib_C1_pixels_to_apply_weights=round(recs["contrib C=1 +pixels"]["ms_median"] / recs["apply_weights C=1"]["ms_median"], 3),
        kernel_contrib_C0_to_apply_weights=round(recs["contrib C=0"]["ms_median"] / recs["apply_weights C=1"]["ms_median"], 3),
        call_contrib_C0_to_backward_trick=round(crecs["contrib C=0"]["ms_median"] / crecs["backward-trick"]["ms_median"], 3),
        call_contrib_C1_pixels_to_backward_trick=round(crecs["contrib C=1 +pixels"]["ms_median"] / crecs["backward-trick"]["ms_median"], 3))),
        flush=True)


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
