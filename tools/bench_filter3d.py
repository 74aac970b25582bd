#!/usr/bin/env python3
"""Mip-Splatting's 3D filter (gaussianeditor_amd/filter3d.py): the camera sweep at --points (1 M)
rows with V in --views (1, 64, 200) cameras of 1920 x 1080, and the fused apply, forward plus backward, at the same rows with
both `from_raw` settings -- the native route against the same mathematics written in float32 torch operators on the same
GPU: Mip-Splatting's per-camera loop for the sweep, its two getters with autograd for the apply.  The two routes take turns
step by step in one process; every step is timed with device events; median of --reps (30) with the interquartile range.
The apply's two kernels are then timed alone through the C ABI (--batch launches between two events) and set against the
bytes they must move: 36 B per row forward (five floats in, four out), 52 B per row backward (nine in, four out).
Prints two small markdown tables and one JSON line.

Kernel times come from a separate run under the profiler, with the native route alone:

    rocprofv3 --kernel-trace --stats -- python tools/bench_filter3d.py --native-only --reps 10
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def summary(ms):
    a = np.sort(np.asarray(ms))
    return float(np.median(a)), float(np.percentile(a, 75) - np.percentile(a, 25))


def torch_compute_3d_filter(xyz, cameras):
    """Mip-Splatting's compute_3D_filter: one pass of some fifteen float32 operators per camera over all rows"""
    P = xyz.shape[0]
    distance = torch.full((P,), 100000.0, device=xyz.device)
    seen = torch.zeros(P, dtype=torch.bool, device=xyz.device)
    focal = 0.0
    for cam in cameras:
        W, H = cam.image_width, cam.image_height
        fx, fy = W / (2.0 * math.tan(cam.FoVx / 2.0)), H / (2.0 * math.tan(cam.FoVy / 2.0))
        V = cam.world_view_transform
        p = xyz @ V[:3, :3] + V[3:4, :3]
        in_front = p[:, 2] > 0.2
        z = torch.clamp(p[:, 2], min=0.001)
        u = p[:, 0] / z * fx + W / 2.0
        v = p[:, 1] / z * fy + H / 2.0
        in_screen = torch.logical_and(torch.logical_and(u >= -0.15 * W, u <= 1.15 * W), torch.logical_and(v >= -0.15 * H, v <= 1.15 * H))
        valid = torch.logical_and(in_front, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        seen = torch.logical_or(seen, valid)
        focal = max(focal, fx)
    distance[~seen] = distance[seen].max()
    return (distance / focal * (0.2 ** 0.5))[..., None]


def torch_apply_3d_filter(scales, opacity, filter_3D, from_raw):
    """get_scaling_with_3D_filter and get_opacity_with_3D_filter"""
    s = torch.exp(scales) if from_raw else scales
    o = torch.sigmoid(opacity) if from_raw else opacity
    s2 = torch.square(s)
    e = s2 + torch.square(filter_3D)
    coef = torch.sqrt(s2.prod(dim=1) / e.prod(dim=1))
    return torch.sqrt(e), o * coef[..., None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--views", default="1,64,200", help="camera counts of the sweep, comma separated (empty: none)")
    ap.add_argument("--batch", type=int, default=20, help="launches between two events when a kernel is timed alone")
    ap.add_argument("--native-only", action="store_true", help="the native route alone (for a run under the profiler)")
    a = ap.parse_args()
    from gaussianeditor_amd import _native
    from gaussianeditor_amd import filter3d as F3
    from gaussianeditor_amd.synth import ring_cameras, synth_scene

    assert torch.cuda.is_available(), "this benchmark measures the MI355X: there is nothing to time without it"
    dev = torch.device("cuda:0")
    P = a.points
    sc = synth_scene(P, seed=0, s0=0.01, sh_degree=0)
    xyz = sc["xyz"].to(dev).contiguous()
    rng = np.random.default_rng(0)
    steps = {}
    for V in (int(v) for v in a.views.split(",") if v):
        cams = [c.to(dev) for c in ring_cameras(V, 1920, 1080)]
        packed = F3.pack_cameras(cams, dev)
        steps[f"sweep {P} rows x {V} cameras"] = (lambda packed=packed: (F3.compute_3d_filter(xyz, packed),),
                                                   lambda cams=cams: (torch_compute_3d_filter(xyz, cams),))
        if V > 1:
            steps[f"sweep {P} rows x {V} cameras, packed on every call"] = (lambda cams=cams: (F3.compute_3d_filter(xyz, cams),),
                                                                             lambda cams=cams: (torch_compute_3d_filter(xyz, cams),))
    filt = F3.compute_3d_filter(xyz, F3.pack_cameras(ring_cameras(8, 1920, 1080), dev))
    g_s = torch.tensor(rng.standard_normal((P, 3)).astype(np.float32)).to(dev)
    g_o = torch.tensor(rng.standard_normal((P, 1)).astype(np.float32)).to(dev)
    inputs = {False: (sc["scaling"].to(dev).contiguous(), sc["opacity"].to(dev).contiguous()),
              True: (torch.log(sc["scaling"]).to(dev).contiguous(), torch.logit(sc["opacity"]).to(dev).contiguous())}
    for from_raw, (s0, o0) in inputs.items():
        def run(fn, s0=s0, o0=o0, from_raw=from_raw):
            s, o = s0.clone().requires_grad_(True), o0.clone().requires_grad_(True)
            torch.autograd.backward(list(fn(s, o, filt, from_raw)), [g_s, g_o])
            return s.grad, o.grad

        steps[f"apply forward + backward {P} rows, from_raw={from_raw}"] = (lambda run=run: run(F3.apply_3d_filter),
                                                                           lambda run=run: run(torch_apply_3d_filter))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    results = {}
    print("| step | native ms (IQR) | torch float32 ms (IQR) | torch / native | largest difference |")
    print("|---|---|---|---|---|")
    for name, (native, ref) in steps.items():
        ms = {"native": [], "torch": []}
        worst = 0.0
        for i in range(a.warmup + a.reps):
            tn, on = timed(native)
            tt, ot = (float("nan"), None) if a.native_only else timed(ref)
            if i >= a.warmup:
                ms["native"].append(tn)
                ms["torch"].append(tt)
            if ot is not None and i == 0:
                worst = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(on, ot))
        (n_med, n_iqr), (t_med, t_iqr) = summary(ms["native"]), summary(ms["torch"])
        results[name] = dict(native_ms=n_med, native_iqr=n_iqr, torch_ms=t_med, torch_iqr=t_iqr, rel_diff=worst)
        print(f"| {name} | {n_med:.3f} ({n_iqr:.3f}) | {t_med:.3f} ({t_iqr:.3f}) | {t_med / n_med:.1f}x | {worst:.1e} of the largest entry |")

    # the apply's kernels alone, through the C ABI, against the bytes they must move
    L = _native.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    s_eff, o_eff = torch.empty_like(inputs[True][0]), torch.empty_like(inputs[True][1])
    d_s, d_o = torch.empty_like(s_eff), torch.empty_like(o_eff)
    print()
    print("| kernel | ms per launch (IQR) | bytes moved | GB/s | of the 8 TB/s peak |")
    print("|---|---|---|---|---|")
    for from_raw, (s0, o0) in inputs.items():
        calls = {
            "forward": (36 * P, lambda s0=s0, o0=o0, r=int(from_raw): L.gsr_filter3d_apply_forward(
                st, P, r, s0.data_ptr(), o0.data_ptr(), filt.data_ptr(), s_eff.data_ptr(), o_eff.data_ptr())),
            "backward": (52 * P, lambda s0=s0, o0=o0, r=int(from_raw): L.gsr_filter3d_apply_backward(
                st, P, r, s0.data_ptr(), o0.data_ptr(), filt.data_ptr(), g_s.data_ptr(), g_o.data_ptr(), d_s.data_ptr(), d_o.data_ptr())),
        }
        for which, (nbytes, call) in calls.items():
            def batch(call=call):
                for _ in range(a.batch):
                    assert call() == 0
            per = [timed(batch)[0] / a.batch for _ in range(a.warmup + a.reps)][a.warmup:]
            med, iqr = summary(per)
            gbs = nbytes / (med * 1e-3) / 1e9
            results[f"apply {which} kernel, from_raw={from_raw}"] = dict(ms=med, iqr=iqr, bytes=nbytes, gb_per_s=gbs)
            print(f"| apply {which}, from_raw={from_raw} | {med:.4f} ({iqr:.4f}) | {nbytes} | {gbs:.0f} | {gbs / HBM_PEAK_GBS:.2f} |")
    print(json.dumps(dict(reps=a.reps, points=P, steps=results)))


if __name__ == "__main__":
    main()
