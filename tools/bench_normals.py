#!/usr/bin/env python3
"""Surface normals (gaussianeditor_amd/normals.py): forward plus backward of the depth-to-normals
stage and of the consistency loss at 1920 x 1080 and 512 x 512, and of gaussian_normals at 1 M rows -- the fused route
against the same mathematics written in float32 torch operators with autograd, on the same GPU.  The two routes take turns
step by step in one process; every step is timed with device events; median of --reps (30) with the interquartile range.
Prints a small markdown table and one JSON line.

Kernel times come from a separate run under the profiler, with the fused route alone:

    rocprofv3 --kernel-trace --stats -- python tools/bench_normals.py --native-only --reps 10 --sizes 1920x1080

(one size per run: the profiler's table is per kernel name).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    a = np.sort(np.asarray(ms))
    return float(np.median(a)), float(np.percentile(a, 75) - np.percentile(a, 25))


def torch_depth_normals(depth, alpha, k, alpha_min):
    """((3,H,W), (H,W) validity): the torch-operator route, in the dtype of its inputs"""
    fx, fy, cx, cy = k
    _, H, W = depth.shape
    z = depth[0] / alpha[0].clamp_min(1e-8)
    tap = (alpha[0] > alpha_min) & (z > 0)
    rx = (torch.arange(W, dtype=depth.dtype, device=depth.device) - cx) / fx
    ry = (torch.arange(H, dtype=depth.dtype, device=depth.device) - cy) / fy
    p = torch.stack([z * rx[None, :], z * ry[:, None], z], dim=0)
    c = torch.cross(p[:, 2:, 1:-1] - p[:, :-2, 1:-1], p[:, 1:-1, 2:] - p[:, 1:-1, :-2], dim=0)
    len2 = (c * c).sum(0)
    valid = tap[1:-1, 1:-1] & tap[2:, 1:-1] & tap[:-2, 1:-1] & tap[1:-1, 2:] & tap[1:-1, :-2] & (len2 >= 1e-30)
    n = torch.where(valid, c / torch.sqrt(torch.where(valid, len2, torch.ones_like(len2))), torch.zeros_like(c))
    return torch.nn.functional.pad(n, (1, 1, 1, 1)), torch.nn.functional.pad(valid, (1, 1, 1, 1))


def torch_loss(normals, depth, alpha, k, alpha_min):
    n_d, valid = torch_depth_normals(depth, alpha, k, alpha_min)
    term = alpha[0].detach() - (normals * n_d).sum(0)
    return torch.where(valid, term, torch.zeros_like(term)).sum() / (depth.shape[1] * depth.shape[2])


def torch_gaussian_normals(rot, scales, xyz, V):
    q = rot / rot.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    k = torch.argmin(scales, dim=1)
    n_c = torch.gather(R, 2, k[:, None, None].expand(-1, 3, 1))[:, :, 0] @ V[:3, :3]
    p_c = xyz @ V[:3, :3] + V[3, :3]
    return torch.where((n_c * p_c).sum(1, keepdim=True) > 0, -n_c, n_c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000, help="rows of the gaussian_normals step (0: skip it)")
    ap.add_argument("--sizes", default="1920x1080,512x512", help="image sizes, WxH, comma separated (empty: none)")
    ap.add_argument("--native-only", action="store_true", help="the fused route alone (for a run under the profiler)")
    a = ap.parse_args()
    from gaussianeditor_amd import normals as N
    from gaussianeditor_amd.synth import ring_cameras, synth_scene

    assert torch.cuda.is_available(), "this benchmark measures the MI355X: there is nothing to time without it"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    steps = {}

    def image_inputs(H, W):
        y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        z = 2.4 + 0.4 * np.sin(0.02 * x) + 0.3 * np.cos(0.03 * y) + 0.02 * rng.uniform(-1, 1, size=(H, W))
        hole = rng.uniform(size=(H, W)) < 0.1
        A = np.where(hole, rng.uniform(0.0, 0.45, size=(H, W)), rng.uniform(0.55, 1.0, size=(H, W)))
        t = lambda v: torch.tensor(v.astype(np.float32)).to(dev)  # noqa: E731
        nrm = rng.standard_normal((3, H, W))
        nrm = nrm / np.linalg.norm(nrm, axis=0, keepdims=True) * A[None] * 0.9
        return t((z * A)[None]), t(A[None]), t(nrm), t(rng.standard_normal((3, H, W)) / (H * W))

    for W, H in (tuple(int(v) for v in size.split("x")) for size in a.sizes.split(",") if size):
        depth, alpha, nrm, dout = image_inputs(H, W)
        k = (0.9 * W, 0.9 * W, (W - 1) / 2.0, (H - 1) / 2.0)
        kw = dict(fx=k[0], fy=k[1], cx=k[2], cy=k[3], alpha_min=0.5)

        def dn_native(depth=depth, alpha=alpha, dout=dout, kw=kw):
            d, al = depth.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
            N.depth_to_normals(d, al, **kw).backward(dout)
            return d.grad, al.grad

        def dn_torch(depth=depth, alpha=alpha, dout=dout, k=k):
            d, al = depth.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
            torch_depth_normals(d, al, k, 0.5)[0].backward(dout)
            return d.grad, al.grad

        def loss_native(depth=depth, alpha=alpha, nrm=nrm, kw=kw):
            n, d, al = (t.clone().requires_grad_(True) for t in (nrm, depth, alpha))
            N.normal_consistency_loss(n, d, al, **kw).backward()
            return n.grad, d.grad, al.grad

        def loss_torch(depth=depth, alpha=alpha, nrm=nrm, k=k):
            n, d, al = (t.clone().requires_grad_(True) for t in (nrm, depth, alpha))
            torch_loss(n, d, al, k, 0.5).backward()
            return n.grad, d.grad, al.grad

        steps[f"depth_to_normals {W}x{H}"] = (dn_native, dn_torch)
        steps[f"normal_consistency_loss {W}x{H}"] = (loss_native, loss_torch)

    P = a.points
    sc = synth_scene(max(P, 1), seed=0, s0=0.01, sh_degree=0)
    rot, scales, xyz = (sc[k].to(dev).contiguous() for k in ("rotation", "scaling", "xyz"))
    V = ring_cameras(4, 1920, 1080)[0].world_view_transform.to(dev).contiguous()
    gout = torch.tensor(rng.standard_normal((max(P, 1), 3)).astype(np.float32)).to(dev)

    def gn_native():
        q = rot.clone().requires_grad_(True)
        N.gaussian_normals(q, scales, xyz, V).backward(gout)
        return (q.grad,)

    def gn_torch():
        q = rot.clone().requires_grad_(True)
        torch_gaussian_normals(q, scales, xyz, V).backward(gout)
        return (q.grad,)

    if P > 0:
        steps[f"gaussian_normals {P} rows"] = (gn_native, gn_torch)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    results = {}
    print("| step (forward + backward) | fused ms (IQR) | torch float32 ms (IQR) | torch / fused | largest difference |")
    print("|---|---|---|---|---|")
    for name, (native, ref) in steps.items():
        ms = {"native": [], "torch": []}
        worst = 0.0
        for i in range(a.warmup + a.reps):
            tn, on = timed(native)
            if a.native_only:
                tt, ot = float("nan"), None
            else:
                tt, ot = timed(ref)
            if i >= a.warmup:
                ms["native"].append(tn)
                ms["torch"].append(tt)
            if ot is not None and i == 0:
                worst = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(on, ot))
        (n_med, n_iqr), (t_med, t_iqr) = summary(ms["native"]), summary(ms["torch"])
        results[name] = dict(native_ms=n_med, native_iqr=n_iqr, torch_ms=t_med, torch_iqr=t_iqr, rel_diff=worst)
        print(f"| {name} | {n_med:.3f} ({n_iqr:.3f}) | {t_med:.3f} ({t_iqr:.3f}) | {t_med / n_med:.1f}x | {worst:.1e} of the largest entry |")
    print(json.dumps(dict(reps=a.reps, steps=results)))


if __name__ == "__main__":
    main()
