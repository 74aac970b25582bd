#!/usr/bin/env python3
"""TSDF fusion and mesh extraction (gaussianeditor_amd/tsdf.py): --views (64) depth maps of
--image (512) squared pixels of a unit sphere, with alpha and colour, fused into a volume of --grids (256, 512) cubed lattice
points over [-1.5, 1.5]^3 with a truncation of four voxels --

  * by one fused `integrate` call,
  * by one `integrate` call per view,
  * by the same integration composed from float32 torch operators on the same GPU, one pass per view (the baseline),

and `extract_mesh` on the fused volume.  The routes take turns in one process; every step starts from a fresh volume (made
outside the timed window) and is timed with device events; median with the interquartile range of --reps (10; the torch
baseline: --torch-reps, 3).  The fused call is also set against the bytes the volume must move once: 20 B per lattice point
each way.  Prints one markdown table and one JSON line.

Kernel times come from a separate run under the profiler, with the native route alone:

    rocprofv3 --kernel-trace --stats -- python tools/bench_tsdf.py --native-only --reps 5
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
NEAR = 0.2


def summary(ms):
    a = np.sort(np.asarray(ms))
    return float(np.median(a)), float(np.percentile(a, 75) - np.percentile(a, 25))


def sphere_views(cams, W, H, dev):
    """(depth_3dgs (V,1,H,W), alpha (V,1,H,W), colour (V,3,H,W)) of the unit sphere as the rasterizer's conventions give them:
    view-space z of the first hit through every pixel centre, alpha 0.9 on the sphere and 0 beside it, depth alpha-weighted"""
    depth, alpha, color = [], [], []
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    for c in cams:
        M = c.world_view_transform.to(dev).double()
        fx, fy = W / (2.0 * np.tan(c.FoVx / 2.0)), H / (2.0 * np.tan(c.FoVy / 2.0))
        d_cam = torch.stack([(u - (W - 1) / 2.0) / fx, (v - (H - 1) / 2.0) / fy, torch.ones_like(u)], dim=-1)  # z = 1 along the axis
        R, t = M[:3, :3], M[3, :3]            # x_cam = x_world R + t
        eye = -(t @ R.T)
        d_world = d_cam @ R.T
        a, b, cc = (d_world * d_world).sum(-1), 2.0 * (d_world @ eye), float(eye @ eye) - 1.0
        disc = b * b - 4.0 * a * cc
        hit = disc > 0
        z = torch.where(hit, (-b - torch.sqrt(disc.clamp_min(0.0))) / (2.0 * a), torch.zeros_like(a))  # (the ray parameter IS z)
        al = torch.where(hit, 0.9, 0.0)
        p = eye + z[..., None] * d_world
        depth.append((z * al).float()[None])
        alpha.append(al.float()[None])
        color.append((0.5 + 0.5 * p).clamp(0, 1).permute(2, 0, 1).float() * hit)
    return torch.stack(depth).contiguous(), torch.stack(alpha).contiguous(), torch.stack(color).contiguous()


class TorchVolume:
    """The same integration from float32 torch operators, one pass over the volume per view."""

    def __init__(self, origin, vs, n, trunc, dev):
        self.trunc, self.n = trunc, n
        ax = [origin[a] + vs * torch.arange(n, device=dev, dtype=torch.float32) for a in range(3)]
        self.x, self.y, self.z = (g.contiguous() for g in torch.meshgrid(*ax, indexing="ij"))
        self.reset()

    def reset(self):
        dev, n = self.x.device, self.n
        self.tsdf, self.weight = torch.ones((n, n, n), device=dev), torch.zeros((n, n, n), device=dev)
        self.color = torch.zeros((3, n, n, n), device=dev)

    def integrate(self, depth, alpha, color, mats, fxs, fys, alpha_min=0.5):
        V, _, H, W = depth.shape
        for i in range(V):
            M = mats[i]
            zc = self.x * M[0, 2] + self.y * M[1, 2] + self.z * M[2, 2] + M[3, 2]
            p0 = self.x * M[0, 0] + self.y * M[1, 0] + self.z * M[2, 0] + M[3, 0]
            p1 = self.x * M[0, 1] + self.y * M[1, 1] + self.z * M[2, 1] + M[3, 1]
            zs = zc.clamp_min(1e-6)
            iu = torch.floor(p0 / zs * fxs[i] + (W - 1) / 2.0 + 0.5).long()
            iv = torch.floor(p1 / zs * fys[i] + (H - 1) / 2.0 + 0.5).long()
            ok = (zc > NEAR) & (iu >= 0) & (iu < W) & (iv >= 0) & (iv < H)
            pix = (iv.clamp(0, H - 1) * W + iu.clamp(0, W - 1)).reshape(-1)
            a = alpha[i, 0].reshape(-1)[pix].reshape(zc.shape)
            d = depth[i, 0].reshape(-1)[pix].reshape(zc.shape) / a
            sdf = d - zc
            ok = ok & (a >= alpha_min) & (d > 0) & (sdf >= -self.trunc)
            obs = (sdf / self.trunc).clamp_max(1.0)
            w1 = self.weight + 1.0
            self.tsdf = torch.where(ok, (self.tsdf * self.weight + obs) / w1, self.tsdf)
            rgb = color[i].reshape(3, -1)[:, pix].reshape((3,) + tuple(zc.shape))
            self.color = torch.where(ok[None], (self.color * self.weight[None] + rgb) / w1[None], self.color)
            self.weight = torch.where(ok, w1, self.weight)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grids", default="256,512", help="lattice points per axis, comma separated")
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--native-only", action="store_true", help="the native route alone (for a run under the profiler)")
    a = ap.parse_args()
    from gaussianeditor_amd import filter3d as F3
    from gaussianeditor_amd import tsdf as T
    from gaussianeditor_amd.synth import ring_cameras

    assert torch.cuda.is_available(), "this benchmark measures the MI355X: there is nothing to time without it"
    dev = torch.device("cuda:0")
    V, W = a.views, a.image
    cams = ring_cameras(V, W, W)
    packed = F3.pack_cameras(cams, dev)
    depth, alpha, color = sphere_views(cams, W, W, dev)
    mats = [c.world_view_transform.to(dev).float() for c in cams]
    fxs = [float(r[12]) for r in packed.records.cpu().numpy()]
    fys = [float(r[13]) for r in packed.records.cpu().numpy()]
    singles = [(depth[i:i + 1], F3.PackedCameras(packed.records[i:i + 1].contiguous(), packed.f_max), alpha[i:i + 1], color[i:i + 1])
               for i in range(V)]

    def timed(fn, before=None):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    results = {}
    print(f"{V} views of {W} x {W}")
    print("| lattice | step | ms (IQR) | note |")
    print("|---|---|---|---|")
    for n in (int(g) for g in a.grids.split(",") if g):
        vs = 3.0 / (n - 1)
        vol = T.TSDFVolume((-1.5, -1.5, -1.5), vs, (n, n, n), 4.0 * vs, device=dev)

        def fused():
            vol.integrate(depth, packed, alpha=alpha, color=color)

        def one_by_one():
            for d, p, al, co in singles:
                vol.integrate(d, p, alpha=al, color=co)

        steps = [("fused integrate", fused, a.reps), (f"{V} one-view integrate calls", one_by_one, a.reps)]
        tv = None
        if not a.native_only:
            tv = TorchVolume((-1.5, -1.5, -1.5), vs, n, 4.0 * vs, dev)
            steps.append(("torch operators, one pass per view", lambda tv=tv: tv.integrate(depth, alpha, color, mats, fxs, fys), a.torch_reps))
        res = {}
        for name, fn, reps in steps:
            reset = tv.reset if name.startswith("torch") else vol.reset
            ms = [timed(fn, reset)[0] for _ in range(a.warmup + reps)][a.warmup:]
            res[name] = summary(ms)
        med = res["fused integrate"][0]
        gbs = 2 * 20 * n ** 3 / (med * 1e-3) / 1e9
        notes = {"fused integrate": f"{gbs:.0f} GB/s of the volume's 40 B per point ({gbs / HBM_PEAK_GBS:.2f} of the 8 TB/s peak)",
                 f"{V} one-view integrate calls": f"{res[f'{V} one-view integrate calls'][0] / med:.2f}x the fused call"}
        if tv is not None:
            notes["torch operators, one pass per view"] = f"{res['torch operators, one pass per view'][0] / med:.1f}x the fused call"
            vol.reset()
            fused()
            diff = float((vol.tsdf - tv.tsdf).abs().max())
            wdiff = int((vol.weight != tv.weight).sum())
            notes["torch operators, one pass per view"] += f"; largest tsdf difference {diff:.1e}, {wdiff} weights differ (float32 projection)"
            tv = None
            torch.cuda.empty_cache()
        else:
            vol.reset()
            fused()
        for name, _, _ in steps:
            print(f"| {n}^3 | {name} | {res[name][0]:.3f} ({res[name][1]:.3f}) | {notes[name]} |")
        ms, mesh = [], None
        for _ in range(a.warmup + a.reps):
            t, mesh = timed(vol.extract_mesh)
            ms.append(t)
        res["extract_mesh"] = summary(ms[a.warmup:])
        print(f"| {n}^3 | extract_mesh | {res['extract_mesh'][0]:.3f} ({res['extract_mesh'][1]:.3f}) | {mesh[0].shape[0]} vertices, "
              f"{mesh[1].shape[0]} faces; includes the host read-back of the two counts |")
        results[str(n)] = {k: dict(ms=v[0], iqr=v[1]) for k, v in res.items()}
        results[str(n)]["vertices"], results[str(n)]["faces"] = int(mesh[0].shape[0]), int(mesh[1].shape[0])
        del vol, mesh
        torch.cuda.empty_cache()
    print(json.dumps(dict(reps=a.reps, torch_reps=a.torch_reps, views=V, image=W, grids=results)))


if __name__ == "__main__":
    main()
