#!/usr/bin/env python3
"""Where K7's longest items run and what their compute unit does meanwhile (gsr_debug_blend_backward_profile): for the ten
longest items of the headline view their rank in the work list (by the forward's estimate), queue, unit and slot, how many
items the workgroups of the same unit ran and when those ended relative to the long item's end, and when the long item's
queue ran empty (profiles/k7_heavy_units_ab.md).
Run on the GPU box: python tools/k7_heavy_profile.py [--s0 0.01] [--gaussians 1000000] [--out k7_heavy.json]"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianeditor_amd import _native  # noqa: E402
from gaussianeditor_amd.diff_gaussian_rasterization import _C  # noqa: E402
from gaussianeditor_amd.synth import ring_cameras, seed_gradient, synth_scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gaussians", type=int, default=1_000_000)
ap.add_argument("--s0", type=float, default=0.01)
ap.add_argument("--out", default=None)
a = ap.parse_args()
P, W, H = a.gaussians, 1920, 1080
T = ((W + 15) // 16) * ((H + 15) // 16)
dev = torch.device("cuda:0")
sc = synth_scene(P, seed=0, s0=a.s0)
cam = ring_cameras(8, W, H)[0]
tfx, tfy = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
d = lambda t: t.to(dev)  # noqa: E731
e = torch.empty(0, device=dev)
bg = d(sc["bg"])
R, color, depth, radii, geom, binning, img = _C.rasterize_gaussians(
    bg, d(sc["xyz"]), e, d(sc["opacity"]), d(sc["scaling"]), d(sc["rotation"]), 1.0, e, d(cam.world_view_transform),
    d(cam.full_proj_transform), tfx, tfy, H, W, d(sc["features"]), 3, d(cam.camera_center), False, False)
L = _native.lib()
s = torch.cuda.current_stream(dev).cuda_stream
G = seed_gradient(H, W, 0).to(dev)
z = torch.zeros(P * _native.ACC_ROW, device=dev)
n = ctypes.c_int64(0)
L.gsr_debug_blend_backward_profile(s, P, R, W, H, bg.data_ptr(), geom.data_ptr(), binning.data_ptr(), img.data_ptr(),
                                   G.data_ptr(), z.data_ptr(), 1, 0, ctypes.byref(n))
n = int(n.value)
rec = torch.zeros((n + T, 8), dtype=torch.int64, device=dev)
for _ in range(3):
    z.zero_()
    _native.check("profile", L.gsr_debug_blend_backward_profile(s, P, R, W, H, bg.data_ptr(), geom.data_ptr(), binning.data_ptr(),
                                                                img.data_ptr(), G.data_ptr(), z.data_ptr(), rec.data_ptr(), n + T,
                                                                ctypes.byref(ctypes.c_int64(0))))
torch.cuda.synchronize()
r = rec.cpu().numpy().view(np.uint64)
wg = r[:n].astype(np.int64)
t0, t1, ntiles, longest, first = wg[:, 0], wg[:, 1], wg[:, 3] >> 32, wg[:, 4], wg[:, 5]
dur = t1 - t0
span = int(dur.max())
units = n // 4  # (4 residency slots of 4-wave workgroups per compute unit: first_item_of_block)
b = np.arange(n)
unit, slot, queue = b % units, b // units, (wg[:, 2] >> 32) & 7  # (the queue a workgroup pops from: its XCD's)
items = r[n:].reshape(-1, 4)
cyc = items[:, 0].astype(np.int64)
used = cyc > 0
q = [((items[:, 1] >> np.uint64(16 * k)) & np.uint64(0xffff)).astype(np.int64) for k in range(4)]
code = items[:, 3].astype(np.int64)
half, part = (code & 0x80000000) != 0, (code & 0x40000000) != 0
est = np.where(half, np.where(part, q[2] + q[3], q[0] + q[1]), q[0] + q[1] + q[2] + q[3])
est = np.where(used, est, -1)
rank = np.empty(len(est), dtype=np.int64)
rank[np.argsort(-est, kind="stable")] = np.arange(len(est))  # (the list is ordered by buckets of 16: a rank is exact to a bucket)
fair = est[used].sum() / n
corr = float(np.corrcoef(est[used], cyc[used])[0, 1])
out = dict(P=P, s0=a.s0, workgroups=n, items=int(used.sum()), span=span, mean_workgroup_frac=float(dur.mean() / span),
           critical_item_frac=float(cyc.max() / span), fair_share=float(fair), corr_est_cycles=corr,
           top=[])
print(f"P={P} s0={a.s0}: {n} workgroups, {int(used.sum())} items, span {span} ticks, mean workgroup {dur.mean() / span:.3f}, longest item "
      f"{cyc.max() / span:.3f} of it; fair share {fair:.0f} entries; corr(estimate, ticks) {corr:.2f}")
print(f"estimates in fair shares: max {est.max() / fair:.2f}; items >= 1.0: {int((est >= fair).sum())}, >= 0.875: {int((est >= 0.875 * fair).sum())}, "
      f">= 0.75: {int((est >= 0.75 * fair).sum())}, >= 0.625: {int((est >= 0.625 * fair).sum())}, >= 0.5: {int((est >= 0.5 * fair).sum())}")
# when a queue ran empty: the first failed pop of a workgroup that serves it, i.e. the shortest such workgroup (the clocks of
# two compute units do not compare: a workgroup's own end - start does, all start within the first microsecond)
q_empty = np.array([dur[(queue == x) & (t1 > 0)].min() if ((queue == x) & (t1 > 0)).any() else 0 for x in range(8)])
print("rank = position by estimate; times in units of the span, relative to the long item's end (negative: before it)")
for i in np.argsort(-cyc)[:10]:
    owner = np.nonzero(longest == cyc[i])[0]
    row = dict(ticks_frac=float(cyc[i] / span), est_fair=float(est[i] / fair), rank=int(rank[i]), half=bool(half[i]))
    if len(owner) != 1:
        print(f"  item {cyc[i] / span:.3f} est {est[i] / fair:.2f} rank {rank[i]}: owner not unique")
        out["top"].append(row)
        continue
    o = int(owner[0])
    is_first = bool(first[o] == cyc[i])
    end = t0[o] + first[o] if is_first else t1[o]  # (a popped item: taken as its workgroup's last)
    mates = [m for m in np.nonzero(unit == unit[o])[0] if m != o]
    rel = lambda t: float((t - end) / span)  # noqa: E731
    row.update(queue=int(queue[o]), unit=int(unit[o]), slot=int(slot[o]), first_item=is_first, owner_items=int(ntiles[o]),
               end_frac=float((end - t0[o]) / span), queue_empty=float((q_empty[queue[o]] - (end - t0[o])) / span),
               mates=[dict(slot=int(slot[m]), items=int(ntiles[m]), end=rel(t1[m])) for m in mates])
    out["top"].append(row)
    print(f"  item {row['ticks_frac']:.3f} est {row['est_fair']:.2f} fair rank {row['rank']:4d} {'half' if half[i] else 'tile'} | queue {row['queue']} unit "
          f"{row['unit']:3d} slot {row['slot']} {'first' if is_first else 'popped'} owner ran {row['owner_items']} ends at {row['end_frac']:.3f} | queue "
          f"empty {row['queue_empty']:+.3f} | mates: "
          + "; ".join(f"s{m['slot']} n={m['items']} end {m['end']:+.3f}" for m in row["mates"]))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"))
