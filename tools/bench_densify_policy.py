#!/usr/bin/env python3
"""Densification policy: the native route (gaussianeditor_amd/densify.py: add_densification_stats, densify_and_prune) against
the reference's torch lines (tests/densify_helpers.py: stats_torch, densify_and_prune_torch) on a 1 M Gaussian synth scene,
with gradients and radii from real renders of two 512 x 512 views.  The two routes alternate in one process; every repetition
is timed with the host clock around a device synchronise.  Prints a small markdown table and one JSON line.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def summary(ms):
    """(median, interquartile range) of a list of milliseconds: the spread is what a single run's figure may be off by."""
    a = np.sort(np.asarray(ms))
    return float(np.median(a)), float(np.percentile(a, 75) - np.percentile(a, 25))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max-densify-percent", type=float, default=0.01)
    a = ap.parse_args()
    import densify_helpers as dh

    from gaussianeditor_amd import densify
    from gaussianeditor_amd.gaussian_renderer import render
    from gaussianeditor_amd.synth import ring_cameras, seed_gradient, synth_scene

    dev = torch.device("cuda:0")
    sc = synth_scene(a.points, seed=0, s0=0.01, sh_degree=3)
    f = sc["features"].to(dev)
    par = dict(xyz=sc["xyz"].to(dev), f_dc=f[:, :1].contiguous(), f_rest=f[:, 1:].contiguous(),
               opacity=torch.logit(sc["opacity"].clamp(1e-4, 1 - 1e-4)).to(dev).reshape(-1, 1), scaling=torch.log(sc["scaling"]).to(dev),
               rotation=sc["rotation"].to(dev))
    P = a.points

    class Model:  # what render() reads of a GaussianModel
        active_sh_degree = max_sh_degree = 3
        p = {k: v.clone().requires_grad_(True) for k, v in par.items()}
        get_xyz = property(lambda s: s.p["xyz"])
        get_opacity = property(lambda s: torch.sigmoid(s.p["opacity"]))
        get_scaling = property(lambda s: torch.exp(s.p["scaling"]))
        get_rotation = property(lambda s: torch.nn.functional.normalize(s.p["rotation"]))
        get_features = property(lambda s: torch.cat((s.p["f_dc"], s.p["f_rest"]), dim=1))

    pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    bg = torch.zeros(3, device=dev)
    G = seed_gradient(a.size, a.size).to(dev)
    grads, radii = [], []
    for cam in ring_cameras(8, a.size, a.size)[:2]:
        out = render(cam.to(dev), Model(), pipe, bg)
        (out["render"] * G).sum().backward()
        grads.append(out["viewspace_points"].grad.detach().clone())
        radii.append(out["radii"].detach().clone())
    del out
    visible = int((torch.max(radii[0], radii[1]) > 0).sum())

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def alternate(routes, reps, warmup):
        ms = {k: [] for k in routes}
        for i in range(warmup + reps):
            for k, fn in routes.items():
                t = timed(fn)
                if i >= warmup:
                    ms[k].append(t)
        return {k: summary(v) for k, v in ms.items()}

    # --- (a) the per-step statistics
    st_t = [torch.zeros((P, 1), device=dev), torch.zeros((P, 1), device=dev), torch.zeros(P, device=dev)]
    st_n = [t.clone() for t in st_t]
    res_stats = alternate({"torch": lambda: dh.stats_torch(*st_t, grads, radii),
                           "native": lambda: densify.add_densification_stats(*st_n, grads, radii)}, a.reps, a.warmup)
    same_stats = all(torch.equal(x, y) for x, y in zip(st_t[1:], st_n[1:]))

    # --- (b) one full densify_and_prune from the same state: five steps of statistics, Adam moments, half the scene masked
    extra = dict(xyz_gradient_accum=torch.zeros((P, 1), device=dev), denom=torch.zeros((P, 1), device=dev),
                 max_radii2D=torch.zeros(P, device=dev), mask=torch.rand(P, device=dev) < 0.5,
                 generation=torch.zeros(P, dtype=torch.int64, device=dev))
    for _ in range(5):
        densify.add_densification_stats(extra["xyz_gradient_accum"], extra["denom"], extra["max_radii2D"], grads, radii)
    g = extra["xyz_gradient_accum"] / extra["denom"]
    g = g[(g > 0) & extra["mask"][:, None]]
    smax = torch.exp(par["scaling"]).max(dim=1).values
    kw = dict(max_grad=float(g.median()), max_densify_percent=a.max_densify_percent, min_opacity=0.005, extent=1.0,
              max_screen_size=20, percent_dense=float(smax.median()), N=2, generation_num=1)
    moments = {k: (torch.randn_like(v) * 1e-3, torch.rand_like(v) * 1e-6) for k, v in par.items()}
    params0 = {k: torch.nn.Parameter(v.clone()) for k, v in par.items()}
    opt = torch.optim.Adam([dict(params=[params0[k]], lr=1e-4, name=k) for k in NAMES], lr=0.0, eps=1e-15)
    counts = {}

    def torch_route():
        gen = torch.Generator(device=dev).manual_seed(7)
        r = dh.densify_and_prune_torch(par, moments, extra, lambda n: torch.randn((n, 3), device=dev, generator=gen),
                                       with_bound=False, **kw)
        counts["torch"] = r[3]

    def native_route():
        for group, k in zip(opt.param_groups, NAMES):  # the same start every time (nothing is updated in place)
            group["params"][0] = params0[k]
        opt.state.clear()
        for k in NAMES:
            opt.state[params0[k]] = dict(step=torch.tensor(2.0), exp_avg=moments[k][0], exp_avg_sq=moments[k][1])
        r = densify.densify_and_prune(opt, extra, generator=torch.Generator(device=dev).manual_seed(7), **kw)
        counts["native"] = r[2]

    res_dp = alternate({"torch": torch_route, "native": native_route}, a.reps, a.warmup)

    def verdict(r):
        gain = r["torch"][0] - r["native"][0]
        return gain > r["torch"][1] + r["native"][1], gain

    print(f"| {P} Gaussians, {visible} visible in 2 views at {a.size}^2, {a.reps} alternating repetitions | torch route, median "
          f"(IQR) | native route, median (IQR) | native wins by more than the spread |")
    print("|---|---|---|---|")
    for name, r in (("per-step statistics", res_stats), ("densify_and_prune", res_dp)):
        print(f"| {name} | {r['torch'][0]:.3f} ms ({r['torch'][1]:.3f}) | {r['native'][0]:.3f} ms ({r['native'][1]:.3f}) | "
              f"{verdict(r)[0]} ({verdict(r)[1]:+.3f} ms) |")
    print(f"densify_and_prune (before, n_clone, n_split, n_pruned): torch {counts['torch']}, native {counts['native']}; "
          f"statistics equal: {same_stats}")
    print(json.dumps(dict(points=P, visible=visible, reps=a.reps, stats_ms=res_stats, densify_and_prune_ms=res_dp,
                          counts=counts, stats_equal=same_stats, params=kw)))


if __name__ == "__main__":
    main()
