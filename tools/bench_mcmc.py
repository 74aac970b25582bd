#!/usr/bin/env python3
"""The 3DGS-MCMC strategy: the native route (gaussianeditor_amd/mcmc.py: inject_noise, mcmc_refine) against the same steps
from torch ops (tests/mcmc_helpers.py: noise_torch, mcmc_refine_torch) on a 1 M Gaussian synth scene whose opacities are the
scene's own, about 2 % of them forced dead.  The two routes alternate in one process; every repetition starts from a fresh
copy of the state (made outside the timed region) and is timed with the host clock around a device synchronise.  Prints a
small markdown table and one JSON line.  """
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def summary(ms):
    """(median, interquartile range) of a list of milliseconds."""
    a = np.sort(np.asarray(ms))
    return float(np.median(a)), float(np.percentile(a, 75) - np.percentile(a, 25))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dead", type=float, default=0.02)
    a = ap.parse_args()
    import mcmc_helpers as mh

    from gaussianeditor_amd import mcmc
    from gaussianeditor_amd.synth import synth_scene

    dev = torch.device("cuda:0")
    P = a.points
    sc = synth_scene(P, seed=0, s0=0.01, sh_degree=3)
    g = torch.Generator(device=dev).manual_seed(1)
    opacity = sc["opacity"].clamp(1e-4, 1 - 1e-4).to(dev).reshape(-1, 1)
    opacity[torch.rand(P, device=dev, generator=g) < a.dead] = 0.002
    f = sc["features"].to(dev)
    par = dict(xyz=sc["xyz"].to(dev), f_dc=f[:, :1].contiguous(), f_rest=f[:, 1:].contiguous(), opacity=torch.logit(opacity),
               scaling=torch.log(sc["scaling"]).to(dev), rotation=sc["rotation"].to(dev))
    moments = {k: (torch.randn_like(v) * 1e-3, torch.rand_like(v) * 1e-6) for k, v in par.items()}
    mask = torch.rand(P, device=dev, generator=g) < 0.5
    extra = dict(xyz_gradient_accum=torch.zeros((P, 1), device=dev), denom=torch.zeros((P, 1), device=dev),
                 max_radii2D=torch.zeros(P, device=dev), mask=mask, generation=torch.zeros(P, dtype=torch.int64, device=dev))

    def timed(fn, setup=None):
        if setup is not None:
            setup()
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def alternate(routes, reps, warmup):
        ms = {k: [] for k in routes}
        for i in range(warmup + reps):
            for k, (fn, setup) in routes.items():
                t = timed(fn, setup)
                if i >= warmup:
                    ms[k].append(t)
        return {k: summary(v) for k, v in ms.items()}

    # --- (a) the per-step noise (the random numbers are drawn outside: both routes take the same torch.randn)
    noise = torch.randn(P, 3, device=dev, generator=g)
    x_t, x_n = par["xyz"].clone(), par["xyz"].clone()
    scaler = 5e5 * 1.6e-4
    res_noise = alternate({
        "torch": (lambda: mh.noise_torch(x_t, par["scaling"], par["rotation"], par["opacity"], noise, scaler, mask), None),
        "native": (lambda: mcmc.inject_noise(x_n, par["scaling"], par["rotation"], par["opacity"], noise, scaler=scaler, mask=mask), None),
    }, a.reps, a.warmup)
    noise_diff = float((x_t - x_n).abs().max())

    # --- (b) one refine from the same state: relocation of the dead rows, then growth by 5 %
    kw = dict(cap_max=2 * P, min_opacity=0.005, grow=1.05, generation_num=1)
    state, counts = {}, {}
    opt = torch.optim.Adam([dict(params=[torch.nn.Parameter(par[k].clone())], lr=1e-4, name=k) for k in NAMES], lr=0.0, eps=1e-15)

    def fresh_torch():
        state["par"] = {k: v.clone() for k, v in par.items()}
        state["mom"] = {k: (m1.clone(), m2.clone()) for k, (m1, m2) in moments.items()}

    def torch_route():
        r = mh.mcmc_refine_torch(state["par"], state["mom"], extra, generator=torch.Generator(device=dev).manual_seed(7), copy=False, **kw)
        counts["torch"] = r[3]

    def fresh_native():
        opt.state.clear()
        for group, k in zip(opt.param_groups, NAMES):
            p = torch.nn.Parameter(par[k].clone())
            group["params"][0] = p
            opt.state[p] = dict(step=torch.tensor(2.0), exp_avg=moments[k][0].clone(), exp_avg_sq=moments[k][1].clone())

    def native_route():
        r = mcmc.mcmc_refine(opt, extra, generator=torch.Generator(device=dev).manual_seed(7), **kw)
        counts["native"] = r[2]

    res_refine = alternate({"torch": (torch_route, fresh_torch), "native": (native_route, fresh_native)}, a.reps, a.warmup)

    def verdict(r):
        gain = r["torch"][0] - r["native"][0]
        return gain > r["torch"][1] + r["native"][1], gain

    gbs = 68.0 * P / (res_noise["native"][0] * 1e-3) / 1e9
    print(f"| {P} Gaussians, {a.reps} alternating repetitions | torch route, median (IQR) | native route, median (IQR) | native "
          f"wins by more than the spread |")
    print("|---|---|---|---|")
    for name, r in (("per-step noise", res_noise), ("mcmc_refine", res_refine)):
        print(f"| {name} | {r['torch'][0]:.3f} ms ({r['torch'][1]:.3f}) | {r['native'][0]:.3f} ms ({r['native'][1]:.3f}) | "
              f"{verdict(r)[0]} ({verdict(r)[1]:+.3f} ms) |")
    print(f"noise kernel: {68.0 * P / 1e6:.0f} MB in {res_noise['native'][0]:.3f} ms = {gbs:.0f} GB/s (host clock, launch included); "
          f"max |xyz torch - xyz native| after all repetitions {noise_diff:.3e}")
    print(f"mcmc_refine (P, n_dead, n_relocated, n_added): torch {counts['torch']}, native {counts['native']}")
    print(json.dumps(dict(points=P, reps=a.reps, noise_ms=res_noise, refine_ms=res_refine, counts=counts, noise_gbs=gbs,
                          noise_max_diff=noise_diff)))


if __name__ == "__main__":
    main()
