#!/usr/bin/env python3
"""One similarity transform of a Gaussian model: the native route (gaussianeditor_amd/transform.py: transform_gaussians,
one launch) against the same operations composed from torch operators on the same GPU -- a matmul for the positions, a
quaternion product from elementwise operators, exp / log for the scales and one einsum per SH band with the same D^l -- on
1 M Gaussians with SH degree 3.  Three cases: the full similarity, a rotation that leaves the SH coefficients alone (the
reference's rotate_gaussians) and a translation.  The two routes alternate in one process; every repetition starts from a
fresh copy of the model (made outside the timed region) and is timed with device events.  Next to each time: the traffic
the algorithm needs (every tensor the case writes, read once and written once) over the time, and that rate as a share of
the 8 TB/s HBM peak.  Prints a small markdown table and one JSON line.  """
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes per second (spec)
ROW_BYTES = dict(_xyz=12, _rotation=16, _scaling=12, _features_rest=180)


def summary(ms):
    """(median, interquartile range) of a list of milliseconds."""
    a = np.sort(np.asarray(ms))
    return float(np.median(a)), float(np.percentile(a, 75) - np.percentile(a, 25))


class Model:
    def __init__(self, tensors):
        for k, v in tensors.items():
            setattr(self, k, v.clone())

    def restore(self, tensors):
        for k, v in tensors.items():
            getattr(self, k).copy_(v)


def quat_mul(a, b):
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    from gaussianeditor_amd import transform as T
    from gaussianeditor_amd.synth import synth_scene

    assert torch.cuda.is_available(), "this benchmark measures the MI355X: there is nothing to time without it"
    dev = torch.device("cuda:0")
    P = a.points
    sc = synth_scene(P, seed=0, s0=0.01, sh_degree=3)
    start = dict(_xyz=sc["xyz"].to(dev), _rotation=sc["rotation"].to(dev), _scaling=torch.log(sc["scaling"]).to(dev),
                 _features_rest=sc["features"][:, 1:].contiguous().to(dev))
    ang = math.radians(70.0)
    axis = np.array([0.3, -1.0, 0.5]) / np.linalg.norm([0.3, -1.0, 0.5])
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    R = np.eye(3) + math.sin(ang) * K + (1.0 - math.cos(ang)) * (K @ K)
    t, s = [0.4, -0.3, 0.6], 1.3
    q, Rh = T.rotation_hat(R)
    Rd = torch.tensor(Rh, dtype=torch.float32, device=dev)
    qd = torch.tensor(q, dtype=torch.float32, device=dev)
    td = torch.tensor(t, dtype=torch.float32, device=dev)
    D = [torch.tensor(d, dtype=torch.float32, device=dev) for d in T.sh_rotation(R)]
    bands = ((0, 3), (3, 8), (8, 15))

    def torch_route(m, rotate, sh, scale, translate):
        """The reference's way: new tensors assigned to .data, one torch operator after the other."""
        x = m._xyz.data
        if rotate:
            x = torch.einsum("ij,bj->bi", Rd, x)
            m._rotation.data = quat_mul(qd.expand_as(m._rotation.data), m._rotation.data)
        if scale:
            x = x * s
            m._scaling.data = torch.log(torch.exp(m._scaling.data) * s)
        if translate:
            x = x + td[None, :]
        m._xyz.data = x
        if sh:
            f = m._features_rest.data
            m._features_rest.data = torch.cat([torch.einsum("mk,pkc->pmc", Dl, f[:, lo:hi]) for Dl, (lo, hi) in zip(D, bands)], 1)

    cases = {
        "full similarity": (dict(rotation=R, translation=t, scale=s), dict(rotate=True, sh=True, scale=True, translate=True),
                            ("_xyz", "_rotation", "_scaling", "_features_rest")),
        "rotation, SH left alone": (dict(rotation=R, rotate_sh=False), dict(rotate=True, sh=False, scale=False, translate=False),
                                    ("_xyz", "_rotation")),
        "translation": (dict(translation=t), dict(rotate=False, sh=False, scale=False, translate=True), ("_xyz",)),
    }
    native_model, torch_model = Model(start), Model(start)

    def timed(fn, model):
        model.restore(start)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    results = {}
    print(f"| case ({P} Gaussians, SH3) | native ms (IQR) | torch ms (IQR) | speed-up | bytes needed | native GB/s | of 8 TB/s |")
    print("|---|---|---|---|---|---|---|")
    for name, (kw, tk, written) in cases.items():
        ms = {"native": [], "torch": []}
        for i in range(a.warmup + a.reps):
            tn = timed(lambda: T.transform_gaussians(native_model, **kw), native_model)
            tt = timed(lambda: torch_route(torch_model, **tk), torch_model)
            if i >= a.warmup:
                ms["native"].append(tn)
                ms["torch"].append(tt)
        (n_med, n_iqr), (t_med, t_iqr) = summary(ms["native"]), summary(ms["torch"])
        need = 2 * P * sum(ROW_BYTES[k] for k in written)
        rate = need / (n_med * 1e-3)
        # the two routes agree (float32 torch against binary64 rounded once): a few float32 ulp of the tensor's scale
        worst = max(float((getattr(native_model, k) - getattr(torch_model, k)).abs().max()) for k in written)
        results[name] = dict(native_ms=n_med, native_iqr=n_iqr, torch_ms=t_med, torch_iqr=t_iqr, bytes=need,
                             native_gbps=rate / 1e9, hbm_fraction=rate / HBM_PEAK, max_abs_diff=worst)
        print(f"| {name} | {n_med:.3f} ({n_iqr:.3f}) | {t_med:.3f} ({t_iqr:.3f}) | {t_med / n_med:.1f}x | {need / 1e6:.0f} MB | "
              f"{rate / 1e9:.0f} | {100 * rate / HBM_PEAK:.0f} % |")
    print(json.dumps(dict(points=P, reps=a.reps, cases=results)))


if __name__ == "__main__":
    main()
