#!/usr/bin/env python3
"""CPU only: the figures behind the bars of tests/pose_helpers.py (the camera gradient), none of them from the kernel.
    python tools/pose_bars.py [--camera NAME] [case ...]
--camera NAME: under the general camera NAME of tests/camera_cases.py (unequal focal lengths, roll, off-centre axis), on the
rows of camera_cases.POSE_PAIRS for it with their seeds, and the identity on identity_case(camera=NAME).
Per case of pose_helpers.POSE_CASES, with the float32 oracle (oracle/cpu.py) and float64 autograd (oracle/torch_ref.py):
  * flipped pixels between the float32 oracle's forward and float64, Gaussians on the cone edge (the conditions);
  * dL/dcampos: the oracle-difference reference (dL_dmeans3D with SHs minus the same with colors_precomp = the forward's
    rgb, summed in float64) against float64, relative to the largest float64 entry -> CAMPOS_ORACLE_WORST;
  * dL/dprojmatrix: its per-Gaussian terms formed in float32 from the oracle's dL_dmeans2D, summed in float64, against
    float64, relative to the largest entry.
Then the translation identity on pose_helpers.identity_case(): float64 against itself (the CPU self-check's 1e-12) and the
float32 oracle's - sum dL/dmu against float64's c.grad, relative to sum |dL/dmu| -> IDENTITY_ORACLE_RATIO."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def proj_terms_f32(r, f, g):
    """dL/dprojmatrix from the float32 oracle's dL_dmeans2D: float32 terms, float64 sum."""
    case = r["case"]
    mu = case["sc"]["xyz"].numpy().astype(np.float32)
    PV = case["cam"].full_proj_transform.numpy().astype(np.float32)
    ph = np.concatenate([mu, np.ones((mu.shape[0], 1), np.float32)], 1)
    hom = ph @ PV
    m_w = (np.float32(1) / (hom[:, 3] + np.float32(1e-7))).astype(np.float32)
    g2 = np.asarray(g["dL_dmeans2D"], np.float32)
    vis = f["radii"] > 0
    cols = np.zeros((mu.shape[0], 4), np.float32)
    cols[:, 0], cols[:, 1] = g2[:, 0] * m_w, g2[:, 1] * m_w
    cols[:, 3] = -(hom[:, 0] * m_w * m_w * g2[:, 0] + hom[:, 1] * m_w * m_w * g2[:, 1])
    terms = (ph[:, :, None] * cols[:, None, :]).astype(np.float32)[vis]
    return terms.astype(np.float64).sum(axis=0)


def main():
    import f64_regimes as R
    import pose_helpers as PH
    from helpers import flipped_pixels, oracle_backward, oracle_forward
    from oracle import cpu
    from oracle.torch_ref import render_f64

    ap = argparse.ArgumentParser()
    ap.add_argument("--camera", default=None, help="a name of tests/camera_cases.py CAMERAS")
    ap.add_argument("cases", nargs="*")
    args = ap.parse_args()
    cpu.build()
    camera = args.camera
    if camera is None:
        rows = [(name, None) for name in (args.cases or PH.POSE_CASES)]
    else:
        import camera_cases as CC

        rows = [(name, seed) for cam, name, seed in CC.POSE_PAIRS if cam == camera and (not args.cases or name in args.cases)]
        print(f"camera {camera}: (roll deg, fx / fy, cx, cy) = {CC.CAMERAS[camera]}")
    worst = 0.0
    print(f"{'case':18s} {'seed':>5s} {'flips':>5s} {'edge':>4s} {'campos ref':>11s} {'proj ref':>9s} {'|sum dm| / sum |dm|':>20s}")
    for name, seed in rows:
        r = PH.pose_regime(name, camera=camera, seed=seed)
        f, g = R.oracle_run(cpu, r)
        want_cam, _, stats = PH.f64_pose(f, r)
        flips = flipped_pixels(stats["n_contrib"].numpy(), stats["final_T"].numpy(), f["n_contrib"], f["final_T"]).size
        edge = int((R.cone_edge_rows(r) & (f["radii"] > 0)).sum())
        proj = proj_terms_f32(r, f, g)
        e_proj = np.abs(proj - want_cam["proj"]).max() / np.abs(want_cam["proj"]).max()
        e_cam, cancel = float("nan"), float("nan")
        if r["colors_precomp"] is None:
            kw = dict(cov3D_precomp=r["cov3D_precomp"], D=r["D"], scale_modifier=r["sm"])
            g_sh = oracle_backward(cpu, r["case"], f, r["G"], **kw)
            rgb = torch.from_numpy(np.ascontiguousarray(f["rgb"]))
            f2 = oracle_forward(cpu, r["case"], colors_precomp=rgb, **kw)
            g_pc = oracle_backward(cpu, r["case"], f2, r["G"], colors_precomp=rgb, **kw)
            dm = (np.asarray(g_sh["dL_dmeans3D"], np.float32) - np.asarray(g_pc["dL_dmeans3D"], np.float32)).astype(np.float64)
            ref = -dm.sum(axis=0)
            e_cam = float(np.abs(ref - want_cam["campos"]).max() / np.abs(want_cam["campos"]).max())
            cancel = float((np.abs(dm.sum(axis=0)) / np.abs(dm).sum(axis=0)).min())
            worst = max(worst, e_cam)
        print(f"{name:18s} {'own' if seed is None else seed:>5} {flips:5d} {edge:4d} {e_cam:11.2e} {e_proj:9.2e} {cancel:20.3f}", flush=True)
    print(f"CAMPOS_ORACLE_WORST = {worst:.2e}")

    # the translation identity
    case = PH.identity_case(camera=camera)
    H, W = case["H"], case["W"]
    G = PH.seed_gradient(H, W, 19) * H * W
    f = oracle_forward(cpu, case)
    g = oracle_backward(cpu, case, f, G)
    sc = case["sc"]
    d = torch.float64
    leaf = lambda t: t.to(d).clone().requires_grad_(True)  # noqa: E731
    xyz = leaf(sc["xyz"])
    c, V, PV, C = PH.moved_camera(case["cam"], d)
    render_f64(f, xyz, None, sc["opacity"].to(d), sc["scaling"].to(d), sc["rotation"].to(d), sc["features"].to(d), None, None,
               V, PV, C, case["bg"], W, H, case["tfx"], case["tfy"], 1.0, 3, dL_dimage=G.to(d))
    g64 = xyz.grad.numpy()
    self_ratio = np.abs(c.grad.numpy() + g64.sum(axis=0)) / np.abs(g64).sum(axis=0)
    g32 = np.asarray(g["dL_dmeans3D"], np.float64)
    ratio = np.abs(c.grad.numpy() + g32.sum(axis=0)) / np.abs(g32).sum(axis=0)
    print(f"translation identity on identity_case(): float64 self-check {self_ratio.max():.2e}; "
          f"float32 oracle against float64 {ratio.max():.2e}  -> IDENTITY_ORACLE_RATIO")


if __name__ == "__main__":
    main()
