"""The float64 expectation of antialiased renders (gaussianeditor_amd.set_antialiasing; include/gsr.h GSR_FLAG_ANTIALIAS).

An antialiased render is the ordinary render with every opacity o replaced by o * h, h = sqrt(max(2.5e-5, r)),
r = det(S) / det(S + w I), w = 0.3, S the 2D covariance BEFORE the dilation.  oracle/torch_ref.render_f64 takes any
differentiable `opacities`, so the expectation is render_f64(opacities = o * h) with h computed here, in float64, by a
restatement of render_f64's projection (the same equations; the clamped tx / ty of off-cone Gaussians detached, as there):
autograd then carries the h-term to means3D, scales, rotations and cov3D_precomp.  The instance lists render_f64 walks
come from the float32 oracle in reference tile bounds, which do not depend on the opacity.  The float32 oracle at the
product's effective opacities (rec0.w) supplies n_contrib / final_T for the flipped-pixel masks.
"""
import functools

import numpy as np
import torch

import f64_regimes as R
from helpers import flipped_pixels, gaussians_under, make_case, seed_gradient

W_AA = 0.3
FLOOR = 2.5e-5
NEAR_FLOOR_REL = 1e-4   # rows with |r - FLOOR| < NEAR_FLOOR_REL * FLOOR: float32 and float64 may disagree on the floor
ILL_COND = 1e-3         # rows with det(S) < ILL_COND * x * y: x * y - z^2 cancels in float32 (see cov2d_f64)


def cov2d_f64(means3D, scales, rotations, cov3D_precomp, viewmatrix, W, H, tanfovx, tanfovy, scale_modifier=1.0):
    """-> (x, y, z): the undilated 2D covariance S00, S11, S01 of every Gaussian, float64, differentiable (render_f64's
    equations: covariance from scale / rotation or the precomputed one, J of the clamped tx / ty, T = J W)."""
    dt = torch.float64
    V = viewmatrix.to(dt).reshape(4, 4)
    P = means3D.shape[0]
    p_view = torch.cat([means3D, torch.ones(P, 1, dtype=dt)], dim=1) @ V
    if cov3D_precomp is None:
        s = scale_modifier * scales
        r, x, y, z = rotations[:, 0], rotations[:, 1], rotations[:, 2], rotations[:, 3]
        Rm = torch.stack([
            1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(P, 3, 3)
        Mm = Rm * s[:, None, :]
        Sigma = Mm @ Mm.transpose(1, 2)
    else:
        c = cov3D_precomp
        Sigma = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]],
                            dim=1).reshape(P, 3, 3)
    fx, fy = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    tz = p_view[:, 2]
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    txtz, tytz = p_view[:, 0] / tz, p_view[:, 1] / tz
    offx, offy = (txtz.abs() > limx).detach(), (tytz.abs() > limy).detach()
    tx = torch.where(offx, (torch.clamp(txtz, -limx, limx) * tz).detach(), p_view[:, 0])
    ty = torch.where(offy, (torch.clamp(tytz, -limy, limy) * tz).detach(), p_view[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz), zero, fy / tz, -(fy * ty) / (tz * tz)], dim=1).reshape(P, 2, 3)
    T = J @ V[:3, :3].transpose(0, 1)
    cov2 = T @ Sigma @ T.transpose(1, 2)
    return cov2[:, 0, 0], cov2[:, 1, 1], cov2[:, 0, 1]


def ratio_f64(x, y, z):
    """r = det(S) / det(S + w I)."""
    return (x * y - z * z) / ((x + W_AA) * (y + W_AA) - z * z)


def h_f64(x, y, z):
    """h = sqrt(max(FLOOR, r)) (where the floor is active h is a constant: clamp_min passes no gradient)."""
    return torch.sqrt(torch.clamp_min(ratio_f64(x, y, z), FLOOR))


def h_of_case(case, sc=None, cov3D_precomp=None, scale_modifier=1.0):
    """float64 (h, r, x, y, z) of every Gaussian of a tests/helpers.make_case case, as numpy (no gradient)."""
    sc = case["sc"] if sc is None else sc
    d = torch.float64
    cov = None if cov3D_precomp is None else torch.as_tensor(cov3D_precomp).to(d)
    x, y, z = cov2d_f64(sc["xyz"].to(d), None if cov is not None else sc["scaling"].to(d),
                        None if cov is not None else sc["rotation"].to(d), cov, case["cam"].world_view_transform,
                        case["W"], case["H"], case["tfx"], case["tfy"], scale_modifier)
    r = ratio_f64(x, y, z)
    return (h_f64(x, y, z).numpy(), r.numpy(), x.numpy(), y.numpy(), z.numpy())


# ---- sparse sub-pixel scene: the intent of the filter ------------------------------------------------------------------
def sparse_case(W, H, n_side=12, sigma_world=0.004, opacity=0.6, seed=5):
    """A grid of n_side^2 isolated, round, sub-pixel Gaussians (3D scale sigma_world) facing a camera at distance 4, spaced
    so that no two of them overlap at any of the resolutions used, on a black background with colours 1."""
    from gaussianeditor_amd.synth import look_at_camera

    g = torch.Generator().manual_seed(seed)
    u = (torch.arange(n_side, dtype=torch.float32) - (n_side - 1) / 2) * (1.6 / n_side)
    gy, gx = torch.meshgrid(u, u, indexing="ij")
    P = n_side * n_side
    jitter = (torch.rand(P, 2, generator=g) - 0.5) * 0.02
    xyz = torch.stack([gx.reshape(-1) + jitter[:, 0], gy.reshape(-1) + jitter[:, 1], torch.zeros(P)], 1).contiguous()
    sc = dict(xyz=xyz, scaling=torch.full((P, 3), sigma_world), rotation=torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1),
              opacity=torch.full((P, 1), opacity), features=torch.zeros(P, 16, 3))
    cam = look_at_camera([0.0, 0.0, -4.0], [0.0, 0.0, 0.0], W, H, fovy_deg=30.0)
    case = make_case(16, W, H, seed=1, nviews=1, bg=(0.0, 0.0, 0.0))
    case.update(sc=sc, cam=cam, tfx=float(np.tan(cam.FoVx / 2)), tfy=float(np.tan(cam.FoVy / 2)), D=0)
    return case


def coverage(final_T, W, H):
    """sum over pixels of (1 - T_final) times the pixel's area in units of the full-resolution image (area 1 / (W H) of the
    image each): the screen-space mass the Gaussians occupy, comparable across resolutions."""
    return float(np.sum(1.0 - np.asarray(final_T, dtype=np.float64))) / (W * H)


# ---- new regimes (the f64 regime matrix under the flag) ----------------------------------------------------------------
NEW_CASES = ["sub_pixel", "floor", "edit_view"]


def regime(name, camera=None):
    """The cases of f64_regimes.regime() and three that only the flag has: sub_pixel (many visible rows with
    0.05 < h < 0.9), floor (needles whose r lies below the floor) and edit_view (a 512 x 512 view with long lists).
    `camera`: as in f64_regimes.regime."""
    mk = functools.partial(make_case, camera=camera)
    if name == "saturated":
        # under the flag an opacity of 0.998 becomes o h < 0.99 on most footprints: larger Gaussians (h ~ 0.997) and
        # opacities in [0.9995, 0.99999] keep o h G > 0.99 near their centres (~130 saturated pairs, ~10 000 stopped pixels)
        r = R.regime(name, camera=camera)
        sc = dict(r["case"]["sc"], scaling=(r["case"]["sc"]["scaling"] * 2.5).contiguous())
        u = torch.rand(sc["xyz"].shape[0], 1, generator=torch.Generator().manual_seed(62))
        sc["opacity"] = (0.9995 + 0.00049 * u).contiguous()
        r["case"]["sc"] = sc
        return r
    if name in R.CASES:
        return R.regime(name, camera=camera)
    D, sm = 3, 1.0
    if name == "sub_pixel":
        # small Gaussians far from a low-resolution camera: most footprints are below a pixel
        case = mk(3000, 120, 88, seed=91, s0=0.006, view=1, scale_xyz=0.8, bg=(0.2, 0.5, 0.7))
    elif name == "floor":
        # half of the Gaussians are needles (scales 0.01 x 1e-6 x 1e-6): their footprints are lines a few pixels long whose
        # det(S) / det(S + w I) lies far below the floor -- and short enough that float32's x y - z^2 stays far below it too
        # (its rounding is ~1e-7 x y / D < 1e-8 here)
        case = mk(3000, 200, 136, seed=93, s0=0.04, view=2, scale_xyz=0.8, bg=(0.2, 0.5, 0.7))
        s = case["sc"]["scaling"].clone()
        s[:1500] = torch.tensor([0.01, 1e-6, 1e-6])
        case["sc"]["scaling"] = s.contiguous()
    elif name == "edit_view":
        # mean list ~330 entries per tile, ~200 of the 1 024 tiles longer than 256 (cut into segments when forced)
        case = mk(8000, 512, 512, seed=95, s0=0.1, view=0, scale_xyz=0.6, bg=(0.2, 0.5, 0.7))
    else:
        raise KeyError(name)
    case["D"] = D
    H, W = case["H"], case["W"]
    G = seed_gradient(H, W, 7 + len(name)) * H * W
    return dict(name=name, case=case, D=D, sm=sm, colors_precomp=None, cov3D_precomp=None, G=G, GD=None)


def f64_run_aa(f, r):
    """f64_regimes.f64_run with opacities o * h: float64 autograd of the case's loss under the flag.  `f` is the float32
    oracle forward (its instance lists).  -> (gradients in the reference's conventions, render_f64 stats, image, r)."""
    from oracle.torch_ref import render_f64

    case, d = r["case"], torch.float64
    sc, cam = case["sc"], case["cam"]
    P, W, H = sc["xyz"].shape[0], case["W"], case["H"]
    leaf = lambda t: t.to(d).clone().requires_grad_(True)  # noqa: E731
    xyz, op, m2 = leaf(sc["xyz"]), leaf(sc["opacity"]), torch.zeros(P, 3, dtype=d, requires_grad=True)
    leaves = dict(dL_dmeans3D=xyz, dL_dmeans2D=m2, dL_dopacity=op)
    sh = cols = scl = rot = cov = None
    if r["colors_precomp"] is None:
        sh = leaves["dL_dsh"] = leaf(sc["features"])
    else:
        cols = leaves["dL_dcolors"] = leaf(r["colors_precomp"])
    if r["cov3D_precomp"] is None:
        scl, rot = leaves["dL_dscales"], leaves["dL_drotations"] = leaf(sc["scaling"]), leaf(sc["rotation"])
    else:
        cov = leaves["dL_dcov3D"] = leaf(r["cov3D_precomp"])
    x, y, z = cov2d_f64(xyz, scl, rot, cov, cam.world_view_transform, W, H, case["tfx"], case["tfy"], r["sm"])
    ratio = ratio_f64(x, y, z)
    op_eff = op * h_f64(x, y, z)[:, None]
    geo = (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)
    stats = {}
    img = render_f64(f, xyz, m2, op_eff, scl, rot, sh, cols, cov, *geo, case["bg"], W, H, case["tfx"], case["tfy"], r["sm"],
                     r["D"], dL_dimage=r["G"].to(d), stats=stats)
    if r["GD"] is not None:
        V = cam.world_view_transform.to(d).reshape(4, 4)
        tz = xyz @ V[:3, 2] + V[3, 2]
        dcol = torch.stack([tz, torch.zeros_like(tz), torch.zeros_like(tz)], dim=1)
        gd = torch.zeros(3, H, W, dtype=d)
        gd[0] = r["GD"].to(d).reshape(H, W)
        x2, y2, z2 = cov2d_f64(xyz, scl, rot, cov, cam.world_view_transform, W, H, case["tfx"], case["tfy"], r["sm"])
        render_f64(f, xyz, m2, op * h_f64(x2, y2, z2)[:, None], scl, rot, None, dcol, cov, *geo, torch.zeros(3), W, H,
                   case["tfx"], case["tfy"], r["sm"], r["D"], dL_dimage=gd)
    want = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for k, t in leaves.items()}
    if "dL_dscales" in want:
        want["dL_dscales"] = want["dL_dscales"] / r["sm"]
    geom = dict(r=ratio.detach().numpy(), x=x.detach().numpy(), y=y.detach().numpy(), z=z.detach().numpy())
    return want, stats, img, geom


def masked_rows_aa(r, f, stats, geom):
    """-> (mask, counts): the rows a comparison with float64 may leave out under the flag, each kind counted and bounded:
    Gaussians under flipped pixels and on the cone edge (f64_regimes.masked_rows), rows within NEAR_FLOOR_REL of the floor,
    and ill-conditioned footprints (det(S) < ILL_COND x y: float32's x y - z^2 cancels, and with it r)."""
    P, W = r["case"]["sc"]["xyz"].shape[0], r["case"]["W"]
    N = W * r["case"]["H"]
    vis = f["radii"] > 0
    flips = flipped_pixels(stats["n_contrib"].numpy(), stats["final_T"].numpy(), f["n_contrib"], f["final_T"])
    under = gaussians_under(flips, W, f, stats["n_contrib"].numpy())
    edge = R.cone_edge_rows(r) & vis
    rr, x, y, z = geom["r"], geom["x"], geom["y"], geom["z"]
    near_floor = (np.abs(rr - FLOOR) < NEAR_FLOOR_REL * FLOOR) & vis
    ill = ((x * y - z * z) < ILL_COND * x * y) & vis & ~(rr < FLOOR * (1 - NEAR_FLOOR_REL))
    counts = dict(flipped=int(flips.size), under=int(under.sum()), edge=int(edge.sum()), near_floor=int(near_floor.sum()),
                  ill=int(ill.sum()))
    assert flips.size <= 4 + 2e-4 * N, (r["name"], counts)
    assert under.sum() <= 0.02 * P + 64, (r["name"], counts)
    assert edge.sum() <= 4, (r["name"], counts)
    assert near_floor.sum() <= 4, (r["name"], counts)
    assert ill.sum() <= 0.02 * vis.sum() + 16, (r["name"], counts)
    return under | edge | near_floor | ill, counts


def aa_regime_count(r, f, geom):
    """The three new regimes assert that they are hit; -> the count (None for the cases of f64_regimes, which
    f64_regimes.regime_count checks)."""
    name, vis = r["name"], f["radii"] > 0
    h = np.sqrt(np.maximum(FLOOR, geom["r"]))
    if name == "sub_pixel":
        n = int(((h > 0.05) & (h < 0.9) & vis).sum())
        assert n >= 500, (name, n)
    elif name == "floor":
        n = int(((geom["r"] < FLOOR) & vis).sum())
        assert n >= 20, (name, n)
    elif name == "edit_view":
        T = ((r["case"]["W"] + 15) // 16) * ((r["case"]["H"] + 15) // 16)
        n = int(f["num_rendered"]) // T  # mean list length
        assert n >= 300, (name, n)
    else:
        return None
    print(f"[{name}] regime count {n}")
    return n


__all__ = ["cov2d_f64", "ratio_f64", "h_f64", "h_of_case", "sparse_case", "coverage", "regime", "f64_run_aa",
           "masked_rows_aa", "aa_regime_count", "NEW_CASES", "FLOOR"]
