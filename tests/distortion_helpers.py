"""The yardstick of the depth-distortion image (`return_distortion` of GaussianRasterizer / render(); include/gsr.h
gsr_blend_forward_distortion, gsr_blend_backward_distortion): float64 autograd through the existing
oracle/torch_ref.py::render_f64, unchanged.

Per pixel D = 1/2 sum_{i != j} w_i w_j (m_i - m_j)^2 = A M2 - M1^2, A = sum w, M1 = sum w m, M2 = sum w m^2, w = alpha T.
The depths are DATA: the float32 oracle's `depths`, promoted to float64 (m = z, or 2DGS's mapping of z).  render_f64 with
colors_precomp = (1, m - c, (m - c)^2), c a constant (D does not change under a shift of m), on background 0 gives
(A, M1, M2).  D is not linear in them, so the expectation takes two renders: one for the three images, one whose pixel
gradient is gD (dD/dA, dD/dM1, dD/dM2) = gD (M2, -2 M1, A).  Its autograd gives the geometry gradients through w; its
dL/dcolors_precomp = (d_0, d_1, d_2) gives dL/dz_k = mu_k (d_1 + 2 (m_k - c) d_2), mu = dm/dz, and dL/dz times the view
matrix's z row joins dL_dmeans3D.  (d_0 needs no chain: the first colour is the constant 1.)

The bar of every comparison is f64_regimes.TOL (2e-5 of a tensor's largest entry, plus the per-row rule of
helpers.assert_grads_close), as tests/test_gpu_f64_regimes.py uses it; rows under pixels whose discrete decisions differ
between float64 and float32 are counted by f64_regimes.masked_rows, and the distortion cases assert that there are none."""
import functools
import math

import numpy as np
import torch

import f64_regimes as R
from helpers import make_case, oracle_forward, seed_gradient

DEV = "cuda:0"
TOL = R.TOL
KEYS = ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dscales", "dL_drotations"]
SHARE_KEYS = ["dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_dmeans2D"]
NEAR_FAR = (0.2, 100.0)
#: the cases of the issue's table: make_case arguments (the far slab is built by far_slab_case)
CASES = {"partial": dict(P=300, W=17, H=9, s0=0.08), "p2000": dict(P=2000, W=64, H=64, s0=0.05),
         "ragged": dict(P=2000, W=70, H=45, s0=0.05), "p4000": dict(P=4000, W=40, H=24, s0=0.12)}


def mapped(z, near_far):
    """m(z), mu = dm/dz of a depth: linear (near_far None) or 2DGS's mapping f (z - n) / ((f - n) z)."""
    if near_far is None:
        return z, np.ones_like(z)
    n, f = near_far
    return f * (z - n) / ((f - n) * z), (f * n / (f - n)) / (z * z)


def far_slab_case(P=500, W=32, H=32, z_lo=50.0, spread=0.05, seed=9):
    """About `P` Gaussians whose view-space depth lies in [z_lo, z_lo + spread], spread over a W x H image: a thin surface far
    from the camera, where the unshifted float32 moments A M2 - M1^2 cancel.  Screen-space sigma 2.5 .. 4 px, opacity
    0.05 .. 0.3: every pixel blends tens of entries."""
    case = make_case(P, W, H, seed=seed, s0=0.05)
    sc, cam = dict(case["sc"]), case["cam"]
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    z = z_lo + spread * u(P)
    px, py = -2.0 + (W + 4.0) * u(P), -2.0 + (H + 4.0) * u(P)
    focal = W / (2.0 * case["tfx"])
    p_cam = torch.stack([((2.0 * px + 1.0) / W - 1.0) * case["tfx"] * z, ((2.0 * py + 1.0) / H - 1.0) * case["tfy"] * z, z,
                         torch.ones(P, dtype=torch.float64)], dim=1)
    xyz = (p_cam @ cam.world_view_transform.double().inverse())[:, :3]
    sigma = 2.5 + 1.5 * u(P, 1)
    aniso = 0.7 + 0.6 * u(P, 3)
    q = torch.randn(P, 4, generator=g, dtype=torch.float64)
    sc.update(xyz=xyz.float().contiguous(), scaling=(sigma * z[:, None] / focal * aniso).float().contiguous(),
              rotation=(q / q.norm(dim=1, keepdim=True)).float().contiguous(),
              opacity=(0.05 + 0.25 * u(P, 1)).float().contiguous())
    return dict(case, sc=sc)


def single_contributor_case():
    """A 32 x 32 image with three small, well separated Gaussians and one pair that overlaps: most covered pixels blend
    exactly one entry (D = 0 and no gradient there), a few blend two."""
    W = H = 32
    case = make_case(5, W, H, seed=4, s0=0.05)
    sc, cam = dict(case["sc"]), case["cam"]
    focal = W / (2.0 * case["tfx"])
    centres = [(5.0, 5.0, 3.0), (25.0, 6.0, 3.5), (6.0, 25.0, 4.0), (22.0, 22.0, 3.0), (23.5, 23.0, 4.5)]
    P = len(centres)
    px, py, z = (torch.tensor(v, dtype=torch.float64) for v in zip(*centres))
    p_cam = torch.stack([((2.0 * px + 1.0) / W - 1.0) * case["tfx"] * z, ((2.0 * py + 1.0) / H - 1.0) * case["tfy"] * z, z,
                         torch.ones(P, dtype=torch.float64)], dim=1)
    xyz = (p_cam @ cam.world_view_transform.double().inverse())[:, :3]
    rot = torch.zeros(P, 4)
    rot[:, 0] = 1.0
    sc.update(xyz=xyz.float().contiguous(), scaling=(1.6 * z[:, None] / focal).expand(P, 3).float().contiguous(),
              rotation=rot.contiguous(), opacity=torch.full((P, 1), 0.8), features=sc["features"][:P].contiguous())
    return dict(case, sc=sc)


@functools.lru_cache(maxsize=None)
def get_case(name):
    """The case `name` -- built once, never modified."""
    if name == "far_slab":
        return far_slab_case()
    if name == "single":
        return single_contributor_case()
    kw = CASES[name]
    return make_case(kw["P"], kw["W"], kw["H"], s0=kw["s0"])


def weights(case, k=5):
    """(1,H,W) pixel gradient of the distortion image: seed_gradient's first channel, scaled as the colour gradients are."""
    H, W = case["H"], case["W"]
    return (seed_gradient(H, W, k)[:1] * H * W).contiguous()


def colour_weights(case):
    H, W = case["H"], case["W"]
    return (seed_gradient(H, W, 3) * H * W).contiguous()


def _leaves(case, d=torch.float64):
    sc = case["sc"]
    leaf = lambda t: t.to(d).clone().requires_grad_(True)  # noqa: E731
    P = sc["xyz"].shape[0]
    lv = dict(dL_dmeans3D=leaf(sc["xyz"]), dL_dmeans2D=torch.zeros(P, 3, dtype=d, requires_grad=True),
              dL_dopacity=leaf(sc["opacity"]), dL_dsh=leaf(sc["features"]), dL_dscales=leaf(sc["scaling"]),
              dL_drotations=leaf(sc["rotation"]))
    return lv


def f64_distortion(f, case, GDist, near_far=None, G=None, with_colour_only=False):
    """float64 expectation of <GDist, D> (+ <G, C>), the discrete structure from the float32 oracle forward `f`.
    -> dict(image (H,W) float64, want {key: gradient}, stats of render_f64, [colour_only {key: gradient of <G, C> alone}])."""
    from oracle.torch_ref import render_f64

    d = torch.float64
    cam, W, H = case["cam"], case["W"], case["H"]
    geo = (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)
    tail = (W, H, case["tfx"], case["tfy"], 1.0, case["D"])
    z = f["depths"].astype(np.float64)  # the data: float32 values
    vis = f["radii"] > 0
    z = np.where(vis, z, 1.0)  # (a culled Gaussian is on no list: its depth, 0 in the oracle's table, must not reach 1 / z)
    m, mu = mapped(z, near_far)
    c = float(np.median(m[vis])) if vis.any() else 0.0
    mc = torch.from_numpy(m - c)
    moment_colours = torch.stack([torch.ones_like(mc), mc, mc * mc], dim=1)
    bg0 = torch.zeros(3)
    # (1) the three images
    lv = _leaves(case)
    stats = {}
    with torch.no_grad():
        img = render_f64(f, lv["dL_dmeans3D"], lv["dL_dmeans2D"], lv["dL_dopacity"], lv["dL_dscales"], lv["dL_drotations"], None,
                         moment_colours, None, *geo, bg0, *tail, stats=stats)
    A, M1, M2 = img[0], img[1], img[2]
    Dimg = A * M2 - M1 * M1
    # (2) the gradient: gD (M2, -2 M1, A) into the three images
    gD = GDist.to(d).reshape(H, W)
    cols = moment_colours.clone().requires_grad_(True)
    render_f64(f, lv["dL_dmeans3D"], lv["dL_dmeans2D"], lv["dL_dopacity"], lv["dL_dscales"], lv["dL_drotations"], None, cols, None,
               *geo, bg0, *tail, dL_dimage=torch.stack([gD * M2, -2.0 * gD * M1, gD * A]))
    dcol = cols.grad if cols.grad is not None else torch.zeros_like(cols)
    dz = torch.from_numpy(mu) * (dcol[:, 1] + 2.0 * mc * dcol[:, 2])
    Vz = cam.world_view_transform.to(d).reshape(4, 4)[:3, 2]
    share = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy().copy() for k, t in lv.items()}
    share["dL_dmeans3D"] = share["dL_dmeans3D"] + (dz[:, None] * Vz[None, :]).numpy()
    out = dict(image=Dimg.numpy(), stats=stats, share=share, dL_dz=dz.numpy())
    want = share
    if G is not None:
        lc = _leaves(case)
        render_f64(f, lc["dL_dmeans3D"], lc["dL_dmeans2D"], lc["dL_dopacity"], lc["dL_dscales"], lc["dL_drotations"], lc["dL_dsh"],
                   None, None, *geo, case["bg"], *tail, dL_dimage=G.to(d))
        colour = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for k, t in lc.items()}
        out["colour_only"] = colour
        want = {k: share[k] + colour[k] for k in share}
    out["want"] = want
    return out


@functools.lru_cache(maxsize=None)
def expectation(name, near_far=None, colour=False):
    """(case, float32 oracle forward, f64_distortion(...), masked rows) of a case -- computed once, shared by the tests.
    `colour`: the loss is <colour_weights, C> + lam <weights, D>, and e["lam"] is its weight lam: the power of ten that brings
    the distortion share of dL_dmeans3D nearest the colour loss's (a regulariser's weight; D is of order 1e-12 on the mapped
    far slab and of order 0.1 on the synthetic scenes).  It is chosen from the float64 expectation alone; the gradient is
    linear in it, so the share is scaled exactly.  e["lam"] = 1 without `colour`."""
    from oracle import cpu

    cpu.build()
    case = get_case(name)
    f = oracle_forward(cpu, case)
    e, masked = expectation_of(case, f, name, near_far=near_far, colour=colour)
    return case, f, e, masked


def expectation_of(case, f, name, near_far=None, colour=False, GDist=None, lam=None):
    """`expectation` of any case and its float32 oracle forward `f` -> (f64_distortion(...) with "lam", masked rows).
    `GDist`: another pixel gradient than weights(case); `lam`: a given weight instead of the one chosen here."""
    e = f64_distortion(f, case, weights(case) if GDist is None else GDist, near_far=near_far,
                       G=colour_weights(case) if colour else None)
    e["lam"] = 1.0
    if colour:
        if lam is None:
            ratio = float(np.abs(e["colour_only"]["dL_dmeans3D"]).max()) / float(np.abs(e["share"]["dL_dmeans3D"]).max())
            lam = 10.0 ** round(math.log10(ratio))
        e["lam"] = lam
        e["share"] = {k: v * lam for k, v in e["share"].items()}
        e["dL_dz"] = e["dL_dz"] * lam
        e["want"] = {k: e["share"][k] + e["colour_only"][k] for k in e["share"]}
    r = dict(name="distortion:" + name, case=case)
    masked, report = R.masked_rows(r, f, e["stats"])
    print(f"[distortion:{name}] {report}")
    return e, masked


def assert_share_visible(e, tag=""):
    """The distortion share exceeds ten bars of the expectation (colour + distortion) on the four tensors the issue names."""
    for k in SHARE_KEYS:
        s, scale = float(np.abs(e["share"][k]).max()), float(np.abs(e["want"][k]).max())
        print(f"  {tag}: {k} distortion share {s / scale:.2e} of the expectation's maximum (ten bars: {10 * TOL:.0e})")
        assert s > 10 * TOL * scale, (tag, k, s, scale)


def run_hip(case, GDist=None, near_far=None, G=None, flags=0, return_distortion=True, pose=False, abs_grad=False, GD=None,
            GA=None, feats=None, GF=None):
    """One render (+ backward of <GDist, D> + <G, C> + ...) through GaussianRasterizer under options.override(flags).
    -> (gradients by the oracle's names | None, dict of outputs as numpy)."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer
    from helpers import settings

    sc = case["sc"]
    rs = settings(case, DEV)
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)  # noqa: E731
    cams = None
    if pose:
        cams = dict(view=leaf(rs.viewmatrix), proj=leaf(rs.projmatrix), campos=leaf(rs.campos))
        rs = rs._replace(viewmatrix=cams["view"], projmatrix=cams["proj"], campos=cams["campos"])
    lv = dict(dL_dmeans3D=leaf(sc["xyz"]), dL_dopacity=leaf(sc["opacity"]), dL_dsh=leaf(sc["features"]),
              dL_dscales=leaf(sc["scaling"]), dL_drotations=leaf(sc["rotation"]))
    m2d = lv["dL_dmeans2D"] = torch.zeros_like(lv["dL_dmeans3D"], requires_grad=True)
    kw = {}
    if return_distortion:
        kw["return_distortion"] = True if near_far is None else near_far
    if GA is not None:
        kw["return_alpha"] = True
    if feats is not None:
        kw["features"] = lv["dL_dfeatures"] = leaf(feats)
    f = (flags | (options.FLAG_ABS_GRAD if abs_grad else 0) | (options.FLAG_DEPTH_GRAD if GD is not None else 0)
         | (options.FLAG_POSE_GRAD if pose else 0))
    with options.override(f):
        outs = GaussianRasterizer(rs)(lv["dL_dmeans3D"], m2d, lv["dL_dopacity"], shs=lv["dL_dsh"], scales=lv["dL_dscales"],
                                      rotations=lv["dL_drotations"], **kw)
    assert len(outs) == 3 + (GA is not None) + (feats is not None) + bool(return_distortion)
    color, radii, depth = outs[:3]
    dist = outs[-1] if return_distortion else None
    rest = outs[3:len(outs) - (1 if return_distortion else 0)]
    loss = 0.0
    if G is not None:
        loss = loss + (color * G.to(DEV)).sum()
    if GDist is not None:
        loss = loss + (dist * GDist.to(DEV)).sum()
    if GD is not None:
        loss = loss + (depth * GD.to(DEV)).sum()
    if GA is not None:
        loss = loss + (rest[0] * GA.to(DEV)).sum()
    if GF is not None:
        loss = loss + (rest[-1] * GF.to(DEV)).sum()
    grads = None
    if isinstance(loss, torch.Tensor):
        loss.backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).cpu().numpy() for k, v in lv.items()}
    torch.cuda.synchronize()
    npy = lambda t: None if t is None else t.detach().cpu().numpy()  # noqa: E731
    pg = None if cams is None else {k: npy(v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in cams.items()}
    return grads, dict(color=npy(color), depth=npy(depth), radii=npy(radii), distortion=npy(dist),
                       absgrad=npy(getattr(m2d, "absgrad", None)), pose=pg)


# ---- a float32 model of one pixel's accumulation (tests/test_cpu_distortion.py) ------------------------------------------
def pixel_weights(alpha):
    """w = alpha T front to back (float64)."""
    T = np.concatenate([[1.0], np.cumprod(1.0 - alpha)[:-1]])
    return alpha * T


def f32_moments(w, z, shifted, near_far=None):
    """The kernel's accumulation of one pixel in numpy float32 -> (D, dD/dw, dD/dm) as float64 arrays: the moments of the
    shifted depth m' (from the difference of the z's) or, `shifted` False, of m itself."""
    f = np.float32
    w, z = w.astype(f), z.astype(f)
    if shifted:
        z0 = z[0]
        if near_far is None:
            m = z - z0
        else:
            kappa = f(near_far[1] * near_far[0] / (near_far[1] - near_far[0]))
            m = (f(kappa / z0) * (z - z0)) * (f(1.0) / z)
    else:
        m = z if near_far is None else (f(near_far[1]) * (z - f(near_far[0])) / (f(near_far[1] - near_far[0]) * z)).astype(f)
    A = M1 = M2 = f(0.0)
    for i in range(w.size):
        A = f(A + w[i])
        M1 = f(M1 + f(w[i] * m[i]))
        M2 = f(M2 + f(f(w[i] * m[i]) * m[i]))
    D = f(f(A * M2) - f(M1 * M1))
    c = (m * (m * A + f(-2.0) * M1) + M2).astype(f)
    dm = (f(2.0) * w * (m * A - M1)).astype(f)
    return float(D), c.astype(np.float64), dm.astype(np.float64)


def slab_pixel(n=40, z_lo=50.0, spread=0.05, seed=0):
    """(alpha (n,) float64, z (n,) float32 values as float64, ascending) of one pixel of the far slab."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.01, 0.31, n)
    z = np.sort(z_lo + spread * rng.uniform(0.0, 1.0, n)).astype(np.float32).astype(np.float64)
    return alpha, z


# ---- a CPU stand-in for the new `_C` entry points (tests/test_cpu_distortion.py) ------------------------------------------
class DistortionBackend:
    """features_helpers.FeatureBackend plus `rasterize_distortion` and the `distortion_moments` / `dL_dout_distortion` /
    `distortion_near_far` keywords.  The image is a fixed function of the arguments (zeros plus the mapped flag): the layer
    tests are about arity, argument tuples and refusals, not about values.  Records what it is asked."""

    def __init__(self, inner):
        self.inner = inner  # a FeatureBackend
        self.distortion_calls = []
        self.backward_kw = []

    def rasterize_distortion(self, num_points, num_rendered, geomBuffer, binningBuffer, imgBuffer, H, W, near_far=None,
                             with_moments=True, debug=False, flags=None):
        from gaussianeditor_amd.diff_gaussian_rasterization import _C

        _C.check_near_far(near_far)
        self.distortion_calls.append(dict(P=int(num_points), near_far=near_far, with_moments=bool(with_moments)))
        self.inner.calls.append(("rasterize_distortion", 9, ("flags",)))
        out = torch.full((1, int(H), int(W)), 0.25 if near_far is None else 0.5)
        return out, (torch.ones(int(H), int(W), 4) if with_moments else None)

    def backward(self, *args, distortion_moments=None, dL_dout_distortion=None, distortion_near_far=None, **kw):
        self.backward_kw.append(dict(moments=distortion_moments is not None, grad=dL_dout_distortion is not None,
                                     near_far=distortion_near_far, other=tuple(sorted(kw))))
        return self.inner.backward(*args, **kw)


def install(monkeypatch):
    """features_helpers.install plus the stand-ins above -> (the package, the feature backend, the distortion backend)."""
    import features_helpers as FH

    dgr, be = FH.install(monkeypatch)
    db = DistortionBackend(be)
    monkeypatch.setattr(dgr._C, "rasterize_distortion", db.rasterize_distortion, raising=True)
    monkeypatch.setattr(dgr._C, "rasterize_gaussians_backward", db.backward)
    return dgr, be, db
