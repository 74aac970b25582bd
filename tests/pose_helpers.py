"""Expectations and bars of the camera gradient (gaussianeditor_amd.set_pose_grad): dL/dviewmatrix, dL/dprojmatrix,
dL/dcampos of a render, against float64 autograd (oracle/torch_ref.py render_f64 keeps the three camera tensors in the
graph when they are float64 leaves) and against the translation identity.

Translation identity.  With a leaf c, A = V[:3,:3] and Pm = V^-1 PV, build V[3,:3] = -c A, PV = V Pm, campos = c: the
camera is then the same camera moved to c, and moving the camera by dc is moving every Gaussian by -dc, so
    c.grad = - sum_i dL/dmu_i
whatever the flags.  It ties the three raw partials (composed by autograd through this construction) to the gradient of the
means, which the existing suite pins, and it holds for the flag combinations render_f64 does not restate (antialiasing).

Bars.
  * dL/dviewmatrix, dL/dprojmatrix: f64_regimes.TOL (2e-5) x the tensor's largest float64 entry.
  * dL/dcampos is a cancelling sum: sum_i |dm_i| is 10-25x the result.  Its bar comes from a float32 REFERENCE that is not
    the kernel: the float32 oracle's dL_dmeans3D with SHs minus the same with colors_precomp = the forward's rgb (what is
    left is the dnormvdv term dm_i, in float32), summed over the Gaussians in float64, against float64 autograd.  Measured
    on the CPU (tools/pose_bars.py), relative to the largest float64 entry of dL/dcampos:

        case               oracle-difference reference vs float64     |sum dm| / sum |dm|
        sh_D1              1.29e-05                                    0.010
        sh_D3              2.07e-06                                    0.024
        clamped_colours    1.04e-06                                    0.088
        scale_mod_1.7      2.42e-06                                    0.050
        cov3D_precomp      1.53e-06                                    0.025
        off_cone           6.97e-06                                    0.019
        saturated          2.36e-06                                    0.085
        unnormalised_quat  1.84e-06                                    0.090
        off_cone+depth     6.97e-06                                    0.019

    (On all ten cases the float32 oracle's forward has 0 flipped pixels against float64 and no visible Gaussian within float
    rounding of the cone edge; dL/dprojmatrix formed the same way from the oracle's dL_dmeans2D is within 0.7 - 5.5e-6.)
    CAMPOS_TOL = 4 x the worst of them (the kernel sums other terms in another order than that construction does), and
    never below TOL.
  * translation identity: per component 7e-7 x sum_i |dL/dmu_i|, 4 x the worst ratio (1.7e-7) the float32 oracle shows
    against float64 on this identity; on the scene of identity_case() the oracle shows IDENTITY_ORACLE_RATIO.
  * general cameras (camera_cases.py: unequal focal lengths, roll, off-centre axis; rows of camera_cases.POSE_PAIRS): the
    same bars.  tools/pose_bars.py --camera NAME shows campos reference figures of at most 3.49e-06 (below
    CAMPOS_ORACLE_WORST) and an identity ratio of 1.5e-7 under `all` (below 1.7e-7); the tables are in DESIGN.md section 19.
"""
import numpy as np
import torch

import f64_regimes as R
from helpers import make_case, seed_gradient

POSE_CASES = ["sh_D1", "sh_D3", "clamped_colours", "scale_mod_1.7", "colors_precomp", "cov3D_precomp", "off_cone", "saturated",
              "unnormalised_quat", "off_cone+depth"]
CAMPOS_ORACLE_WORST = 1.29e-05  # the table above (sh_D1)
CAMPOS_TOL = max(4 * CAMPOS_ORACLE_WORST, R.TOL)
IDENTITY_TOL = 7e-7
IDENTITY_ORACLE_RATIO = 4.8e-8  # re-measured on identity_case() (tools/pose_bars.py); other seeds / views: DESIGN.md section 19


def pose_regime(name, camera=None, seed=None):
    """The regime `name` of POSE_CASES: a case of f64_regimes, `off_cone+depth` = off_cone with a depth gradient.  `camera`,
    `seed`: as in f64_regimes.regime."""
    if name == "off_cone+depth":
        r = R.regime("off_cone", camera=camera, seed=seed)
        H, W = r["case"]["H"], r["case"]["W"]
        return dict(r, GD=seed_gradient(H, W, 81)[:1] * H * W)
    return R.regime(name, camera=camera, seed=seed)


class LeafCam:
    """A camera whose three tensors are float64 leaves: handed to f64_regimes.f64_run in the case's place, render_f64 keeps
    them in the graph and their .grad are the raw partials."""

    def __init__(self, cam):
        leaf = lambda t: t.detach().to(torch.float64).clone().requires_grad_(True)  # noqa: E731
        self.world_view_transform = leaf(cam.world_view_transform)
        self.full_proj_transform = leaf(cam.full_proj_transform)
        self.camera_center = leaf(cam.camera_center)

    def grads(self):
        g = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy().copy()  # noqa: E731
        return dict(view=g(self.world_view_transform), proj=g(self.full_proj_transform), campos=g(self.camera_center))


def f64_pose(f, r):
    """float64 autograd of the case's loss with the camera tensors as leaves, the list structure taken from the forward `f`.
    -> (camera gradients dict(view (4,4), proj (4,4), campos (3,)), Gaussian gradients, render_f64 stats)."""
    cam = LeafCam(r["case"]["cam"])
    want, stats, _ = R.f64_run(f, dict(r, case=dict(r["case"], cam=cam)))
    return cam.grads(), want, stats


def assert_pose_close(got, want, tag, colors_precomp=False):
    """got / want: dict(view, proj, campos).  The bars of the module docstring and the structural zeros; prints each figure
    before it asserts.  -> the three relative errors."""
    errs = {}
    for k in ("view", "proj", "campos"):
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert a.shape == b.shape and np.isfinite(a).all(), (tag, k, a.shape)
        scale = float(np.abs(b).max())
        errs[k] = float(np.abs(a - b).max() / scale) if scale > 0 else float(np.abs(a).max())
    print(f"  {tag}: dL/dviewmatrix {errs['view']:.2e}, dL/dprojmatrix {errs['proj']:.2e}, dL/dcampos {errs['campos']:.2e} "
          f"(bars {R.TOL:.1e}, {R.TOL:.1e}, {CAMPOS_TOL:.1e})")
    assert not np.any(np.asarray(got["view"])[:, 3] != 0), (tag, "dL/dviewmatrix[:, 3] is not exactly zero")
    assert not np.any(np.asarray(got["proj"])[:, 2] != 0), (tag, "dL/dprojmatrix[:, 2] is not exactly zero")
    assert np.abs(want["view"]).max() > 0 and np.abs(want["proj"]).max() > 0, (tag, "the expectation is empty")
    assert not np.any(want["view"][:, 3] != 0) and not np.any(want["proj"][:, 2] != 0)  # (float64 agrees on the structure)
    if colors_precomp:
        assert not np.any(np.asarray(got["campos"]) != 0), (tag, "dL/dcampos is not exactly zero with precomputed colours")
        assert not np.any(want["campos"] != 0)
    assert errs["view"] <= R.TOL, (tag, "dL/dviewmatrix", errs["view"])
    assert errs["proj"] <= R.TOL, (tag, "dL/dprojmatrix", errs["proj"])
    assert errs["campos"] <= CAMPOS_TOL, (tag, "dL/dcampos", errs["campos"])
    return errs


# ---- translation identity -------------------------------------------------------------------------------------------
def identity_case(P=2000, W=136, H=120, seed=11, view=0, camera=None):
    """A synth-v2 view from inside the scene's dome (Gaussians beside and behind the camera, some off the cone); `camera`: a
    name of camera_cases.CAMERAS, the view through that general camera."""
    from gaussianeditor_amd.synth import synth_scene_v2

    case = make_case(P, W, H, seed=seed, view=view, nviews=8, bg=(0.2, 0.5, 0.7), camera=camera)
    case["sc"] = synth_scene_v2(P, seed=seed)
    return case


def moved_camera(cam, dtype, device="cpu"):
    """-> (c leaf, viewmatrix, projmatrix, campos): the camera `cam` rebuilt from its centre c (module docstring); the
    constants A and Pm are computed in float64 and cast."""
    V64, PV64 = cam.world_view_transform.double(), cam.full_proj_transform.double()
    A = V64[:3, :3].to(dtype=dtype, device=device)
    Pm = (torch.linalg.inv(V64) @ PV64).to(dtype=dtype, device=device)
    c = cam.camera_center.double().to(dtype=dtype, device=device).clone().requires_grad_(True)
    col = torch.tensor([[0.0], [0.0], [0.0], [1.0]], dtype=dtype, device=device)
    V = torch.cat([torch.cat([A, (-c @ A)[None, :]], dim=0), col], dim=1)
    return c, V, V @ Pm, c


def assert_identity(c_grad, means_grad, tag, tol=IDENTITY_TOL):
    """c.grad = - sum_i dL/dmu_i, per component within tol x sum_i |dL/dmu_i| (sums in float64)."""
    g = np.asarray(means_grad, np.float64)
    lhs, rhs, scale = np.asarray(c_grad, np.float64), -g.sum(axis=0), np.abs(g).sum(axis=0)
    ratio = np.abs(lhs - rhs) / np.maximum(scale, 1e-300)
    print(f"  {tag}: |c.grad + sum dL/dmu| / sum |dL/dmu| = {ratio.max():.2e} (bar {tol:.1e}); c.grad {lhs}, sum |dL/dmu| {scale}")
    assert np.isfinite(lhs).all() and scale.min() > 0 and np.abs(lhs).max() > 0, (tag, lhs, scale)
    assert (ratio <= tol).all(), (tag, ratio)
    return float(ratio.max())
