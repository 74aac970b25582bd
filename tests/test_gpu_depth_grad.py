"""-m gpu: depth gradients (opt-in, gaussianeditor_amd.set_depth_grad / options.FLAG_DEPTH_GRAD).  The product's gradients of
<gC, C> + <gD, D> against the linearity construction of depth_helpers (two ordinary oracle backwards), under the parity bars
of helpers.assert_grads_close; the switch off leaves today's behaviour; the accumulator table is left clean."""
import types

import numpy as np
import pytest
import torch

from depth_helpers import DEV, depth_colors, depth_expectation, grads_hip
from helpers import assert_grads_close, make_case, oracle_forward, rel_err, seed_gradient

pytestmark = pytest.mark.gpu


def _flags(*extra):
    from gaussianeditor_amd import options

    f = options.FLAG_DEPTH_GRAD
    for e in extra:
        f |= e
    return f


def _grads(case, seed):
    H, W = case["H"], case["W"]
    G = seed_gradient(H, W, seed) * (H * W)
    GD = seed_gradient(H, W, seed + 11)[:1] * (H * W)
    return G, GD


CASES = {
    "sh3": lambda: (make_case(10000, 256, 256, seed=1, s0=0.03), {}),
    "sh0": lambda: (make_case(10000, 256, 256, seed=2, s0=0.03, sh_degree=0), {}),
    "scale_modifier": lambda: (make_case(8000, 256, 192, seed=3, s0=0.04), dict(scale_modifier=0.7)),
    "1080p": lambda: (make_case(60000, 1920, 1080, seed=5, s0=0.01), {}),
    # the editor's view: a small image of a large scene -- deep tile lists, whose ordinary backward cuts list segments
    "edit512": lambda: (make_case(300000, 512, 512, seed=6, s0=0.01), {}),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("depth_only", [False, True])
def test_depth_grad_vs_linearity(oracle, name, depth_only):
    case, kw = CASES[name]()
    G, GD = _grads(case, 3)
    want = depth_expectation(oracle, case, None if depth_only else G, GD, **kw)
    got = grads_hip(case, G, GD, flags=_flags(), depth_only=depth_only, **kw)
    assert np.abs(want["dL_ddepth"]).max() > 0
    assert_grads_close(got, want, tag=f"depth {name} depth_only={depth_only}", keys=list(got))


def test_depth_grad_precomputed_colours_and_covariance(oracle):
    case = make_case(4000, 192, 128, seed=9, s0=0.05)
    G, GD = _grads(case, 9)
    cols = torch.rand(4000, 3, generator=torch.Generator().manual_seed(3))
    cov = torch.from_numpy(oracle_forward(oracle, case)["cov3D"].copy())
    for kw in (dict(colors_precomp=cols), dict(cov3D_precomp=cov), dict(colors_precomp=cols, cov3D_precomp=cov)):
        want = depth_expectation(oracle, case, G, GD, **kw)
        got = grads_hip(case, G, GD, flags=_flags(), **kw)
        assert_grads_close(got, want, tag=f"depth precomp {sorted(kw)}", keys=list(got))


def test_depth_grad_tile_bounds_alpha(oracle):
    from gaussianeditor_amd import options

    case = make_case(10000, 256, 256, seed=4, s0=0.03)
    G, GD = _grads(case, 4)
    want = depth_expectation(oracle, case, G, GD)
    got = grads_hip(case, G, GD, flags=_flags(options.FLAG_TILE_BOUNDS_ALPHA))
    assert_grads_close(got, want, tag="depth tile bounds alpha", keys=list(got))


def test_depth_grad_fast_exp_is_linear():
    """GSR_FLAG_FAST_EXP: the product's own exp decisions (its bar against the oracle masks the flipped pixels, test_gpu_round2),
    so the yardstick is the same linearity from two product backwards under the flag: the colour loss, plus the render
    with colours (d, 0, 0) on background 0 and pixel gradient (gD, 0, 0), plus dL_dd (view[2], view[6], view[10])."""
    from gaussianeditor_amd import options

    from depth_helpers import view_z_row

    case = make_case(20000, 512, 512, seed=4, s0=0.02)
    G, GD = _grads(case, 5)
    fe = options.FLAG_FAST_EXP
    got = grads_hip(case, G, GD, flags=_flags(fe))
    g1 = grads_hip(case, G, GD, flags=fe)  # (flag off: the depth loss carries nothing)
    from oracle import cpu as O
    from helpers import oracle_forward as of

    dcol = depth_colors(of(O, case)["depths"])
    G2 = torch.zeros_like(G)
    G2[0] = GD[0]
    case0 = dict(case, bg=torch.zeros(3))
    g2 = grads_hip(case0, G2, torch.zeros_like(GD), colors_precomp=dcol, flags=fe)
    want = {k: g1[k].astype(np.float64) + g2[k].reshape(g1[k].shape) for k in g1 if k != "dL_dsh"}
    want["dL_dsh"] = g1["dL_dsh"]
    want["dL_dmeans3D"] = want["dL_dmeans3D"] + g2["dL_dcolors"][:, :1].astype(np.float64) * view_z_row(case)[None, :]
    assert_grads_close(got, want, tag="depth fast exp", keys=list(got))


def test_depth_grad_matches_float64_autograd(oracle):
    """A small case end to end against float64 autograd of the loss (the depth as colours (tz(means3D), 0, 0), bg 0)."""
    from oracle.torch_ref import render_f64

    W, H, P = 48, 40, 150  # (the configuration of test_cpu_oracle's float64 check: no pixel on a float32 / float64 decision edge)
    case = make_case(P, W, H, seed=4, s0=0.1, view=2, scale_xyz=0.5)
    sc, cam = case["sc"], case["cam"]
    cols = torch.rand(P, 3, generator=torch.Generator().manual_seed(5))
    G, GD = _grads(case, 2)
    got = grads_hip(case, G, GD, colors_precomp=cols, flags=_flags())
    f = oracle_forward(oracle, case, colors_precomp=cols)
    d = torch.float64
    xyz, op = sc["xyz"].to(d).requires_grad_(True), sc["opacity"].to(d).requires_grad_(True)
    scl, rot = sc["scaling"].to(d).requires_grad_(True), sc["rotation"].to(d).requires_grad_(True)
    c64 = cols.to(d).requires_grad_(True)
    args = (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)
    img = render_f64(f, xyz, None, op, scl, rot, None, c64, None, *args, case["bg"], W, H, case["tfx"], case["tfy"], 1.0, 0)
    V = cam.world_view_transform.to(d).reshape(4, 4)
    z = xyz @ V[:3, 2] + V[3, 2]
    dimg = render_f64(f, xyz, None, op, scl, rot, None, torch.stack([z, torch.zeros_like(z), torch.zeros_like(z)], 1), None,
                      *args, torch.zeros(3), W, H, case["tfx"], case["tfy"], 1.0, 0)
    ((img * G.to(d)).sum() + (dimg[0] * GD[0].to(d)).sum()).backward()
    for k, t in (("dL_dmeans3D", xyz), ("dL_dopacity", op), ("dL_dscales", scl), ("dL_drotations", rot), ("dL_dcolors", c64)):
        e = rel_err(got[k].reshape(t.shape), t.grad.numpy())
        assert e < 2e-5, (k, e)


def test_flag_off_depth_loss_is_ignored():
    """Switch off: a depth loss leaves the gradients what the colour loss alone gives (the same kernels: within the backward's
    run-to-run spread, test_backward_run_to_run_spread), and a depth-only loss gives the reference's all-zero gradients."""
    case = make_case(10000, 256, 256, seed=1, s0=0.03)
    G, GD = _grads(case, 1)
    plain = grads_hip(case, G, torch.zeros_like(GD), flags=0)
    with_depth = grads_hip(case, G, GD, flags=0)
    for k in plain:
        assert rel_err(with_depth[k], plain[k]) <= 2e-6, k
    only = grads_hip(case, G, GD, flags=0, depth_only=True)
    for k, v in only.items():
        assert not np.any(v), k


def test_flag_on_depth_unused_changes_nothing():
    case = make_case(10000, 256, 256, seed=1, s0=0.03)
    G, GD = _grads(case, 1)
    off = grads_hip(case, G, torch.zeros_like(GD), flags=0)
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer
    from helpers import settings

    sc = case["sc"]
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)  # noqa: E731
    xyz, op, sh, scl, rot = leaf(sc["xyz"]), leaf(sc["opacity"]), leaf(sc["features"]), leaf(sc["scaling"]), leaf(sc["rotation"])
    m2d = torch.zeros_like(xyz, requires_grad=True)
    with options.override(_flags()):
        color, radii, depth = GaussianRasterizer(settings(case, DEV))(xyz, m2d, op, shs=sh, scales=scl, rotations=rot)
    (color * G.to(DEV)).sum().backward()  # (the depth output is not used: grad_depth is None)
    on = dict(dL_dmeans3D=xyz, dL_dopacity=op, dL_dmeans2D=m2d, dL_dsh=sh, dL_dscales=scl, dL_drotations=rot)
    for k, t in on.items():
        assert rel_err(t.grad.cpu().numpy(), off[k]) <= 2e-6, k


def test_accumulator_table_is_clean_after_a_depth_backward():
    """The binding keeps one accumulator table per stream across backwards (GSR_FLAG_ACC_SELF_CLEAN): after a depth
    backward it is all zero again -- also rows that held a depth entry only -- and a following plain backward is unaffected."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    case = make_case(10000, 256, 256, seed=7, s0=0.03)
    G, GD = _grads(case, 7)
    before = grads_hip(case, G, torch.zeros_like(GD), flags=0)
    grads_hip(case, G, GD, flags=_flags(), depth_only=True)  # (rows with only a depth entry: colour gradient zero)
    grads_hip(case, G, GD, flags=_flags())
    torch.cuda.synchronize()
    tables = [t for t in _C._ACC_TABLES.values() if t.numel() == 16 * 10000]
    assert tables and all(int(torch.count_nonzero(t)) == 0 for t in tables)
    after = grads_hip(case, G, torch.zeros_like(GD), flags=0)
    for k in before:
        assert rel_err(after[k], before[k]) <= 2e-6, k


class _Model:
    def __init__(self, sc):
        d = lambda t: t.to(DEV).clone().contiguous().requires_grad_(True)  # noqa: E731
        self._xyz, self._features = d(sc["xyz"]), d(sc["features"])
        self._opacity, self._scaling, self._rotation = d(sc["opacity"]), d(sc["scaling"]), d(sc["rotation"])
        self.active_sh_degree = self.max_sh_degree = 3

    get_xyz = property(lambda s: s._xyz)
    get_features = property(lambda s: s._features)
    get_opacity = property(lambda s: s._opacity)
    get_scaling = property(lambda s: s._scaling)
    get_rotation = property(lambda s: s._rotation)


def _camera(case):
    c = case["cam"]
    return types.SimpleNamespace(FoVx=c.FoVx, FoVy=c.FoVy, image_height=case["H"], image_width=case["W"],
                                 world_view_transform=c.world_view_transform.to(DEV),
                                 full_proj_transform=c.full_proj_transform.to(DEV), camera_center=c.camera_center.to(DEV))


@pytest.mark.parametrize("reused", [False, True])
def test_editor_render_depth_loss(reused):
    """Through the unmodified render() mirror: depth_3dgs.mean().backward() moves _xyz with the switch on and not at all with
    it off -- also for the depth of the colour-override render that view reuse serves from the first render's state."""
    import gaussianeditor_amd
    from gaussianeditor_amd.gaussian_renderer import render

    case = make_case(5000, 192, 160, seed=8, s0=0.04)
    pipe = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    cam = _camera(case)
    res = {}
    for on in (False, True):
        m = _Model(case["sc"])
        gaussianeditor_amd.set_depth_grad(on)
        try:
            out = render(cam, m, pipe, bg)
            if reused:
                mask = torch.rand(5000, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
                out = render(cam, m, pipe, bg, override_color=mask)
            out["depth_3dgs"].mean().backward()
        finally:
            gaussianeditor_amd.set_depth_grad(False)
        torch.cuda.synchronize()
        res[on] = m._xyz.grad
    assert res[False] is None or not torch.any(res[False])
    assert res[True] is not None and torch.any(res[True])
