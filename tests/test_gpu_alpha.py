"""-m gpu: the alpha image (accumulated opacity A = 1 - final_T; `return_alpha=True`, gaussianeditor_amd.set_alpha_output) and
its gradient (gsr_alpha_image, gsr_blend_backward_alpha: the ALPHA instantiations of K7).

Forward: bit-identical to 1 - final_T of the image state and of the CPU oracle.  Backward: against the linearity construction
of alpha_helpers (held to float64 autograd and to finite differences by tests/test_cpu_alpha.py) on every route, with the
discrimination condition asserted in each test -- (i) the alpha share of the expectation exceeds 1e-2 of the total's maximum
on >= 100 rows of each of dL_dmeans3D, dL_dopacity, dL_dscales (dL_dcov3D on the precomputed-covariance route, which has no
scales) and dL_dmeans2D, (ii) the product's gradients differ from its own colour-only gradients by more than ten bars.
Shapes: 64 x 64 (16 tiles, every one far above 1.25 fair shares of the persistent grid: whole-tile, half-tile and, forced,
segment items all occur), 70 x 45 for the ragged edge.
Measured on the MI355X: every gradient within 4.9e-7 of its tensor's maximum (bar 1e-5), the whole file in 7.5 s."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import alpha_helpers as AH
from helpers import assert_grads_close, hip_state, make_case, oracle_forward, seed_gradient, settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _case(name="p2000", camera=None):
    """(case, G, GA) -- built once per process, never modified.  `camera`: a name of camera_cases.CAMERAS."""
    if (name, camera) not in _cache:
        P, W, H, s0 = {"p2000": (2000, 64, 64, 0.05), "p20000": (20000, 64, 64, 0.03), "ragged": (2000, 70, 45, 0.05)}[name]
        case = make_case(P, W, H, s0=s0, camera=camera)
        _cache[name, camera] = (case, seed_gradient(H, W, 3) * H * W, seed_gradient(H, W, 5)[:1] * H * W)
    return _cache[name, camera]


def _forward_state(case, flags=0, **kw):
    """_C.rasterize_gaussians of the case -> (R, color, depth, radii, geom, binning, img), on the device."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    sc, rs = case["sc"], settings(case, DEV)
    e = torch.empty(0, device=DEV)
    t = lambda k: sc[k].to(DEV)  # noqa: E731
    return _C.rasterize_gaussians(rs.bg, t("xyz"), e, t("opacity"), t("scaling"), t("rotation"), 1.0, e, rs.viewmatrix,
                                  rs.projmatrix, rs.tanfovx, rs.tanfovy, case["H"], case["W"], t("features"), 3, rs.campos,
                                  False, False, flags=flags)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# forward
@pytest.mark.parametrize("name", ["p2000", "ragged"])
def test_alpha_is_one_minus_final_t_bit_for_bit(oracle, name):
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    case, _, _ = _case(name)
    H, W, P = case["H"], case["W"], case["sc"]["xyz"].shape[0]
    f = oracle_forward(oracle, case)
    R, color, depth, radii, geom, binning, img = _forward_state(case)
    alpha = _C.alpha_image(img, H, W)
    assert alpha.shape == (1, H, W) and alpha.dtype == torch.float32 and alpha.device == img.device
    st = hip_state(P, R, W, H, geom, binning, img)
    a = alpha.cpu().numpy()
    assert np.array_equal(_bits(a), _bits(np.float32(1.0) - st["final_T"]))
    assert np.array_equal(_bits(a), _bits(np.float32(1.0) - f["final_T"].astype(np.float32)))
    assert 0.0 <= a.min() and a.max() <= 1.0 and ((a > 0.01) & (a < 0.99)).mean() > 0.05
    # ... through the L1 module too, and the image state is left as it was
    _, out = AH.run_hip(case, GA=torch.zeros(1, H, W))
    assert np.array_equal(_bits(out["alpha"]), _bits(a))
    assert np.array_equal(_bits(hip_state(P, R, W, H, geom, binning, img)["final_T"]), _bits(st["final_T"]))


def test_alpha_of_a_view_that_sees_nothing_is_zero():
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    case, _, _ = _case("ragged")
    # (the scene shrunk and moved behind the camera, which looks at the origin from camera_center)
    far = dict(case, sc=dict(case["sc"], xyz=(0.01 * case["sc"]["xyz"] + 3.0 * case["cam"].camera_center[None, :]).contiguous()))
    R, color, depth, radii, geom, binning, img = _forward_state(far)
    assert R == 0 and not bool(radii.any())
    alpha = _C.alpha_image(img, case["H"], case["W"])
    assert alpha.shape == (1, case["H"], case["W"]) and not bool(alpha.any())


def test_alpha_under_no_grad_and_forward_only_state(oracle):
    """A render nothing of which requires a gradient runs with GSR_FLAG_FORWARD_ONLY: K6 still writes final_T."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import _C, GaussianRasterizer

    case, _, _ = _case("p2000")
    sc, H, W = case["sc"], case["H"], case["W"]
    want = np.float32(1.0) - oracle_forward(oracle, case)["final_T"].astype(np.float32)
    with torch.no_grad():
        outs = GaussianRasterizer(settings(case, DEV))(sc["xyz"].to(DEV), torch.zeros(sc["xyz"].shape, device=DEV),
                                                       sc["opacity"].to(DEV), shs=sc["features"].to(DEV),
                                                       scales=sc["scaling"].to(DEV), rotations=sc["rotation"].to(DEV),
                                                       return_alpha=True)
    assert len(outs) == 4 and not outs[3].requires_grad
    assert np.array_equal(_bits(outs[3].cpu().numpy()), _bits(want))
    st = _forward_state(case, flags=options.FLAG_FORWARD_ONLY)
    assert np.array_equal(_bits(_C.alpha_image(st[6], H, W).cpu().numpy()), _bits(want))


def test_alpha_with_aux_colors_is_the_last_of_five(oracle):
    case, G, GA = _case("p2000")
    P = case["sc"]["xyz"].shape[0]
    aux = torch.rand(P, 3, generator=torch.Generator().manual_seed(2))
    want = np.float32(1.0) - oracle_forward(oracle, case)["final_T"].astype(np.float32)
    _, out = AH.run_hip(case, G=G, GA=GA, aux_colors=aux)  # (asserts the arity: 5)
    assert np.array_equal(_bits(out["alpha"]), _bits(want)) and out["aux"].shape == (3, case["H"], case["W"])
    f_aux = oracle_forward(oracle, case, colors_precomp=aux)
    assert np.abs(out["aux"] - f_aux["color"]).max() < 1e-5  # (the auxiliary render wrote no final_T of its own over it)


def test_alpha_of_a_render_served_by_view_reuse(oracle):
    import gaussianeditor_amd
    from gaussianeditor_amd.diff_gaussian_rasterization import _reuse
    from gaussianeditor_amd.gaussian_renderer import render
    from test_gpu_round6 import _PC, _Pipe

    case, G, GA = _case("p2000")
    case = dict(case)
    P, H, W = case["sc"]["xyz"].shape[0], case["H"], case["W"]
    pc = _PC(case["sc"], DEV)
    with torch.no_grad():
        case["sc"] = dict(case["sc"], opacity=pc.get_opacity.cpu().contiguous(), scaling=pc.get_scaling.cpu().contiguous(),
                          rotation=pc.get_rotation.cpu().contiguous())
    cam, bg = case["cam"].to(DEV), case["bg"].to(DEV)
    mask = (torch.rand(P, 1, generator=torch.Generator().manual_seed(1)) > 0.6).float().repeat(1, 3)
    want_a = np.float32(1.0) - oracle_forward(oracle, case)["final_T"].astype(np.float32)
    was = gaussianeditor_amd.get_view_reuse()
    gaussianeditor_amd.set_view_reuse(True)
    _reuse.forget()
    hits = _reuse.stats["hits"]
    try:
        a = render(cam, pc, _Pipe, bg)
        b = render(cam, pc, _Pipe, bg, override_color=mask.to(DEV), return_alpha=True)
        assert _reuse.stats["hits"] == hits + 1 and "alpha" not in a and b["alpha"].shape == (1, H, W)
        assert np.array_equal(_bits(b["alpha"].detach().cpu().numpy()), _bits(want_a))
        ((b["render"] * G.to(DEV)).sum() + (b["alpha"] * GA.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
    finally:
        gaussianeditor_amd.set_view_reuse(was)
        _reuse.forget()
    want, _ = AH.alpha_expectation(oracle, case, G, GA, colors_precomp=mask)
    assert_grads_close(dict(m2=b["viewspace_points"].grad.cpu().numpy(), m3=pc._xyz.grad.cpu().numpy()),
                       dict(m2=want["dL_dmeans2D"], m3=want["dL_dmeans3D"]), tag="reused render: colour + alpha")


# ---------------------------------------------------------------------------------------------------------------------
# backward
def _check(oracle, name, tag, alpha_only=False, with_depth=False, camera=None, **kw):
    case, G, GA = _case(name, camera)
    H, W = case["H"], case["W"]
    G = None if alpha_only else G
    GD = seed_gradient(H, W, 7)[:1] * H * W if with_depth else None
    keys = tuple("dL_dcov3D" if (k == "dL_dscales" and kw.get("cov3D_precomp") is not None) else k for k in AH.SHARE_KEYS)
    want, share = AH.alpha_expectation(oracle, case, G, GA, GD=GD, **kw)
    AH.assert_share_visible(want, share, tag=tag, keys=keys)
    got, out = AH.run_hip(case, G=G, GA=GA, GD=GD, **kw)
    got0 = AH.run_hip(case, G=torch.zeros(3, H, W) if G is None else G, GD=GD, **kw)[0]
    AH.assert_differs_from_colour_only(got, got0, want, tag=tag, keys=keys)
    for k in got:
        print(f"  {tag}: {k} max |got - want| / max = {np.abs(got[k] - want[k].reshape(got[k].shape)).max() / max(np.abs(want[k]).max(), 1e-30):.2e}")
    assert_grads_close(got, want, tag=tag, keys=list(got))
    return got, want


@pytest.mark.parametrize("name", ["p2000", "p20000", "ragged"])
def test_alpha_backward_sh(oracle, name):
    _check(oracle, name, "SH " + name)


def test_alpha_backward_precomputed_colours(oracle):
    cols = torch.rand(2000, 3, generator=torch.Generator().manual_seed(3))
    _check(oracle, "p2000", "colors_precomp", colors_precomp=cols)


def test_alpha_backward_precomputed_covariance(oracle):
    cov = torch.from_numpy(oracle_forward(oracle, _case("p2000")[0])["cov3D"].copy())
    _check(oracle, "p2000", "cov3D_precomp", cov3D_precomp=cov)


def test_alpha_only_loss(oracle):
    got, _ = _check(oracle, "p2000", "alpha only", alpha_only=True)
    assert not np.any(got["dL_dsh"])  # (a zero colour gradient: A does not depend on the colours)


def test_alpha_backward_with_the_depth_loss(oracle):
    """DEPTH + ALPHA: the expectation is depth_expectation plus the alpha share."""
    got, want = _check(oracle, "p2000", "depth + alpha", with_depth=True)
    assert np.abs(want["dL_ddepth"]).max() > 0


@pytest.mark.parametrize("flag", ["FLAG_ANTIALIAS", "FLAG_FAST_EXP"])
def test_alpha_backward_under_a_mode_the_oracle_lacks(flag):
    """The expectation is the linearity construction run on the product's own backwards without the alpha image, under the
    same flag: existing kernels as the yardstick."""
    from gaussianeditor_amd import options

    fl = getattr(options, flag)
    case, G, GA = _case("p2000")
    want, share = AH.product_expectation(case, G, GA, fl)
    AH.assert_share_visible(want, share, tag=flag)
    got, _ = AH.run_hip(case, G=G, GA=GA, flags=fl)
    got0, _ = AH.run_hip(case, G=G, flags=fl)
    AH.assert_differs_from_colour_only(got, got0, want, tag=flag)
    worst = assert_grads_close(got, want, tag=flag, keys=list(got))
    print(f"  {flag}: worst {worst:.2e}")


def test_alpha_backward_with_forced_list_segments():
    """The 20 000-Gaussian case again in a fresh process with the backward cutting every tile's list into segments that start
    from the forward's checkpoints (GSR_BWD_SEG=1, a checkpoint every 256 positions; lists up to 6 319 entries): the
    SEG + ALPHA kernel -- an alpha backward keeps list segments."""
    env = dict(os.environ, GSR_CK_CHUNKS="4", GSR_BWD_SEG="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "test_alpha_backward_sh and p20000"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "1 passed" in p.stdout, p.stdout[-2000:]
    print(p.stdout[-900:])


# ---------------------------------------------------------------------------------------------------------------------
# absgrad under alpha, and what an alpha backward leaves behind
def _one_pixel(oracle, case):
    """The mask of ONE pixel: the half-transparent one (final_T of the oracle nearest 0.5), where dA/dalpha = final_T /
    (1 - alpha) is neither negligible nor everything."""
    H, W = case["H"], case["W"]
    p = int(np.abs(oracle_forward(oracle, case)["final_T"].reshape(-1).astype(np.float64) - 0.5).argmin())
    m = torch.zeros(1, H, W)
    m[0, p // W, p % W] = 1.0
    return m


def test_absgrad_under_alpha(oracle):
    case, G, GA = _case("p2000")
    m = _one_pixel(oracle, case)
    # one pixel with gC and gA non-zero: every Gaussian has one term, absgrad == |grad| -- alpha's share included (the sums
    # differ from the colour-only ones by more than ten bars, as the gradients must: discrimination condition (ii))
    g1, o1 = AH.run_hip(case, G=G * m, GA=GA * m, abs_grad=True)
    g1c, o1c = AH.run_hip(case, G=G * m, abs_grad=True)
    s = np.abs(g1["dL_dmeans2D"][:, :2])
    print(f"  one pixel: rows {(s.max(axis=1) > 0).sum()}, max |absgrad - colour-only absgrad| / max = "
          f"{np.abs(o1['absgrad'] - o1c['absgrad']).max() / s.max():.2e}")
    assert (s.max(axis=1) > 0).sum() > 0 and np.abs(o1["absgrad"] - o1c["absgrad"]).max() > 10 * 1e-5 * s.max()
    assert_grads_close(dict(absgrad=o1["absgrad"][:, :2]), dict(absgrad=s), tag="one pixel: absgrad == |grad|")
    # full gradient: dominance, and the signed gradients are the expectation
    want, _ = AH.alpha_expectation(oracle, case, G, GA)
    g, o = AH.run_hip(case, G=G, GA=GA, abs_grad=True)
    assert_grads_close(g, want, tag="ABS + ALPHA: signed gradients", keys=list(g))
    a, sg = o["absgrad"][:, :2].astype(np.float64), np.abs(g["dL_dmeans2D"][:, :2].astype(np.float64))
    assert (o["absgrad"][:, 2] == 0).all() and (sg - a).max() <= 1e-5 * a.max() and (a - sg).max() > 1e-3 * a.max()


def test_an_alpha_backward_leaves_the_tables_zero_and_plain_backwards_unchanged(oracle):
    """The one-pixel gradient makes a backward deterministic (every accumulator cell receives at most one add), so bit
    identity is a meaningful demand (tests/test_gpu_abs_grad.py)."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    case, G, GA = _case("p20000")
    m = _one_pixel(oracle, case)
    before, _ = AH.run_hip(case, G=G * m)
    AH.run_hip(case, G=G, GA=GA)
    AH.run_hip(case, G=G, GA=GA, GD=GA, abs_grad=True)
    torch.cuda.synchronize()
    assert _C._ACC_TABLES, "the persistent accumulator table is not in use"
    assert all(not bool(t.any()) for t in _C._ACC_TABLES.values())
    after, _ = AH.run_hip(case, G=G * m)
    for k in before:
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), (k, "not bit-identical")
