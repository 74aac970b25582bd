"""-m gpu: the depth-distortion image and its gradient (`return_distortion`; gsr_blend_forward_distortion,
gsr_blend_backward_distortion) against the float64 yardstick of distortion_helpers, at f64_regimes.TOL with the per-row rule.

Measured on the MI355X (worst tensor-wide error of each case next to the bar 2e-5): see DESIGN.md section 27."""
import numpy as np
import pytest
import torch

import distortion_helpers as DH
from helpers import assert_grads_close, hip_state, settings

pytestmark = pytest.mark.gpu
DEV = DH.DEV
TOL = DH.TOL


def _one_pixel(case, f):
    """(1,H,W) mask of ONE pixel, the half-transparent one (final_T of the oracle nearest 0.5): under a colour gradient on that
    pixel alone every accumulator cell receives at most one add, so bit identity of two backwards is a meaningful demand (the
    order of float atomics is not fixed)."""
    H, W = case["H"], case["W"]
    p = int(np.abs(f["final_T"].reshape(-1).astype(np.float64) - 0.5).argmin())
    m = torch.zeros(1, H, W)
    m[0, p // W, p % W] = 1.0
    return m


def _check_image(got, want, tag):
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64).reshape(want.shape) - want).max()) / scale
    print(f"  {tag}: image error {err:.2e} of {scale:.3e} (bar {TOL:.0e})")
    assert err <= TOL, (tag, err)
    return err


@pytest.mark.parametrize("name,near_far", [("partial", None), ("p2000", None), ("ragged", None), ("p4000", None), ("far_slab", None),
                                           ("p2000", DH.NEAR_FAR), ("far_slab", DH.NEAR_FAR)])
def test_image_and_gradients_equal_float64(name, near_far):
    case, f, e, masked = DH.expectation(name, near_far=near_far, colour=True)  # <G, C> + lam <GDist, D>
    assert int(masked.sum()) == 0
    got, outs = DH.run_hip(case, GDist=e["lam"] * DH.weights(case), G=DH.colour_weights(case), near_far=near_far)
    tag = f"distortion [{name}{'' if near_far is None else ', mapped'}]"
    assert np.array_equal(outs["radii"], f["radii"])
    _check_image(outs["distortion"], e["image"], tag)
    DH.assert_share_visible(e, tag)
    assert all(np.isfinite(v).all() for v in got.values())
    worst = assert_grads_close(got, e["want"], tol=TOL, tag=tag, masked=masked, keys=DH.KEYS)
    print(f"  {tag}: worst gradient error {worst:.2e} (bar {TOL:.0e}), lam {e['lam']:.0e}")
    # the colours get no share: dL_dsh is the colour loss's alone
    assert_grads_close(got, e["colour_only"], tol=TOL, tag=tag + " dL_dsh", masked=masked, keys=["dL_dsh"])
    # ... and the distortion loss alone leaves it exactly zero
    alone, _ = DH.run_hip(case, GDist=DH.weights(case), near_far=near_far)
    assert not np.any(alone["dL_dsh"] != 0)


def test_pixels_with_one_contributor_and_empty_pixels_are_exactly_zero():
    case, f, e, masked = DH.expectation("single")
    got, outs = DH.run_hip(case, GDist=DH.weights(case))
    nc = e["stats"]["n_contrib"].numpy().reshape(case["H"], case["W"])
    img = outs["distortion"][0]
    assert np.array_equal(nc, f["n_contrib"].reshape(nc.shape).astype(np.int64))
    assert (nc == 1).sum() > 20 and np.all(img[nc <= 1] == 0.0) and (img > 0).sum() >= 4
    _check_image(outs["distortion"], e["image"], "distortion [single]")
    assert_grads_close(got, e["want"], tol=TOL, tag="distortion [single]", masked=masked, keys=DH.KEYS)
    # Gaussians 0 .. 2 are alone under every pixel they reach: no gradient at all
    for k in DH.KEYS:
        assert not np.any(got[k][:3] != 0), k


def test_empty_view_and_empty_scene_give_exact_zeros():
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    case = DH.get_case("p2000")
    # the scene behind the camera: nothing is rendered (R = 0)
    sc = dict(case["sc"])
    cam_pos = case["cam"].camera_center
    sc["xyz"] = (2.0 * cam_pos[None, :] - sc["xyz"]).contiguous()
    got, outs = DH.run_hip(dict(case, sc=sc), GDist=DH.weights(case))
    assert not np.any(outs["radii"] > 0) and not np.any(outs["distortion"] != 0)
    assert all(not np.any(v != 0) for v in got.values())
    # P = 0
    rs = settings(case, DEV)
    z = lambda *s: torch.zeros(*s, device=DEV, requires_grad=True)  # noqa: E731
    xyz = z(0, 3)
    outs = GaussianRasterizer(rs)(xyz, z(0, 3), z(0, 1), shs=z(0, 0, 3), scales=z(0, 3), rotations=z(0, 4), return_distortion=True)
    assert len(outs) == 4 and outs[-1].shape == (1, case["H"], case["W"]) and not bool(outs[-1].any())
    (outs[-1].sum() + outs[0].sum()).backward()
    assert xyz.grad is None or xyz.grad.numel() == 0


def test_no_grad_render_is_forward_only_and_equal():
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    case, f, e, masked = DH.expectation("ragged")
    sc = case["sc"]
    with torch.no_grad():
        outs = GaussianRasterizer(settings(case, DEV))(sc["xyz"].to(DEV), None, sc["opacity"].to(DEV), shs=sc["features"].to(DEV),
                                                       scales=sc["scaling"].to(DEV), rotations=sc["rotation"].to(DEV),
                                                       return_distortion=True)
    assert len(outs) == 4 and not outs[-1].requires_grad
    _, ref = DH.run_hip(case, GDist=DH.weights(case))
    assert np.array_equal(outs[-1].cpu().numpy(), ref["distortion"])


def _composition(case, f, flags, GDist, near_far=None):
    """The product's own composition under `flags`: features = [m - c, (m - c)^2] + the alpha image, D = A M2 - M1^2 formed in
    float64 from the three float32 images, autograd through the feature and alpha routes; dL/dfeatures chained to the depth by
    hand, as the yardstick does.  c = the median depth: the composition's own cancellation stays near 1e-6 of D on these
    scenes (depth spread of order 1 around c), well inside the bar."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    sc = case["sc"]
    z = f["depths"].astype(np.float64)
    m, mu = DH.mapped(z, near_far)
    c = float(np.median(m[f["radii"] > 0]))
    feats = torch.from_numpy(np.stack([m - c, (m - c) ** 2], axis=1)).float().to(DEV).requires_grad_(True)
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)  # noqa: E731
    lv = dict(dL_dmeans3D=leaf(sc["xyz"]), dL_dopacity=leaf(sc["opacity"]), dL_dscales=leaf(sc["scaling"]),
              dL_drotations=leaf(sc["rotation"]))
    m2d = lv["dL_dmeans2D"] = torch.zeros_like(lv["dL_dmeans3D"], requires_grad=True)
    with options.override(flags):
        outs = GaussianRasterizer(settings(case, DEV))(lv["dL_dmeans3D"], m2d, lv["dL_dopacity"], shs=sc["features"].to(DEV),
                                                       scales=lv["dL_dscales"], rotations=lv["dL_drotations"],
                                                       return_alpha=True, features=feats)
    A, F = outs[-2].double()[0], outs[-1].double()
    D = A * F[1] - F[0] * F[0]
    (D * GDist.to(DEV).double()[0]).sum().backward()
    torch.cuda.synchronize()
    want = {k: v.grad.cpu().numpy().astype(np.float64) for k, v in lv.items()}
    df = feats.grad.cpu().numpy().astype(np.float64)
    dz = mu * (df[:, 0] + 2.0 * (m - c) * df[:, 1])
    Vz = case["cam"].world_view_transform.double().reshape(4, 4)[:3, 2].numpy()
    want["dL_dmeans3D"] = want["dL_dmeans3D"] + dz[:, None] * Vz[None, :]
    return D.detach().cpu().numpy(), want


@pytest.mark.parametrize("flag", ["FLAG_FAST_EXP", "FLAG_ANTIALIAS", "FLAG_TILE_BOUNDS_ALPHA"])
def test_flags_against_the_products_own_composition(flag):
    from gaussianeditor_amd import options

    flags = getattr(options, flag)
    case, f, e, masked = DH.expectation("p2000", colour=True)
    G, GDist = DH.colour_weights(case), e["lam"] * DH.weights(case)
    img, share = _composition(case, f, flags, GDist)
    rest, _ = DH.run_hip(case, G=G, flags=flags, return_distortion=False)  # the product's own colour backward under the flag
    want = {k: rest[k].astype(np.float64) + share[k] for k in DH.KEYS}
    got, outs = DH.run_hip(case, GDist=GDist, G=G, flags=flags)
    _check_image(outs["distortion"], img, f"distortion [{flag}] vs composition")
    DH.assert_share_visible(dict(share=share, want=want), f"distortion [{flag}]")
    keys = [k for k in DH.KEYS]
    worst = assert_grads_close(got, want, tol=TOL, tag=f"distortion [{flag}] vs composition", keys=keys)
    print(f"  [{flag}] worst gradient error against the composition {worst:.2e} (bar {TOL:.0e})")
    if flag != "FLAG_TILE_BOUNDS_ALPHA":  # (the bounds change which tiles list a Gaussian, never a pixel's blended entries)
        base, _ = DH.run_hip(case, GDist=GDist, G=G)
        assert any(np.any(base[k] != got[k]) for k in keys), "the flag changed nothing: the comparison shows nothing"


def test_together_with_colour_depth_alpha_and_feature_losses_in_one_backward():
    import features_helpers as FH
    from helpers import seed_gradient

    case, f, e, masked = DH.expectation("ragged")
    H, W, P = case["H"], case["W"], case["sc"]["xyz"].shape[0]
    G, GDist = DH.colour_weights(case), DH.weights(case)
    GD, GA = seed_gradient(H, W, 11)[:1] * H * W, seed_gradient(H, W, 12)[:1] * H * W
    feats, GF = FH.make_features(P, 5), FH.feature_gradient(H, W, 5)
    rest, o0 = DH.run_hip(case, G=G, GD=GD, GA=GA, feats=feats, GF=GF, return_distortion=False)  # the product without the image
    got, o1 = DH.run_hip(case, GDist=GDist, G=G, GD=GD, GA=GA, feats=feats, GF=GF)
    for k in ("color", "depth", "radii"):
        assert np.array_equal(o0[k], o1[k]), k
    want = {k: rest[k].astype(np.float64) + e["share"][k] for k in DH.KEYS}
    DH.assert_share_visible(dict(share=e["share"], want=want), "all losses [ragged]")
    worst = assert_grads_close(got, want, tol=TOL, tag="all losses [ragged]", masked=masked, keys=DH.KEYS)
    print(f"  all losses [ragged]: worst gradient error {worst:.2e} (bar {TOL:.0e})")
    # the colours and the features get no share (two backwards differ by the order of their float adds alone)
    assert_grads_close(got, rest, tol=TOL, tag="all losses [ragged], no share", keys=["dL_dsh", "dL_dfeatures"])


def test_pose_gradient_is_the_sum_of_the_products_own_shares():
    case, f, e, masked = DH.expectation("p2000", colour=True)
    G, GDist = DH.colour_weights(case), e["lam"] * DH.weights(case)
    _, a = DH.run_hip(case, G=G, pose=True, return_distortion=False)
    gb, b = DH.run_hip(case, GDist=GDist, pose=True)
    gc, c = DH.run_hip(case, GDist=GDist, G=G, pose=True)
    DH.assert_share_visible(e, "distortion with POSE_GRAD")
    assert_grads_close(gb, e["share"], tol=TOL, tag="distortion alone with POSE_GRAD", masked=masked, keys=DH.KEYS)
    assert_grads_close(gc, e["want"], tol=TOL, tag="colour + distortion with POSE_GRAD", masked=masked, keys=DH.KEYS)
    for k in ("view", "proj", "campos"):
        want = a["pose"][k].astype(np.float64) + b["pose"][k].astype(np.float64)
        scale = max(float(np.abs(want).max()), float(np.abs(a["pose"][k]).max()), float(np.abs(b["pose"][k]).max()))
        err = float(np.abs(c["pose"][k] - want).max()) / scale
        print(f"  pose {k}: both losses against the sum of the shares {err:.2e}; distortion share "
              f"{float(np.abs(b['pose'][k]).max()) / scale:.2e} of the scale")
        assert err <= TOL, (k, err)
    for k in ("view", "proj"):  # (campos reaches the image through the SH colours alone: the distortion image has no share)
        assert np.abs(b["pose"][k]).max() > 10 * TOL * np.abs(c["pose"][k]).max(), k
    assert not np.any(b["pose"]["campos"] != 0)


def test_absgrad_is_what_it_is_without_the_distortion_loss():
    case, f, e, masked = DH.expectation("p2000")
    G, GDist = DH.colour_weights(case) * _one_pixel(case, f), DH.weights(case)  # (one pixel: see _one_pixel)
    g0, o0 = DH.run_hip(case, G=G, abs_grad=True, return_distortion=False)
    g1, o1 = DH.run_hip(case, G=G, GDist=GDist, abs_grad=True)
    assert o0["absgrad"] is not None and np.abs(o0["absgrad"]).max() > 0
    assert np.array_equal(o0["absgrad"], o1["absgrad"])
    assert np.any(g0["dL_dmeans2D"] != g1["dL_dmeans2D"])
    want = {k: g0[k].astype(np.float64) + e["share"][k] for k in DH.KEYS}
    DH.assert_share_visible(dict(share=e["share"], want=want), "distortion with ABS_GRAD")
    assert_grads_close(g1, want, tol=TOL, tag="distortion with ABS_GRAD", masked=masked, keys=DH.KEYS)


def test_state_outputs_and_the_accumulator_table_are_left_as_they_were():
    """final_T, n_contrib, colour, depth and radii are untouched by the forward; after the backwards the persistent accumulator
    table is all zero, and a plain backward is bit-identical to one taken before."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    case, f, _, _ = DH.expectation("ragged")
    sc, H, W = case["sc"], case["H"], case["W"]
    P = sc["xyz"].shape[0]
    G = DH.colour_weights(case) * _one_pixel(case, f)  # (one pixel: see _one_pixel)
    plain0, o0 = DH.run_hip(case, G=G, return_distortion=False)
    rs = settings(case, DEV)
    e = torch.empty(0, device=DEV)
    t = lambda k: sc[k].to(DEV)  # noqa: E731
    R_, color, depth, radii, geom, binning, img = _C.rasterize_gaussians(
        rs.bg, t("xyz"), e, t("opacity"), t("scaling"), t("rotation"), 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
        rs.tanfovy, H, W, t("features"), case["D"], rs.campos, False, False)
    before = hip_state(P, R_, W, H, geom, binning, img)
    c0, d0 = color.clone(), depth.clone()
    dist, moments = _C.rasterize_distortion(P, R_, geom, binning, img, H, W)
    dist2, none = _C.rasterize_distortion(P, R_, geom, binning, img, H, W, near_far=DH.NEAR_FAR, with_moments=False)
    assert none is None and moments.shape == (H, W, 4)
    after = hip_state(P, R_, W, H, geom, binning, img)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert torch.equal(color, c0) and torch.equal(depth, d0)
    mom = moments.cpu().numpy().astype(np.float64)
    nc = after["n_contrib"].reshape(H, W)
    assert np.all(mom[nc == 0] == 0) and np.all(mom[..., 1][nc > 0] > 0)  # (z0, A, M1', M2') = 0 where nothing is blended
    DH.run_hip(case, G=DH.colour_weights(case), GDist=DH.weights(case))
    DH.run_hip(case, GDist=DH.weights(case), near_far=DH.NEAR_FAR)
    torch.cuda.synchronize()
    assert _C._ACC_TABLES, "the persistent accumulator table was not returned"
    for table in _C._ACC_TABLES.values():
        assert not bool(table.any()), "the persistent accumulator table is not all zero after a distortion backward"
    plain1, o1 = DH.run_hip(case, G=G, return_distortion=False)
    for k in plain0:
        assert np.array_equal(plain0[k], plain1[k]), k
    for k in ("color", "depth", "radii"):
        assert np.array_equal(o0[k], o1[k]), k
