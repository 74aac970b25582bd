"""-m gpu: the feature image (`features=`: per-Gaussian feature vectors of C channels composited into a (C,H,W) image;
include/gsr.h gsr_blend_forward_features, gsr_blend_backward_features) and its gradient.

Forward: equal as floats, channel by channel, to the product's auxiliary render of the three-channel slices on background 0
and to the CPU oracle.  Backward: against the slice construction of features_helpers (held to float64 autograd by
tests/test_cpu_features.py) at the project's bar of 1e-5 -- the tensor bar and the per-row rule, the scale the larger of the
total's maximum and the largest single slice share's maximum -- with the discrimination conditions asserted: (i) the feature
share exceeds 1e-2 of the total's maximum on >= 100 rows of every SHARE_KEYS tensor, (ii) the gradients differ from the
colour-only ones by more than ten bars.  Shapes: the four of features_helpers.CASES (64 x 64 C = 7, 70 x 45 C = 16 -- a full
block and a ragged edge --, 48 x 48 C = 1, 40 x 24 C = 33 -- two full blocks and a one-channel one).
Measured on the MI355X: every gradient within 6.2e-7 of its scale (bar 1e-5), the camera gradient within 2.2e-7 (bars 2e-5),
the forward bit-identical everywhere; the whole file in 4 s."""
import numpy as np
import pytest
import torch

import features_helpers as FH
import f64_regimes as R
from helpers import hip_state, make_case, oracle_forward, seed_gradient, settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def _forward_state(case, flags=0, sm=1.0):
    """_C.rasterize_gaussians of the case -> (R, color, depth, radii, geom, binning, img), on the device."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    sc, rs = case["sc"], settings(case, DEV)
    e = torch.empty(0, device=DEV)
    t = lambda k: sc[k].to(DEV)  # noqa: E731
    return _C.rasterize_gaussians(rs.bg, t("xyz"), e, t("opacity"), t("scaling"), t("rotation"), sm, e, rs.viewmatrix,
                                  rs.projmatrix, rs.tanfovx, rs.tanfovy, case["H"], case["W"], t("features"), case["D"], rs.campos,
                                  False, False, flags=flags)


def _aux_slices(state, feats, H, W, flags=0):
    """(C,H,W): the product's own auxiliary renders of the three-channel slices on background 0."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    R_, _, _, _, geom, binning, img = state
    out = np.zeros((feats.shape[1], H, W), np.float32)
    bg0 = torch.zeros(3, device=DEV)
    for k, n, cols, _ in FH.slices(feats):
        out[3 * k:3 * k + n] = _C.rasterize_gaussians_aux(bg0, cols.to(DEV), R_, geom, binning, img, H, W, flags=flags).cpu().numpy()[:n]
    return out


def _features(state, feats, H, W, flags=0):
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    R_, _, _, _, geom, binning, img = state
    out = _C.rasterize_features(feats.to(DEV), R_, geom, binning, img, H, W, flags=flags)
    assert out.shape == (feats.shape[1], H, W) and out.dtype == torch.float32 and out.is_contiguous()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# forward
@pytest.mark.parametrize("name", list(FH.CASES))
def test_feature_image_equals_the_slice_renders_as_floats(oracle, name):
    case, _, _, feats = FH.feature_case(name)
    H, W, P = case["H"], case["W"], feats.shape[0]
    st = _forward_state(case)
    before = hip_state(P, st[0], W, H, st[4], st[5], st[6])
    got = _features(st, feats, H, W)
    aux = _aux_slices(st, feats, H, W)
    assert np.array_equal(_bits(got), _bits(aux)), np.abs(got - aux).max()
    assert np.array_equal(_bits(got), _bits(FH.oracle_feature_image(oracle, case, feats)))
    assert np.abs(got).max() > 0.1
    after = hip_state(P, st[0], W, H, st[4], st[5], st[6])
    assert np.array_equal(before["n_contrib"], after["n_contrib"]) and np.array_equal(_bits(before["final_T"]), _bits(after["final_T"]))


@pytest.mark.parametrize("C", [1, 7, 16, 33])
def test_feature_image_channel_counts_on_a_tiny_ragged_image(C):
    """17 x 9: two tiles, both partial in x or y; every channel count on it."""
    case = make_case(300, 17, 9, s0=0.1)
    feats = FH.make_features(300, C, seed=C)
    st = _forward_state(case)
    got = _features(st, feats, 9, 17)
    assert np.array_equal(_bits(got), _bits(_aux_slices(st, feats, 9, 17))) and np.abs(got).max() > 0.05


def test_feature_image_with_the_largest_channel_count():
    case, _, _, _ = FH.feature_case("p600")
    feats = FH.make_features(600, 256, seed=256)
    st = _forward_state(case)
    got = _features(st, feats, case["H"], case["W"])
    assert np.array_equal(_bits(got), _bits(_aux_slices(st, feats, case["H"], case["W"])))
    assert all(np.abs(got[c]).max() > 0.05 for c in range(256))


def test_feature_image_where_pixels_stop_early(oracle):
    """The `saturated` regime of f64_regimes: opacities near 1, a pixel stops after two entries (T < 1e-4)."""
    case = R.regime("saturated")["case"]
    feats = FH.make_features(case["sc"]["xyz"].shape[0], 7, seed=3)
    st = _forward_state(case)
    got = _features(st, feats, case["H"], case["W"])
    assert np.array_equal(_bits(got), _bits(_aux_slices(st, feats, case["H"], case["W"])))
    assert np.array_equal(_bits(got), _bits(FH.oracle_feature_image(oracle, case, feats)))


def test_feature_image_of_an_empty_view_and_of_no_gaussians():
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    case, _, _, feats = FH.feature_case("ragged")
    H, W = case["H"], case["W"]
    far = dict(case, sc=dict(case["sc"], xyz=(0.01 * case["sc"]["xyz"] + 3.0 * case["cam"].camera_center[None, :]).contiguous()))
    st = _forward_state(far)
    assert st[0] == 0
    got = _features(st, feats, H, W)
    assert got.shape == (16, H, W) and not np.any(got)
    g, o = FH.run_hip(far, GF=FH.feature_gradient(H, W, 16), feats=feats)  # (the backward of nothing: zeros everywhere)
    assert not np.any(o["features"]) and all(not np.any(v) for v in g.values())
    e = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    outs = GaussianRasterizer(settings(case, DEV))(e(0, 3), e(0, 3), e(0, 1), shs=e(0, 16, 3), scales=e(0, 3), rotations=e(0, 4),
                                                   features=e(0, 5))
    assert len(outs) == 4 and outs[3].shape == (5, H, W) and not bool(outs[3].any())


def test_feature_image_under_no_grad_with_aux_and_alpha(oracle):
    """Arity with everything asked for, the forward-only state of a render under no_grad, and: colour, depth and radii of a
    render with `features=` are bit-identical to those of one without."""
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    case, G, GF, feats = FH.feature_case("p2000")
    sc, H, W = case["sc"], case["H"], case["W"]
    want = FH.oracle_feature_image(oracle, case, feats)
    aux = torch.rand(feats.shape[0], 3, generator=torch.Generator().manual_seed(2))
    args = (sc["xyz"].to(DEV), torch.zeros(sc["xyz"].shape, device=DEV), sc["opacity"].to(DEV))
    kw = dict(shs=sc["features"].to(DEV), scales=sc["scaling"].to(DEV), rotations=sc["rotation"].to(DEV))
    with torch.no_grad():
        plain = GaussianRasterizer(settings(case, DEV))(*args, **kw)
        outs = GaussianRasterizer(settings(case, DEV))(*args, **kw, features=feats.to(DEV))
        full = GaussianRasterizer(settings(case, DEV))(*args, **kw, features=feats.to(DEV), aux_colors=aux.to(DEV), return_alpha=True)
    assert len(plain) == 3 and len(outs) == 4 and len(full) == 6 and not outs[3].requires_grad
    assert np.array_equal(_bits(outs[3].cpu().numpy()), _bits(want)) and np.array_equal(_bits(full[5].cpu().numpy()), _bits(want))
    assert full[3].shape == (3, H, W) and full[4].shape == (1, H, W)
    for a, b in zip(plain, outs[:3]):
        assert torch.equal(a, b)
    for a, b in zip(plain, full[:3]):
        assert torch.equal(a, b)
    # ... and through a render that takes gradients
    _, o = FH.run_hip(case, G=G, GF=GF, feats=feats, aux_colors=aux, GA=seed_gradient(H, W, 5)[:1])
    assert np.array_equal(_bits(o["features"]), _bits(want)) and np.array_equal(_bits(o["color"]), _bits(plain[0].cpu().numpy()))
    assert np.array_equal(o["radii"], plain[1].cpu().numpy()) and np.array_equal(_bits(o["depth"]), _bits(plain[2].cpu().numpy()))


@pytest.mark.parametrize("flag", ["FLAG_FAST_EXP", "FLAG_ANTIALIAS"])
def test_feature_image_under_a_mode_the_oracle_lacks(flag):
    from gaussianeditor_amd import options

    fl = getattr(options, flag)
    case, _, _, feats = FH.feature_case("ragged")
    st, st0 = _forward_state(case, flags=fl), _forward_state(case)
    got = _features(st, feats, case["H"], case["W"], flags=fl)
    assert np.array_equal(_bits(got), _bits(_aux_slices(st, feats, case["H"], case["W"], flags=fl)))
    assert not np.array_equal(_bits(got), _bits(_features(st0, feats, case["H"], case["W"])))  # (the mode is really on)


def test_a_skipped_entrys_features_never_enter_a_pixels_sum(oracle):
    """The accumulation is a masked region, not 0 * f: a Gaussian whose features are all NaN makes NaN exactly the pixels that
    blend it (the CPU oracle's set), and every other pixel -- most of the entry's quadrant evaluates it and skips it -- is
    bit-equal to the render with that row zeroed."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _reuse

    case, feats, row = FH.small_gaussian_case(C=5)
    blends = FH.oracle_blend_mask(oracle, case, row)
    assert 0 < int(blends.sum()) < 64 and not blends[8:, :].any() and not blends[:, 8:].any()  # (inside its 8 x 8 quadrant)
    nan_feats, zero_feats = feats.clone(), feats.clone()
    nan_feats[row] = float("nan")
    zero_feats[row] = 0.0
    hits = _reuse.stats["hits"]
    got = FH.run_hip(case, feats=nan_feats)[1]["features"]
    ref = FH.run_hip(case, feats=zero_feats)[1]["features"]
    assert _reuse.stats["hits"] == hits  # (neither render was served by view reuse)
    assert got.shape == ref.shape == (5, 16, 16) and not np.isnan(ref).any() and np.abs(ref).max() > 0.05
    for c in range(5):
        assert np.array_equal(np.isnan(got[c]), blends), c
    assert np.array_equal(_bits(got[:, ~blends]), _bits(ref[:, ~blends]))


# ---------------------------------------------------------------------------------------------------------------------
# backward
def _check(oracle, name, tag, colour=True, depth=False, alpha=False, camera=None, **kw):
    case, G, GF, feats = FH.feature_case(name, camera=camera)
    H, W = case["H"], case["W"]
    G = G if colour else None
    GD = seed_gradient(H, W, 81)[:1] * H * W if depth else None
    GA = seed_gradient(H, W, 5)[:1] * H * W if alpha else None
    keys = tuple("dL_dcov3D" if (k == "dL_dscales" and kw.get("cov3D_precomp") is not None) else k for k in FH.SHARE_KEYS)
    want, share, dfeat, smax = FH.feature_expectation(oracle, case, G, GF, feats, GD=GD, GA=GA, **kw)
    FH.assert_share_visible(want, share, tag=tag, keys=keys)
    got, out = FH.run_hip(case, G=G, GF=GF, feats=feats, GD=GD, GA=GA, **kw)
    got0, _ = FH.run_hip(case, G=torch.zeros(3, H, W) if G is None else G, feats=feats, GD=GD, GA=GA, **kw)
    FH.assert_differs_from_colour_only(got, got0, want, tag=tag, keys=keys)
    assert not np.any(got0["dL_dfeatures"])
    want = dict(want, dL_dfeatures=dfeat)
    worst = FH.assert_feature_grads_close(got, want, smax, tol=BAR, tag=tag, keys=list(got))
    # Gaussians no pixel blends: their feature gradient is exactly zero
    never = ~np.any(dfeat != 0, axis=1)
    assert not np.any(got["dL_dfeatures"][never]), tag
    assert never.sum() > 0 or name != "p2000"  # (the case that has such Gaussians; p600 has none)
    print(f"  {tag}: worst {worst:.2e}; rows never blended {int(never.sum())} of {never.size}")
    return got, want


def test_feature_backward_features_only(oracle):
    got, _ = _check(oracle, "p2000", "features only C=7", colour=False)
    assert not np.any(got["dL_dsh"])  # (a zero colour gradient: the feature image does not depend on the colours)


@pytest.mark.parametrize("name", ["ragged", "p600", "p4000"])
def test_feature_backward_with_the_colour_loss(oracle, name):
    _check(oracle, name, f"features + colour, {name} C={FH.CASES[name]['C']}")


def test_feature_backward_with_the_depth_and_alpha_losses(oracle):
    got, want = _check(oracle, "p2000", "features + colour + depth + alpha", depth=True, alpha=True)
    assert np.abs(want["dL_dmeans3D"]).max() > 0 and not np.array_equal(got["dL_dsh"], np.zeros_like(got["dL_dsh"]))


def test_feature_backward_precomputed_covariance(oracle):
    cov = torch.from_numpy(oracle_forward(oracle, FH.feature_case("p2000")[0])["cov3D"].copy())
    _check(oracle, "p2000", "features, cov3D_precomp", cov3D_precomp=cov)


@pytest.mark.parametrize("mode", ["FLAG_ANTIALIAS", "FLAG_FAST_EXP", "alpha_bounds"])
def test_feature_backward_under_a_mode_the_oracle_lacks(mode):
    """The expectation is the slice construction run on the product's own three-channel backwards under the same flag."""
    from gaussianeditor_amd import options

    fl = options.FLAG_TILE_BOUNDS_ALPHA if mode == "alpha_bounds" else getattr(options, mode)
    case, G, GF, feats = FH.feature_case("p2000")
    want, share, dfeat, smax, _ = FH.product_expectation(case, G, GF, feats, fl)
    FH.assert_share_visible(want, share, tag=mode)
    got, _ = FH.run_hip(case, G=G, GF=GF, feats=feats, flags=fl)
    got0, _ = FH.run_hip(case, G=G, flags=fl)
    FH.assert_differs_from_colour_only(got, got0, want, tag=mode)
    worst = FH.assert_feature_grads_close(got, dict(want, dL_dfeatures=dfeat), smax, tol=BAR, tag=mode, keys=list(got))
    print(f"  {mode}: worst {worst:.2e}")


def test_absgrad_is_what_it_is_without_the_feature_loss(oracle):
    """FLAG_ABS_GRAD: the eight gradients hold the feature share, `absgrad` does not -- bit-identical to that of the same step
    without the feature loss (a one-pixel colour gradient: every accumulator cell receives at most one add, so bit identity
    is a meaningful demand)."""
    from test_gpu_alpha import _one_pixel

    case, G, GF, feats = FH.feature_case("p2000")
    m = _one_pixel(oracle, case)
    g1, o1 = FH.run_hip(case, G=G * m, GF=GF, feats=feats, abs_grad=True)
    g0, o0 = FH.run_hip(case, G=G * m, feats=feats, abs_grad=True)
    assert o1["absgrad"] is not None and np.abs(o1["absgrad"]).max() > 0
    assert np.array_equal(_bits(o1["absgrad"]), _bits(o0["absgrad"]))
    want, share, dfeat, smax = FH.feature_expectation(oracle, case, G * m, GF, feats)
    FH.assert_differs_from_colour_only(g1, g0, want, tag="ABS")
    FH.assert_feature_grads_close(g1, dict(want, dL_dfeatures=dfeat), smax, tol=BAR, tag="ABS + features", keys=list(g1))


def test_pose_gradient_holds_the_feature_share():
    """FLAG_POSE_GRAD: the 35 camera floats == the sum of the product's own camera gradients of the colour render and of the
    slice renders, at the camera gradient's bars (tools/pose_bars.py, tests/pose_helpers.py)."""
    import pose_helpers as PH

    case, G, GF, feats = FH.feature_case("p2000")
    want_g, share, dfeat, smax, psum = FH.product_expectation(case, G, GF, feats, 0, pose=True)
    got, o = FH.run_hip(case, G=G, GF=GF, feats=feats, pose=True)
    _, o0 = FH.run_hip(case, G=G, pose=True)
    as4 = lambda d: dict(view=np.asarray(d["view"]).reshape(4, 4), proj=np.asarray(d["proj"]).reshape(4, 4),  # noqa: E731
                         campos=np.asarray(d["campos"]).reshape(3))
    PH.assert_pose_close(as4(o["pose"]), as4(psum), "pose + features")
    for k in ("view", "proj"):  # (the share is visible: more than ten bars away from the colour-only camera gradient)
        assert np.abs(o["pose"][k] - o0["pose"][k]).max() > 10 * R.TOL * np.abs(psum[k]).max(), k
    FH.assert_feature_grads_close(got, dict(want_g, dL_dfeatures=dfeat), smax, tol=BAR, tag="pose + features", keys=list(got))


# ---------------------------------------------------------------------------------------------------------------------
# state
def test_a_feature_backward_leaves_the_table_zero_and_plain_backwards_unchanged(oracle):
    from gaussianeditor_amd.diff_gaussian_rasterization import _C
    from test_gpu_alpha import _one_pixel

    case, G, GF, feats = FH.feature_case("p2000")
    m = _one_pixel(oracle, case)
    before, _ = FH.run_hip(case, G=G * m)
    a, _ = FH.run_hip(case, G=G, GF=GF, feats=feats)
    b, _ = FH.run_hip(case, G=G, GF=GF, feats=feats)
    FH.run_hip(case, GF=GF, feats=feats, GD=seed_gradient(case["H"], case["W"], 81)[:1], abs_grad=True)
    torch.cuda.synchronize()
    assert _C._ACC_TABLES, "the persistent accumulator table is not in use"
    assert all(not bool(t.any()) for t in _C._ACC_TABLES.values())
    after, _ = FH.run_hip(case, G=G * m)
    for k in before:
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), (k, "not bit-identical")
    # two feature backwards in a row: equal up to the order of the float adds, both inside the bar
    want, _, dfeat, smax = FH.feature_expectation(oracle, case, G, GF, feats)
    want = dict(want, dL_dfeatures=dfeat)
    for g in (a, b):
        FH.assert_feature_grads_close(g, want, smax, tol=BAR, tag="repeated", keys=list(g))
    for k in a:
        d = np.abs(a[k].astype(np.float64) - b[k]).max() / max(np.abs(want[k]).max(), smax.get(k, 0.0))
        assert d <= 2 * BAR, (k, d)
