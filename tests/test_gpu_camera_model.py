"""-m gpu: every camera-consuming kernel under a general camera (tests/camera_cases.py).

Every other test renders through synth.look_at_camera: equal focal lengths in pixels, no roll, a centred principal axis.
Here K1, K8+K9, the pose backward and every route built on them run under the cameras that lift those accidents one at a
time (`focal`, `roll`, `offcentre`: they tell a failure's cause apart) and all together (`all`), with the checks of the tests
they extend, unchanged: the forward stage by stage against the oracle (and the reference's own kernels where they are
built), the backward of every regime and route against float64 autograd, the opt-in routes through their helpers'
expectations, the camera gradients on camera_cases.POSE_PAIRS, mark_visible / apply_weights, and render().
tests/test_cpu_camera_model.py holds the yardsticks to float64 under the same cameras and shows that they have teeth."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import camera_cases as CC
import f64_regimes as R
import pose_helpers as PH
from helpers import make_case, oracle_forward, seed_gradient, settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- forward, every stage, against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("P,W,H,s0,seed", [(3000, 250, 131, 0.05, 2), (500, 64, 64, 0.1, 3)])
@pytest.mark.parametrize("camera", CC.NAMES)
def test_forward_all_stages(oracle, camera, P, W, H, s0, seed):
    from test_gpu_parity import _compare_forward

    f, _ = _compare_forward(oracle, make_case(P, W, H, seed=seed, s0=s0, camera=camera))
    assert int((f["radii"] > 0).sum()) > P // 4


def test_forward_camera_inside_the_cloud_with_culling(oracle):
    from test_gpu_parity import _compare_forward

    case = make_case(3000, 160, 160, seed=8, s0=0.05, scale_xyz=4.0, camera="all")
    f, _ = _compare_forward(oracle, case, scale_modifier=0.7)
    assert (f["radii"] == 0).any() and (f["radii"] > 0).any()


def test_forward_three_way_with_the_reference(oracle):
    """Oracle == reference (contraction off) bit for bit, product against the reference's natural build, and the product's
    integers against the contraction-free build, under `all`."""
    import test_gpu_reference as TR

    case = make_case(3000, 250, 131, seed=2, s0=0.05, camera="all")
    TR._check_oracle_is_pinned(oracle, case)
    TR._check_product_vs_reference_fma(case, 2)
    TR._check_product_vs_reference_nofma_integers(case)


# ---- backward against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_l1_backward_matches_float64_all(name):
    from test_gpu_f64_regimes import _check

    _check(name, "l1", camera="all")


@pytest.mark.parametrize("name", ["sh_D3", "off_cone", "depth"])
@pytest.mark.parametrize("camera", ["focal", "roll", "offcentre"])
def test_l1_backward_matches_float64_single_factor(camera, name):
    from test_gpu_f64_regimes import _check

    _check(name, "l1", camera=camera)


@pytest.mark.parametrize("route", ["direct", "rgb", "persistent"])
@pytest.mark.parametrize("name", ["sh_D3", "scale_mod_1.7", "off_cone"])
def test_view_grads_backward_matches_float64_all(name, route):
    from test_gpu_f64_regimes import _check

    _check(name, route, camera="all")


# ---- opt-in routes, each through its own helper's expectation ------------------------------------------------------------
def test_absgrad_vs_per_pixel_oracle(oracle):
    import abs_helpers as AB
    from test_gpu_abs_grad import _check_small

    case = make_case(2000, 64, 64, s0=0.05, camera="all")
    pixels = AB.block_pixels(64, 64, 8)
    G = seed_gradient(64, 64, 3) * 64 * 64 * AB.pixel_mask(64, 64, pixels)
    _check_small(oracle, case, G, pixels, "p2000 [all]")


@pytest.mark.parametrize("name", ["sub_pixel", "floor", "off_cone"])
def test_antialiased_forward_is_the_plain_forward_at_rec0w(name):
    from test_gpu_antialias import _check_forward_at_rec0w

    _check_forward_at_rec0w(name, "reference", camera="all")


@pytest.mark.parametrize("name", ["sub_pixel", "floor", "off_cone", "sh_D3"])
def test_antialiased_l1_backward_matches_float64(name):
    from test_gpu_antialias import _check

    _check(name, "l1", camera="all")


def test_alpha_backward(oracle):
    from test_gpu_alpha import _check

    _check(oracle, "ragged", "SH ragged [all]", camera="all")
    _check(oracle, "p2000", "depth + alpha [all]", with_depth=True, camera="all")


@pytest.mark.parametrize("name", ["p600", "p2000"])  # (C = 1, the smallest, and C = 7)
def test_feature_backward_with_the_colour_loss(oracle, name):
    import features_helpers as FH
    from test_gpu_features import _check

    _check(oracle, name, f"features + colour, {name} C={FH.CASES[name]['C']} [all]", camera="all")


# ---- pose ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera,name,seed", CC.POSE_PAIRS, ids=[f"{c}-{n}" for c, n, _ in CC.POSE_PAIRS])
def test_pose_gradients_match_float64(camera, name, seed):
    import test_gpu_pose_grad as TP

    r, f, want_cam, want, stats, flips = TP._expectation(name, camera, seed)
    assert flips == 0, (camera, name, "the product's forward and float64 differ in a discrete decision", flips)
    R.regime_count(r, f, want, stats)
    got, _ = TP._product_pose(r)
    PH.assert_pose_close(got, want_cam, f"product vs float64 [{camera}, {name}]", colors_precomp=r["colors_precomp"] is not None)


@functools.lru_cache(maxsize=None)
def _identity_case():
    return PH.identity_case(camera="all")


@pytest.mark.parametrize("everything", [False, True], ids=["no_flags", "aa_depth_alpha"])
def test_translation_identity(everything):
    from gaussianeditor_amd import options
    from test_gpu_pose_grad import _identity_run

    cg, mg = _identity_run(_identity_case(), options.FLAG_ANTIALIAS if everything else 0, everything, everything)
    PH.assert_identity(cg, mg, f"identity [all] aa = depth = alpha = {everything}")


@pytest.mark.parametrize("camera", CC.NAMES)
def test_camera_tensors_reproduce_the_general_camera(camera):
    """pose.camera_tensors on the device, fed the camera's (R, T, projection): the three tensors the tests render through,
    within the bars of test_cpu_pose_grad's fixture test."""
    from gaussianeditor_amd.pose import camera_tensors
    from gaussianeditor_amd.synth import ring_cameras

    W, H = 200, 136
    base = ring_cameras(4, W, H)[1]
    cam, _, _ = CC.named_camera(camera, base, W, H)
    W2C, P, _, _ = CC.camera_parts(base, W, H, *CC.CAMERAS[camera])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    Rm, T, proj = t(W2C[:3, :3].T), t(W2C[:3, 3]), t(P.T)
    eps = 4 * 2.0 ** -24
    view, full, center = camera_tensors(Rm, T, proj)
    assert view.dtype == torch.float64 and view.device.type == "cuda"
    for got, want in ((view, cam.world_view_transform), (full, cam.full_proj_transform), (center, cam.camera_center)):
        want = want.double().numpy()
        assert np.abs(got.cpu().numpy() - want).max() <= eps * np.abs(want).max()
    v32 = camera_tensors(Rm.float(), T.float(), proj.float())[0]
    assert v32.dtype == torch.float32 and np.array_equal(v32.cpu().numpy(), cam.world_view_transform.numpy())


# ---- mark_visible, apply_weights ------------------------------------------------------------------------------------------
def test_mark_visible(oracle):
    from test_gpu_parity import _check_mark_visible

    _check_mark_visible(oracle, camera="all")


@pytest.mark.parametrize("C,W,H", [(1, 250, 131), (3, 100, 100)])
def test_apply_weights(oracle, C, W, H):
    from test_gpu_parity import _check_apply_weights

    _check_apply_weights(oracle, C, W, H, camera="all")


# ---- render() ---------------------------------------------------------------------------------------------------------------
def test_render_equals_the_l1_call_bit_for_bit(oracle):
    """render() reads FoVx / FoVy off the camera object: with the general camera's symmetric angles it hands the rasterizer
    the tan_fovx / tan_fovy of the case, and image, depth and radii are those of the L1 call, which the oracle pins."""
    import math

    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer
    from gaussianeditor_amd.gaussian_renderer import render
    from test_gpu_pose_grad import _PC

    case = make_case(3000, 250, 131, seed=2, s0=0.05, camera="all")
    cam, sc, H, W = case["cam"], case["sc"], case["H"], case["W"]
    assert np.float32(math.tan(cam.FoVx * 0.5)) == np.float32(case["tfx"])
    assert np.float32(math.tan(cam.FoVy * 0.5)) == np.float32(case["tfy"])
    camera = SimpleNamespace(FoVx=cam.FoVx, FoVy=cam.FoVy, image_height=H, image_width=W,
                             world_view_transform=cam.world_view_transform.to(DEV),
                             full_proj_transform=cam.full_proj_transform.to(DEV), camera_center=cam.camera_center.to(DEV))
    pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    with torch.no_grad():
        out = render(camera, _PC(sc), pipe, case["bg"].to(DEV))
        t = lambda k: sc[k].to(DEV)  # noqa: E731
        color, radii, depth = GaussianRasterizer(settings(case, DEV))(t("xyz"), torch.zeros(sc["xyz"].shape, device=DEV),
                                                                      t("opacity"), shs=t("features"), scales=t("scaling"),
                                                                      rotations=t("rotation"))
    torch.cuda.synchronize()
    assert torch.equal(out["render"].view(torch.int32), color.view(torch.int32))
    assert torch.equal(out["depth_3dgs"].view(torch.int32), depth.view(torch.int32))
    assert torch.equal(out["radii"], radii) and torch.equal(out["visibility_filter"], radii > 0)
    f = oracle_forward(oracle, case)
    assert np.array_equal(radii.cpu().numpy(), f["radii"]) and np.abs(color.cpu().numpy() - f["color"]).max() <= 1e-5
    assert int((f["radii"] > 0).sum()) > 500
