"""The camera model without a GPU (tests/camera_cases.py): unequal focal lengths, roll, an off-centre principal axis.
  1. the float32 oracle against float64 autograd on every case of the regime matrix under each of the four cameras, with
     the unchanged checks of test_cpu_f64_regimes.py: the yardstick of tests/test_gpu_camera_model.py is right there;
  2. teeth: an oracle handed the equal-focal tan_fovx, the un-rolled view matrix or the centred projection -- what a
     focal_x / focal_y mix-up, a dropped rotation entry or a pixel position rebuilt without P[0,2], P[1,2] amount to, and
     what no ring camera can see -- misses the bar by at least 10 x;
  3. the conditions of the pose comparison (camera_cases.POSE_PAIRS): no flipped pixel, no Gaussian on the cone edge;
  4. the cameras themselves: the matrices are what the builder says, and pose.camera_tensors reproduces them."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import camera_cases as CC
import f64_regimes as R
import pose_helpers as PH
from helpers import assert_grads_close, flipped_pixels


@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("camera", CC.NAMES)
def test_oracle_backward_matches_float64_under_a_general_camera(oracle, camera, name):
    r = R.regime(name, camera=camera)
    f, g = R.oracle_run(oracle, r)
    want, stats, img = R.f64_run(f, r)
    R.regime_count(r, f, want, stats, got=g)
    masked, report = R.masked_rows(r, f, stats)
    keep = np.ones(f["color"].shape[1] * f["color"].shape[2], bool)
    keep[R.flipped_pixels(stats["n_contrib"].numpy(), stats["final_T"].numpy(), f["n_contrib"], f["final_T"])] = False
    dc = np.abs(img.numpy() - f["color"]).reshape(3, -1)[:, keep]
    print(f"  {report}; colour max diff outside the flipped pixels {dc.max():.2e}")
    assert dc.max() < 5e-6
    worst = assert_grads_close(g, want, tol=R.TOL, tag=f"oracle vs float64 [{camera}, {name}]", masked=masked,
                               keys=R.grad_keys(r))
    print(f"  worst tensor-wide error {worst:.2e}")


# ---- teeth ------------------------------------------------------------------------------------------------------------
def _worst(got, want, masked, keys):
    """The tensor-wide figure of assert_grads_close (max |a - b| over the unmasked rows / max |b|), without its assertions."""
    worst = {}
    for k in keys:
        a = np.asarray(got[k], np.float64)
        a = a.reshape(a.shape[0], -1)
        b = np.asarray(want[k], np.float64).reshape(a.shape)
        worst[k] = float(np.abs(a - b).max(axis=1)[~masked].max() / np.abs(b).max())
    return worst


def _teeth(oracle, camera, mutate):
    """sh_D3 under `camera`: the oracle's gradients meet float64 within R.TOL with the camera it is given, and miss it by
    at least 10 x once `mutate` has replaced one of the camera's inputs by what the ring cameras cannot tell from it."""
    r = R.regime("sh_D3", camera=camera)
    f, g = R.oracle_run(oracle, r)
    want, stats, _ = R.f64_run(f, r)
    masked, _ = R.masked_rows(r, f, stats)
    keys = R.grad_keys(r)
    right = _worst(g, want, masked, keys)
    _, g_wrong = R.oracle_run(oracle, dict(r, case=mutate(r["case"])))
    wrong = _worst(g_wrong, want, masked, keys)
    print(f"  [{camera}] right camera {max(right.values()):.2e}; mutated {wrong}")
    assert max(right.values()) <= R.TOL
    assert max(wrong.values()) >= 10 * R.TOL, (camera, wrong)
    return wrong


def test_teeth_equal_focal_lengths_miss_the_bar(oracle):
    """tan_fovx = tfy W / H: focal_x = focal_y, what reading focal_y (or h_y) where focal_x (h_x) belongs amounts to."""
    wrong = _teeth(oracle, "focal", lambda case: dict(case, tfx=case["tfy"] * case["W"] / case["H"]))
    assert wrong["dL_dscales"] >= 10 * R.TOL  # (the focal lengths enter through the 2D covariance)


def test_teeth_unrolled_view_matrix_misses_the_bar(oracle):
    def unroll(case):
        base = R.regime("sh_D3")["case"]["cam"]
        assert not torch.equal(base.world_view_transform, case["cam"].world_view_transform)
        return dict(case, cam=dataclasses.replace(case["cam"], world_view_transform=base.world_view_transform))
    _teeth(oracle, "roll", unroll)


def test_teeth_centred_projection_misses_the_bar(oracle):
    def centre(case):
        base = R.regime("sh_D3")["case"]["cam"]
        roll, ratio, cx, cy = CC.CAMERAS["offcentre"]
        assert cx != 0 and cy != 0
        centred = CC.general_camera(base, case["W"], case["H"], roll, ratio, 0.0, 0.0)
        assert torch.equal(centred.world_view_transform, case["cam"].world_view_transform)
        return dict(case, cam=dataclasses.replace(case["cam"], full_proj_transform=centred.full_proj_transform))
    _teeth(oracle, "offcentre", centre)


# ---- the conditions of the pose comparison ----------------------------------------------------------------------------
def test_pose_pairs_cover_every_camera():
    need = {"sh_D3", "scale_mod_1.7", "cov3D_precomp", "off_cone", "off_cone+depth"}
    for camera in CC.NAMES:
        have = {case for cam, case, _ in CC.POSE_PAIRS if cam == camera}
        assert need <= have, (camera, need - have)
    assert len(set((cam, case) for cam, case, _ in CC.POSE_PAIRS)) == len(CC.POSE_PAIRS)
    assert all(case in PH.POSE_CASES for _, case, _ in CC.POSE_PAIRS)


@pytest.mark.parametrize("camera,name,seed", CC.POSE_PAIRS, ids=[f"{c}-{n}" for c, n, _ in CC.POSE_PAIRS])
def test_pose_pair_has_no_flipped_pixel_and_no_cone_edge_gaussian(oracle, camera, name, seed):
    """A camera gradient is a sum over all Gaussians: a flipped pixel cannot be masked, so the pairs are chosen without."""
    r = PH.pose_regime(name, camera=camera, seed=seed)
    f, _ = R.oracle_run(oracle, r)
    want_cam, want, stats = PH.f64_pose(f, r)
    flips = flipped_pixels(stats["n_contrib"].numpy(), stats["final_T"].numpy(), f["n_contrib"], f["final_T"])
    edge = int((R.cone_edge_rows(r) & (f["radii"] > 0)).sum())
    print(f"[{camera}, {name}, seed {seed}] flipped pixels {flips.size}, visible Gaussians on the cone edge {edge}")
    assert flips.size == 0 and edge == 0, (camera, name, seed, flips.size, edge)
    R.regime_count(r, f, want, stats)
    assert np.abs(want_cam["view"]).max() > 0 and np.abs(want_cam["proj"]).max() > 0


# ---- the cameras themselves -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CC.NAMES)
def test_general_camera_is_what_it_says(camera):
    from gaussianeditor_amd.pose import camera_tensors
    from gaussianeditor_amd.synth import ring_cameras

    W, H = 200, 136
    base = ring_cameras(4, W, H)[1]
    roll, ratio, cx, cy = CC.CAMERAS[camera]
    cam, tfx, tfy = CC.named_camera(camera, base, W, H)
    V, PV = cam.world_view_transform.double().numpy(), cam.full_proj_transform.double().numpy()
    eps = 4 * 2.0 ** -24
    # the accident the camera lifts is lifted, the others are kept
    fx, fy = W / (2 * tfx), H / (2 * tfy)
    assert abs(fx / fy - ratio) < 1e-12 and tfy == math.tan(base.FoVy / 2)
    # right.y: zero in every ring camera (up to the 1e-33 the two inversions of synth._world2view leave)
    assert abs(base.world_view_transform[1, 0]) < 1e-30 and (abs(V[1, 0]) > 0.1 if roll else abs(V[1, 0]) < 1e-30)
    P = np.linalg.inv(V) @ PV  # (the projection, transposed)
    assert abs(P[2, 0] - cx) < 1e-6 and abs(P[2, 1] - cy) < 1e-6
    assert abs(P[0, 0] - 1 / tfx) < 1e-6 and abs(P[1, 1] - 1 / tfy) < 1e-6 and abs(P[2, 3] - 1) < 1e-6
    # a rigid motion: the rotation is orthonormal, the centre is the base's, and maps to the view-space origin
    assert np.abs(V[:3, :3] @ V[:3, :3].T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(V[:3, :3]) - 1) < 1e-6
    assert np.abs(cam.camera_center.numpy() - base.camera_center.numpy()).max() < 1e-5
    assert np.abs(np.append(cam.camera_center.double().numpy(), 1.0) @ V)[:3].max() < 1e-5
    assert abs(math.tan(cam.FoVx / 2) - tfx) < 1e-12 and abs(math.tan(cam.FoVy / 2) - tfy) < 1e-12
    # pose.camera_tensors on the camera's parts: the bars of test_cpu_pose_grad's fixture test
    W2C, Pm, _, _ = CC.camera_parts(base, W, H, roll, ratio, cx, cy)
    Rm, T, proj = torch.from_numpy(W2C[:3, :3].T.copy()), torch.from_numpy(W2C[:3, 3].copy()), torch.from_numpy(Pm.T.copy())
    view, full, center = camera_tensors(Rm, T, proj)
    for got, want in ((view, cam.world_view_transform), (full, cam.full_proj_transform), (center, cam.camera_center)):
        want = want.double().numpy()
        assert np.abs(got.numpy() - want).max() <= eps * np.abs(want).max()
    assert np.array_equal(camera_tensors(Rm.float(), T.float(), proj.float())[0].numpy(), cam.world_view_transform.numpy())
