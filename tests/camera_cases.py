"""General cameras for the camera-model tests: what synth.look_at_camera never produces.

Every ring camera has equal focal lengths in pixels (fovx is derived from fovy and W / H), no roll (the world up vector is
fixed, so one entry of the W2C rotation is exactly zero) and a centred principal axis (P[0,2] = P[1,2] = 0).  A kernel that
reads focal_y where focal_x belongs, drops the rotation entry that is always zero, or rebuilds the pixel position from view
space and a focal length instead of from the projection matrix passes every test that renders through them.
`general_camera` lifts each of the three accidents; CAMERAS names the three single-factor cameras (they tell a failure's
cause apart) and the one with all three.

The rasterizer receives tan_fovx = tfx and tan_fovy = tfy, the SYMMETRIC half-angles: what a caller with a shifted
principal point passes.  The 1.3 tan(fov) cone stays centred on the view axis, as in the reference.
"""
import math

import numpy as np
import torch

from gaussianeditor_amd.synth import Camera

# name -> (roll in degrees, focal_x / focal_y in pixels, P[0,2], P[1,2])
CAMERAS = {"focal": (0.0, 1.3, 0.0, 0.0), "roll": (25.0, 1.0, 0.0, 0.0), "offcentre": (0.0, 1.0, 0.18, -0.12),
           "all": (25.0, 1.3, 0.18, -0.12)}
NAMES = list(CAMERAS)

# (camera, case of pose_helpers.POSE_CASES, scene seed or None for the case's own): the pairs of the pose comparison.  A camera
# gradient is a sum over all Gaussians, so a pixel whose discrete decisions differ between float32 and float64 cannot be
# masked: every pair has 0 flipped pixels and 0 visible Gaussians on the cone edge in the float32 oracle
# (test_cpu_camera_model asserts it per row).  Where the case's own seed shows a flip under a camera (all / sh_D1,
# focal / cov3D_precomp, roll / cov3D_precomp, roll / off_cone, offcentre / off_cone: 1 pixel each) the seed is the first of
# own + 100, own + 200, ... without one.  The count can depend on the host: focal / off_cone with its own seed shows 0 flipped
# pixels on one CPU and 1 on another (the same oracle binary; the inputs are built with torch and numpy on the host), so its
# seed is one that is clean on both; every row was checked on two hosts with different CPUs.
POSE_PAIRS = [
    ("all", "sh_D1", 122), ("all", "sh_D3", None), ("all", "clamped_colours", None), ("all", "scale_mod_1.7", None),
    ("all", "colors_precomp", None), ("all", "cov3D_precomp", None), ("all", "off_cone", None), ("all", "saturated", None),
    ("all", "unnormalised_quat", None), ("all", "off_cone+depth", None),
    ("focal", "sh_D3", None), ("focal", "scale_mod_1.7", None), ("focal", "cov3D_precomp", 251), ("focal", "off_cone", 111),
    ("focal", "off_cone+depth", 111),
    ("roll", "sh_D3", None), ("roll", "scale_mod_1.7", None), ("roll", "cov3D_precomp", 151), ("roll", "off_cone", 211),
    ("roll", "off_cone+depth", 211),
    ("offcentre", "sh_D3", None), ("offcentre", "scale_mod_1.7", None), ("offcentre", "cov3D_precomp", None),
    ("offcentre", "off_cone", 111), ("offcentre", "off_cone+depth", 111),
]


def camera_parts(base, W, H, roll_deg, fx_over_fy, cx, cy):
    """-> (W2C (4,4), projection P (4,4), tfx, tfy), float64 numpy: the general camera built on the ring camera `base`."""
    W2C0 = base.world_view_transform.double().numpy().T
    a = math.radians(roll_deg)
    Rz = np.eye(4)
    Rz[0, 0], Rz[0, 1], Rz[1, 0], Rz[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    W2C = Rz @ W2C0
    tfy = math.tan(base.FoVy / 2)
    tfx = tfy * W / H / fx_over_fy
    zn, zf = base.znear, base.zfar
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 1.0 / tfx, 1.0 / tfy
    P[0, 2], P[1, 2] = cx, cy
    P[3, 2] = 1.0
    P[2, 2] = zf / (zf - zn)
    P[2, 3] = -zf * zn / (zf - zn)
    return W2C, P, tfx, tfy


def general_camera(base, W, H, roll_deg, fx_over_fy, cx, cy):
    """The ring camera `base` rolled about its view axis by `roll_deg`, with focal_x = fx_over_fy * focal_y (in pixels) and
    the principal point moved by (cx, cy) in NDC -> synth.Camera.  FoVx / FoVy are the symmetric angles 2 atan(tfx / tfy)."""
    W2C, P, tfx, tfy = camera_parts(base, W, H, roll_deg, fx_over_fy, cx, cy)
    wv = torch.from_numpy(np.float32(W2C.T)).contiguous()
    full = torch.from_numpy(np.float32(W2C.T @ P.T)).contiguous()
    center = torch.from_numpy(np.float32(np.linalg.inv(W2C)[:3, 3])).contiguous()
    return Camera(H, W, 2.0 * math.atan(tfx), 2.0 * math.atan(tfy), wv, full, center, base.znear, base.zfar)


def named_camera(name, base, W, H):
    """-> (camera, tfx, tfy) of CAMERAS[name] on `base`; tfx / tfy as computed (not round-tripped through atan)."""
    cam = general_camera(base, W, H, *CAMERAS[name])
    _, _, tfx, tfy = camera_parts(base, W, H, *CAMERAS[name])
    return cam, tfx, tfy
