"""Camera tensors from a pose, in differentiable torch: what a pose refinement hands to `render()`.

The rasterizer reads three camera tensors -- `world_view_transform`, `full_proj_transform`, `camera_center` -- and, with
`gaussianeditor_amd.set_pose_grad(True)`, returns the gradient of each.  `camera_tensors` builds them from a pose with
the reference's conventions (scene/cameras.py, utils/graphics_utils.py getWorld2View2), so that autograd carries those
gradients on to whatever parametrises the pose:

    R, T        the reference's camera pose: R the camera-to-world rotation (3,3), T the world-to-camera translation (3,)
    W2C       = [[R^T, T], [0, 1]]
    world_view_transform = W2C^T                       (row-vector convention: (x, y, z, 1) @ world_view_transform)
    full_proj_transform  = world_view_transform @ projection
    camera_center        = inverse(world_view_transform)[3, :3]

`projection` is the reference's `projection_matrix` attribute, i.e. getProjectionMatrix(...) already transposed.
"""
from __future__ import annotations

from typing import Tuple

import torch


def camera_tensors(R: torch.Tensor, T: torch.Tensor, projection: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(R (3,3), T (3,), projection (4,4)) -> (world_view_transform (4,4), full_proj_transform (4,4), camera_center (3,)),
    in the dtype and on the device of `R`, each a differentiable function of the arguments that require a gradient."""
    if R.shape != (3, 3) or T.shape != (3,) or projection.shape != (4, 4):
        raise ValueError(f"camera_tensors: expected R (3,3), T (3,), projection (4,4); got {tuple(R.shape)}, {tuple(T.shape)}, "
                         f"{tuple(projection.shape)}")
    T = T.to(dtype=R.dtype, device=R.device)
    last = torch.zeros(4, 1, dtype=R.dtype, device=R.device)
    last[3, 0] = 1.0
    # W2C^T: rows 0..2 = (R | 0), row 3 = (T | 1)
    view = torch.cat([torch.cat([R, T[None, :]], dim=0), last], dim=1)
    full = view @ projection.to(dtype=R.dtype, device=R.device)
    center = torch.linalg.inv(view)[3, :3]
    return view, full, center
