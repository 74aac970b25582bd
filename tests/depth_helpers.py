"""Expected gradients of a loss on the depth image (gaussianeditor_amd.set_depth_grad), built from the existing backward
alone by linearity.  The depth image D = sum_i d_i alpha_i T_i is the colour image of the same geometry with colours
(d_i, 0, 0) and background 0, where d_i = view-space z of Gaussian i.  So the gradient of <gC, C> + <gD, D> is
  (i)  the ordinary backward with gC, plus
  (ii) the backward of that "depth colour" render with pixel gradient (gD, 0, 0) -- its colour gradient's first column is
       dL/dd_i -- and dL/dd_i * dd_i/dmeans3D = dL/dd_i * (view[2], view[6], view[10]) on means3D (no SH gradient: the
       depth does not depend on the colour)."""
import numpy as np
import torch

from helpers import oracle_backward, oracle_forward, settings

DEV = "cuda:0"


def depth_colors(depths) -> torch.Tensor:
    d = torch.as_tensor(np.asarray(depths, dtype=np.float32))
    return torch.stack([d, torch.zeros_like(d), torch.zeros_like(d)], dim=1).contiguous()


def view_z_row(case) -> np.ndarray:
    """d(view-space z)/d(means3D): entries 2, 6, 10 of the flat 16-float view matrix (transformPoint4x3)."""
    return case["cam"].world_view_transform.reshape(-1).numpy()[[2, 6, 10]].astype(np.float64)


def depth_expectation(O, case, G, GD, colors_precomp=None, cov3D_precomp=None, D=None, scale_modifier=1.0):
    """Oracle gradients of <G, C> + <GD, D> (G: (3,H,W) or None, GD: (1,H,W)), by linearity (module docstring)."""
    H, W = case["H"], case["W"]
    kw = dict(cov3D_precomp=cov3D_precomp, D=D, scale_modifier=scale_modifier)
    f1 = oracle_forward(O, case, colors_precomp=colors_precomp, **kw)
    g1 = oracle_backward(O, case, f1, torch.zeros(3, H, W) if G is None else G, colors_precomp=colors_precomp, **kw)
    case0 = dict(case, bg=torch.zeros(3))
    dcol = depth_colors(f1["depths"])  # K1's float32 depths
    f2 = oracle_forward(O, case0, colors_precomp=dcol, **kw)
    G2 = torch.zeros(3, H, W)
    G2[0] = torch.as_tensor(GD).reshape(H, W)
    g2 = oracle_backward(O, case0, f2, G2, colors_precomp=dcol, **kw)
    out = {}
    for k in g1:
        a = np.asarray(g1[k], dtype=np.float64)
        if k in ("dL_dcolors", "dL_dsh"):
            out[k] = a  # (the depth does not depend on the colour)
        else:
            out[k] = a + np.asarray(g2[k], dtype=np.float64).reshape(a.shape)
    gd = np.asarray(g2["dL_dcolors"], dtype=np.float64).reshape(-1, 3)[:, 0]
    out["dL_dmeans3D"] = out["dL_dmeans3D"].reshape(-1, 3) + gd[:, None] * view_z_row(case)[None, :]
    out["dL_ddepth"] = gd
    return out


def grads_hip(case, G, GD, colors_precomp=None, cov3D_precomp=None, D=None, scale_modifier=1.0, flags=None,
              depth_only=False):
    """Product gradients of <G, C> + <GD, D> through GaussianRasterizer, the render started under options.override(flags)
    (None: the current flags).  depth_only: the loss is <GD, D> alone (the colour output unused)."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    sc = case["sc"]
    rs = settings(case, DEV, D=D, scale_modifier=scale_modifier)
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)  # noqa: E731
    xyz, op = leaf(sc["xyz"]), leaf(sc["opacity"])
    m2d = torch.zeros_like(xyz, requires_grad=True)
    kw, leaves = {}, dict(dL_dmeans3D=xyz, dL_dopacity=op, dL_dmeans2D=m2d)
    if colors_precomp is None:
        kw["shs"] = leaves["dL_dsh"] = leaf(sc["features"])
    else:
        kw["colors_precomp"] = leaves["dL_dcolors"] = leaf(colors_precomp)
    if cov3D_precomp is None:
        kw["scales"] = leaves["dL_dscales"] = leaf(sc["scaling"])
        kw["rotations"] = leaves["dL_drotations"] = leaf(sc["rotation"])
    else:
        kw["cov3D_precomp"] = leaves["dL_dcov3D"] = leaf(cov3D_precomp)
    with options.override(options.current_flags() if flags is None else flags):
        color, radii, depth = GaussianRasterizer(rs)(xyz, m2d, op, **kw)
    loss = (depth * GD.to(DEV)).sum()
    if not depth_only:
        loss = loss + (color * G.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).cpu().numpy() for k, v in leaves.items()}
