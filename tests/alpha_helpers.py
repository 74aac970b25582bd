"""Expected gradients of a loss on the alpha image (accumulated opacity, `return_alpha=True` /
gaussianeditor_amd.set_alpha_output), built from the existing backward alone by linearity.

A = 1 - prod_i (1 - alpha_i) = sum_i alpha_i T_i (telescoping) is the first channel of the colour image of the same geometry
with colours (1, 1, 1) and background 0.  So the gradient of <gC, C> + <gA, A> (+ <gD, D>) is
  (i)  the ordinary backward with gC (with gD: depth_helpers.depth_expectation), plus
  (ii) the backward of that "ones" render with pixel gradient (gA, 0, 0), without its colour / SH gradient (A does not depend
       on the colours).
tests/test_cpu_alpha.py holds this builder to float64 autograd and to finite differences of 1 - final_T."""
import numpy as np
import torch

from helpers import oracle_backward, oracle_forward, settings

DEV = "cuda:0"
COLOUR_KEYS = ("dL_dcolors", "dL_dsh")
#: the tensors on which a gradient test must be able to see the alpha share (discrimination condition)
SHARE_KEYS = ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_dmeans2D")
SHARE_REL, SHARE_ROWS = 1e-2, 100


def ones_gradient(GA, H, W):
    g = torch.zeros(3, H, W)
    g[0] = torch.as_tensor(GA).reshape(H, W)
    return g


def alpha_expectation(O, case, G, GA, GD=None, colors_precomp=None, cov3D_precomp=None, D=None, scale_modifier=1.0):
    """Oracle gradients of <G, C> + <GA, A> (+ <GD, D>) -> (total, alpha share): dicts by the oracle's names, float64.
    G: (3,H,W) or None, GA: (1,H,W), GD: (1,H,W) or None."""
    H, W, P = case["H"], case["W"], case["sc"]["xyz"].shape[0]
    kw = dict(cov3D_precomp=cov3D_precomp, D=D, scale_modifier=scale_modifier)
    G = torch.zeros(3, H, W) if G is None else G
    if GD is None:
        g1 = oracle_backward(O, case, oracle_forward(O, case, colors_precomp=colors_precomp, **kw), G,
                             colors_precomp=colors_precomp, **kw)
    else:
        from depth_helpers import depth_expectation

        g1 = depth_expectation(O, case, G, GD, colors_precomp=colors_precomp, **kw)
    case0, ones = dict(case, bg=torch.zeros(3)), torch.ones(P, 3)
    f2 = oracle_forward(O, case0, colors_precomp=ones, **kw)
    g2 = oracle_backward(O, case0, f2, ones_gradient(GA, H, W), colors_precomp=ones, **kw)
    total, share = {}, {}
    for k in g1:
        a = np.asarray(g1[k], dtype=np.float64)
        if k in COLOUR_KEYS or k not in g2:
            total[k] = a
            continue
        share[k] = np.asarray(g2[k], dtype=np.float64).reshape(a.shape)
        total[k] = a + share[k]
    return total, share


def assert_share_visible(total, share, tag="", keys=SHARE_KEYS):
    """Discrimination condition (i): the alpha share exceeds SHARE_REL of the total's maximum on >= SHARE_ROWS rows of each of
    SHARE_KEYS -> {key: rows}."""
    rows = {}
    for k in keys:
        P = np.asarray(total[k]).shape[0]
        s = np.abs(np.asarray(share[k], dtype=np.float64).reshape(P, -1)).max(axis=1)
        rows[k] = int((s > SHARE_REL * np.abs(total[k]).max()).sum())
    print(f"  {tag}: rows whose alpha share > {SHARE_REL} of the total's maximum: {rows}")
    assert all(n >= SHARE_ROWS for n in rows.values()), (tag, rows)
    return rows


def assert_differs_from_colour_only(got, got_colour_only, want, bar=1e-5, tag="", keys=SHARE_KEYS):
    """Discrimination condition (ii): what is under test differs from its own colour-only gradients by more than ten bars."""
    for k in keys:
        d = np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(got_colour_only[k], dtype=np.float64).reshape(got[k].shape)).max()
        assert d > 10 * bar * np.abs(want[k]).max(), (tag, k, d / np.abs(want[k]).max())


def run_hip(case, G=None, GA=None, GD=None, flags=0, colors_precomp=None, cov3D_precomp=None, D=None, scale_modifier=1.0,
            bg=None, abs_grad=False, aux_colors=None):
    """One render + backward of <G, C> + <GA, A> (+ <GD, D>) through GaussianRasterizer under options.override(flags); the
    alpha image is asked for iff GA is given.  `bg`: another background than the case's.
    -> (gradients by the oracle's names, numpy; dict(color, depth, alpha | None, absgrad | None, aux | None) as numpy)."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    sc = case["sc"]
    rs = settings(case if bg is None else dict(case, bg=bg), DEV, D=D, scale_modifier=scale_modifier)
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
    if aux_colors is not None:
        kw["aux_colors"] = aux_colors.to(DEV)
    if GA is not None:
        kw["return_alpha"] = True
    f = flags | (options.FLAG_ABS_GRAD if abs_grad else 0) | (options.FLAG_DEPTH_GRAD if GD is not None else 0)
    with options.override(f):
        outs = GaussianRasterizer(rs)(xyz, m2d, op, **kw)
    assert len(outs) == 3 + (aux_colors is not None) + (GA is not None)
    color, radii, depth = outs[:3]
    alpha = outs[-1] if GA is not None else None
    loss = 0.0
    if G is not None:
        loss = loss + (color * G.to(DEV)).sum()
    if GA is not None:
        loss = loss + (alpha * GA.to(DEV)).sum()
    if GD is not None:
        loss = loss + (depth * GD.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).cpu().numpy() for k, v in leaves.items()}
    a = getattr(m2d, "absgrad", None)
    npy = lambda t: None if t is None else t.detach().cpu().numpy()  # noqa: E731
    return grads, dict(color=npy(color), depth=npy(depth), alpha=npy(alpha), absgrad=npy(a),
                       aux=npy(outs[3]) if aux_colors is not None else None)


def product_expectation(case, G, GA, flags, **kw):
    """The linearity construction with the PRODUCT's own backwards that know nothing of the alpha image, under `flags` (the
    antialiased filter, the fast exponential: modes the oracle does not have) -> (total, alpha share), float64."""
    H, W, P = case["H"], case["W"], case["sc"]["xyz"].shape[0]
    g1, _ = run_hip(case, G=G, flags=flags, **kw)
    kw2 = {k: v for k, v in kw.items() if k != "colors_precomp"}
    g2, _ = run_hip(case, G=ones_gradient(GA, H, W), flags=flags, colors_precomp=torch.ones(P, 3), bg=torch.zeros(3), **kw2)
    total, share = {}, {}
    for k, a in g1.items():
        a = a.astype(np.float64)
        if k in COLOUR_KEYS:
            total[k] = a
            continue
        share[k] = g2[k].astype(np.float64)
        total[k] = a + share[k]
    return total, share
