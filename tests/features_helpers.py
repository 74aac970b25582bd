"""Expected outputs and gradients of the feature image (`features=` of GaussianRasterizer / render(); include/gsr.h
gsr_blend_forward_features, gsr_blend_backward_features), built from the existing three-channel forward / backward alone.

F_c = sum_i f_ic alpha_i T_i is channel c % 3 of an ordinary render with colors_precomp = f[:, 3 k : 3 k + 3] (zero padded),
k = c // 3, on background 0.  By linearity the gradient of <G, C> + sum_c <GF_c, F_c> is
  (i)  the ordinary backward with G (with a depth / alpha loss: the builders of depth_helpers / alpha_helpers), plus
  (ii) for every three-channel slice the backward of that slice render with the slice of GF, of which the geometry gradients
       are the feature image's share and dL_dcolors is dL_dfeatures[:, 3 k : 3 k + 3].
tests/test_cpu_features.py holds this builder to float64 autograd.  The slices' shares may cancel against one another, so the
scale of a comparison is the larger of the total's maximum and the largest single slice share's maximum."""
import numpy as np
import torch

import alpha_helpers as AH
from helpers import ROW_FLOOR, ROW_FRACTION, ROW_REL, make_case, oracle_backward, oracle_forward, seed_gradient, settings

DEV = AH.DEV
COLOUR_KEYS = AH.COLOUR_KEYS
SHARE_KEYS, SHARE_REL, SHARE_ROWS = AH.SHARE_KEYS, AH.SHARE_REL, AH.SHARE_ROWS
#: the four cases of every feature test (make_case arguments, channels)
CASES = {"p2000": dict(P=2000, W=64, H=64, s0=0.05, C=7), "ragged": dict(P=2000, W=70, H=45, s0=0.05, C=16),
         "p600": dict(P=600, W=48, H=48, s0=0.08, C=1), "p4000": dict(P=4000, W=40, H=24, s0=0.12, C=33)}
_cache = {}


def make_features(P, C, seed=41):
    """(P,C) float32, uniform in [-1, 1]."""
    return (torch.rand(P, C, generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0).contiguous()


def feature_gradient(H, W, C):
    """(C,H,W): slice k carries seed_gradient(H, W, 7 + k) * H W (its first channels, where the last slice is partial)."""
    g = torch.cat([seed_gradient(H, W, 7 + k) * H * W for k in range((C + 2) // 3)], dim=0)
    return g[:C].contiguous()


def feature_case(name, C=None, camera=None):
    """(case, G, GF, feats) of CASES[name] (with another channel count if `C` is given, through the camera `camera` of
    camera_cases.CAMERAS if one is) -- built once, never modified."""
    kw = CASES[name]
    C = kw["C"] if C is None else C
    if (name, C, camera) not in _cache:
        case = make_case(kw["P"], kw["W"], kw["H"], s0=kw["s0"], camera=camera)
        H, W = case["H"], case["W"]
        _cache[(name, C, camera)] = (case, seed_gradient(H, W, 3) * H * W, feature_gradient(H, W, C), make_features(kw["P"], C))
    return _cache[(name, C, camera)]


def small_gaussian_case(C=5):
    """(case, feats, row): one 16 x 16 image -- one tile --, eight Gaussians, C channels.  Gaussian `row` is SMALL: isotropic,
    screen-space sigma 0.7 px (the 0.3 px^2 dilation included), opacity 0.9, centred on pixel (2.3, 2.4).  It passes the cull of
    its 8 x 8 quadrant and reaches alpha >= 1/255 only within sigma sqrt(2 ln(0.9 * 255)) = 2.3 px: most of the quadrant's pixels
    evaluate the entry and skip it."""
    import math

    W = H = 16
    case = make_case(8, W, H, s0=0.4)
    sc, cam = dict(case["sc"]), case["cam"]
    row, z, sigma, px, py = 0, 4.0, 0.7, 2.3, 2.4
    focal = W / (2.0 * case["tfx"])
    p_cam = torch.tensor([((2.0 * px + 1.0) / W - 1.0) * case["tfx"] * z, ((2.0 * py + 1.0) / H - 1.0) * case["tfy"] * z, z, 1.0])
    xyz, scaling, rotation, opacity = (sc[k].clone() for k in ("xyz", "scaling", "rotation", "opacity"))
    xyz[row] = (p_cam @ cam.world_view_transform.inverse())[:3]
    scaling[row] = math.sqrt(sigma * sigma - 0.3) * z / focal
    rotation[row] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    opacity[row] = 0.9
    sc.update(xyz=xyz.contiguous(), scaling=scaling.contiguous(), rotation=rotation.contiguous(), opacity=opacity.contiguous())
    return dict(case, sc=sc), make_features(8, C, seed=5), row


def oracle_blend_mask(O, case, row):
    """(H,W) bool: the pixels where the CPU oracle blends Gaussian `row` -- where the image of the features that are 1 for
    that Gaussian and 0 for every other is not zero (a blended entry adds alpha T >= 1e-4 / 255 > 0)."""
    P = case["sc"]["xyz"].shape[0]
    one_hot = torch.zeros(P, 1)
    one_hot[row] = 1.0
    return oracle_feature_image(O, case, one_hot)[0] != 0.0


def slices(feats, GF=None):
    """The three-channel slices: (k, n channels, colours (P,3) zero padded, pixel gradient (3,H,W) zero padded | None)."""
    P, C = feats.shape
    for k in range((C + 2) // 3):
        n = min(3, C - 3 * k)
        cols = torch.zeros(P, 3, dtype=feats.dtype)
        cols[:, :n] = feats[:, 3 * k:3 * k + n]
        g = None
        if GF is not None:
            g = torch.zeros(3, GF.shape[1], GF.shape[2], dtype=GF.dtype)
            g[:n] = GF[3 * k:3 * k + n]
        yield k, n, cols.contiguous(), g


def oracle_feature_image(O, case, feats, **kw):
    """(C,H,W) float32: channel c of the feature image == channel c % 3 of the oracle's slice render on background 0."""
    case0 = dict(case, bg=torch.zeros(3))
    out = np.zeros((feats.shape[1], case["H"], case["W"]), np.float32)
    for k, n, cols, _ in slices(feats):
        out[3 * k:3 * k + n] = oracle_forward(O, case0, colors_precomp=cols, **kw)["color"][:n]
    return out


def feature_expectation(O, case, G, GF, feats, GD=None, GA=None, colors_precomp=None, cov3D_precomp=None, D=None,
                        scale_modifier=1.0):
    """Oracle gradients of <G, C> + sum_c <GF_c, F_c> (+ <GD, D>) (+ <GA, A>) -> (total, feature share, dL_dfeatures,
    slice_max): the first two dicts by the oracle's names, dL_dfeatures (P,C), slice_max {key: the largest single slice
    share's maximum}; everything float64.  G: (3,H,W) or None."""
    H, W = case["H"], case["W"]
    kw = dict(cov3D_precomp=cov3D_precomp, D=D, scale_modifier=scale_modifier)
    G = torch.zeros(3, H, W) if G is None else G
    if GA is not None:
        g1, _ = AH.alpha_expectation(O, case, G, GA, GD=GD, colors_precomp=colors_precomp, **kw)
    elif GD is not None:
        from depth_helpers import depth_expectation

        g1 = depth_expectation(O, case, G, GD, colors_precomp=colors_precomp, **kw)
    else:
        g1 = oracle_backward(O, case, oracle_forward(O, case, colors_precomp=colors_precomp, **kw), G,
                             colors_precomp=colors_precomp, **kw)
    case0 = dict(case, bg=torch.zeros(3))
    total = {k: np.asarray(v, dtype=np.float64).copy() for k, v in g1.items()}
    share, slice_max = {}, {}
    dfeat = np.zeros(tuple(feats.shape), np.float64)
    for k, n, cols, g in slices(feats, GF):
        f2 = oracle_forward(O, case0, colors_precomp=cols, **kw)
        g2 = oracle_backward(O, case0, f2, g, colors_precomp=cols, **kw)
        dfeat[:, 3 * k:3 * k + n] = np.asarray(g2["dL_dcolors"], dtype=np.float64).reshape(-1, 3)[:, :n]
        for key in total:
            if key in COLOUR_KEYS or key not in g2:
                continue
            s = np.asarray(g2[key], dtype=np.float64).reshape(total[key].shape)
            share[key] = share.get(key, 0.0) + s
            slice_max[key] = max(slice_max.get(key, 0.0), float(np.abs(s).max()))
    for key, s in share.items():
        total[key] = total[key] + s
    return total, share, dfeat, slice_max


def assert_feature_grads_close(got, want, slice_max=None, tol=1e-5, tag="", masked=None, keys=None):
    """helpers.assert_grads_close -- the tensor bar and the per-row rule -- with the scale of a tensor the larger of the
    expectation's maximum and the largest single slice share's maximum (`slice_max`), so that cancellation between the
    slices cannot tighten the bar.  Prints every figure before it asserts -> the worst tensor-wide error."""
    worst = 0.0
    for k in (keys if keys is not None else got.keys()):
        a = np.asarray(got[k], dtype=np.float64)
        a = a.reshape(a.shape[0], -1)
        b = np.asarray(want[k], dtype=np.float64).reshape(a.shape)
        if a.size == 0:
            continue
        m = np.zeros(a.shape[0], bool) if masked is None else masked
        scale = max(float(np.abs(b).max()), float((slice_max or {}).get(k, 0.0)), 1e-30)
        d = np.abs(a - b).max(axis=1)
        e = float((d[~m] / scale).max()) if (~m).any() else 0.0
        row = np.abs(b).max(axis=1)
        bad = (d > ROW_FLOOR * scale + ROW_REL * row) & ~m
        live = (row > 0) & ~m
        print(f"  {tag}: {k} error {e:.2e} of {scale:.3e} (bar {tol:.0e}), rows over the row rule {int(bad.sum())} of {int(live.sum())}")
        worst = max(worst, e)
        assert e <= tol, (tag, k, e)
        assert int(bad.sum()) <= ROW_FRACTION * max(1, int(live.sum())) + 2, (tag, k, int(bad.sum()), int(live.sum()))
    return worst


def assert_share_visible(total, share, tag="", keys=SHARE_KEYS):
    """Discrimination condition (i): the feature share exceeds SHARE_REL of the total's maximum on >= SHARE_ROWS rows."""
    return AH.assert_share_visible(total, share, tag=tag, keys=keys)


def assert_differs_from_colour_only(got, got_colour_only, want, bar=1e-5, tag="", keys=SHARE_KEYS):
    """Discrimination condition (ii): differs from the colour-only gradients by more than ten bars."""
    return AH.assert_differs_from_colour_only(got, got_colour_only, want, bar=bar, tag=tag, keys=keys)


def run_hip(case, G=None, GF=None, feats=None, GA=None, GD=None, flags=0, colors_precomp=None, cov3D_precomp=None, D=None,
            scale_modifier=1.0, bg=None, abs_grad=False, aux_colors=None, pose=False):
    """One render + backward of <G, C> + sum_c <GF_c, F_c> (+ <GA, A>) (+ <GD, D>) through GaussianRasterizer under
    options.override(flags); the feature image is asked for iff `feats` is given, its loss taken iff `GF` is.
    -> (gradients by the oracle's names plus "dL_dfeatures", numpy; dict(color, depth, radii, alpha, features, absgrad, aux,
    pose) as numpy | None; pose = the 35 camera floats as dict(view, proj, campos))."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    sc = case["sc"]
    rs = settings(case if bg is None else dict(case, bg=bg), DEV, D=D, scale_modifier=scale_modifier)
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)  # noqa: E731
    cams = None
    if pose:
        cams = dict(view=leaf(rs.viewmatrix), proj=leaf(rs.projmatrix), campos=leaf(rs.campos))
        rs = rs._replace(viewmatrix=cams["view"], projmatrix=cams["proj"], campos=cams["campos"])
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
    if feats is not None:
        kw["features"] = leaves["dL_dfeatures"] = leaf(feats)
    f = (flags | (options.FLAG_ABS_GRAD if abs_grad else 0) | (options.FLAG_DEPTH_GRAD if GD is not None else 0)
         | (options.FLAG_POSE_GRAD if pose else 0))
    with options.override(f):
        outs = GaussianRasterizer(rs)(xyz, m2d, op, **kw)
    assert len(outs) == 3 + (aux_colors is not None) + (GA is not None) + (feats is not None)
    color, radii, depth = outs[:3]
    fimg = outs[-1] if feats is not None else None
    alpha = outs[-1 - (feats is not None)] if GA is not None else None
    loss = 0.0
    if G is not None:
        loss = loss + (color * G.to(DEV)).sum()
    if GF is not None:
        loss = loss + (fimg * GF.to(DEV)).sum()
    if GA is not None:
        loss = loss + (alpha * GA.to(DEV)).sum()
    if GD is not None:
        loss = loss + (depth * GD.to(DEV)).sum()
    if isinstance(loss, torch.Tensor):
        loss.backward()
    torch.cuda.synchronize()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).cpu().numpy() for k, v in leaves.items()}
    npy = lambda t: None if t is None else t.detach().cpu().numpy()  # noqa: E731
    pg = None if cams is None else {k: npy(v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in cams.items()}
    return grads, dict(color=npy(color), depth=npy(depth), radii=npy(radii), alpha=npy(alpha), features=npy(fimg),
                       absgrad=npy(getattr(m2d, "absgrad", None)), aux=npy(outs[3]) if aux_colors is not None else None, pose=pg)


def product_expectation(case, G, GF, feats, flags, pose=False, **kw):
    """The linearity construction with the PRODUCT's own three-channel backwards, which know nothing of the feature image,
    under `flags` (modes the oracle does not have) -> (total, feature share, dL_dfeatures, slice_max, pose sums | None)."""
    H, W = case["H"], case["W"]
    g1, o1 = run_hip(case, G=torch.zeros(3, H, W) if G is None else G, flags=flags, pose=pose, **kw)
    total = {k: v.astype(np.float64) for k, v in g1.items()}
    psum = None if not pose else {k: v.astype(np.float64) for k, v in o1["pose"].items()}
    share, slice_max = {}, {}
    dfeat = np.zeros(tuple(feats.shape), np.float64)
    kw2 = {k: v for k, v in kw.items() if k != "colors_precomp"}
    for k, n, cols, g in slices(feats, GF):
        g2, o2 = run_hip(case, G=g, flags=flags, colors_precomp=cols, bg=torch.zeros(3), pose=pose, **kw2)
        dfeat[:, 3 * k:3 * k + n] = g2["dL_dcolors"].astype(np.float64)[:, :n]
        for key in total:
            if key in COLOUR_KEYS or key not in g2:
                continue
            s = g2[key].astype(np.float64).reshape(total[key].shape)
            share[key] = share.get(key, 0.0) + s
            slice_max[key] = max(slice_max.get(key, 0.0), float(np.abs(s).max()))
        if pose:
            for key in psum:
                psum[key] = psum[key] + o2["pose"][key].astype(np.float64)
    for key, s in share.items():
        total[key] = total[key] + s
    return total, share, dfeat, slice_max, psum


# ---- a CPU stand-in for the new `_C` entry points -----------------------------------------------------------------------
class FeatureBackend:
    """`tests/oracle_backend.py` plus `alpha_image` / `dL_dout_alpha` (the stand-in of tests/test_cpu_alpha.py) plus
    `rasterize_features` and the `features` / `dL_dout_features` / `feature_grad_out` keywords: the image is the oracle's slice
    renders on background 0, the gradient's share the stand-in's own backward of those renders.  Records what it is asked."""

    def __init__(self):
        from test_cpu_alpha import _AlphaBackend

        self.alpha = _AlphaBackend()
        self.inner = self.alpha.inner
        self.calls = []  # (name, number of positional arguments, sorted keyword names)
        self.feature_images = self.feature_backwards = 0

    def forward(self, *args, **kw):
        self.calls.append(("rasterize_gaussians", len(args), tuple(sorted(kw))))
        return self.alpha.forward(*args, **kw)

    def aux(self, *args, **kw):
        self.calls.append(("rasterize_gaussians_aux", len(args), tuple(sorted(kw))))
        return self.inner.rasterize_gaussians_aux(*args, **kw)

    def alpha_image(self, *args):
        self.calls.append(("alpha_image", len(args), ()))
        return self.alpha.alpha_image(*args)

    def rasterize_features(self, features, num_rendered, geomBuffer, binningBuffer, imgBuffer, H, W, debug=False, flags=None):
        self.calls.append(("rasterize_features", 8, ("flags",)))
        self.feature_images += 1
        assert features.dtype == torch.float32 and features.dim() == 2 and not features.requires_grad
        out = torch.zeros(features.shape[1], int(H), int(W))
        for k, n, cols, _ in slices(features):
            out[3 * k:3 * k + n] = self.inner.rasterize_gaussians_aux(torch.zeros(3), cols, num_rendered, geomBuffer,
                                                                      binningBuffer, imgBuffer, H, W)[:n]
        return out

    def backward(self, *args, features=None, dL_dout_features=None, feature_grad_out=None, **kw):
        self.calls.append(("rasterize_gaussians_backward", len(args), tuple(sorted(
            list(kw) + (["features", "dL_dout_features", "feature_grad_out"] if features is not None else [])))))
        out = list(self.alpha.backward(*args, **kw))
        if features is None:
            assert dL_dout_features is None and feature_grad_out is None
            return tuple(out)
        self.feature_backwards += 1
        from test_cpu_alpha import args_opacity

        (bg, means3D, radii, colors, scales, rotations, smod, cov, view, proj, tfx, tfy, G, sh, degree, campos) = args[:16]
        H, W, P = G.shape[1], G.shape[2], means3D.shape[0]
        assert tuple(dL_dout_features.shape) == (features.shape[1], H, W) and tuple(feature_grad_out.shape) == tuple(features.shape)
        assert not bool(feature_grad_out.any()), "feature_grad_out must arrive zeroed"
        e = torch.empty(0)
        for k, n, cols, g in slices(features.detach(), dL_dout_features):
            fw = self.inner.rasterize_gaussians(torch.zeros(3), means3D.detach(), cols, args_opacity(self.alpha, args), scales,
                                                rotations, smod, cov, view, proj, tfx, tfy, H, W, e, degree, campos, False, False)
            a = list(args)
            a[0], a[3], a[12], a[13], a[16], a[17] = torch.zeros(3), cols, g, e, fw[4], fw[0]
            share = self.inner.rasterize_gaussians_backward(*a, flags=kw.get("flags"))
            feature_grad_out[:, 3 * k:3 * k + n] += share[1].reshape(P, 3)[:, :n]
            for i in (0, 2, 3, 4, 6, 7):  # means2D, opacity, means3D, cov3D, scales, rotations: not the colours / SHs
                if out[i] is not None and share[i] is not None and out[i].numel():
                    out[i] = out[i] + share[i].reshape(out[i].shape)
        return tuple(out)


def install(monkeypatch):
    """oracle_backend.install plus the stand-ins above -> (the package, the backend)."""
    import oracle_backend

    import gaussianeditor_amd.diff_gaussian_rasterization as dgr

    oracle_backend.install(monkeypatch)
    be = FeatureBackend()
    monkeypatch.setattr(dgr._C, "rasterize_gaussians", be.forward)
    monkeypatch.setattr(dgr._C, "rasterize_gaussians_backward", be.backward)
    monkeypatch.setattr(dgr._C, "rasterize_gaussians_aux", be.aux)
    monkeypatch.setattr(dgr._C, "alpha_image", be.alpha_image)
    monkeypatch.setattr(dgr._C, "rasterize_features", be.rasterize_features, raising=True)
    return dgr, be
