"""Expected absolute screen-space gradients (gaussianeditor_amd.set_abs_grad, include/gsr.h GSR_FLAG_ABS_GRAD), built from
the existing backward alone.

absgrad[i] = (sum_p |t_x(p, i)|, sum_p |t_y(p, i)|, 0), t(p, i) the term pixel p adds into dL_dmeans2D[i].  A backward whose
pixel gradient is non-zero at ONE pixel p returns exactly t(p, .) in dL_dmeans2D, so for a pixel set S

    expected absgrad = sum_{p in S} | backward(G 1_p)["dL_dmeans2D"][:, :2] |

and the code under test runs ONE backward with G 1_S under the flag.  `backward` is the float32 oracle here (with a depth
loss: depth_helpers.depth_expectation, per pixel); tests/test_cpu_abs_grad.py holds this builder to float64 autograd."""
import numpy as np
import torch

from helpers import oracle_backward, oracle_forward, settings

DEV = "cuda:0"
#: a test discriminates if on at least this share of the rows with a gradient the absolute sum exceeds the absolute value of
#: the signed sum by more than DISCRIMINATE_REL of the tensor's maximum (the oracle alone gives 42 % on the cases used)
DISCRIMINATE_SHARE, DISCRIMINATE_REL = 0.25, 1e-3


def block_pixels(H, W, n):
    """The (y, x) of a centred n x n block of pixels."""
    y0, x0 = (H - n) // 2, (W - n) // 2
    return [(y, x) for y in range(y0, y0 + n) for x in range(x0, x0 + n)]


def pixel_mask(H, W, pixels):
    m = torch.zeros(1, H, W)
    for y, x in pixels:
        m[0, y, x] = 1.0
    return m


def abs_sum(term_of_pixel, pixels, P):
    """sum over `pixels` of |term_of_pixel(y, x)[:, :2]| -> (absgrad (P,3) float64 with z = 0, signed sum (P,2) float64)."""
    a, s = np.zeros((P, 3)), np.zeros((P, 2))
    for y, x in pixels:
        t = np.asarray(term_of_pixel(y, x), dtype=np.float64).reshape(P, -1)[:, :2]
        a[:, :2] += np.abs(t)
        s += t
    return a, s


def abs_expectation(O, case, G, pixels, GD=None, colors_precomp=None, cov3D_precomp=None, D=None, scale_modifier=1.0):
    """Oracle-built expectation for the loss <G 1_S, C> (+ <GD 1_S, D>), S = `pixels` -> (absgrad (P,3), signed sum (P,2))."""
    H, W, P = case["H"], case["W"], case["sc"]["xyz"].shape[0]
    kw = dict(colors_precomp=colors_precomp, cov3D_precomp=cov3D_precomp, D=D, scale_modifier=scale_modifier)
    f = oracle_forward(O, case, **kw) if GD is None else None

    def term(y, x):
        m = pixel_mask(H, W, [(y, x)])
        if GD is None:
            return oracle_backward(O, case, f, G * m, **kw)["dL_dmeans2D"]
        from depth_helpers import depth_expectation

        return depth_expectation(O, case, G * m, GD * m, **kw)["dL_dmeans2D"]
    return abs_sum(term, pixels, P)


def assert_discriminates(absgrad, signed, tag=""):
    """The case must tell the absolute sum from the signed one: on >= DISCRIMINATE_SHARE of the rows with a gradient
    sum|t| - |sum t| > DISCRIMINATE_REL of the tensor's maximum.  -> (rows with a gradient, rows that discriminate)."""
    a, s = np.asarray(absgrad, dtype=np.float64)[:, :2], np.abs(np.asarray(signed, dtype=np.float64)[:, :2])
    live = a.max(axis=1) > 0
    disc = ((a - s).max(axis=1) > DISCRIMINATE_REL * a.max()) & live
    print(f"  {tag}: rows with a gradient {int(live.sum())}, rows where sum|t| - |sum t| > {DISCRIMINATE_REL} max: {int(disc.sum())}")
    assert live.sum() > 0 and disc.sum() >= DISCRIMINATE_SHARE * live.sum(), (tag, int(disc.sum()), int(live.sum()))
    return int(live.sum()), int(disc.sum())


def run_hip(case, G, GD=None, flags=0, abs_grad=True, colors_precomp=None, cov3D_precomp=None, D=None, scale_modifier=1.0):
    """One render + backward of <G, C> (+ <GD, D>) through GaussianRasterizer under options.override(flags [| FLAG_ABS_GRAD])
    -> (gradients by the oracle's names, numpy; means2D.absgrad as numpy, or None if the attribute was not set)."""
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
    f = flags | (options.FLAG_ABS_GRAD if abs_grad else 0) | (options.FLAG_DEPTH_GRAD if GD is not None else 0)
    with options.override(f):
        color, radii, depth = GaussianRasterizer(rs)(xyz, m2d, op, **kw)
    loss = (color * G.to(DEV)).sum()
    if GD is not None:
        loss = loss + (depth * GD.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).cpu().numpy() for k, v in leaves.items()}
    a = getattr(m2d, "absgrad", None)
    return grads, (None if a is None else a.cpu().numpy())
