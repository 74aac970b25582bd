"""What the loss tests share (tests/test_cpu_loss.py, tests/test_gpu_loss.py, tests/golden/make_golden_loss.py):

  * loss64: the loss  w_l1 * mean|x - y| + w_ssim * SSIM(x, y) + c  restated in float64 torch on the CPU -- the 11 x 11
    window as ONE 2D grouped conv2d with zero padding, autograd for its gradient.  This is the yardstick of both files.
  * closed_form_grad64: the gradient the kernels implement (three per-pixel maps, convolved once more), in float64.
  * image_pair: seeded image pairs in [0, 1] (float32 values): a smooth bicubic field plus noise, sigma 0.05 on x and 0.10
    on y; the "flat" variant puts a patch that is exactly 0 in both images over the top-left sixth (x == y: sign(0), and
    the E[x^2] - mu^2 cancellation with nothing but C1 / C2 left) and a saturated patch, x = 1 and y = 0.97, bottom right.
  * the fixture tests/golden/loss_ssim.npz: those inputs and what the reference's own l1_loss / ssim / autograd returned for
    them in float32 on the CPU; fixture_bar turns it into the per-case bar of the GPU test.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "loss_ssim.npz")
LAMBDA = 0.2
C1, C2 = 0.01 ** 2, 0.03 ** 2

#: name -> image shape.  The kernels work on 16 x 64 tiles with a 5-pixel halo: 5 x 7 and 11 x 11 are all halo, 45 x 70 and
#: 33 x 130 have two or more tiles in both directions with ragged remainders (13 rows / 6 columns, 1 row / 2 columns),
#: 64 x 64 is exactly four full tiles of one column, the last one is a batch (planes = N * C).
SHAPES = {"5x7": (3, 5, 7), "11x11": (3, 11, 11), "45x70": (3, 45, 70), "33x130": (1, 33, 130), "64x64": (3, 64, 64),
          "batch": (2, 3, 24, 40)}
CASES = [f"{v}_{k}" for k in SHAPES for v in ("tex", "flat")]


def window64():
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    return g / g.sum()


def _planes(t):
    """(..., H, W) -> (1, planes, H, W)"""
    return t.reshape(1, -1, t.shape[-2], t.shape[-1])


def _blur2d(t):
    n = t.shape[1]
    g = window64()
    w = (g[:, None] * g[None, :]).expand(n, 1, 11, 11).contiguous()
    return F.conv2d(t, w, padding=5, groups=n)


def ssim_map64(x, y):
    x, y = _planes(x), _planes(y)
    mu1, mu2 = _blur2d(x), _blur2d(y)
    s1, s2, s12 = _blur2d(x * x) - mu1 * mu1, _blur2d(y * y) - mu2 * mu2, _blur2d(x * y) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def loss64(x, y, w_l1, w_ssim, c):
    """(loss, l1, ssim) as float64 0-dim tensors; x, y: float64 tensors (..., H, W)."""
    l1 = (x - y).abs().mean()
    ssim = ssim_map64(x, y).mean()
    return w_l1 * l1 + w_ssim * ssim + c, l1, ssim


def weights(lam=LAMBDA):
    """(w_l1, w_ssim, c) of (1 - lam) * L1 + lam * (1 - SSIM)"""
    return 1.0 - lam, -lam, lam


def loss_and_grad64(x, y, w_l1, w_ssim, c):
    """float64 autograd: (loss, l1, ssim, dloss/dx) from float32 / float64 arrays or tensors."""
    x = torch.as_tensor(np.asarray(x)).double().clone().requires_grad_(True)
    y = torch.as_tensor(np.asarray(y)).double()
    loss, l1, ssim = loss64(x, y, w_l1, w_ssim, c)
    loss.backward()
    return float(loss.detach()), float(l1.detach()), float(ssim.detach()), x.grad.numpy().copy()


def closed_form_grad64(x, y, w_l1, w_ssim):
    """The kernels' formula in float64: dloss/dx = w_l1 sign(x - y) / N + w_ssim [K(Dmu) + 2 x K(dm_ds1) + y K(dm_ds12)] / N."""
    shape = tuple(np.asarray(x).shape)
    x = _planes(torch.as_tensor(np.asarray(x)).double())
    y = _planes(torch.as_tensor(np.asarray(y)).double())
    N = x.numel()
    mu1, mu2 = _blur2d(x), _blur2d(y)
    s1, s2, s12 = _blur2d(x * x) - mu1 * mu1, _blur2d(y * y) - mu2 * mu2, _blur2d(x * y) - mu1 * mu2
    A1, A2, B1, B2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2, mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    m = A1 * A2 / (B1 * B2)
    dm_dmu1 = 2 * mu2 * A2 / (B1 * B2) - 2 * mu1 * m / B1
    dm_ds1 = -m / B2
    dm_ds12 = 2 * A1 / (B1 * B2)
    Dmu = dm_dmu1 - 2 * mu1 * dm_ds1 - mu2 * dm_ds12
    dssim = (_blur2d(Dmu) + 2 * x * _blur2d(dm_ds1) + y * _blur2d(dm_ds12)) / N
    return (w_l1 * torch.sign(x - y) / N + w_ssim * dssim).reshape(shape).numpy()


def case_seed(name):
    return 1000 + sorted(SHAPES).index(name)


def image_pair(shape, seed, flat):
    """(x, y): float32 arrays of `shape` = (..., H, W), values in [0, 1]."""
    H, W = shape[-2], shape[-1]
    n = int(np.prod(shape[:-2]))
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(1, n, H // 8 + 2, W // 8 + 2, generator=g, dtype=torch.float64)
    base = F.interpolate(lo, size=(H, W), mode="bicubic", align_corners=False)[0].clamp(0, 1)
    x = (base + 0.05 * torch.randn(n, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    y = (base + 0.10 * torch.randn(n, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    if flat:
        x[:, :H // 3, :W // 2] = 0.0
        y[:, :H // 3, :W // 2] = 0.0
        r0, c0 = H - max(1, H // 4), W - max(1, W // 3)
        x[:, r0:, c0:] = 1.0
        y[:, r0:, c0:] = 0.97
    return x.float().reshape(shape).numpy(), y.float().reshape(shape).numpy()


def case_inputs(case):
    variant, name = case.split("_", 1)
    return image_pair(SHAPES[name], case_seed(name), variant == "flat")


_fixture = None


def fixture():
    """The committed arrays: per case <case>/x, /y, /l1, /ssim, /loss, /grad (float32)."""
    global _fixture
    if _fixture is None:
        with np.load(FIXTURE) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


_expect = {}


def expectation(case):
    """The float64 yardstick of one fixture case, computed once: dict(loss, l1, ssim, grad, grad_l1, grad_ssim)."""
    if case not in _expect:
        fx = fixture()
        x, y = fx[f"{case}/x"], fx[f"{case}/y"]
        w_l1, w_ssim, c = weights()
        loss, l1, ssim, grad = loss_and_grad64(x, y, w_l1, w_ssim, c)
        _expect[case] = dict(loss=loss, l1=l1, ssim=ssim, grad=grad, grad_l1=closed_form_grad64(x, y, w_l1, 0.0),
                             grad_ssim=closed_form_grad64(x, y, 0.0, w_ssim))
    return _expect[case]


def reference_error(case):
    """|the reference's float32 result - float64| per quantity (the gradient's as its largest entry's)."""
    fx, e = fixture(), expectation(case)
    return dict(loss=abs(float(fx[f"{case}/loss"]) - e["loss"]), l1=abs(float(fx[f"{case}/l1"]) - e["l1"]),
                ssim=abs(float(fx[f"{case}/ssim"]) - e["ssim"]),
                grad=float(np.abs(fx[f"{case}/grad"].astype(np.float64) - e["grad"]).max()))


def fixture_bar(case):
    """The bar of the GPU test per quantity: max(2 x the reference's own float32 error against float64 on this case,
    1e-6 absolute for the scalars / 1e-6 of the largest entry for the gradient).  The factor 2 covers another summation
    order in the same cancelling arithmetic, the floor the cases where the reference is within a few ulp."""
    r, e = reference_error(case), expectation(case)
    return dict(loss=max(2 * r["loss"], 1e-6), l1=max(2 * r["l1"], 1e-6), ssim=max(2 * r["ssim"], 1e-6),
                grad=max(2 * r["grad"], 1e-6 * float(np.abs(e["grad"]).max())))


# ----------------------------------------------------------------------------------------------------------------------
# a shape beyond the fixture (tests/test_cpu_size_regimes.py, tests/test_gpu_size_regimes.py): 3 x 10 x 10 = 300 tiles of
# 16 x 64, ragged in both directions (1 row, 1 column), so that loss_finish_kernel's threads add more than one slot each.
# Its float32 arrays would be 3 MB per case, so the fixture does not hold it; the bar's "reference's own float32 error" is
# taken from the same formula evaluated in float32 torch on the CPU, which tests/test_cpu_size_regimes.py pins to the
# fixture's arrays on every fixture case.
# ----------------------------------------------------------------------------------------------------------------------
LARGE_SHAPE = (3, 145, 577)
LARGE_SEED = 1100


def loss_and_grad32(x, y, w_l1, w_ssim, c):
    """loss_and_grad64's formula in float32 throughout (window, conv2d, autograd): (loss, l1, ssim, dloss/dx) float32."""
    x = torch.as_tensor(np.asarray(x, np.float32)).clone().requires_grad_(True)
    y = torch.as_tensor(np.asarray(y, np.float32))
    n = int(np.prod(x.shape[:-2]))
    g = window64().float()
    w = (g[:, None] * g[None, :]).expand(n, 1, 11, 11).contiguous()
    blur = lambda t: F.conv2d(t, w, padding=5, groups=n)  # noqa: E731
    xp, yp = _planes(x), _planes(y)
    mu1, mu2 = blur(xp), blur(yp)
    s1, s2, s12 = blur(xp * xp) - mu1 * mu1, blur(yp * yp) - mu2 * mu2, blur(xp * yp) - mu1 * mu2
    ssim = (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean()
    l1 = (x - y).abs().mean()
    loss = w_l1 * l1 + w_ssim * ssim + c
    loss.backward()
    return (np.float32(loss.detach().numpy()), np.float32(l1.detach().numpy()), np.float32(ssim.detach().numpy()),
            x.grad.numpy().copy())


def float32_error(x, y, e):
    """reference_error with loss_and_grad32 in the place of the fixture's arrays; e: dict(loss, l1, ssim, grad) in float64."""
    r32 = loss_and_grad32(x, y, *weights())
    return dict(loss=abs(float(r32[0]) - e["loss"]), l1=abs(float(r32[1]) - e["l1"]), ssim=abs(float(r32[2]) - e["ssim"]),
                grad=float(np.abs(r32[3].astype(np.float64) - e["grad"]).max()))


def bar_of_error(r, e):
    """fixture_bar's formula on an error dict r and the float64 yardstick e."""
    return dict(loss=max(2 * r["loss"], 1e-6), l1=max(2 * r["l1"], 1e-6), ssim=max(2 * r["ssim"], 1e-6),
                grad=max(2 * r["grad"], 1e-6 * float(np.abs(e["grad"]).max())))


_large = {}


def large_case(variant):
    """variant 'tex' | 'flat' at LARGE_SHAPE, computed once: dict(x, y, loss, l1, ssim, grad [float64 yardstick], ref_error,
    bar) where bar is fixture_bar's formula with the float32 evaluation above in the place of the fixture's arrays."""
    if variant not in _large:
        x, y = image_pair(LARGE_SHAPE, LARGE_SEED, variant == "flat")
        loss, l1, ssim, grad = loss_and_grad64(x, y, *weights())
        c = dict(x=x, y=y, loss=loss, l1=l1, ssim=ssim, grad=grad)
        c["ref_error"] = float32_error(x, y, c)
        c["bar"] = bar_of_error(c["ref_error"], c)
        _large[variant] = c
    return _large[variant]
