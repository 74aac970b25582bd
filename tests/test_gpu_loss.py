"""-m gpu: the fused L1 + SSIM loss (gaussianeditor_amd.losses; gsr_photometric_loss_forward / _backward, csrc/loss/gsr_loss.hip)
against the float64 restatement of tests/loss_helpers.py (pinned by tests/test_cpu_loss.py) on every case of
tests/golden/loss_ssim.npz.

The bar, per case and quantity (loss_helpers.fixture_bar): the product's error against float64 must not exceed
max(2 x the error of the reference's own float32 result against float64 on that case, 1e-6 absolute for the three scalars /
1e-6 of the largest entry for the gradient).  The formula is ill-conditioned in float32 wherever an image is flat (E[x^2] -
mu^2 against C2 = 9e-4), so the bar is the reference's own float32 error and not a constant.

Discrimination: in every case each term's share of the expected gradient (L1: 0.8 sign / N; SSIM: -0.2 dSSIM/dx) exceeds TEN
bars of that case on at least min(100, N / 4) values, so a gradient without either term misses the bar of every case; and the
condition "the share exceeds 10 % of the gradient's maximum on at least 100 pixels", for both terms, holds on the two
45 x 70 cases (2 x 3 tiles, ragged in both directions) and on the batch -- in 33 x 130 and 64 x 64 single outliers of the SSIM
gradient are more than ten times the uniform 0.8 / N of the L1 term, so no L1 share reaches 10 % of that maximum there.

Measured on the MI355X, the product's error against float64 / the bar (gradient: as a fraction of its largest entry):
    case          loss               l1                 ssim               gradient
    tex_5x7       2.8e-09 / 1.0e-06  3.8e-09 / 1.0e-06  2.9e-08 / 1.0e-06  1.1e-07 / 1.0e-06
    flat_5x7      3.6e-09 / 1.0e-06  2.6e-09 / 1.0e-06  7.4e-09 / 1.0e-06  1.9e-07 / 1.0e-06
    tex_11x11     4.4e-09 / 1.0e-06  2.0e-09 / 1.0e-06  1.4e-08 / 1.0e-06  3.4e-07 / 4.0e-06
    flat_11x11    8.1e-09 / 1.0e-06  4.0e-09 / 1.0e-06  2.7e-08 / 1.0e-06  4.5e-07 / 2.4e-06
    tex_45x70     2.6e-09 / 1.0e-06  3.4e-09 / 1.0e-06  2.7e-08 / 1.0e-06  2.8e-06 / 1.5e-05
    flat_45x70    8.8e-08 / 2.2e-06  2.3e-09 / 1.0e-06  4.4e-07 / 1.1e-05  4.8e-06 / 5.0e-05
    tex_33x130    7.3e-10 / 1.0e-06  8.9e-10 / 1.0e-06  3.7e-08 / 1.0e-06  1.8e-06 / 1.4e-05
    flat_33x130   1.4e-08 / 1.0e-06  8.2e-10 / 1.0e-06  3.5e-08 / 1.6e-06  4.0e-06 / 4.4e-05
    tex_64x64     7.1e-09 / 1.0e-06  1.5e-09 / 1.0e-06  1.6e-08 / 1.0e-06  4.7e-06 / 1.3e-05
    flat_64x64    2.5e-07 / 4.8e-06  2.2e-09 / 1.0e-06  1.2e-06 / 2.4e-05  1.5e-05 / 7.5e-05
    tex_batch     2.5e-09 / 1.0e-06  8.1e-10 / 1.0e-06  2.9e-08 / 1.0e-06  1.8e-06 / 9.3e-06
    flat_batch    3.6e-09 / 1.0e-06  4.8e-10 / 1.0e-06  3.5e-08 / 1.0e-06  1.4e-06 / 9.3e-06
i.e. the gradient lands at 0.09 .. 0.35 of its bar (0.2 .. 0.7 of the reference's own float32 error where that sets the bar);
end to end (render -> loss -> backward against the same render fed the fused dL/dimg): 1.2e-7.  The file runs in 3.4 s.
"""
import math

import numpy as np
import pytest
import torch

import loss_helpers as LH
from helpers import assert_grads_close, make_case, settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).reshape(-1).view(np.uint32)


def _inputs(case, requires_grad=True):
    fx = LH.fixture()
    x = torch.from_numpy(fx[f"{case}/x"]).to(DEV).requires_grad_(requires_grad)
    return x, torch.from_numpy(fx[f"{case}/y"]).to(DEV)


def _run(case, scale=None):
    from gaussianeditor_amd.losses import photometric_loss

    x, y = _inputs(case)
    loss, l1, ssim = photometric_loss(x, y, lambda_dssim=LH.LAMBDA, return_terms=True)
    (loss if scale is None else scale * loss).backward()
    torch.cuda.synchronize()
    return loss, l1, ssim, x.grad


@pytest.mark.parametrize("case", LH.CASES)
def test_loss_terms_and_gradient_against_float64(case):
    e, bar = LH.expectation(case), LH.fixture_bar(case)
    gmax, n = float(np.abs(e["grad"]).max()), e["grad"].size
    # discrimination, asserted on the expectation: dropping either term misses this case's bar by far
    need = min(100, n // 4)
    for k in ("grad_l1", "grad_ssim"):
        assert int((np.abs(e[k]) > 10 * bar["grad"]).sum()) >= need, (case, k)
    if case.endswith(("45x70", "batch")):
        for k in ("grad_l1", "grad_ssim"):
            assert int((np.abs(e[k]) > 0.1 * gmax).sum()) >= 100, (case, k)
    loss, l1, ssim, grad = _run(case)
    assert loss.shape == () and loss.requires_grad and not l1.requires_grad and not ssim.requires_grad
    assert grad.shape == tuple(LH.fixture()[f"{case}/x"].shape) and grad.dtype == torch.float32
    got = dict(loss=loss.detach().item(), l1=l1.item(), ssim=ssim.item())
    err = {k: abs(got[k] - e[k]) for k in got}
    err["grad"] = float(np.abs(grad.cpu().numpy().astype(np.float64) - e["grad"]).max())
    print(f"  {case}: " + "  ".join(f"{k} {err[k] / (gmax if k == 'grad' else 1.0):.1e} (bar {bar[k] / (gmax if k == 'grad' else 1.0):.1e})"
                                   for k in ("loss", "l1", "ssim", "grad")) + "  [grad: of its maximum]")
    for k in ("loss", "l1", "ssim", "grad"):
        assert err[k] <= bar[k], (case, k, err[k], bar[k])


def test_upstream_gradient_scales_within_one_ulp():
    g1, g2 = _run("tex_45x70")[3], _run("tex_45x70", scale=3.5)[3]
    want = 3.5 * g1
    ulp = torch.abs(torch.nextafter(want, torch.full_like(want, math.inf)) - want)
    assert bool((g2 != g1).any()) and bool((torch.abs(g2 - want) <= ulp).all())


def test_two_runs_give_the_same_bits():
    a, b = _run("flat_33x130"), _run("flat_33x130")
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v))


def _peak_bytes(fn):
    """(result, device bytes the call allocated at its peak, above what was allocated before it)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def test_metric_path_gives_the_training_value_and_allocates_no_maps():
    """The maps are 12 N bytes (113 400 at 3 x 45 x 70); everything else a forward allocates is the workspace and the three
    output floats (a few 512-byte blocks).  Under torch.no_grad() no maps may be allocated even when the image requires a
    gradient; nor in grad mode when it does not."""
    from gaussianeditor_amd import losses

    x, y = _inputs("tex_45x70", requires_grad=True)
    maps_bytes = 12 * x.numel()
    t = _run("tex_45x70")

    def metric(img):
        with torch.no_grad():
            return losses.photometric_loss(img, y, return_terms=True), losses.ssim(img, y)

    for img in (x, x.detach()):
        (m, s), peak = _peak_bytes(lambda: metric(img))
        assert peak < maps_bytes // 8, (peak, maps_bytes)
        assert not m[0].requires_grad and m[0].grad_fn is None
        for u, w in zip(m, t[:3]):
            assert np.array_equal(_bits(u), _bits(w))
        assert np.array_equal(_bits(s), _bits(t[2]))
    m2, peak = _peak_bytes(lambda: losses.photometric_loss(x.detach(), y, return_terms=True))  # grad mode, nothing to differentiate
    assert peak < maps_bytes // 8 and not m2[0].requires_grad and np.array_equal(_bits(m2[0]), _bits(t[0]))
    # the training path does allocate them (the measurement sees what it is meant to see)
    tr, peak = _peak_bytes(lambda: losses.photometric_loss(x, y))
    assert peak >= maps_bytes and tr.requires_grad and np.array_equal(_bits(tr), _bits(t[0]))
    with pytest.raises(RuntimeError):  # the backward is once-differentiable: no silent second-order graph
        g, = torch.autograd.grad(losses.photometric_loss(x, y), x, create_graph=True)
        g.sum().backward()


def test_channels_last_view_gives_the_bits_of_its_contiguous_copy():
    from gaussianeditor_amd.losses import photometric_loss

    fx = LH.fixture()
    xs, ys = (torch.from_numpy(fx[f"tex_batch/{k}"]).to(DEV) for k in ("x", "y"))
    outs = []
    for nc in (False, True):
        x, y = xs.clone(), ys.clone()
        if nc:
            x, y = (t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for t in (x, y))  # NHWC storage, NCHW view
            assert not x.is_contiguous()
        x.requires_grad_(True)
        loss = photometric_loss(x, y)
        loss.backward()
        assert x.grad.shape == xs.shape
        outs.append((loss, x.grad.contiguous()))
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and np.array_equal(_bits(outs[0][1]), _bits(outs[1][1]))


def test_ssim_and_l1_alone_agree_with_the_combined_terms():
    from gaussianeditor_amd import losses

    case = "flat_45x70"
    e = LH.expectation(case)
    loss, l1, ssim, grad = _run(case)
    x, y = _inputs(case)
    a = losses.l1_loss(x, y)
    a.backward()
    g_l1 = x.grad.clone()
    x.grad = None
    s = losses.ssim(x, y)
    s.backward()
    g_s = x.grad.clone()
    assert np.array_equal(_bits(a), _bits(l1)) and np.array_equal(_bits(s), _bits(ssim))
    # the L1 gradient is exactly sign / N (0 where the images are equal), the two alone recombine to the combined gradient
    n = x.numel()
    sign = torch.sign(x.detach() - y)
    assert bool((sign == 0).any()) and np.array_equal(_bits(g_l1), _bits(sign * np.float32(1.0 / n)))
    gmax = float(np.abs(e["grad"]).max())
    comb = (0.8 * g_l1.double() - 0.2 * g_s.double()).cpu().numpy()
    assert np.abs(comb - grad.cpu().numpy()).max() <= 1e-6 * gmax
    assert np.abs(g_s.cpu().numpy() * -0.2 - e["grad_ssim"]).max() <= LH.fixture_bar(case)["grad"]
    # and the trainers' line written with the two functions
    assert abs((0.8 * a + 0.2 * (1.0 - s)).detach().item() - loss.detach().item()) <= 1e-6


def test_gt_gets_no_gradient_and_is_refused_if_it_wants_one():
    from gaussianeditor_amd.losses import photometric_loss

    x, y = _inputs("tex_11x11")
    photometric_loss(x, y).backward()
    assert y.grad is None and x.grad is not None
    with pytest.raises(RuntimeError, match="gt requires a gradient"):
        photometric_loss(x, y.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        photometric_loss(x.detach().cpu(), y.cpu())


def test_render_then_loss_end_to_end():
    """Route one: render -> photometric_loss -> backward.  Route two: the same render, image.backward(gradient = the fused
    dL/dimg).  The same bits enter the rasterizer's backward on both routes, so only K7's run-to-run order differs."""
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer
    from gaussianeditor_amd.losses import photometric_loss

    case = make_case(2000, 64, 64, s0=0.05)
    sc, H, W = case["sc"], case["H"], case["W"]
    gt = torch.from_numpy(LH.image_pair((3, H, W), 77, False)[1]).to(DEV)
    names = ("xyz", "scaling", "rotation", "opacity", "features")

    def render():
        leaves = {k: sc[k].to(DEV).requires_grad_(True) for k in names}
        m2d = torch.zeros_like(leaves["xyz"], requires_grad=True)
        image = GaussianRasterizer(settings(case, DEV))(leaves["xyz"], m2d, leaves["opacity"], shs=leaves["features"],
                                                        scales=leaves["scaling"], rotations=leaves["rotation"])[0]
        return image, leaves, m2d

    def grads(leaves, m2d):
        torch.cuda.synchronize()
        return dict(dL_dmeans3D=leaves["xyz"].grad.cpu().numpy(), dL_dscales=leaves["scaling"].grad.cpu().numpy(),
                    dL_drotations=leaves["rotation"].grad.cpu().numpy(), dL_dopacity=leaves["opacity"].grad.cpu().numpy(),
                    dL_dsh=leaves["features"].grad.cpu().numpy(), dL_dmeans2D=m2d.grad.cpu().numpy())

    image, leaves, m2d = render()
    photometric_loss(image, gt).backward()
    one = grads(leaves, m2d)
    image2, leaves2, m2d2 = render()
    assert np.array_equal(_bits(image), _bits(image2))
    leaf = image2.detach().clone().requires_grad_(True)
    photometric_loss(leaf, gt).backward()
    image2.backward(gradient=leaf.grad)
    two = grads(leaves2, m2d2)
    assert int((np.abs(one["dL_dmeans3D"]).max(axis=1) > 0).sum()) >= 100
    worst = assert_grads_close(one, two, tol=1e-5, tag="render + loss")
    print(f"  end to end: worst {worst:.1e}")
