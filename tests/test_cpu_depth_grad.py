"""Depth gradients (opt-in, gaussianeditor_amd.set_depth_grad; include/gsr.h GSR_FLAG_DEPTH_GRAD) without a GPU: the
switch and its per-thread override, argument validation of the new entry points, and the yardstick the GPU tests use --
the linearity construction of depth_helpers -- against float64 autograd."""
import ctypes
import threading

import numpy as np
import pytest
import torch

from depth_helpers import depth_colors, depth_expectation
from helpers import make_case, oracle_forward, rel_err, seed_gradient


def test_set_depth_grad_round_trip():
    import gaussianeditor_amd
    from gaussianeditor_amd import options

    assert not gaussianeditor_amd.get_depth_grad() and options.current_flags() == 0
    gaussianeditor_amd.set_fast_exp(True)
    gaussianeditor_amd.set_depth_grad(True)
    try:
        assert gaussianeditor_amd.get_depth_grad() and gaussianeditor_amd.get_fast_exp()
        assert options.current_flags() == options.FLAG_DEPTH_GRAD | options.FLAG_FAST_EXP == 66
        gaussianeditor_amd.set_depth_grad(False)
        assert not gaussianeditor_amd.get_depth_grad() and options.current_flags() == options.FLAG_FAST_EXP
    finally:
        gaussianeditor_amd.set_depth_grad(False)
        gaussianeditor_amd.set_fast_exp(False)
    assert options.current_flags() == 0


def test_depth_flag_override_is_per_thread_and_unknown_bits_are_refused():
    from gaussianeditor_amd import options

    assert options.FLAG_DEPTH_GRAD == 64 and options.FLAG_ALL & options.FLAG_DEPTH_GRAD
    options.set_default_flags(options.FLAG_DEPTH_GRAD)  # caller-settable
    options.set_default_flags(0)
    seen = {}
    with options.override(options.FLAG_DEPTH_GRAD):
        assert options.current_flags() == 64
        t = threading.Thread(target=lambda: seen.setdefault("other", options.current_flags()))
        t.start()
        t.join()
    assert seen["other"] == 0 and options.current_flags() == 0
    for bad in (8, 128, 64 | 256):
        with pytest.raises(ValueError):
            options.set_default_flags(bad)
        with pytest.raises(ValueError):
            with options.override(bad):
                pass


def test_depth_flag_never_reaches_the_forward_entry_points():
    """The library's forward / trace / plain backward entry points refuse the bit; the binding keeps it to itself."""
    from gaussianeditor_amd import _native, options
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    with options.override(options.FLAG_DEPTH_GRAD | options.FLAG_FAST_EXP):
        assert _C._flags(None) == options.FLAG_FAST_EXP
    assert _C._flags(options.FLAG_DEPTH_GRAD) == 0
    assert _native.ACC_DEPTH == 11 and _native.ACC_DEPTH == _native.ACC_COLOR + 3


def test_depth_entry_points_validate_arguments_without_a_gpu():
    from gaussianeditor_amd import _native

    L = _native.lib()
    one = ctypes.c_void_p(256)
    acc = ctypes.c_void_p(1 << 12)  # (64-byte aligned)
    # (P = 0: nothing to do, no pointer is looked at)
    assert L.gsr_blend_backward_depth(None, 0, 5, 64, 64, None, None, None, None, None, None, None, None, 0) == 0
    # negative sizes, unknown flags, forward-only / self-clean on the blend half, a misaligned table, no depth gradient
    assert L.gsr_blend_backward_depth(None, -1, 5, 64, 64, one, one, one, one, one, one, acc, None, 0) == -1
    assert L.gsr_blend_backward_depth(None, 10, -5, 64, 64, one, one, one, one, one, one, acc, None, 0) == -1
    assert L.gsr_blend_backward_depth(None, 10, 5, -64, 64, one, one, one, one, one, one, acc, None, 0) == -1
    assert L.gsr_blend_backward_depth(None, 10, 5, 64, 64, one, one, one, one, one, one, acc, None, 128) == -1
    assert L.gsr_blend_backward_depth(None, 10, 5, 64, 64, one, one, one, one, one, one, acc, None, 8) == -1
    assert L.gsr_blend_backward_depth(None, 10, 5, 64, 64, one, one, one, one, one, one, acc, None, 32) == -1
    assert L.gsr_blend_backward_depth(None, 10, 5, 64, 64, one, one, one, one, one, one, ctypes.c_void_p(4096 + 16),
                                      None, 0) == -1
    assert L.gsr_blend_backward_depth(None, 10, 5, 64, 64, one, one, one, one, one, None, acc, None, 64) == -1
    assert L.gsr_blend_backward_depth(None, 10, 5, 64, 64, None, one, one, one, one, one, acc, None, 64) == -1
    assert L.gsr_blend_backward_depth(None, 10, 5, 16400, 16400, one, one, one, one, one, one, acc, None, 0) == -1
    # the plain halves keep refusing the bit (their depth-aware twins take it)
    assert L.gsr_blend_backward(None, 10, 5, 64, 64, one, one, one, one, one, acc, None, 64) == -1

    def full(P, R, flags, dL_ddepth=one, acc_=acc, binning=one, m3=one):
        return L.gsr_backward_depth(None, P, 3, 16, R, 64, 64, one, m3, one, None, one, 1.0, one, None, one, one, one, 1.0, 1.0,
                                    one, one, binning, one, one, dL_ddepth, acc_, one, one, None, one, None, one, one, one,
                                    flags)
    assert full(0, 5, 0) == 0
    assert full(-1, 5, 0) == -1
    assert full(10, 5, 1 << 9) == -1
    assert full(10, 5, 32 | 4) == -1  # self-clean and clear together
    assert full(10, 5, 0, binning=None) == -1
    assert full(10, 5, 0, dL_ddepth=None) == -1
    assert full(10, 5, 0, acc_=ctypes.c_void_p(4096 + 8)) == -1
    # K8+K9 alone: the flag is accepted next to GSR_FLAG_ACC_SELF_CLEAN, other bits are not; missing arrays are refused
    pb = lambda flags, m3=one: L.gsr_preprocess_backward(  # noqa: E731
        None, 10, 3, 16, 64, 64, m3, one, one, 1.0, one, None, one, one, one, 1.0, 1.0, one, one, acc, one, one, None, one,
        None, one, one, one, flags)
    assert pb(64 | 4) == -1 and pb(64 | 8) == -1
    assert pb(64, m3=None) == -1 and pb(64 | 32, m3=None) == -1
    pr = lambda flags: L.gsr_preprocess_backward_rgb(  # noqa: E731
        None, 10, 3, 16, 64, 64, None, one, one, 1.0, one, None, one, one, one, 1.0, 1.0, one, one, acc, one, one, one, None,
        one, one, one, flags)
    assert pr(64 | 2) == -1 and pr(64) == -1  # (no means3D)


def _tz(xyz, view):
    """view-space z of every mean, differentiably (row-vector convention of oracle.torch_ref: p_view = (x, y, z, 1) @ V)."""
    V = view.to(xyz.dtype).reshape(4, 4)
    return xyz @ V[:3, 2] + V[3, 2]


@pytest.mark.parametrize("depth_only", [False, True])
def test_linearity_expectation_equals_float64_autograd(oracle, depth_only):
    """The GPU tests' expectation (float32 oracle, two existing backwards added) == float64 autograd of the loss
    <gC, C> + <gD, D>, D rendered as the colour image of colours (tz(means3D), 0, 0) on background 0."""
    from oracle.torch_ref import render_f64

    W, H, P = 48, 40, 150
    case = make_case(P, W, H, seed=4, s0=0.1, view=2, scale_xyz=0.5)
    sc, cam = case["sc"], case["cam"]
    cols = torch.rand(P, 3, generator=torch.Generator().manual_seed(5))
    G = None if depth_only else seed_gradient(H, W, 2) * H * W
    GD = seed_gradient(H, W, 7)[:1] * H * W
    want = depth_expectation(oracle, case, G, GD, colors_precomp=cols)
    f = oracle_forward(oracle, case, colors_precomp=cols)
    assert (f["radii"] > 0).sum() > 20
    # (the oracle's K1 depths are the view-space z that the f64 construction differentiates)
    vis = f["radii"] > 0
    assert rel_err(depth_colors(f["depths"])[vis, 0].numpy(), _tz(sc["xyz"].double(), cam.world_view_transform)[vis].numpy()) < 1e-6
    d = torch.float64
    xyz, op = sc["xyz"].to(d).requires_grad_(True), sc["opacity"].to(d).requires_grad_(True)
    scl, rot = sc["scaling"].to(d).requires_grad_(True), sc["rotation"].to(d).requires_grad_(True)
    c64 = cols.to(d).requires_grad_(True)
    args = (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)
    loss = 0.0
    if not depth_only:
        img = render_f64(f, xyz, None, op, scl, rot, None, c64, None, *args, case["bg"], W, H, case["tfx"], case["tfy"], 1.0, 0)
        loss = (img * G.to(d)).sum()
    z = _tz(xyz, cam.world_view_transform)
    dimg = render_f64(f, xyz, None, op, scl, rot, None, torch.stack([z, torch.zeros_like(z), torch.zeros_like(z)], 1), None,
                      *args, torch.zeros(3), W, H, case["tfx"], case["tfy"], 1.0, 0)
    loss = loss + (dimg[0] * GD[0].to(d)).sum()
    loss.backward()
    for k, t in (("dL_dmeans3D", xyz), ("dL_dopacity", op), ("dL_dscales", scl), ("dL_drotations", rot)):
        e = rel_err(want[k].reshape(t.shape), t.grad.numpy())
        assert e < 2e-5, (k, e)
    if not depth_only:
        assert rel_err(want["dL_dcolors"].reshape(c64.shape), c64.grad.numpy()) < 2e-5
    # the depth share is really there: without it the means3D gradient is a different one
    assert np.abs(want["dL_ddepth"]).max() > 0
