"""Antialiased rendering (opt-in, gaussianeditor_amd.set_antialiasing; include/gsr.h GSR_FLAG_ANTIALIAS) without a GPU: the
switch and its per-thread override, argument validation of the entry points that read or accept the bit, and the yardstick
the GPU tests use -- the float64 opacity factor h of aa_helpers -- against finite differences and against the purpose of
the filter."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import aa_helpers as A
from helpers import oracle_forward

ONE = ctypes.c_void_p(256)
ACC = ctypes.c_void_p(1 << 12)  # (64-byte aligned)


def test_flag_value_setter_and_per_thread_override():
    import gaussianeditor_amd
    from gaussianeditor_amd import options

    # (1024, not 512: tests/test_cpu_depth_grad.py pins 128, 256 and 512 as bits the library refuses)
    assert options.FLAG_ANTIALIAS == 1024 and options.FLAG_ALL & options.FLAG_ANTIALIAS
    assert not gaussianeditor_amd.get_antialiasing() and options.current_flags() == 0
    gaussianeditor_amd.set_antialiasing(True)
    gaussianeditor_amd.set_depth_grad(True)
    try:
        assert gaussianeditor_amd.get_antialiasing()
        assert options.current_flags() == options.FLAG_ANTIALIAS | options.FLAG_DEPTH_GRAD
        gaussianeditor_amd.set_antialiasing(False)
        assert not gaussianeditor_amd.get_antialiasing() and options.current_flags() == options.FLAG_DEPTH_GRAD
    finally:
        gaussianeditor_amd.set_antialiasing(False)
        gaussianeditor_amd.set_depth_grad(False)
    assert options.current_flags() == 0
    seen = {}
    with options.override(options.FLAG_ANTIALIAS):
        assert options.current_flags() == 1024 and not gaussianeditor_amd.get_antialiasing()
        t = threading.Thread(target=lambda: seen.setdefault("other", options.current_flags()))
        t.start()
        t.join()
    assert seen["other"] == 0 and options.current_flags() == 0
    for bad in (128, 256, 512, 128 | 1024):
        with pytest.raises(ValueError):
            options.set_default_flags(bad)
        with pytest.raises(ValueError):
            with options.override(bad):
                pass


def test_binding_keeps_the_bit_and_the_header_agrees():
    import os

    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import _C, _reuse

    # the forward, backward and trace calls of a render all receive it (only FLAG_DEPTH_GRAD is the binding's own)
    assert _C._flags(options.FLAG_ANTIALIAS | options.FLAG_DEPTH_GRAD) == options.FLAG_ANTIALIAS
    with options.override(options.FLAG_ANTIALIAS | options.FLAG_FAST_EXP):
        assert _C._flags(None) == options.FLAG_ANTIALIAS | options.FLAG_FAST_EXP
    # a render under the flag leaves another state: it never serves a render without it (or the other way round)
    assert not _reuse._IGNORED_FLAGS & options.FLAG_ANTIALIAS
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsr.h")).read()
    assert "#define GSR_FLAG_ANTIALIAS 1024u" in hdr and "#define GSR_ABI_VERSION 6" in hdr
    assert "#define GSR_FLAG_ALL (127u | GSR_FLAG_ANTIALIAS)" in hdr


def test_entry_points_accept_or_refuse_the_bit_without_a_gpu():
    """The bit is accepted where include/gsr.h says so: each call below gets otherwise invalid arguments, so an accepted
    bit shows as the same GSR_ERR_BAD_ARGUMENT the call returns without it -- and a refused one as -1 with VALID arguments
    where the flags are checked first (no call here reaches the device)."""
    from gaussianeditor_amd import _native

    L = _native.lib()
    AA = 1024
    r = (ctypes.c_int64 * 2)()
    tk = ctypes.c_void_p()
    # K1: read (P = 0 is an empty call, with or without the bit; a missing geometry buffer is refused either way)
    for f in (0, AA, AA | 1):
        assert L.gsr_preprocess(None, 0, 3, 16, None, None, 1.0, None, None, None, None, None, None, None, None, 64, 64, 1.0,
                                1.0, 0, 0, f, None, None, r) == 0
        assert L.gsr_preprocess(None, 10, 3, 16, ONE, ONE, 1.0, ONE, ONE, ONE, None, None, ONE, ONE, ONE, 64, 64, 1.0, 1.0,
                                0, 0, f, ONE, None, r) == -1
        assert L.gsr_preprocess_begin(None, 10, 3, 16, ONE, ONE, 1.0, ONE, ONE, ONE, None, None, ONE, ONE, ONE, 64, 64, 1.0,
                                      1.0, 0, 0, f, ONE, None, ctypes.byref(tk)) == -1
    # the neighbouring unknown bits stay refused everywhere
    for bad in (512, 2048, AA | 512):
        assert L.gsr_blend_forward(None, 10, 5, 64, 64, ONE, ONE, ONE, ONE, ONE, ONE, bad) == -1
        assert L.gsr_blend_backward(None, 10, 5, 64, 64, ONE, ONE, ONE, ONE, ONE, ACC, None, bad) == -1
        assert L.gsr_trace_weights(None, 10, 5, 64, 64, 1, ONE, ONE, ONE, ONE, ONE, ONE, bad) == -1
    # blend / trace: accepted and ignored (R = 0: nothing to blend, nothing is launched)
    assert L.gsr_blend_backward(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ACC, None, AA) == 0
    assert L.gsr_blend_backward_depth(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ONE, ACC, None, AA | 64) == 0
    assert L.gsr_trace_weights(None, 10, 0, 64, 64, 1, ONE, ONE, ONE, ONE, ONE, ONE, AA) == 0
    assert L.gsr_blend_forward(None, 10, 5, -64, 64, ONE, ONE, ONE, ONE, ONE, ONE, AA) == -1  # (the size, not the bit)
    # K8+K9: read by every entry point (m3 = None is the argument error that stops each call before the device)
    pb = lambda flags, m3=ONE: L.gsr_preprocess_backward(  # noqa: E731
        None, 10, 3, 16, 64, 64, m3, ONE, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE, ACC, ONE, ONE, None, ONE,
        None, ONE, ONE, ONE, flags)
    assert pb(AA | 512) == -1 and pb(AA | 4) == -1
    assert pb(0, m3=None) == -1 and pb(AA | 32 | 64, m3=None) == -1
    assert L.gsr_preprocess_backward(None, 0, 3, 16, 64, 64, None, None, None, 1.0, None, None, None, None, None, 1.0, 1.0,
                                     None, None, None, None, None, None, None, None, None, None, None, AA | 32) == 0
    pr = lambda flags: L.gsr_preprocess_backward_rgb(  # noqa: E731
        None, 10, 3, 16, 64, 64, None, ONE, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE, ACC, ONE, ONE, ONE, None,
        ONE, ONE, ONE, flags)
    assert pr(AA | 2) == -1 and pr(AA) == -1  # (no means3D)

    def rows(flags, row_state=ONE, P=10):
        return L.gsr_preprocess_backward_rows_flags(
            None, P, 3, 16, 64, 64, None, ONE, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE, ACC, ONE, ONE, None,
            ONE, None, ONE, None, ONE, ONE, row_state, flags)
    # the twin: 0 and the bit, nothing else; P = 0 with the bit is an empty call, as without it
    for bad in (1, 32, 64, 512, AA | 64, AA | 32):
        assert rows(bad, P=0) == -1
    assert rows(0, P=0) == 0 and rows(AA, P=0) == 0
    assert rows(AA, row_state=None) == -1 and rows(AA) == -1  # (no row state; no means3D)

    def full(fn, flags, m3=ONE, depth=False):
        extra = (ONE,) if depth else ()
        return fn(None, 10, 3, 16, 5, 64, 64, ONE, m3, ONE, None, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE, ONE,
                  ONE, ONE, *extra, ACC, ONE, ONE, None, ONE, None, ONE, ONE, ONE, flags)
    for fn, dep in ((L.gsr_backward, False), (L.gsr_backward_depth, True)):
        assert full(fn, AA | 512, depth=dep) == -1
        assert full(fn, AA | 32 | 4, depth=dep) == -1  # self-clean and clear together, with the bit as without it
        assert full(fn, AA | 8, depth=dep) == -1       # a forward-only view has no backward


def test_h_matches_finite_differences():
    """The float64 h of aa_helpers (and the r it is made of) against central differences on a tiny case: the derivative
    autograd then carries to means3D, scales and rotations is the derivative of the stated formula."""
    case = A.sparse_case(40, 32, n_side=3, sigma_world=0.02)
    d = torch.float64
    g = torch.Generator().manual_seed(3)
    sc = case["sc"]
    xyz = (sc["xyz"].to(d) + 0.05 * torch.randn(9, 3, generator=g, dtype=d)).requires_grad_(True)
    scl = (sc["scaling"].to(d) * torch.exp(0.5 * torch.randn(9, 3, generator=g, dtype=d))).requires_grad_(True)
    rot = (torch.tensor([[1.0, 0, 0, 0]], dtype=d) + 0.3 * torch.randn(9, 4, generator=g, dtype=d)).requires_grad_(True)
    cam = case["cam"]

    def h_of(xyz, scl, rot):
        x, y, z = A.cov2d_f64(xyz, scl, rot, None, cam.world_view_transform, 40, 32, case["tfx"], case["tfy"])
        return A.h_f64(x, y, z)
    h = h_of(xyz, scl, rot)
    assert (h > 0.05).all() and (h < 0.99).all()  # (every row is in the filter's range, none on the floor)
    wts = torch.rand(9, generator=g, dtype=d)
    (h * wts).sum().backward()
    eps = 1e-6
    for t, name in ((xyz, "means3D"), (scl, "scales"), (rot, "rotations")):
        num = torch.zeros_like(t)
        with torch.no_grad():
            for idx in np.ndindex(*t.shape):
                tp, tm = t.detach().clone(), t.detach().clone()
                tp[idx] += eps
                tm[idx] -= eps
                args = {"means3D": (tp, scl.detach(), rot.detach()), "scales": (xyz.detach(), tp, rot.detach()),
                        "rotations": (xyz.detach(), scl.detach(), tp)}[name]
                argm = {"means3D": (tm, scl.detach(), rot.detach()), "scales": (xyz.detach(), tm, rot.detach()),
                        "rotations": (xyz.detach(), scl.detach(), tm)}[name]
                num[idx] = ((h_of(*args) - h_of(*argm)) * wts).sum() / (2 * eps)
        err = float((num - t.grad).abs().max() / t.grad.abs().max())
        assert err < 1e-6, (name, err)
    # r against its closed form for a diagonal footprint, and the floor
    x, y, z = torch.tensor([0.1, 4.0, 1e-9], dtype=d), torch.tensor([0.2, 9.0, 1e-9], dtype=d), torch.zeros(3, dtype=d)
    r = A.ratio_f64(x, y, z)
    assert torch.allclose(r, x * y / ((x + 0.3) * (y + 0.3)))
    assert float(A.h_f64(x, y, z)[2]) == pytest.approx(np.sqrt(2.5e-5))


def test_intent_sparse_sub_pixel_scene_keeps_its_mass_across_resolutions(oracle):
    """What the filter is for.  A 12 x 12 grid of isolated round Gaussians (3D sigma 0.004 at distance 4, 30 degree fov:
    sigma ~ 0.5 px at 512 x 512, 0.12 px at 128 x 128), colour 1 on black, opacity 0.6.  The screen-space mass
    sum(1 - T_final) x pixel area (aa_helpers.coverage) is what the scene looks like from afar.  At 512 x 512 the footprints
    are about a pixel wide.  At a quarter of that resolution, without the filter, every Gaussian becomes the 0.55 px blob
    of the dilation at full opacity: the mass is 4.7 x the full-resolution one.  With the filter it stays within 10 %
    (measured 0.97 x); the bars are 1.15 and 3, far from both."""
    cov = {}
    for aa in (False, True):
        for W in (512, 128):
            c = A.sparse_case(W, W)
            h = A.h_of_case(c)[0]
            sc = dict(c["sc"])
            if aa:
                sc["opacity"] = (sc["opacity"].double() * torch.from_numpy(h)[:, None]).float()
            f = oracle_forward(oracle, dict(c, sc=sc), colors_precomp=torch.ones(sc["xyz"].shape[0], 3))
            assert (f["radii"] > 0).all()
            cov[aa, W] = A.coverage(f["final_T"], W, W)
            if W == 128:
                assert np.median(h) < 0.25  # (sub-pixel: the filter is active)
    plain, aa = cov[False, 128] / cov[False, 512], cov[True, 128] / cov[True, 512]
    print(f"  mass at 1/4 resolution over full resolution: plain {plain:.3f}, antialiased {aa:.3f}")
    assert plain > 3.0
    assert abs(aa - 1.0) < 0.15


@pytest.mark.parametrize("name", A.NEW_CASES)
def test_new_regimes_hit_their_regime(oracle, name):
    """The three regimes only the flag has are built to be hit (counted on the float32 oracle and the float64 h)."""
    r = A.regime(name)
    f = oracle_forward(oracle, r["case"], D=r["D"])
    h, ratio, x, y, z = A.h_of_case(r["case"])
    assert A.aa_regime_count(r, f, dict(r=ratio, x=x, y=y, z=z)) > 0
