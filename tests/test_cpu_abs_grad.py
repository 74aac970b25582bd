"""Absolute screen-space gradients (opt-in, gaussianeditor_amd.set_abs_grad; include/gsr.h GSR_FLAG_ABS_GRAD) without a GPU:
the switch and its per-thread override, which entry points take the bit, argument validation of gsr_abs_grad_take, the
yardstick of the GPU tests -- the per-pixel construction of abs_helpers -- against float64 autograd, and the L1 layer
(`means2D.absgrad`) over a CPU stand-in for `_C`."""
import ctypes
import os
import threading

import numpy as np
import pytest
import torch

import abs_helpers as AB
import f64_regimes as R
from helpers import assert_grads_close, make_case, oracle_forward, seed_gradient, settings

ONE = ctypes.c_void_p(256)
ACC = ctypes.c_void_p(1 << 12)  # (64-byte aligned)
ABS = 4096


def test_flag_value_setter_and_per_thread_override():
    import gaussianeditor_amd
    from gaussianeditor_amd import options

    assert options.FLAG_ABS_GRAD == ABS and options.FLAG_ALL & options.FLAG_ABS_GRAD
    assert not gaussianeditor_amd.get_abs_grad() and options.current_flags() == 0
    gaussianeditor_amd.set_abs_grad(True)
    gaussianeditor_amd.set_depth_grad(True)
    try:
        assert gaussianeditor_amd.get_abs_grad()
        assert options.current_flags() == options.FLAG_ABS_GRAD | options.FLAG_DEPTH_GRAD
        gaussianeditor_amd.set_abs_grad(False)
        assert not gaussianeditor_amd.get_abs_grad() and options.current_flags() == options.FLAG_DEPTH_GRAD
    finally:
        gaussianeditor_amd.set_abs_grad(False)
        gaussianeditor_amd.set_depth_grad(False)
    assert options.current_flags() == 0
    seen = {}
    with options.override(options.FLAG_ABS_GRAD):
        assert options.current_flags() == ABS and not gaussianeditor_amd.get_abs_grad()
        t = threading.Thread(target=lambda: seen.setdefault("other", options.current_flags()))
        t.start()
        t.join()
    assert seen["other"] == 0 and options.current_flags() == 0
    for bad in (128, 256, 512, 2048, 8192, ABS | 2048):
        with pytest.raises(ValueError):
            options.set_default_flags(bad)
        with pytest.raises(ValueError):
            with options.override(bad):
                pass


def test_binding_keeps_the_bit_to_itself_and_the_header_agrees():
    from gaussianeditor_amd import _native, options
    from gaussianeditor_amd.diff_gaussian_rasterization import _C, _reuse

    assert _C._flags(options.FLAG_ABS_GRAD) == 0
    assert _C._flags(options.FLAG_ABS_GRAD | options.FLAG_ANTIALIAS | options.FLAG_DEPTH_GRAD) == options.FLAG_ANTIALIAS
    with options.override(options.FLAG_ABS_GRAD | options.FLAG_FAST_EXP):
        assert _C._flags(None) == options.FLAG_FAST_EXP
    # a forward under the flag leaves the state of one without it: either serves the other's colour-override render
    assert _reuse._IGNORED_FLAGS & options.FLAG_ABS_GRAD
    assert _native.ACC_ABS2D == 12 and _native.ACC_ROW == 16
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsr.h")).read()
    assert "#define GSR_FLAG_ABS_GRAD 4096u" in hdr and "#define GSR_ACC_ABS2D 12" in hdr
    assert "#define GSR_ABI_VERSION 6" in hdr and "#define GSR_FLAG_ALL (127u | GSR_FLAG_ANTIALIAS)" in hdr


def test_entry_points_accept_or_refuse_the_bit_without_a_gpu():
    """The bit is accepted by the two blend backwards (R = 0: nothing is launched) and by nothing else; its unknown
    neighbours stay refused; gsr_abs_grad_take validates its arguments.  No call here reaches the device."""
    from gaussianeditor_amd import _native

    L = _native.lib()
    # the blend halves: with the bit, alone and next to the other bits they take
    for f in (ABS, ABS | 2, ABS | 16, ABS | 1024):  # (not | 4: with R = 0 that bit is a clear of the table)
        assert L.gsr_blend_backward(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ACC, None, f) == 0
        assert L.gsr_blend_backward_depth(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ONE, ACC, None, f | 64) == 0
    assert L.gsr_blend_backward(None, 10, 5, -64, 64, ONE, ONE, ONE, ONE, ONE, ACC, None, ABS) == -1  # (the size, not the bit)
    assert L.gsr_blend_backward(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ACC, None, ABS | 64) == -1  # (depth: the twin)
    for bad in (128, 256, 512, 2048, 8192, ABS | 2048, ABS | 8192, ABS | 8, ABS | 32):
        assert L.gsr_blend_backward(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ACC, None, bad) == -1
        assert L.gsr_blend_backward_depth(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ONE, ACC, None, bad) == -1
    # forward, auxiliary forward, trace, K1: refused (valid sizes, R = 0 where that is an empty call without the bit)
    r = (ctypes.c_int64 * 2)()
    tk = ctypes.c_void_p()
    assert L.gsr_blend_forward(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ONE, ABS) == -1
    assert L.gsr_blend_forward_aux(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ONE, None, ABS) == -1
    assert L.gsr_trace_weights(None, 10, 0, 64, 64, 1, ONE, ONE, ONE, ONE, ONE, ONE, ABS) == -1
    assert L.gsr_trace_weights(None, 10, 0, 64, 64, 1, ONE, ONE, ONE, ONE, ONE, ONE, 0) == 0
    assert L.gsr_preprocess(None, 10, 3, 16, ONE, ONE, 1.0, ONE, ONE, ONE, None, None, ONE, ONE, ONE, 64, 64, 1.0, 1.0, 0, 0,
                            ABS, ONE, ONE, r) == -1
    assert L.gsr_preprocess_begin(None, 10, 3, 16, ONE, ONE, 1.0, ONE, ONE, ONE, None, None, ONE, ONE, ONE, 64, 64, 1.0, 1.0,
                                  0, 0, ABS, ONE, ONE, ctypes.byref(tk)) == -1
    # K8+K9: every entry point refuses it (P = 0 is an empty call without it: the flags are checked first)
    pb = lambda flags: L.gsr_preprocess_backward(  # noqa: E731
        None, 10, 3, 16, 64, 64, ONE, ONE, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE, ACC, ONE, ONE, None, ONE,
        None, ONE, ONE, ONE, flags)
    assert pb(ABS) == -1 and pb(ABS | 32) == -1
    pr = lambda flags: L.gsr_preprocess_backward_rgb(  # noqa: E731
        None, 10, 3, 16, 64, 64, ONE, ONE, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE, ACC, ONE, ONE, ONE, None,
        ONE, ONE, ONE, flags)
    assert pr(ABS) == -1
    rows = lambda flags: L.gsr_preprocess_backward_rows_flags(  # noqa: E731
        None, 0, 3, 16, 64, 64, None, ONE, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE, ACC, ONE, ONE, None, ONE,
        None, ONE, None, ONE, ONE, ONE, flags)
    assert rows(0) == 0 and rows(ABS) == -1

    # the fused backwards have no output for it: refused with otherwise valid arguments (R = 0, which they accept without it)
    def full(fn, flags, depth=False, R_=0):
        extra = (ONE,) if depth else ()
        return fn(None, 10, 3, 16, R_, 64, 64, ONE, None, ONE, None, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE, ONE,
                  ONE, ONE, *extra, ACC, ONE, ONE, None, ONE, None, ONE, ONE, ONE, flags)
    for fn, dep in ((L.gsr_backward, False), (L.gsr_backward_depth, True)):
        assert full(fn, ABS, depth=dep) == -1 and full(fn, ABS | 4, depth=dep) == -1 and full(fn, ABS | 32, depth=dep) == -1
        assert full(fn, 8192, depth=dep) == -1

    # gsr_abs_grad_take: P = 0 is an empty call; NULL acc / absgrad, a misaligned table and a negative P are refused
    take = L.gsr_abs_grad_take
    assert take(None, 0, None, None, None) == 0
    assert take(None, 10, None, ONE, ONE) == -1
    assert take(None, 10, ACC, ONE, None) == -1
    assert take(None, 10, ACC, None, None) == -1
    assert take(None, 10, ctypes.c_void_p(4096 + 16), ONE, ONE) == -1
    assert take(None, -1, ACC, ONE, ONE) == -1


def _f64_abs(case, f, G, pixels, GD=None):
    """sum_p |float64 autograd gradient of <G 1_p, C> (+ <GD 1_p, D>) by the means2D offset| -> (absgrad, signed, stats)."""
    from oracle.torch_ref import render_f64

    d = torch.float64
    sc, cam = case["sc"], case["cam"]
    P, W, H = sc["xyz"].shape[0], case["W"], case["H"]
    geo = (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)
    xyz, op, scl, rot, sh = (sc[k].to(d) for k in ("xyz", "opacity", "scaling", "rotation", "features"))
    stats = {}

    def term(y, x):
        m = AB.pixel_mask(H, W, [(y, x)]).to(d)
        m2 = torch.zeros(P, 3, dtype=d, requires_grad=True)
        render_f64(f, xyz, m2, op, scl, rot, sh, None, None, *geo, case["bg"], W, H, case["tfx"], case["tfy"], 1.0, case["D"],
                   dL_dimage=G.to(d) * m, stats=stats if not stats else None)
        if GD is not None:
            V = cam.world_view_transform.to(d).reshape(4, 4)
            tz = xyz @ V[:3, 2] + V[3, 2]
            dcol = torch.stack([tz, torch.zeros_like(tz), torch.zeros_like(tz)], dim=1)
            gd = torch.zeros(3, H, W, dtype=d)
            gd[0] = (GD.to(d) * m).reshape(H, W)
            render_f64(f, xyz, m2, op, scl, rot, None, dcol, None, *geo, torch.zeros(3), W, H, case["tfx"], case["tfy"], 1.0,
                       case["D"], dL_dimage=gd)
        return m2.grad.numpy()
    a, s = AB.abs_sum(term, pixels, P)
    return a, s, stats


@pytest.mark.parametrize("with_depth", [False, True])
def test_expectation_builder_equals_float64_autograd(oracle, with_depth):
    """The GPU tests' expectation (per-pixel float32 oracle backwards, summed in absolute value) == per-pixel float64
    autograd backwards of render_f64 summed in absolute value, within the project's float32-vs-float64 bar (f64_regimes.TOL),
    rows under pixels whose discrete decisions differ counted and masked as f64_regimes.masked_rows does.  Measured: max
    difference 4.2e-7 of the tensor's maximum over 263 rows with a gradient (colour loss; 4.0e-7 over 189 with the depth loss),
    nothing masked."""
    W = H = 64
    case = make_case(2000, W, H, s0=0.05)
    G = seed_gradient(H, W, 3) * H * W
    GD = seed_gradient(H, W, 7)[:1] * H * W if with_depth else None
    pixels = AB.block_pixels(H, W, 4 if with_depth else 6)
    f = oracle_forward(oracle, case)
    want, signed64, stats = _f64_abs(case, f, G, pixels, GD)
    got, signed32 = AB.abs_expectation(oracle, case, G, pixels, GD=GD)
    masked, report = R.masked_rows(dict(case=case, name="absgrad"), f, stats)
    live, disc = AB.assert_discriminates(want, signed64, tag="float64 per-pixel expectation")
    worst = assert_grads_close(dict(absgrad=got), dict(absgrad=want), tol=R.TOL, tag="oracle-built absgrad vs float64",
                               masked=masked)
    assert_grads_close(dict(signed=signed32), dict(signed=signed64), tol=R.TOL, tag="signed per-pixel sum vs float64",
                       masked=masked)
    print(f"  absgrad expectation vs float64: worst {worst:.2e} over {live} rows, {report}")
    assert (got[:, 2] == 0).all() and (got[:, :2] >= np.abs(signed32) - 1e-12).all()


class _AbsBackend:
    """`tests/oracle_backend.py` with the `abs_grad_out` keyword: the absolute sums by abs_helpers.abs_sum over the pixels
    that carry a gradient, each from one oracle backward.  Counts the backwards that asked for it."""

    def __init__(self):
        import oracle_backend

        self.inner, self.asked = oracle_backend, 0

    def backward(self, *args, flags=None, grad_allocator=None, abs_grad_out=None, **kw):
        out = self.inner.rasterize_gaussians_backward(*args, flags=flags, grad_allocator=grad_allocator, **kw)
        if abs_grad_out is not None:
            self.asked += 1
            G = args[12]
            P = args[1].shape[0]
            assert tuple(abs_grad_out.shape) == (P, 3) and abs_grad_out.dtype == torch.float32
            pixels = [(int(y), int(x)) for y, x in (G.abs().sum(0) != 0).nonzero().tolist()]

            def term(y, x):
                a = list(args)
                a[12] = G * AB.pixel_mask(G.shape[1], G.shape[2], [(y, x)])
                return self.inner.rasterize_gaussians_backward(*a, flags=flags)[0].numpy()
            abs_grad_out.copy_(torch.from_numpy(AB.abs_sum(term, pixels, P)[0]).float())
        return out


def test_l1_sets_means2d_absgrad_over_a_cpu_backend(oracle, monkeypatch):
    import oracle_backend

    import gaussianeditor_amd.diff_gaussian_rasterization as dgr
    from gaussianeditor_amd import options

    oracle_backend.install(monkeypatch)
    be = _AbsBackend()
    monkeypatch.setattr(dgr._C, "rasterize_gaussians_backward", be.backward)
    W = H = 48
    case = make_case(600, W, H, s0=0.08)
    sc = case["sc"]
    P = sc["xyz"].shape[0]
    pixels = AB.block_pixels(H, W, 3)
    G = seed_gradient(H, W, 3) * H * W * AB.pixel_mask(H, W, pixels)
    want, signed = AB.abs_expectation(oracle, case, G, pixels)
    assert (want.max(axis=1) > 0).sum() > 10
    rs = settings(case, "cpu")

    def render(flags, G_, m2d=None, reuse_entry=None):
        xyz = sc["xyz"].clone().requires_grad_(True)
        m2d = torch.zeros(P, 3, requires_grad=True) if m2d is None else m2d
        with options.override(flags):
            if reuse_entry is None:
                color, radii, depth = dgr.GaussianRasterizer(rs)(xyz, m2d, sc["opacity"], shs=sc["features"], scales=sc["scaling"],
                                                                 rotations=sc["rotation"])
            else:
                cols = torch.rand(P, 3, generator=torch.Generator().manual_seed(9)).requires_grad_(True)
                e = torch.empty(0)
                color, radii, depth = dgr._ReusedRender.apply(xyz, m2d, e, cols, sc["opacity"], sc["scaling"], sc["rotation"], e,
                                                              rs, reuse_entry)
        (color * G_).sum().backward()
        return m2d

    # flag off: the attribute is never set, the backend is never asked
    m = render(0, G)
    assert not hasattr(m, "absgrad") and be.asked == 0 and m.grad is not None
    # flag on: set, (P,3) float32, the expected values; >= |grad|
    m = render(options.FLAG_ABS_GRAD, G)
    assert be.asked == 1 and m.absgrad.shape == (P, 3) and m.absgrad.dtype == torch.float32 and not m.absgrad.requires_grad
    assert_grads_close(dict(absgrad=m.absgrad.numpy()), dict(absgrad=want), tag="L1 absgrad over the CPU backend")
    assert_grads_close(dict(g=m.grad.numpy()[:, :2]), dict(g=signed), tag="L1 means2D.grad over the CPU backend")
    # a second backward on the same screen-space tensor ASSIGNS a new tensor (the gradient itself accumulates)
    first, g_first = m.absgrad, m.grad.clone()
    m = render(options.FLAG_ABS_GRAD, 2.0 * G, m2d=m)
    assert m.absgrad is not first
    assert_grads_close(dict(absgrad=m.absgrad.numpy()), dict(absgrad=2.0 * want), tag="second backward: assigned")
    assert_grads_close(dict(g=m.grad.numpy()), dict(g=3.0 * g_first.numpy()), tag="second backward: .grad accumulated")
    # ... and a following render WITHOUT the flag neither sets nor clears it
    kept = m.absgrad
    m = render(0, G, m2d=m)
    assert m.absgrad is kept and be.asked == 2
    # the colour-override render served from a remembered state: its backward sets the attribute too
    f = oracle_forward(oracle, case)
    entry = type("Entry", (), {})()
    n, color, depth, radii, geom, binning, img = dgr._C.rasterize_gaussians(
        rs.bg, sc["xyz"], torch.empty(0), sc["opacity"], sc["scaling"], sc["rotation"], 1.0, torch.empty(0), rs.viewmatrix,
        rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, sc["features"], 3, rs.campos, False, False)
    entry.R, entry.geom, entry.binning, entry.img, entry.radii, entry.depth = n, geom, binning, img, radii, depth
    assert np.array_equal(radii.numpy(), f["radii"])
    m = render(options.FLAG_ABS_GRAD, G, reuse_entry=entry)
    assert be.asked == 3 and m.absgrad.shape == (P, 3) and float(m.absgrad.abs().max()) > 0
    assert (m.absgrad.numpy()[:, :2] >= np.abs(m.grad.numpy()[:, :2]) * (1 - 1e-5) - 1e-12).all()
    m = render(0, G, reuse_entry=entry)
    assert not hasattr(m, "absgrad") and be.asked == 3


def test_binding_checks_abs_grad_out_by_name():
    """Device / dtype / shape of `abs_grad_out` are checked before anything else is looked at."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    P = 5
    m3 = torch.zeros(P, 3)
    args = (None, m3, None, None, None, None, 1.0, None, None, None, 1.0, 1.0, torch.zeros(3, 8, 8), torch.empty(0), 0, None,
            None, 0, None, None, False)
    for bad, word in ((torch.zeros(P, 3, dtype=torch.float64), "float32"), (torch.zeros(P, 2), "(5, 3)"),
                      (torch.zeros(3, P).t(), "contiguous"), ("x", "float32")):
        with pytest.raises(RuntimeError, match="abs_grad_out"):
            _C.rasterize_gaussians_backward(*args, abs_grad_out=bad)
        try:
            _C.rasterize_gaussians_backward(*args, abs_grad_out=bad)
        except RuntimeError as e:
            assert word in str(e), (word, str(e))
