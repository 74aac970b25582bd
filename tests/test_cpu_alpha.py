"""The alpha image (accumulated opacity A = 1 - final_T, `return_alpha=True` / gaussianeditor_amd.set_alpha_output; include/gsr.h
gsr_alpha_image, gsr_blend_backward_alpha) without a GPU: the binding-level switch, argument validation of the two entry
points, the yardstick of the GPU tests -- the linearity construction of alpha_helpers -- against float64 autograd and against
finite differences of 1 - final_T, and the L1 / render() layers over a CPU stand-in for `_C`."""
import ctypes
import os
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import alpha_helpers as AH
import f64_regimes as R
from helpers import assert_grads_close, make_case, oracle_forward, seed_gradient, settings

ONE = ctypes.c_void_p(256)
ACC = ctypes.c_void_p(1 << 12)  # (64-byte aligned)
ALPHA = 16384
CASES = {"p2000": dict(P=2000, W=64, H=64, s0=0.05), "p600": dict(P=600, W=48, H=48, s0=0.08), "p4000": dict(P=4000, W=40, H=24, s0=0.12)}


def _case(name):
    kw = CASES[name]
    case = make_case(kw["P"], kw["W"], kw["H"], s0=kw["s0"])
    H, W = case["H"], case["W"]
    return case, seed_gradient(H, W, 3) * H * W, seed_gradient(H, W, 5)[:1] * H * W


def test_flag_value_setter_and_per_thread_override():
    import gaussianeditor_amd
    from gaussianeditor_amd import options

    assert options.FLAG_ALPHA_OUT == ALPHA and options.FLAG_ALL & options.FLAG_ALPHA_OUT
    assert not gaussianeditor_amd.get_alpha_output() and options.current_flags() == 0 and options.default_flags() == 0
    gaussianeditor_amd.set_alpha_output(True)
    gaussianeditor_amd.set_depth_grad(True)
    try:
        assert gaussianeditor_amd.get_alpha_output()
        assert options.current_flags() == options.FLAG_ALPHA_OUT | options.FLAG_DEPTH_GRAD
        gaussianeditor_amd.set_alpha_output(False)
        assert not gaussianeditor_amd.get_alpha_output() and options.current_flags() == options.FLAG_DEPTH_GRAD
    finally:
        gaussianeditor_amd.set_alpha_output(False)
        gaussianeditor_amd.set_depth_grad(False)
    assert options.current_flags() == 0
    seen = {}
    with options.override(options.FLAG_ALPHA_OUT):
        assert options.current_flags() == ALPHA and not gaussianeditor_amd.get_alpha_output()
        t = threading.Thread(target=lambda: seen.setdefault("other", options.current_flags()))
        t.start()
        t.join()
    assert seen["other"] == 0 and options.current_flags() == 0
    for bad in (128, 256, 512, 2048, 8192, 32768, ALPHA | 2048, ALPHA | 8192):
        with pytest.raises(ValueError):
            options.set_default_flags(bad)
        with pytest.raises(ValueError):
            with options.override(bad):
                pass


def test_binding_keeps_the_bit_to_itself_and_the_header_pins_hold():
    from gaussianeditor_amd import _native, options
    from gaussianeditor_amd.diff_gaussian_rasterization import _C, _reuse

    assert _C._flags(options.FLAG_ALPHA_OUT) == 0
    assert _C._flags(options.FLAG_ALPHA_OUT | options.FLAG_ANTIALIAS | options.FLAG_ABS_GRAD) == options.FLAG_ANTIALIAS
    with options.override(options.FLAG_ALPHA_OUT | options.FLAG_FAST_EXP):
        assert _C._flags(None) == options.FLAG_FAST_EXP
    assert _reuse._IGNORED_FLAGS & options.FLAG_ALPHA_OUT  # (the state a render leaves is the same)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsr.h")).read()
    assert "#define GSR_ABI_VERSION 6" in hdr and "#define GSR_FLAG_ALL (127u | GSR_FLAG_ANTIALIAS)" in hdr
    assert "16384" not in hdr  # (no library bit)
    for name in ("gsr_alpha_image", "gsr_blend_backward_alpha"):
        assert f"int {name}(" in hdr and name in _native.SIGNATURES and hasattr(_native.lib(), name)


def test_entry_points_validate_arguments_without_a_gpu():
    """No call here reaches the device: R = 0 without GSR_FLAG_CLEAR_GRADS launches nothing, everything else is refused."""
    from gaussianeditor_amd import _native

    L = _native.lib()
    bwd = L.gsr_blend_backward_alpha

    def call(P=10, R_=0, W=64, H=64, bg=ONE, dpix=ONE, ddepth=None, dalpha=ONE, acc=ACC, flags=0):
        return bwd(None, P, R_, W, H, bg, ONE, ONE, ONE, dpix, ddepth, dalpha, acc, None, flags)
    # empty calls: R = 0 (with and without a depth gradient, with every bit the depth twin takes), P = 0
    for f in (0, 2, 16, 1024, 4096, 4096 | 2):
        assert call(flags=f) == 0 and call(flags=f, ddepth=ONE) == 0 and call(flags=f | 64, ddepth=ONE) == 0
    assert call(P=0, acc=None) == 0
    # the alpha gradient is what the entry point is for; the depth bit only with a depth gradient
    assert call(dalpha=None) == -1 and call(P=0, dalpha=None) == -1 and call(R_=5, dalpha=None) == -1
    assert call(flags=64) == -1
    # bad sizes, a missing or misaligned table, unknown / foreign bits
    assert call(P=-1) == -1 and call(R_=-5) == -1 and call(R_=5, W=-64) == -1 and call(R_=5, H=0) == -1
    assert call(R_=5, W=16400, H=16400) == -1 and call(R_=5, bg=None) == -1 and call(R_=5, dpix=None) == -1
    assert call(acc=None) == -1 and call(acc=ctypes.c_void_p(4096 + 16)) == -1
    for bad in (8, 32, 128, 256, 512, 2048, 8192, ALPHA, ALPHA | 4096, 32768):
        assert call(flags=bad) == -1, bad
    img = L.gsr_alpha_image
    assert img(None, 64, 64, None, ONE) == -1 and img(None, 64, 64, ONE, None) == -1
    assert img(None, 0, 64, ONE, ONE) == -1 and img(None, 64, -1, ONE, ONE) == -1
    assert img(None, 64, 64, ctypes.c_void_p(256 + 16), ONE) == -1 and img(None, 64, 64, ONE, ctypes.c_void_p(258)) == -1


def test_the_library_refuses_the_binding_bit_everywhere():
    from gaussianeditor_amd import _native

    L = _native.lib()
    r = (ctypes.c_int64 * 2)()
    tk = ctypes.c_void_p()
    assert L.gsr_blend_forward(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ONE, ALPHA) == -1
    assert L.gsr_blend_forward_aux(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ONE, None, ALPHA) == -1
    assert L.gsr_trace_weights(None, 10, 0, 64, 64, 1, ONE, ONE, ONE, ONE, ONE, ONE, ALPHA) == -1
    assert L.gsr_trace_weights(None, 10, 0, 64, 64, 1, ONE, ONE, ONE, ONE, ONE, ONE, 0) == 0
    assert L.gsr_preprocess(None, 10, 3, 16, ONE, ONE, 1.0, ONE, ONE, ONE, None, None, ONE, ONE, ONE, 64, 64, 1.0, 1.0, 0, 0,
                            ALPHA, ONE, ONE, r) == -1
    assert L.gsr_preprocess_begin(None, 10, 3, 16, ONE, ONE, 1.0, ONE, ONE, ONE, None, None, ONE, ONE, ONE, 64, 64, 1.0, 1.0,
                                  0, 0, ALPHA, ONE, ONE, ctypes.byref(tk)) == -1
    pb = lambda flags: L.gsr_preprocess_backward(  # noqa: E731
        None, 10, 3, 16, 64, 64, ONE, ONE, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE, ACC, ONE, ONE, None, ONE,
        None, ONE, ONE, ONE, flags)
    assert pb(ALPHA) == -1 and pb(ALPHA | 32) == -1
    pr = lambda flags: L.gsr_preprocess_backward_rgb(  # noqa: E731
        None, 10, 3, 16, 64, 64, ONE, ONE, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE, ACC, ONE, ONE, ONE, None,
        ONE, ONE, ONE, flags)
    assert pr(ALPHA) == -1
    rows = lambda flags: L.gsr_preprocess_backward_rows_flags(  # noqa: E731
        None, 0, 3, 16, 64, 64, None, ONE, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE, ACC, ONE, ONE, None, ONE,
        None, ONE, None, ONE, ONE, ONE, flags)
    assert rows(0) == 0 and rows(ALPHA) == -1
    assert L.gsr_blend_backward(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ACC, None, 0) == 0
    assert L.gsr_blend_backward(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ACC, None, ALPHA) == -1
    assert L.gsr_blend_backward_depth(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ONE, ACC, None, ALPHA) == -1

    def full(fn, flags, depth=False):
        extra = (ONE,) if depth else ()
        return fn(None, 10, 3, 16, 0, 64, 64, ONE, None, ONE, None, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE, ONE,
                  ONE, ONE, *extra, ACC, ONE, ONE, None, ONE, None, ONE, ONE, ONE, flags)
    assert full(L.gsr_backward, ALPHA) == -1 and full(L.gsr_backward_depth, ALPHA, depth=True) == -1


def _f64(case, f, G, GA, op_override=None, grads=True):
    """float64: gradients of <G, C> + <GA, A>, A the first channel of the ones render on background 0 -> (gradient dict,
    stats of the ones render, ones image)."""
    from oracle.torch_ref import render_f64

    d = torch.float64
    sc, cam = case["sc"], case["cam"]
    P, W, H = sc["xyz"].shape[0], case["W"], case["H"]
    leaf = lambda t: t.to(d).clone().requires_grad_(grads)  # noqa: E731
    xyz, scl, rot, sh = leaf(sc["xyz"]), leaf(sc["scaling"]), leaf(sc["rotation"]), leaf(sc["features"])
    op = leaf(sc["opacity"] if op_override is None else op_override)
    m2 = torch.zeros(P, 3, dtype=d, requires_grad=grads)
    geo = (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)
    tail = (W, H, case["tfx"], case["tfy"], 1.0, case["D"])
    if G is not None:
        render_f64(f, xyz, m2, op, scl, rot, sh, None, None, *geo, case["bg"], *tail, dL_dimage=G.to(d))
    stats = {}
    ones = torch.ones(P, 3, dtype=d)
    img = render_f64(f, xyz, m2, op, scl, rot, None, ones, None, *geo, torch.zeros(3), *tail,
                     dL_dimage=AH.ones_gradient(GA, H, W).to(d) if grads else None, stats=stats)
    if not grads:
        return None, stats, img
    leaves = dict(dL_dmeans3D=xyz, dL_dmeans2D=m2, dL_dopacity=op, dL_dscales=scl, dL_drotations=rot, dL_dsh=sh)
    return {k: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for k, t in leaves.items()}, stats, img


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("alpha_only", [False, True])
def test_expectation_builder_equals_float64_autograd(oracle, name, alpha_only):
    """The GPU tests' expectation (float32 oracle: the ordinary backward + the backward of the ones render) == float64 autograd
    of <G, C> + <GA, A> at f64_regimes.TOL, rows under flipped pixels masked and bounded as everywhere; the float64 telescoping
    identity C_ones == 1 - final_T; and, on the two cases the GPU tests use, discrimination condition (i).
    Measured: worst 1.1e-6 .. 4.4e-6 of a tensor's maximum over the six runs, |C_ones - (1 - final_T)| <= 6.7e-16, no pixel
    flipped and nothing masked."""
    case, G, GA = _case(name)
    G = None if alpha_only else G
    f = oracle_forward(oracle, case)
    want, share = AH.alpha_expectation(oracle, case, G, GA)
    got64, stats, img = _f64(case, f, G, GA)
    tele = float((img[0].reshape(-1) - (1.0 - stats["final_T"])).abs().max())
    assert tele <= 1e-12, tele
    masked, report = R.masked_rows(dict(case=case, name="alpha " + name), f, stats)
    keys = ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dscales", "dL_drotations"] + ([] if alpha_only else ["dL_dsh"])
    worst = assert_grads_close(want, got64, tol=R.TOL, tag="oracle-built alpha expectation vs float64", masked=masked, keys=keys)
    print(f"  [{name}{' alpha only' if alpha_only else ''}] worst {worst:.2e}, telescoping {tele:.1e}, {report}")
    if alpha_only:
        assert not np.any(want["dL_dsh"]) and not np.any(got64["dL_dsh"])  # (A does not depend on the colours)
    elif name == "p2000":
        AH.assert_share_visible(want, share, tag=name)
    # the float32 oracle's own alpha image: the ones render and 1 - final_T of the ordinary render agree to rounding
    f1 = oracle_forward(oracle, dict(case, bg=torch.zeros(3)), colors_precomp=torch.ones(case["sc"]["xyz"].shape[0], 3))
    assert np.abs(f1["color"][0].reshape(-1) - (1.0 - f["final_T"].reshape(-1))).max() < 2e-6


def test_discrimination_condition_on_the_segment_case(oracle):
    case = make_case(20000, 64, 64, s0=0.03)
    G, GA = seed_gradient(64, 64, 3) * 4096, seed_gradient(64, 64, 5)[:1] * 4096
    want, share = AH.alpha_expectation(oracle, case, G, GA)
    AH.assert_share_visible(want, share, tag="p20000")


def test_expectation_sign_and_term_by_finite_differences(oracle):
    """Independent of any backward: central differences in float64 of L(o) = <GA, 1 - final_T> (render_f64's statistics, no
    autograd) by single opacities against the expectation's dL_dopacity.
    Step and tolerance: at fixed discrete decisions every pixel's final_T is LINEAR in one opacity (alpha_i = o_i G_i enters one
    factor 1 - alpha_i), so the central difference has no truncation error and its rounding error is ~ 2^-52 |L| / h = 1e-9
    for |L| ~ 5e2 and h = 1e-4 -- nothing next to the float32 oracle's own error, which f64_regimes.TOL bounds.  Curvature
    enters only where a decision flips inside +-h (alpha across 1/255: a ring of relative width 2 h / o around the 3.3 sigma
    contour, ~1e-3 sigma^2 pixels) or at the 0.99 clamp, through which the analytic backward differentiates as if it were not
    there: the chosen Gaussians have o < 0.98 (never clamped: G <= 1) and unchanged n_contrib under both steps, asserted.
    Tolerance: TOL of the tensor's maximum.  Measured: max error 1.2e-6 of the maximum over 6 Gaussians."""
    case, _, GA = _case("p2000")
    f = oracle_forward(oracle, case)
    want, _ = AH.alpha_expectation(oracle, case, None, GA)
    g = want["dL_dopacity"].reshape(-1)
    op = case["sc"]["opacity"]
    ok = np.nonzero(op.reshape(-1).numpy() < 0.98)[0]
    picks = ok[np.argsort(-np.abs(g[ok]))[[0, 1, 2, 10, 40, 120]]]
    assert (np.abs(g[picks]) > 1e-3 * np.abs(g).max()).all()
    h, scale = 1e-4, np.abs(g).max()
    _, s0, _ = _f64(case, f, None, GA, grads=False)
    worst = 0.0
    for i in picks.tolist():
        L = []
        for sgn in (+1.0, -1.0):
            o = op.double().clone()
            o[i] += sgn * h
            _, st, _ = _f64(case, f, None, GA, op_override=o, grads=False)
            assert torch.equal(st["n_contrib"], s0["n_contrib"])  # (no discrete decision moved)
            L.append(float((GA[0].reshape(-1).double() * (1.0 - st["final_T"])).sum()))
        fd = (L[0] - L[1]) / (2 * h)
        worst = max(worst, abs(fd - g[i]) / scale)
        assert abs(fd - g[i]) <= R.TOL * scale and fd * g[i] > 0, (i, fd, g[i])
    print(f"  finite differences vs expectation dL_dopacity: worst {worst:.2e} of the maximum over {len(picks)} Gaussians")


class _AlphaBackend:
    """`tests/oracle_backend.py` plus `alpha_image` and the `dL_dout_alpha` keyword.  The image is 1 - final_T of the oracle's
    forward; the gradient's share is the stand-in's own backward of the ones render (alpha_helpers' construction).  The image
    state it hands out is the forward's tag, so that `alpha_image(imgBuffer, H, W)` finds the view.  Counts what it is asked."""

    def __init__(self):
        import oracle_backend

        self.inner, self.images, self.alpha_backwards, self.backwards = oracle_backend, 0, 0, 0

    def forward(self, *args, **kw):
        out = self.inner.rasterize_gaussians(*args, **kw)
        return out[:6] + (out[4].clone(),)

    def alpha_image(self, imgBuffer, H, W):
        self.images += 1
        f = self.inner._registry[int(imgBuffer.view(torch.int64)[0])]
        return torch.from_numpy(np.float32(1.0) - f["final_T"].astype(np.float32)).reshape(1, int(H), int(W))

    def backward(self, *args, flags=None, grad_allocator=None, dL_dout_alpha=None, **kw):
        self.backwards += 1
        out = list(self.inner.rasterize_gaussians_backward(*args, flags=flags, grad_allocator=grad_allocator, **kw))
        if dL_dout_alpha is not None:
            self.alpha_backwards += 1
            (bg, means3D, radii, colors, scales, rotations, smod, cov, view, proj, tfx, tfy, G, sh, degree, campos) = args[:16]
            H, W, P = G.shape[1], G.shape[2], means3D.shape[0]
            assert tuple(dL_dout_alpha.shape) == (1, H, W) and dL_dout_alpha.dtype == torch.float32
            ones, e = torch.ones(P, 3), torch.empty(0)
            fw = self.inner.rasterize_gaussians(torch.zeros(3), means3D.detach(), ones, args_opacity(self, args), scales, rotations,
                                                smod, cov, view, proj, tfx, tfy, H, W, e, degree, campos, False, False)
            a = list(args)
            a[0], a[3], a[12], a[13], a[16], a[17] = torch.zeros(3), ones, AH.ones_gradient(dL_dout_alpha, H, W), e, fw[4], fw[0]
            share = self.inner.rasterize_gaussians_backward(*a, flags=flags)
            for i in (0, 2, 3, 4, 6, 7):  # means2D, opacity, means3D, cov3D, scales, rotations: not the colours / SHs
                if out[i] is not None and share[i] is not None and out[i].numel():
                    out[i] = out[i] + share[i].reshape(out[i].shape)
        return tuple(out)


def args_opacity(be, args):
    """The opacities of the view whose state a backward was handed (the reference's backward signature has none)."""
    return be.inner._registry[int(args[16].view(torch.int64)[0])]["_view_args"][3]


def _install(monkeypatch):
    import oracle_backend

    import gaussianeditor_amd.diff_gaussian_rasterization as dgr

    oracle_backend.install(monkeypatch)
    be = _AlphaBackend()
    monkeypatch.setattr(dgr._C, "rasterize_gaussians", be.forward)
    monkeypatch.setattr(dgr._C, "rasterize_gaussians_backward", be.backward)
    monkeypatch.setattr(dgr._C, "alpha_image", be.alpha_image)
    return dgr, be


GRAD_KEYS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dsh")


def test_l1_returns_alpha_with_its_gradient_over_a_cpu_backend(oracle, monkeypatch):
    dgr, be = _install(monkeypatch)
    case, G, GA = _case("p600")
    sc, H, W = case["sc"], case["H"], case["W"]
    P = sc["xyz"].shape[0]
    rs = settings(case, "cpu")
    f = oracle_forward(oracle, case)
    a_want = np.float32(1.0) - f["final_T"].reshape(1, H, W)

    def run(loss_of, reuse_entry=None, **kw):
        leaf = lambda t: t.clone().requires_grad_(True)  # noqa: E731
        L = dict(dL_dmeans3D=leaf(sc["xyz"]), dL_dmeans2D=torch.zeros(P, 3, requires_grad=True), dL_dopacity=leaf(sc["opacity"]),
                 dL_dscales=leaf(sc["scaling"]), dL_drotations=leaf(sc["rotation"]))
        if reuse_entry is None:
            L["dL_dsh"] = leaf(sc["features"])
            outs = dgr.GaussianRasterizer(rs)(L["dL_dmeans3D"], L["dL_dmeans2D"], L["dL_dopacity"], shs=L["dL_dsh"],
                                              scales=L["dL_dscales"], rotations=L["dL_drotations"], **kw)
        else:
            L["dL_dcolors"] = leaf(reuse_entry.cols)
            e = torch.empty(0)
            outs = dgr._ReusedRender.apply(L["dL_dmeans3D"], L["dL_dmeans2D"], e, L["dL_dcolors"], L["dL_dopacity"], L["dL_dscales"],
                                           L["dL_drotations"], e, rs, reuse_entry, *((True,) if kw.get("return_alpha") else ()))
        loss = loss_of(outs)
        if loss is not None:
            loss.backward()
        return outs, {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in L.items()}

    # without the keyword: three values (four with aux_colors), the backend is never asked and never sees the keyword
    outs, g0 = run(lambda o: (o[0] * G).sum())
    assert len(outs) == 3 and be.images == 0 and be.alpha_backwards == 0 and be.backwards == 1
    aux = torch.rand(P, 3, generator=torch.Generator().manual_seed(2))
    outs, _ = run(lambda o: None, aux_colors=aux)
    assert len(outs) == 4 and be.images == 0
    # with it: alpha is the additional LAST value in both arities, == 1 - final_T, differentiable
    outs, _ = run(lambda o: None, aux_colors=aux, return_alpha=True)
    assert len(outs) == 5 and outs[4].shape == (1, H, W) and outs[3].shape == (3, H, W) and not outs[3].requires_grad
    assert np.array_equal(outs[4].detach().numpy(), a_want) and outs[4].requires_grad and be.images == 1
    # alpha returned but unused: today's backward call, bit for bit today's gradients
    n = be.backwards
    outs, g1 = run(lambda o: (o[0] * G).sum(), return_alpha=True)
    assert len(outs) == 4 and np.array_equal(outs[3].detach().numpy(), a_want)
    assert be.alpha_backwards == 0 and be.backwards == n + 1 and all(np.array_equal(g0[k], g1[k]) for k in g0)
    # colour + alpha loss, and the alpha-only loss (a zero colour gradient is made up for the backend)
    want, share = AH.alpha_expectation(oracle, case, G, GA)
    outs, g = run(lambda o: (o[0] * G).sum() + (o[3] * GA).sum(), return_alpha=True)
    assert be.alpha_backwards == 1
    assert_grads_close(g, want, tag="L1 colour + alpha over the CPU backend", keys=GRAD_KEYS)
    assert max(np.abs(g[k] - g0[k]).max() / np.abs(want[k]).max() for k in AH.SHARE_KEYS) > 1e-2
    want_a, _ = AH.alpha_expectation(oracle, case, None, GA)
    outs, g = run(lambda o: (o[3] * GA).sum(), return_alpha=True)
    assert be.alpha_backwards == 2 and not np.any(g["dL_dsh"])
    assert_grads_close(g, want_a, tag="L1 alpha only over the CPU backend", keys=GRAD_KEYS)
    # the colour-override render served from a remembered state: alpha out of the remembered image state
    e = torch.empty(0)
    n_, color, depth, radii, geom, binning, img = dgr._C.rasterize_gaussians(
        rs.bg, sc["xyz"], e, sc["opacity"], sc["scaling"], sc["rotation"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
        rs.tanfovy, H, W, sc["features"], 3, rs.campos, False, False)
    cols = torch.rand(P, 3, generator=torch.Generator().manual_seed(9))
    entry = SimpleNamespace(R=n_, geom=geom, binning=binning, img=img, radii=radii, depth=depth, cols=cols)
    outs, _ = run(lambda o: None, reuse_entry=entry)
    assert len(outs) == 3
    images = be.images
    outs, g = run(lambda o: (o[0] * G).sum() + (o[3] * GA).sum(), reuse_entry=entry, return_alpha=True)
    assert len(outs) == 4 and be.images == images + 1 and np.array_equal(outs[3].detach().numpy(), a_want)
    want_c, _ = AH.alpha_expectation(oracle, case, G, GA, colors_precomp=cols)
    assert be.alpha_backwards == 3
    assert_grads_close(g, want_c, tag="reused render, colour + alpha", keys=[k for k in GRAD_KEYS if k != "dL_dsh"] + ["dL_dcolors"])


def test_render_adds_alpha_only_under_the_flag_or_the_keyword(oracle, monkeypatch):
    dgr, be = _install(monkeypatch)
    import gaussianeditor_amd
    from gaussianeditor_amd import options
    from gaussianeditor_amd.gaussian_renderer import render
    from test_cpu_host_api import _PC, PIPE

    case, G, GA = _case("p600")
    H, W = case["H"], case["W"]
    base = {"render", "viewspace_points", "visibility_filter", "radii", "depth_3dgs"}
    a_want = np.float32(1.0) - oracle_forward(oracle, case)["final_T"].reshape(1, H, W)
    assert set(render(case["cam"], _PC(case["sc"]), PIPE, case["bg"])) == base and be.images == 0
    out = render(case["cam"], _PC(case["sc"]), PIPE, case["bg"], return_alpha=True)
    assert set(out) == base | {"alpha"} and np.array_equal(out["alpha"].detach().numpy(), a_want)
    sem = torch.rand(case["sc"]["xyz"].shape[0], 3, generator=torch.Generator().manual_seed(4))
    out = render(case["cam"], _PC(case["sc"]), PIPE, case["bg"], semantic_color=sem, return_alpha=True)
    assert set(out) == base | {"alpha", "semantic"} and out["semantic"].shape == (3, H, W) and out["alpha"].shape == (1, H, W)
    with options.override(options.FLAG_ALPHA_OUT):
        assert "alpha" in render(case["cam"], _PC(case["sc"]), PIPE, case["bg"])
        assert "alpha" not in render(case["cam"], _PC(case["sc"]), PIPE, case["bg"], return_alpha=False)
        # the rasterizer's arity never follows process state: unmodified editor code unpacks three values
        rs = settings(case, "cpu")
        sc = case["sc"]
        color, radii, depth = dgr.GaussianRasterizer(rs)(sc["xyz"], torch.zeros_like(sc["xyz"]), sc["opacity"], shs=sc["features"],
                                                         scales=sc["scaling"], rotations=sc["rotation"])
    gaussianeditor_amd.set_alpha_output(True)
    try:
        pc = _PC(case["sc"])
        out = render(case["cam"], pc, PIPE, case["bg"])
        assert "alpha" in out
        (out["alpha"] * GA).sum().backward()
    finally:
        gaussianeditor_amd.set_alpha_output(False)
    want, _ = AH.alpha_expectation(oracle, case, None, GA)
    assert_grads_close(dict(o=pc.get_opacity.grad.numpy(), m=out["viewspace_points"].grad.numpy()),
                       dict(o=want["dL_dopacity"], m=want["dL_dmeans2D"]), tag="render(): alpha-only loss")
    assert "alpha" not in render(case["cam"], _PC(case["sc"]), PIPE, case["bg"])


def test_binding_checks_dl_dout_alpha_by_name():
    """dtype / shape / device of `dL_dout_alpha` are checked before anything else is looked at."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    m3 = torch.zeros(5, 3)
    args = (None, m3, None, None, None, None, 1.0, None, None, None, 1.0, 1.0, torch.zeros(3, 8, 6), torch.empty(0), 0, None,
            None, 0, None, None, False)
    for bad, word in ((torch.zeros(1, 8, 6, dtype=torch.float64), "float32"), (torch.zeros(8, 6), "(1, 8, 6)"),
                      (torch.zeros(1, 6, 8), "(1, 8, 6)"), (torch.zeros(3, 8, 6), "(1, 8, 6)"), ("x", "float32"),
                      (torch.zeros(1, 8, 6, device="meta"), "is on meta")):
        with pytest.raises(RuntimeError, match="dL_dout_alpha") as e:
            _C.rasterize_gaussians_backward(*args, dL_dout_alpha=bad)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(RuntimeError, match="imgBuffer"):
        _C.alpha_image(torch.zeros(4), 8, 6)
    assert _C.alpha_image(torch.empty(0, dtype=torch.uint8), 8, 6).shape == (1, 8, 6)
