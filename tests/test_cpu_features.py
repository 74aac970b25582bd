"""The feature image (`features=`; include/gsr.h gsr_blend_forward_features, gsr_blend_backward_features) without a GPU:
argument validation of the two entry points, the yardstick of the GPU tests -- the slice construction of features_helpers --
against float64 autograd, and the L1 / render() layers over a CPU stand-in for `_C`."""
import ctypes
import os

import numpy as np
import pytest
import torch

import f64_regimes as R
import features_helpers as FH
from helpers import assert_grads_close, oracle_forward, settings

ONE = ctypes.c_void_p(256)
ACC = ctypes.c_void_p(1 << 12)  # (64-byte aligned)
GEO_KEYS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dscales", "dL_drotations")


def test_header_symbols_and_signatures():
    from gaussianeditor_amd import _native
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsr.h")).read()
    assert "#define GSR_ABI_VERSION 6" in hdr and "#define GSR_MAX_FEATURE_CHANNELS 256" in hdr
    assert "#define GSR_FLAG_ALL (127u | GSR_FLAG_ANTIALIAS)" in hdr  # (no new flag bit)
    for name in ("gsr_blend_forward_features", "gsr_blend_backward_features"):
        assert f"int {name}(" in hdr and name in _native.SIGNATURES and hasattr(_native.lib(), name)
    assert _C.MAX_FEATURE_CHANNELS == 256


def test_entry_points_validate_arguments_without_a_gpu():
    """No call here reaches the device: the backward with R = 0 launches nothing, everything else is refused."""
    from gaussianeditor_amd import _native

    L = _native.lib()

    def fwd(P=10, R_=5, W=64, H=64, C=16, geom=ONE, binning=ONE, image=ONE, feats=ONE, out=ONE, flags=0):
        return L.gsr_blend_forward_features(None, P, R_, W, H, C, geom, binning, image, feats, out, flags)

    def bwd(P=10, R_=0, W=64, H=64, C=16, geom=ONE, binning=ONE, image=ONE, feats=ONE, dimg=ONE, acc=ACC, dfeat=ONE, flags=0):
        return L.gsr_blend_backward_features(None, P, R_, W, H, C, geom, binning, image, feats, dimg, acc, dfeat, flags)
    # the backward's empty calls: R = 0, P = 0, under every flag it takes
    for f in (0, 1, 2, 16, 1024, 1 | 2 | 16 | 1024):
        assert bwd(flags=f) == 0 and bwd(P=0, flags=f) == 0
    for C in (1, 7, 255, 256):
        assert bwd(C=C) == 0
    for call in (fwd, bwd):
        for C in (0, -1, 257, 1 << 20):
            assert call(C=C) == -1, C
        for bad in (4, 8, 32, 64, 128, 256, 512, 2048, 4096, 8192, 16384, 32768, 2 | 4096):
            assert call(flags=bad) == -1, bad
        assert call(P=-1) == -1 and call(R_=-5) == -1 and call(W=0) == -1 and call(H=-3) == -1
        assert call(image=None) == -1 and call(feats=None) == -1
        assert call(R_=5, geom=None) == -1 and call(R_=5, binning=None) == -1
        # misaligned scratch buffers are refused before any launch (the aligned dummies above never get this far: the
        # forward below is only ever called with an argument that is refused)
        assert call(R_=5, geom=ctypes.c_void_p(256 + 16)) == -1 and call(R_=5, image=ctypes.c_void_p(256 + 64)) == -1
    assert fwd(out=None) == -1 and fwd(out=ctypes.c_void_p(258)) == -1
    assert bwd(dimg=None) == -1 and bwd(dfeat=None) == -1
    assert bwd(acc=None) == -1 and bwd(acc=ctypes.c_void_p(4096 + 16)) == -1 and bwd(acc=ctypes.c_void_p(4096 + 32)) == -1
    assert bwd(R_=5, W=16400, H=16400) == -1  # (more tiles than the backward's work items can name)


def _f64(case, f, G, GF, feats):
    """float64 autograd of <G, C> + sum_c <GF_c, F_c>, F the slice renders on background 0 -> (gradients, stats, image)."""
    from oracle.torch_ref import render_f64

    d = torch.float64
    sc, cam = case["sc"], case["cam"]
    P, W, H = sc["xyz"].shape[0], case["W"], case["H"]
    leaf = lambda t: t.to(d).clone().requires_grad_(True)  # noqa: E731
    xyz, scl, rot, sh, op = leaf(sc["xyz"]), leaf(sc["scaling"]), leaf(sc["rotation"]), leaf(sc["features"]), leaf(sc["opacity"])
    ft = leaf(feats)
    m2 = torch.zeros(P, 3, dtype=d, requires_grad=True)
    geo = (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)
    tail = (W, H, case["tfx"], case["tfy"], 1.0, case["D"])
    stats = {}
    render_f64(f, xyz, m2, op, scl, rot, sh, None, None, *geo, case["bg"], *tail, dL_dimage=G.to(d), stats=stats)
    img = torch.zeros(feats.shape[1], H, W, dtype=d)
    for k, n, _, g in FH.slices(feats, GF):
        cols = torch.cat([ft[:, 3 * k:3 * k + n], torch.zeros(P, 3 - n, dtype=d)], dim=1)
        img[3 * k:3 * k + n] = render_f64(f, xyz, m2, op, scl, rot, None, cols, None, *geo, torch.zeros(3), *tail,
                                          dL_dimage=g.to(d))[:n]
    leaves = dict(dL_dmeans3D=xyz, dL_dmeans2D=m2, dL_dopacity=op, dL_dscales=scl, dL_drotations=rot, dL_dsh=sh, dL_dfeatures=ft)
    return {k: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for k, t in leaves.items()}, stats, img


@pytest.mark.parametrize("name", list(FH.CASES))
def test_expectation_builder_equals_float64_autograd(oracle, name):
    """The GPU tests' expectation (float32 oracle: the ordinary backward + the backwards of the slice renders) == float64
    autograd of <G, C> + sum_c <GF_c, F_c> at f64_regimes.TOL; masked rows at most 0.1 % of the rows that carry a gradient;
    discrimination condition (i); the oracle's feature image within 1e-5 of the float64 one.
    Measured (worst error of a tensor, relative to its maximum; masked rows): p2000 C=7 3.1e-6 / 0, ragged C=16 3.5e-6 / 0,
    p600 C=1 2.0e-6 / 0, p4000 C=33 1.1e-6 / 0; no pixel flipped; the oracle's image within 2.1e-6 of the float64 one."""
    case, G, GF, feats = FH.feature_case(name)
    f = oracle_forward(oracle, case)
    want, share, dfeat, slice_max = FH.feature_expectation(oracle, case, G, GF, feats)
    got64, stats, img = _f64(case, f, G, GF, feats)
    masked, report = R.masked_rows(dict(case=case, name="features " + name), f, stats)
    carrying = int((np.abs(got64["dL_dmeans3D"]).max(axis=1) > 0).sum())
    assert masked.sum() <= 1e-3 * carrying, (int(masked.sum()), carrying)
    want = dict(want, dL_dfeatures=dfeat)
    worst = assert_grads_close(want, got64, tol=R.TOL, tag="oracle-built feature expectation vs float64", masked=masked,
                               keys=list(GEO_KEYS) + ["dL_dsh", "dL_dfeatures"])
    ratio = max(slice_max[k] / np.abs(want[k]).max() for k in GEO_KEYS)
    print(f"  [{name} C={feats.shape[1]}] worst {worst:.2e}, masked rows {int(masked.sum())} of {carrying}, max slice / total "
          f"{ratio:.2f}, {report}")
    FH.assert_share_visible(want, share, tag=name)
    assert not np.any(dfeat[f["radii"] <= 0])  # (a Gaussian the view does not see gets no feature gradient)
    ours = FH.oracle_feature_image(oracle, case, feats)
    # (bar: |F_c| <= max |f| = 1; a pixel blends at most a few hundred entries, each of which adds one binary32 rounding,
    #  6e-8 of a running sum <= 1, and an alpha whose exponential carries 1e-7 relative: the project's 1e-5 with room)
    err = float(np.abs(ours - img.numpy()).max())
    print(f"  [{name}] oracle feature image vs float64: {err:.2e}")
    assert err <= 1e-5


def test_oracle_feature_image_is_its_slice_render_exactly(oracle):
    """Channel c of the expectation's image is channel c % 3 of the slice render, bit for bit -- and the zero padding of a
    partial slice does not move the channels in front of it (C = 7 against the first 7 channels of C = 9)."""
    case, _, _, feats = FH.feature_case("p2000")
    img = FH.oracle_feature_image(oracle, case, feats)
    case0 = dict(case, bg=torch.zeros(3))
    for k, n, cols, _ in FH.slices(feats):
        ref = oracle_forward(oracle, case0, colors_precomp=cols)["color"]
        assert np.array_equal(img[3 * k:3 * k + n].view(np.uint32), ref[:n].view(np.uint32))
        if n < 3:
            assert not np.any(ref[n:])
    wide = torch.cat([feats, FH.make_features(feats.shape[0], 2, seed=5)], dim=1)
    assert np.array_equal(FH.oracle_feature_image(oracle, case, wide)[:7].view(np.uint32), img.view(np.uint32))


def _leaves(sc, P, feats=None):
    leaf = lambda t: t.clone().requires_grad_(True)  # noqa: E731
    L = dict(dL_dmeans3D=leaf(sc["xyz"]), dL_dmeans2D=torch.zeros(P, 3, requires_grad=True), dL_dopacity=leaf(sc["opacity"]),
             dL_dscales=leaf(sc["scaling"]), dL_drotations=leaf(sc["rotation"]), dL_dsh=leaf(sc["features"]))
    if feats is not None:
        L["dL_dfeatures"] = leaf(feats)
    return L


def _grads(L):
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in L.items()}


def test_l1_returns_the_feature_image_with_its_gradient_over_a_cpu_backend(oracle, monkeypatch):
    dgr, be = FH.install(monkeypatch)
    case, G, GF, feats = FH.feature_case("p600", C=5)
    sc, H, W = case["sc"], case["H"], case["W"]
    P = sc["xyz"].shape[0]
    rs = settings(case, "cpu")
    f_want = FH.oracle_feature_image(oracle, case, feats)

    def run(loss_of, with_features=True, **kw):
        L = _leaves(sc, P, feats if with_features else None)
        if with_features:
            kw["features"] = L["dL_dfeatures"]
        outs = dgr.GaussianRasterizer(rs)(L["dL_dmeans3D"], L["dL_dmeans2D"], L["dL_dopacity"], shs=L["dL_dsh"],
                                          scales=L["dL_dscales"], rotations=L["dL_drotations"], **kw)
        loss = loss_of(outs)
        if loss is not None:
            loss.backward()
        return outs, _grads(L)

    aux = torch.rand(P, 3, generator=torch.Generator().manual_seed(2))
    # arity: the feature image is the LAST value whatever else is asked for
    for kw, n in ((dict(), 4), (dict(aux_colors=aux), 5), (dict(return_alpha=True), 5), (dict(aux_colors=aux, return_alpha=True), 6)):
        outs, _ = run(lambda o: None, **kw)
        assert len(outs) == n and outs[-1].shape == (5, H, W) and outs[-1].requires_grad
        assert np.array_equal(outs[-1].detach().numpy(), f_want)
        if kw.get("return_alpha"):
            assert outs[-2].shape == (1, H, W)
    assert len(run(lambda o: None, with_features=False)[0]) == 3
    # the feature image returned but unused: the backward call of a render without it, and its gradients bit for bit
    _, g0 = run(lambda o: (o[0] * G).sum(), with_features=False)
    n = be.feature_backwards
    _, g1 = run(lambda o: (o[0] * G).sum())
    assert be.feature_backwards == n and all(np.array_equal(g0[k], g1[k]) for k in g0) and not np.any(g1["dL_dfeatures"])
    assert be.calls[-1] == ("rasterize_gaussians_backward", 21, ("flags", "grad_allocator"))
    # colour + feature loss: gradients reach the features and the geometry
    want, share, dfeat, smax = FH.feature_expectation(oracle, case, G, GF, feats)
    _, g = run(lambda o: (o[0] * G).sum() + (o[-1] * GF).sum())
    assert be.feature_backwards == n + 1
    FH.assert_feature_grads_close(g, dict(want, dL_dfeatures=dfeat), smax, tag="L1 colour + features over the CPU backend",
                                  keys=list(GEO_KEYS) + ["dL_dsh", "dL_dfeatures"])
    assert max(np.abs(g[k] - g0[k]).max() / np.abs(want[k]).max() for k in FH.SHARE_KEYS) > 1e-2
    assert np.array_equal(g["dL_dsh"], g0["dL_dsh"])  # (the SHs get no share of the feature image)
    # the feature-only loss (a zero colour gradient is made up for the backend): the SH gradient is zeros
    want_f, _, dfeat_f, smax_f = FH.feature_expectation(oracle, case, None, GF, feats)
    _, g = run(lambda o: (o[-1] * GF).sum(), return_alpha=True)
    assert not np.any(g["dL_dsh"]) and np.array_equal(dfeat_f, dfeat)
    FH.assert_feature_grads_close(g, dict(want_f, dL_dfeatures=dfeat_f), smax_f, tag="L1 features only over the CPU backend",
                                  keys=list(GEO_KEYS) + ["dL_dfeatures"])
    # features + alpha: both extra outputs differentiable side by side
    GA = FH.seed_gradient(H, W, 5)[:1] * H * W
    want_a, _, dfeat_a, smax_a = FH.feature_expectation(oracle, case, G, GF, feats, GA=GA)
    _, g = run(lambda o: (o[0] * G).sum() + (o[-2] * GA).sum() + (o[-1] * GF).sum(), return_alpha=True)
    FH.assert_feature_grads_close(g, dict(want_a, dL_dfeatures=dfeat_a), smax_a, tag="L1 colour + alpha + features",
                                  keys=list(GEO_KEYS) + ["dL_dsh", "dL_dfeatures"])
    # under no_grad: the forward entry point alone
    be.calls.clear()
    with torch.no_grad():
        L = _leaves(sc, P, feats)
        outs = dgr.GaussianRasterizer(rs)(L["dL_dmeans3D"], L["dL_dmeans2D"], L["dL_dopacity"], shs=L["dL_dsh"],
                                          scales=L["dL_dscales"], rotations=L["dL_drotations"], features=L["dL_dfeatures"])
    assert [c[0] for c in be.calls] == ["rasterize_gaussians", "rasterize_features"] and not outs[-1].requires_grad
    assert np.array_equal(outs[-1].numpy(), f_want)


def test_a_call_without_features_passes_the_argument_tuples_it_always_passed(oracle, monkeypatch):
    """A spy on `_RasterizeGaussians.apply` and on the `_C` entry points: without `features=` the tuples are today's (9, 10 or
    11 inputs; the forward's 19 positionals + flags; the backward's 21 + flags, grad_allocator), and rasterize_features is
    never called; with it the features are input 14, behind the camera tensors' slots 11 .. 13."""
    dgr, be = FH.install(monkeypatch)
    case, G, GF, feats = FH.feature_case("p600", C=5)
    sc = case["sc"]
    P = sc["xyz"].shape[0]
    rs = settings(case, "cpu")
    seen = []
    real_apply = dgr._RasterizeGaussians.apply
    monkeypatch.setattr(dgr._RasterizeGaussians, "apply", staticmethod(lambda *a: (seen.append(a), real_apply(*a))[1]))
    aux = torch.rand(P, 3, generator=torch.Generator().manual_seed(2))

    def render(**kw):
        L = _leaves(sc, P)
        outs = dgr.GaussianRasterizer(rs)(L["dL_dmeans3D"], L["dL_dmeans2D"], L["dL_dopacity"], shs=L["dL_dsh"],
                                          scales=L["dL_dscales"], rotations=L["dL_drotations"], **kw)
        (outs[0] * G).sum().backward()
        return outs
    render()
    assert len(seen[-1]) == 9
    render(return_alpha=True)
    assert len(seen[-1]) == 11 and seen[-1][9:] == (None, True)
    render(aux_colors=aux)
    assert len(seen[-1]) == 10 and seen[-1][9] is aux
    render(aux_colors=aux, return_alpha=True)
    assert len(seen[-1]) == 11 and seen[-1][10] is True
    names = [c[0] for c in be.calls]
    assert "rasterize_features" not in names
    assert all(c == ("rasterize_gaussians", 19, ("flags",)) for c in be.calls if c[0] == "rasterize_gaussians")
    assert all(c == ("rasterize_gaussians_backward", 21, ("flags", "grad_allocator")) for c in be.calls if c[0] == "rasterize_gaussians_backward")
    ft = feats.clone().requires_grad_(True)
    render(features=ft, return_alpha=True)
    assert len(seen[-1]) == 15 and seen[-1][14] is ft and seen[-1][11:14] == (None, None, None) and seen[-1][9:11] == (None, True)


def test_render_adds_features_only_with_the_keyword(oracle, monkeypatch):
    dgr, be = FH.install(monkeypatch)
    from gaussianeditor_amd.gaussian_renderer import render
    from test_cpu_host_api import _PC, PIPE

    case, G, GF, feats = FH.feature_case("p600", C=5)
    H, W = case["H"], case["W"]
    base = {"render", "viewspace_points", "visibility_filter", "radii", "depth_3dgs"}
    assert set(render(case["cam"], _PC(case["sc"]), PIPE, case["bg"])) == base and be.feature_images == 0
    f_want = FH.oracle_feature_image(oracle, case, feats)
    ft = feats.clone().requires_grad_(True)
    pc = _PC(case["sc"])
    out = render(case["cam"], pc, PIPE, case["bg"], features=ft)
    assert set(out) == base | {"features"} and np.array_equal(out["features"].detach().numpy(), f_want)
    (out["features"] * GF).sum().backward()
    want, _, dfeat, _ = FH.feature_expectation(oracle, case, None, GF, feats)
    assert_grads_close(dict(f=ft.grad.numpy(), o=pc.get_opacity.grad.numpy(), m=out["viewspace_points"].grad.numpy()),
                       dict(f=dfeat, o=want["dL_dopacity"], m=want["dL_dmeans2D"]), tag="render(): feature-only loss")
    sem = torch.rand(case["sc"]["xyz"].shape[0], 3, generator=torch.Generator().manual_seed(4))
    out = render(case["cam"], _PC(case["sc"]), PIPE, case["bg"], semantic_color=sem, return_alpha=True, features=feats)
    assert set(out) == base | {"alpha", "semantic", "features"}
    assert out["alpha"].shape == (1, H, W) and out["semantic"].shape == (3, H, W) and out["features"].shape == (5, H, W)


def test_features_are_refused_with_the_exchange_modes_of_the_grad_allocator(monkeypatch):
    """`features=` with an allocator that answers "sh_rgb" or "row_state": an error naming the mode, before any native call
    (tensors on the meta device, with the binding's "is it on a GPU" check switched off: nothing here can reach a kernel)."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    monkeypatch.setattr(_C, "_require_cuda", lambda *a: None)

    P, M, C, H, W = 5, 16, 4, 8, 6
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="meta")  # noqa: E731
    e = z(0)
    args = (z(3), z(P, 3), z(P, dt=torch.int32), e, z(P, 3), z(P, 4), 1.0, e, z(4, 4), z(4, 4), 1.0, 1.0, z(3, H, W), z(P, M, 3), 3,
            z(3), z(256, dt=torch.uint8), 0, z(0, dt=torch.uint8), z(256, dt=torch.uint8), False)
    kw = dict(features=z(P, C), dL_dout_features=z(C, H, W), feature_grad_out=z(P, C), flags=0)
    rgb = lambda name, shape, zero: z(*shape) if name == "sh_rgb" else None  # noqa: E731
    rows = lambda name, shape, zero: z(*shape, dt=torch.uint8) if name == "row_state" else None  # noqa: E731
    with pytest.raises(RuntimeError, match="sh_rgb"):
        _C.rasterize_gaussians_backward(*args, grad_allocator=rgb, **kw)
    with pytest.raises(RuntimeError, match="row_state"):
        _C.rasterize_gaussians_backward(*args, grad_allocator=rows, **kw)


def test_binding_checks_the_feature_arguments_by_name():
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    m3 = torch.zeros(5, 3)
    args = (None, m3, None, None, None, None, 1.0, None, None, None, 1.0, 1.0, torch.zeros(3, 8, 6), torch.empty(0), 0, None,
            None, 0, None, None, False)
    ok = dict(features=torch.zeros(5, 4), dL_dout_features=torch.zeros(4, 8, 6), feature_grad_out=torch.zeros(5, 4))
    for key, bad, word in (("features", torch.zeros(5, 4, dtype=torch.float64), "float32"), ("features", torch.zeros(4, 4), "(5, C)"),
                           ("features", torch.zeros(5, 0), "(5, C)"), ("features", torch.zeros(5, 257), "(5, C)"),
                           ("features", torch.zeros(5), "(5, C)"), ("features", "x", "float32"),
                           ("features", torch.zeros(5, 4, device="meta"), "is on meta"),
                           ("dL_dout_features", torch.zeros(4, 8, 6, dtype=torch.float16), "float32"),
                           ("dL_dout_features", torch.zeros(3, 8, 6), "(4, 8, 6)"), ("dL_dout_features", torch.zeros(4, 6, 8), "(4, 8, 6)"),
                           ("dL_dout_features", torch.zeros(4, 8, 6, device="meta"), "is on meta"),
                           ("feature_grad_out", torch.zeros(5, 4, dtype=torch.float64), "float32"),
                           ("feature_grad_out", torch.zeros(5, 3), "(5, 4)"), ("feature_grad_out", torch.zeros(4, 5).t(), "contiguous"),
                           ("feature_grad_out", torch.zeros(5, 4, device="meta"), "is on meta")):
        with pytest.raises(RuntimeError, match=key) as e:
            _C.rasterize_gaussians_backward(*args, **dict(ok, **{key: bad}))
        assert word in str(e.value), (key, word, str(e.value))
    with pytest.raises(RuntimeError, match="together"):
        _C.rasterize_gaussians_backward(*args, features=ok["features"])
    # the public interface refuses before anything is rendered
    rs = None
    for bad, word in ((torch.zeros(5, 4, dtype=torch.float64), "float32"), (torch.zeros(6, 4), "(5, C)"), (torch.zeros(5, 300), "(5, C)"),
                      (torch.zeros(5, 4, device="meta"), "is on meta")):
        with pytest.raises(RuntimeError, match="features") as e:
            GaussianRasterizer(rs)(m3, m3, torch.zeros(5, 1), shs=torch.zeros(5, 16, 3), scales=m3, rotations=torch.zeros(5, 4),
                                   features=bad)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(RuntimeError, match="features"):
        _C.rasterize_features(torch.zeros(5, 4), 0, None, None, None, 8, 6)  # (no CPU path: the tensor is not on a GPU)
