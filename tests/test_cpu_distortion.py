"""The depth-distortion image (`return_distortion`; include/gsr.h gsr_blend_forward_distortion,
gsr_blend_backward_distortion) without a GPU: the mathematics in float64, a float32 model of the shifted accumulation on the
far slab (and of the unshifted one, which must miss the bar), the header and the refusals of the two entry points, the
yardstick of the GPU tests (distortion_helpers.f64_distortion) against a direct autograd of the definition, and the L1 /
render() layers over a CPU stand-in for `_C`."""
import ctypes
import os

import numpy as np
import pytest
import torch

import distortion_helpers as DH
from helpers import settings

ONE = ctypes.c_void_p(256)
ACC = ctypes.c_void_p(1 << 12)  # (64-byte aligned)
f32 = ctypes.c_float


# ---- the mathematics -------------------------------------------------------------------------------------------------------
def _pixel(n=40, seed=0, z_lo=3.0, spread=2.0):
    g = torch.Generator().manual_seed(seed)
    al = (torch.rand(n, dtype=torch.float64, generator=g) * 0.3 + 0.01).requires_grad_()
    m = (z_lo + torch.sort(torch.rand(n, dtype=torch.float64, generator=g))[0] * spread).requires_grad_()
    return al, m


def _pairwise(al, m):
    T = torch.cumprod(torch.cat([al.new_ones(1), 1 - al[:-1]]), 0)
    w = al * T
    return 0.5 * (w[:, None] * w[None, :] * (m[:, None] - m[None, :]) ** 2).sum(), w, T


@pytest.mark.parametrize("z_lo,spread", [(3.0, 2.0), (50.0, 0.05)])
def test_pairwise_moment_and_prefix_forms_agree_in_float64(z_lo, spread):
    al, m = _pixel(z_lo=z_lo, spread=spread)
    D, w, _ = _pairwise(al, m)
    w, md = w.detach(), m.detach() - m.detach()[0]  # (shifted: the three forms are compared where none of them cancels)
    A, M1, M2 = w.sum(), (w * md).sum(), (w * md * md).sum()
    moment = A * M2 - M1 * M1
    pa = pm1 = pm2 = run = torch.zeros((), dtype=torch.float64)
    for i in range(w.numel()):  # 2DGS's running sum
        run = run + w[i] * (md[i] * md[i] * pa + pm2 - 2 * md[i] * pm1)
        pa, pm1, pm2 = pa + w[i], pm1 + w[i] * md[i], pm2 + w[i] * md[i] * md[i]
    for name, v in (("moment", moment), ("prefix", run)):
        assert abs(v.item() - D.item()) <= 1e-12 * abs(D.item()), (name, v.item(), D.item())


def test_closed_form_gradients_and_the_alpha_recurrence_equal_autograd():
    al, m = _pixel()
    D, w, T = _pairwise(al, m)
    gal, gm = torch.autograd.grad(D, [al, m])
    w, T, ald = w.detach(), T.detach(), al.detach()
    md = m.detach() - m.detach()[0]
    A, M1, M2 = w.sum(), (w * md).sum(), (w * md * md).sum()
    c = md * md * A + M2 - 2 * md * M1
    dm = 2 * w * (md * A - M1)
    assert (dm - gm).abs().max() <= 1e-12 * gm.abs().max()
    assert abs(dm.sum().item()) <= 1e-12 * dm.abs().max().item()  # (shift invariance: no term reaches z0)
    # K7's recurrence, back to front: rec <- rec + last_alpha (last_c - rec); dL/dalpha_k = T_k (c_k - rec)
    rec, last_alpha, last_c = 0.0, 0.0, 0.0
    dal = torch.zeros_like(ald)
    for k in range(ald.numel() - 1, -1, -1):
        rec = rec + last_alpha * (last_c - rec)
        dal[k] = T[k] * (c[k] - rec)
        last_alpha, last_c = ald[k].item(), c[k].item()
    assert (dal - gal).abs().max() <= 1e-12 * gal.abs().max()


@pytest.mark.parametrize("near_far", [None, DH.NEAR_FAR])
def test_float32_shifted_accumulation_holds_the_bar_on_the_far_slab_and_the_unshifted_misses_it(near_far):
    """One pixel of the far slab, 40 entries at depth 50, spread 0.05: the float32 model of the kernel's accumulation against
    float64 on the same float32 inputs.  The bar: TOL of the value (D) / of the tensor's largest entry (dD/dw, dD/dm).  The
    unshifted moments miss it by more than 100 bars on D: the test discriminates."""
    alpha, z = DH.slab_pixel()
    w = DH.pixel_weights(alpha)
    m, _ = DH.mapped(z, near_far)
    ms = m - m[0]
    A, M1, M2 = w.sum(), (w * ms).sum(), (w * ms * ms).sum()
    D, c, dm = A * M2 - M1 * M1, ms * ms * A + M2 - 2 * ms * M1, 2 * w * (ms * A - M1)
    assert D > 0
    Ds, cs, dms = DH.f32_moments(w, z, True, near_far)
    errs = (abs(Ds - D) / D, np.abs(cs - c).max() / np.abs(c).max(), np.abs(dms - dm).max() / np.abs(dm).max())
    print(f"shifted float32, near_far {near_far}: D {errs[0]:.2e}, dD/dw {errs[1]:.2e}, dD/dm {errs[2]:.2e} (bar {DH.TOL:.0e})")
    assert max(errs) <= DH.TOL, errs
    Du, _, _ = DH.f32_moments(w, z, False, near_far)
    print(f"unshifted float32: D off by {abs(Du - D) / D:.2e} of its value")
    assert abs(Du - D) / D > 100 * DH.TOL


# ---- header, symbols, refusals ----------------------------------------------------------------------------------------------
def test_header_symbols_and_signatures():
    from gaussianeditor_amd import _native

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gsr.h")).read()
    assert "#define GSR_ABI_VERSION 6" in hdr and _native.lib().gsr_abi_version() == 6
    assert "#define GSR_FLAG_ALL (127u | GSR_FLAG_ANTIALIAS)" in hdr  # (no new flag bit)
    for name in ("gsr_blend_forward_distortion", "gsr_blend_backward_distortion"):
        assert f"int {name}(" in hdr and name in _native.SIGNATURES and hasattr(_native.lib(), name)


def test_entry_points_validate_arguments_without_a_gpu():
    """No call here reaches the device: the backward with R = 0 launches nothing, everything else is refused."""
    from gaussianeditor_amd import _native

    L = _native.lib()

    def fwd(P=10, R_=5, W=64, H=64, geom=ONE, binning=ONE, image=ONE, near=0.0, far=0.0, out=ONE, mom=ONE, flags=0):
        return L.gsr_blend_forward_distortion(None, P, R_, W, H, geom, binning, image, f32(near), f32(far), out, mom, flags)

    def bwd(P=10, R_=0, W=64, H=64, geom=ONE, binning=ONE, image=ONE, near=0.0, far=0.0, mom=ONE, dimg=ONE, acc=ACC, flags=0):
        return L.gsr_blend_backward_distortion(None, P, R_, W, H, geom, binning, image, f32(near), f32(far), mom, dimg, acc, flags)
    # the backward's empty calls: R = 0, P = 0, under every flag it takes, with both depths
    for f in (0, 1, 2, 16, 1024, 1 | 2 | 16 | 1024):
        assert bwd(flags=f) == 0 and bwd(P=0, flags=f) == 0
    assert bwd(near=0.2, far=100.0) == 0 and bwd(near=1e-3, far=1e6) == 0
    inf, nan = float("inf"), float("nan")
    for call in (fwd, bwd):
        for bad in (4, 8, 32, 64, 128, 256, 512, 2048, 4096, 8192, 16384, 32768, 2 | 4096):
            assert call(flags=bad) == -1, bad
        assert call(P=-1) == -1 and call(R_=-5) == -1 and call(W=0) == -1 and call(H=-3) == -1
        assert call(image=None) == -1
        assert call(R_=5, geom=None) == -1 and call(R_=5, binning=None) == -1
        assert call(R_=5, geom=ctypes.c_void_p(256 + 16)) == -1 and call(R_=5, image=ctypes.c_void_p(256 + 64)) == -1
        for near, far in ((0.0, 1.0), (1.0, 0.0), (-1.0, 2.0), (2.0, 2.0), (3.0, 2.0), (0.2, inf), (inf, inf), (nan, 1.0), (0.2, nan),
                          (0.0, -0.0 + 5.0), (-0.5, 0.0)):
            assert call(near=near, far=far) == -1, (near, far)
        assert call(mom=ctypes.c_void_p(256 + 4)) == -1  # (float4 rows)
    assert fwd(out=None) == -1 and fwd(out=ctypes.c_void_p(258)) == -1
    assert bwd(mom=None) == -1 and bwd(dimg=None) == -1 and bwd(dimg=ctypes.c_void_p(258)) == -1
    assert bwd(acc=None) == -1 and bwd(acc=ctypes.c_void_p(4096 + 16)) == -1 and bwd(acc=ctypes.c_void_p(4096 + 32)) == -1
    assert bwd(R_=5, W=16400, H=16400) == -1  # (more tiles than the backward's work items can name)


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
def _direct_autograd(case, f, GDist, near_far):
    """<GDist, D> differentiated in ONE float64 graph, the depth a function of means3D (tz = the view matrix's z row)."""
    from oracle.torch_ref import render_f64

    d = torch.float64
    cam, W, H = case["cam"], case["W"], case["H"]
    lv = DH._leaves(case)
    V = cam.world_view_transform.to(d).reshape(4, 4)
    tz = lv["dL_dmeans3D"] @ V[:3, 2] + V[3, 2]
    if near_far is None:
        m = tz
    else:
        n, fa = near_far
        m = fa * (tz - n) / ((fa - n) * tz)
    m = m - m.detach().median()
    cols = torch.stack([torch.ones_like(m), m, m * m], dim=1)
    img = render_f64(f, lv["dL_dmeans3D"], lv["dL_dmeans2D"], lv["dL_dopacity"], lv["dL_dscales"], lv["dL_drotations"], None, cols,
                     None, cam.world_view_transform, cam.full_proj_transform, cam.camera_center, torch.zeros(3), W, H,
                     case["tfx"], case["tfy"], 1.0, case["D"])
    Dimg = img[0] * img[2] - img[1] * img[1]
    (Dimg * GDist.to(d).reshape(H, W)).sum().backward()
    return Dimg.detach().numpy(), {k: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for k, t in lv.items()}


@pytest.mark.parametrize("near_far", [None, DH.NEAR_FAR])
def test_yardstick_equals_a_direct_autograd_of_the_definition(oracle, near_far):
    """distortion_helpers.f64_distortion -- two renders, the depth gradient chained by hand -- against one float64 graph in
    which the depth is a function of means3D.  The two differ in the depths alone (float32 data against float64 tz): 1e-6."""
    case, f, e, masked = DH.expectation("partial", near_far=near_far)
    Dimg, want = _direct_autograd(case, f, DH.weights(case), near_far)
    assert np.abs(Dimg).max() > 0
    assert np.abs(e["image"] - Dimg).max() <= 1e-5 * np.abs(Dimg).max()
    for k in DH.KEYS:
        err = np.abs(e["want"][k] - want[k]).max() / np.abs(want[k]).max()
        print(f"  yardstick vs direct autograd, near_far {near_far}: {k} {err:.2e}")
        assert err <= 1e-5, (k, err)
    # the depth path matters: without it dL_dmeans3D is off by far more than the bar
    no_depth = e["share"]["dL_dmeans3D"] - (e["dL_dz"][:, None] * case["cam"].world_view_transform.double().reshape(4, 4)[:3, 2].numpy())
    assert np.abs(no_depth - want["dL_dmeans3D"]).max() > 100 * DH.TOL * np.abs(want["dL_dmeans3D"]).max()


@pytest.mark.parametrize("name", ["partial", "p2000", "ragged", "p4000", "far_slab", "single"])
def test_cases_hit_their_regime_and_mask_nothing(oracle, name):
    """Every GPU case: no row is masked (no pixel whose float64 and float32 discrete decisions differ, no Gaussian on the cone
    edge), the image is not trivially zero, and the case exercises what the issue's table says."""
    case, f, e, masked = DH.expectation(name)
    assert int(masked.sum()) == 0, (name, int(masked.sum()))
    nc = f["n_contrib"].reshape(-1)
    ranges = f["ranges"].astype(np.int64)
    longest = int((ranges[:, 1] - ranges[:, 0]).max())
    print(f"[{name}] longest tile list {longest}, deepest contributor {int(nc.max())}, max D {e['image'].max():.3e}")
    assert e["image"].max() > 0 and e["image"].min() >= -1e-12 * e["image"].max()
    if name == "p4000":
        assert longest > 3 * 64  # lists of several chunks
    if name == "far_slab":
        z = f["depths"][f["radii"] > 0]
        assert z.min() >= 49.99 and z.max() <= 50.06 and int(nc.max()) >= 20
    if name == "single":
        # pixels with exactly one contributor: D and the gradient's density are exactly zero there
        w_img = DH.f64_distortion(f, case, DH.weights(case))["image"]
        stats = e["stats"]
        one = (stats["n_contrib"].numpy() == 1)
        assert one.sum() > 20 and np.all(w_img.reshape(-1)[one] == 0.0) and (w_img > 0).sum() >= 4


# ---- the L1 and render() layers over a CPU stand-in ---------------------------------------------------------------------------
def _leaves(sc):
    leaf = lambda t: t.clone().requires_grad_(True)  # noqa: E731
    L = dict(xyz=leaf(sc["xyz"]), op=leaf(sc["opacity"]), sh=leaf(sc["features"]), scl=leaf(sc["scaling"]), rot=leaf(sc["rotation"]))
    L["m2d"] = torch.zeros_like(L["xyz"], requires_grad=True)
    return L


def _render(dgr, rs, sc, **kw):
    L = _leaves(sc)
    return L, dgr.GaussianRasterizer(rs)(L["xyz"], L["m2d"], L["op"], shs=L["sh"], scales=L["scl"], rotations=L["rot"], **kw)


def test_l1_arity_tuples_and_backward_keywords_over_a_cpu_backend(oracle, monkeypatch):
    import features_helpers as FH

    dgr, be, db = DH.install(monkeypatch)
    case, G, GF, feats = FH.feature_case("p600", C=5)
    sc, H, W = case["sc"], case["H"], case["W"]
    P = sc["xyz"].shape[0]
    rs = settings(case, "cpu")
    seen = []
    real_apply = dgr._RasterizeGaussians.apply
    monkeypatch.setattr(dgr._RasterizeGaussians, "apply", staticmethod(lambda *a: (seen.append(a), real_apply(*a))[1]))
    aux = torch.rand(P, 3, generator=torch.Generator().manual_seed(2))
    # without the keyword: today's tuples, today's arity, no distortion call, no distortion keyword in the backward
    for kw, n_in, n_out in ((dict(), 9, 3), (dict(return_alpha=True), 11, 4), (dict(aux_colors=aux), 10, 4),
                            (dict(return_distortion=False), 9, 3), (dict(return_distortion=None), 9, 3)):
        L, outs = _render(dgr, rs, sc, **kw)
        assert len(outs) == n_out and len(seen[-1]) == n_in
        (outs[0] * G).sum().backward()
    assert not db.distortion_calls and "rasterize_distortion" not in [c[0] for c in be.calls]
    assert all(not k["moments"] and not k["grad"] and k["near_far"] is None and k["other"] == ("flags", "grad_allocator")
               for k in db.backward_kw) and len(db.backward_kw) == 5
    assert all(c == ("rasterize_gaussians", 19, ("flags",)) for c in be.calls if c[0] == "rasterize_gaussians")
    # with it: the image is the LAST value whatever else is asked; input 15 is the (near, far) pair
    L, outs = _render(dgr, rs, sc, return_distortion=True)
    assert len(outs) == 4 and outs[-1].shape == (1, H, W) and outs[-1].requires_grad
    assert len(seen[-1]) == 16 and seen[-1][15] == (0.0, 0.0) and seen[-1][9:15] == (None, False, None, None, None, None)
    assert db.distortion_calls[-1] == dict(P=P, near_far=None, with_moments=True)
    n_bw = len(db.backward_kw)
    (outs[-1] * DH.weights(case)).sum().backward()  # the distortion image alone
    assert len(db.backward_kw) == n_bw + 1 and db.backward_kw[-1]["moments"] and db.backward_kw[-1]["grad"]
    assert db.backward_kw[-1]["near_far"] is None
    assert all(L[k].grad is not None for k in ("xyz", "op", "scl", "rot", "m2d"))
    ft = feats.clone().requires_grad_(True)
    L, outs = _render(dgr, rs, sc, return_distortion=(0.2, 100), return_alpha=True, aux_colors=aux, features=ft)
    assert len(outs) == 7 and outs[-1].shape == (1, H, W) and outs[-2].shape == (5, H, W) and outs[-3].shape == (1, H, W)
    assert float(outs[-1].detach()[0, 0, 0]) == 0.5 and seen[-1][15] == (0.2, 100.0) and seen[-1][14] is ft
    assert db.distortion_calls[-1]["near_far"] == (0.2, 100.0)
    ((outs[0] * G).sum() + (outs[-1] * DH.weights(case)).sum() + (outs[-2] * GF).sum()).backward()
    assert db.backward_kw[-1]["near_far"] == (0.2, 100.0) and db.backward_kw[-1]["moments"] and ft.grad is not None
    # the image asked for and not used: a plain backward
    L, outs = _render(dgr, rs, sc, return_distortion=True)
    (outs[0] * G).sum().backward()
    assert not db.backward_kw[-1]["moments"] and not db.backward_kw[-1]["grad"]
    # with the normals (their GPU kernel replaced by a stand-in: the layer under test is the arity): behind them
    from gaussianeditor_amd import normals
    monkeypatch.setattr(normals, "gaussian_normals", lambda rot, scl, xyz, view: rot[:, :3] * 0.5)
    L, outs = _render(dgr, rs, sc, return_distortion=True, return_normals=True)
    assert len(outs) == 5 and outs[-1].shape == (1, H, W) and outs[-2].shape == (3, H, W)
    # no input requires a gradient (the viewer): forward only, no moments
    outs = dgr.GaussianRasterizer(rs)(sc["xyz"], None, sc["opacity"], shs=sc["features"], scales=sc["scaling"],
                                      rotations=sc["rotation"], return_distortion=True)
    assert db.distortion_calls[-1]["with_moments"] is False and not outs[-1].requires_grad


def test_view_reuse_never_serves_a_distortion_render(oracle, monkeypatch):
    import features_helpers as FH

    dgr, be, db = DH.install(monkeypatch)
    case, G, GF, feats = FH.feature_case("p600", C=5)
    sc = case["sc"]
    rs = settings(case, "cpu")
    cols = torch.rand(sc["xyz"].shape[0], 3, generator=torch.Generator().manual_seed(3))
    R = dgr.GaussianRasterizer(rs)
    with torch.no_grad():
        R(sc["xyz"], None, sc["opacity"], shs=sc["features"], scales=sc["scaling"], rotations=sc["rotation"])
        n = len([c for c in be.calls if c[0] == "rasterize_gaussians"])
        outs = R(sc["xyz"], None, sc["opacity"], colors_precomp=cols, scales=sc["scaling"], rotations=sc["rotation"],
                 return_distortion=True)
    assert len(outs) == 4 and len([c for c in be.calls if c[0] == "rasterize_gaussians"]) == n + 1


def test_render_adds_distortion_only_with_the_keyword(oracle, monkeypatch):
    import features_helpers as FH

    dgr, be, db = DH.install(monkeypatch)
    from gaussianeditor_amd.gaussian_renderer import render
    from test_cpu_host_api import _PC, PIPE

    case, G, GF, feats = FH.feature_case("p600", C=5)
    H, W = case["H"], case["W"]
    base = {"render", "viewspace_points", "visibility_filter", "radii", "depth_3dgs"}
    assert set(render(case["cam"], _PC(case["sc"]), PIPE, case["bg"])) == base and not db.distortion_calls
    assert set(render(case["cam"], _PC(case["sc"]), PIPE, case["bg"], return_distortion=False)) == base and not db.distortion_calls
    out = render(case["cam"], _PC(case["sc"]), PIPE, case["bg"], return_distortion=True)
    assert set(out) == base | {"distortion"} and out["distortion"].shape == (1, H, W)
    sem = torch.rand(case["sc"]["xyz"].shape[0], 3, generator=torch.Generator().manual_seed(4))
    from gaussianeditor_amd import normals
    monkeypatch.setattr(normals, "gaussian_normals", lambda rot, scl, xyz, view: rot[:, :3] * 0.5)  # (a stand-in: no GPU here)
    out = render(case["cam"], _PC(case["sc"]), PIPE, case["bg"], semantic_color=sem, return_alpha=True, features=feats,
                 return_normals=True, return_distortion=(0.2, 100.0))
    assert set(out) == base | {"alpha", "semantic", "features", "normals", "distortion"}
    assert out["alpha"].shape == (1, H, W) and out["semantic"].shape == (3, H, W) and out["features"].shape == (5, H, W)
    assert out["normals"].shape == (3, H, W) and out["distortion"].shape == (1, H, W) and float(out["distortion"].detach()[0, 0, 0]) == 0.5


def test_near_far_is_validated_by_name_before_anything_is_rendered():
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    m3 = torch.zeros(5, 3)
    inf, nan = float("inf"), float("nan")
    for bad in ((0.0, 1.0), (1.0, 1.0), (2.0, 1.0), (-1.0, 1.0), (0.2, inf), (nan, 1.0), (0.2, nan), (0.2,), (0.2, 1.0, 2.0), "ab", 3.0,
                ("x", 1.0)):
        with pytest.raises(RuntimeError, match="return_distortion"):
            GaussianRasterizer(None)(m3, m3, torch.zeros(5, 1), shs=torch.zeros(5, 16, 3), scales=m3, rotations=torch.zeros(5, 4),
                                     return_distortion=bad)
        with pytest.raises(RuntimeError, match="near_far"):
            _C.check_near_far(bad)
    assert _C.check_near_far(None) == (0.0, 0.0) and _C.check_near_far((0.2, 100)) == (0.2, 100.0)
    assert _C.check_near_far([1, 2]) == (1.0, 2.0)


def test_binding_checks_the_distortion_arguments_by_name():
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    m3 = torch.zeros(5, 3)
    args = (None, m3, None, None, None, None, 1.0, None, None, None, 1.0, 1.0, torch.zeros(3, 8, 6), torch.empty(0), 0, None,
            None, 0, None, None, False)
    ok = dict(distortion_moments=torch.zeros(8, 6, 4), dL_dout_distortion=torch.zeros(1, 8, 6))
    for key, bad, word in (("distortion_moments", torch.zeros(8, 6, 4, dtype=torch.float64), "float32"),
                           ("distortion_moments", torch.zeros(8, 6, 3), "(8, 6, 4)"), ("distortion_moments", torch.zeros(6, 8, 4), "(8, 6, 4)"),
                           ("distortion_moments", "x", "float32"), ("distortion_moments", torch.zeros(8, 6, 4, device="meta"), "is on meta"),
                           ("dL_dout_distortion", torch.zeros(1, 8, 6, dtype=torch.float16), "float32"),
                           ("dL_dout_distortion", torch.zeros(8, 6), "(1, 8, 6)"), ("dL_dout_distortion", torch.zeros(3, 8, 6), "(1, 8, 6)"),
                           ("dL_dout_distortion", torch.zeros(1, 8, 6, device="meta"), "is on meta")):
        with pytest.raises(RuntimeError, match=key) as e:
            _C.rasterize_gaussians_backward(*args, **dict(ok, **{key: bad}))
        assert word in str(e.value), (key, word, str(e.value))
    with pytest.raises(RuntimeError, match="together"):
        _C.rasterize_gaussians_backward(*args, distortion_moments=ok["distortion_moments"])
    with pytest.raises(RuntimeError, match="together"):
        _C.rasterize_gaussians_backward(*args, dL_dout_distortion=ok["dL_dout_distortion"])
    with pytest.raises(RuntimeError, match="distortion_near_far"):
        _C.rasterize_gaussians_backward(*args, distortion_near_far=(0.2, 100.0))
    with pytest.raises(RuntimeError, match="distortion_near_far"):
        _C.rasterize_gaussians_backward(*args, distortion_near_far=(1.0, 0.5), **ok)
    with pytest.raises(RuntimeError, match="imgBuffer"):  # (no CPU path: the state is not on a GPU)
        _C.rasterize_distortion(5, 1, torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8),
                                torch.zeros(8, dtype=torch.uint8), 8, 6)
    with pytest.raises(RuntimeError, match="near_far"):
        _C.rasterize_distortion(5, 1, None, None, None, 8, 6, near_far=(1.0, 1.0))


def test_distortion_is_refused_with_the_exchange_modes_of_the_grad_allocator(monkeypatch):
    """`distortion_moments=` with an allocator that answers "sh_rgb" or "row_state": an error naming the mode, before any native
    call (tensors on the meta device, with the binding's "is it on a GPU" check switched off)."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    monkeypatch.setattr(_C, "_require_cuda", lambda *a: None)
    P, M, H, W = 5, 16, 8, 6
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="meta")  # noqa: E731
    e = z(0)
    args = (z(3), z(P, 3), z(P, dt=torch.int32), e, z(P, 3), z(P, 4), 1.0, e, z(4, 4), z(4, 4), 1.0, 1.0, z(3, H, W), z(P, M, 3), 3,
            z(3), z(256, dt=torch.uint8), 0, z(0, dt=torch.uint8), z(256, dt=torch.uint8), False)
    kw = dict(distortion_moments=z(H, W, 4), dL_dout_distortion=z(1, H, W), flags=0)
    rgb = lambda name, shape, zero: z(*shape) if name == "sh_rgb" else None  # noqa: E731
    rows = lambda name, shape, zero: z(*shape, dt=torch.uint8) if name == "row_state" else None  # noqa: E731
    with pytest.raises(RuntimeError, match="sh_rgb"):
        _C.rasterize_gaussians_backward(*args, grad_allocator=rgb, **kw)
    with pytest.raises(RuntimeError, match="row_state"):
        _C.rasterize_gaussians_backward(*args, grad_allocator=rows, **kw)
