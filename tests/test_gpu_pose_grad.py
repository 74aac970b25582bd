"""-m gpu: camera pose gradients (gaussianeditor_amd.set_pose_grad; include/gsr.h gsr_pose_backward).
  1. values against float64 autograd with the three camera tensors as leaves, the list structure taken from the PRODUCT's
     forward, zero flipped pixels asserted (a sum over the Gaussians cannot mask rows) -- bars in pose_helpers;
  2. the translation identity c.grad = - sum dL/dmu for every combination of antialiasing x depth x alpha x alpha tile bounds;
  3. the sizes at which the reduction can go wrong (one Gaussian, around a wave, more than one block, more than 1024 blocks);
  4. nothing visible: 35 exact zeros, fully written;  5. bit-identical repeats on one accumulator table;  6. plumbing.
Every test of 1-3 and the pose-only case of 6 fails where the camera receives no gradient."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import f64_regimes as R
import pose_helpers as PH
from helpers import flipped_pixels, hip_state, make_case, seed_gradient

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _settings(case, V, PV, C, D=None, sm=1.0):
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizationSettings

    return GaussianRasterizationSettings(case["H"], case["W"], case["tfx"], case["tfy"], case["bg"].to(DEV), sm, V, PV,
                                         case["D"] if D is None else D, C, False, False)


def _cam_leaves(cam):
    leaf = lambda t: t.detach().to(DEV).float().clone().requires_grad_(True)  # noqa: E731
    return leaf(cam.world_view_transform), leaf(cam.full_proj_transform), leaf(cam.camera_center)


def _gaussians(r, requires_grad=True):
    """-> (means3D, means2D, opacities, keyword arguments of GaussianRasterizer.forward), on the device."""
    sc = r["case"]["sc"]
    leaf = lambda t: t.to(DEV).clone().requires_grad_(requires_grad)  # noqa: E731
    xyz, op = leaf(sc["xyz"]), leaf(sc["opacity"])
    m2d = torch.zeros_like(xyz, requires_grad=requires_grad)
    kw = {}
    if r["colors_precomp"] is None:
        kw["shs"] = leaf(sc["features"])
    else:
        kw["colors_precomp"] = leaf(r["colors_precomp"])
    if r["cov3D_precomp"] is None:
        kw["scales"], kw["rotations"] = leaf(sc["scaling"]), leaf(sc["rotation"])
    else:
        kw["cov3D_precomp"] = leaf(r["cov3D_precomp"])
    return xyz, m2d, op, kw


def _product_forward_state(r):
    """The product's forward of the case, pulled out of its state: what render_f64 takes the list structure from and what
    the flipped-pixel condition compares."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    case, sc = r["case"], r["case"]["sc"]
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    e = torch.empty(0, device=DEV)
    cam = case["cam"]
    P, W, H = sc["xyz"].shape[0], case["W"], case["H"]
    cols, cov = r["colors_precomp"], r["cov3D_precomp"]
    R_, color, depth, radii, geom, binning, img = _C.rasterize_gaussians(
        d(case["bg"]), d(sc["xyz"]), e if cols is None else d(cols), d(sc["opacity"]), e if cov is not None else d(sc["scaling"]),
        e if cov is not None else d(sc["rotation"]), r["sm"], e if cov is None else d(cov), d(cam.world_view_transform),
        d(cam.full_proj_transform), case["tfx"], case["tfy"], H, W, d(sc["features"]) if cols is None else e, r["D"],
        d(cam.camera_center), False, False, flags=0)
    f = hip_state(P, R_, W, H, geom, binning, img,
                  cov_inputs=None if cov is not None else (sc["scaling"], sc["rotation"], r["sm"]))
    f["radii"] = radii.cpu().numpy()
    return f


def _product_pose(r, flags_extra=0):
    """Camera gradients of the case's loss through GaussianRasterizer under FLAG_POSE_GRAD, the three tensors as leaves."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    case = r["case"]
    V, PV, C = _cam_leaves(case["cam"])
    xyz, m2d, op, kw = _gaussians(r)
    flags = options.FLAG_POSE_GRAD | flags_extra | (options.FLAG_DEPTH_GRAD if r["GD"] is not None else 0)
    with options.override(flags):
        color, radii, depth = GaussianRasterizer(_settings(case, V, PV, C, D=r["D"], sm=r["sm"]))(xyz, m2d, op, **kw)
    loss = (color * r["G"].to(DEV)).sum()
    if r["GD"] is not None:
        loss = loss + (depth * r["GD"].to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert V.grad is not None and PV.grad is not None and C.grad is not None, "the camera received no gradient"
    assert V.grad.shape == (4, 4) and PV.grad.shape == (4, 4) and C.grad.shape == (3,)
    return dict(view=V.grad.cpu().numpy(), proj=PV.grad.cpu().numpy(), campos=C.grad.cpu().numpy()), xyz.grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _expectation(name, camera=None, seed=None):
    from oracle import cpu

    cpu.build()  # (the cov3D_precomp regime takes its covariances from the oracle's forward)
    r = PH.pose_regime(name, camera=camera, seed=seed)
    f = _product_forward_state(r)
    want_cam, want, stats = PH.f64_pose(f, r)
    flips = flipped_pixels(stats["n_contrib"].numpy(), stats["final_T"].numpy(), f["n_contrib"], f["final_T"])
    edge = int((R.cone_edge_rows(r) & (f["radii"] > 0)).sum())
    print(f"[{name}] flipped pixels {flips.size}, visible Gaussians on the cone edge {edge}")
    return r, f, want_cam, want, stats, flips.size


# ---- 1. values against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PH.POSE_CASES)
def test_pose_gradients_match_float64(name):
    r, f, want_cam, want, stats, flips = _expectation(name)
    assert flips == 0, (name, "the product's forward and float64 differ in a discrete decision", flips)
    R.regime_count(r, f, want, stats)
    got, _ = _product_pose(r)
    PH.assert_pose_close(got, want_cam, f"product vs float64 [{name}]", colors_precomp=r["colors_precomp"] is not None)


# ---- 2. translation identity, every flag combination ----------------------------------------------------------------------
def _identity_run(case, flags_extra, depth, alpha):
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    sc, H, W = case["sc"], case["H"], case["W"]
    c, V, PV, C = PH.moved_camera(case["cam"], torch.float32, DEV)
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)  # noqa: E731
    xyz, op, sh, scl, rot = (leaf(sc[k]) for k in ("xyz", "opacity", "features", "scaling", "rotation"))
    m2d = torch.zeros_like(xyz, requires_grad=True)
    flags = options.FLAG_POSE_GRAD | flags_extra | (options.FLAG_DEPTH_GRAD if depth else 0)
    with options.override(flags):
        outs = GaussianRasterizer(_settings(case, V, PV, C))(xyz, m2d, op, shs=sh, scales=scl, rotations=rot, return_alpha=alpha)
    loss = (outs[0] * (seed_gradient(H, W, 19) * H * W).to(DEV)).sum()
    if depth:
        loss = loss + (outs[2] * (seed_gradient(H, W, 81)[:1] * H * W).to(DEV)).sum()
    if alpha:
        loss = loss + (outs[3] * (seed_gradient(H, W, 5)[:1] * H * W).to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert c.grad is not None, "the camera received no gradient"
    return c.grad.cpu().numpy(), xyz.grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _identity_case():
    return PH.identity_case()


@pytest.mark.parametrize("bounds", [False, True], ids=["reference_bounds", "alpha_bounds"])
@pytest.mark.parametrize("alpha", [False, True], ids=["no_alpha", "alpha"])
@pytest.mark.parametrize("depth", [False, True], ids=["no_depth", "depth"])
@pytest.mark.parametrize("aa", [False, True], ids=["no_aa", "aa"])
def test_translation_identity(aa, depth, alpha, bounds):
    from gaussianeditor_amd import options

    extra = (options.FLAG_ANTIALIAS if aa else 0) | (options.FLAG_TILE_BOUNDS_ALPHA if bounds else 0)
    cg, mg = _identity_run(_identity_case(), extra, depth, alpha)
    PH.assert_identity(cg, mg, f"identity aa={aa} depth={depth} alpha={alpha} alpha_bounds={bounds}")


def test_translation_identity_with_fast_exp():
    from gaussianeditor_amd import options

    cg, mg = _identity_run(_identity_case(), options.FLAG_FAST_EXP, False, False)
    PH.assert_identity(cg, mg, "identity fast_exp")


# ---- 3. shapes where the reduction can go wrong ---------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
def test_small_counts_match_float64(P):
    """One Gaussian, one short of a wave, a wave, one more, one more than a block: every Gaussian close to the point the
    camera looks at, so that all of them are on the 32 x 32 image."""
    case = make_case(P, 32, 32, seed=90 + P, s0=0.08, view=1, scale_xyz=0.25, bg=(0.2, 0.5, 0.7))
    G = seed_gradient(32, 32, 23) * 32 * 32
    r = dict(name=f"P{P}", case=case, D=3, sm=1.0, colors_precomp=None, cov3D_precomp=None, G=G, GD=None)
    f = _product_forward_state(r)
    assert int((f["radii"] > 0).sum()) == P
    want_cam, _, stats = PH.f64_pose(f, r)
    flips = flipped_pixels(stats["n_contrib"].numpy(), stats["final_T"].numpy(), f["n_contrib"], f["final_T"])
    assert flips.size == 0, (P, flips.size)
    got, _ = _product_pose(r)
    PH.assert_pose_close(got, want_cam, f"product vs float64 [P = {P}]")


def test_more_than_1024_blocks_satisfies_the_identity():
    """300 000 Gaussians: 1 172 blocks of 256, so the kernel's 1 024 blocks stride over the table a second time."""
    case = make_case(300_000, 128, 128, seed=17, s0=0.004, view=2, bg=(0.2, 0.5, 0.7))
    cg, mg = _identity_run(case, 0, False, False)
    assert int((np.abs(mg).max(axis=1) > 0)[1024 * 256:].sum()) > 100  # (rows of the second pass carry a gradient)
    PH.assert_identity(cg, mg, "identity P = 300 000")


# ---- 4. nothing visible ---------------------------------------------------------------------------------------------------
def _behind_camera_case(P=500):
    case = make_case(P, 64, 48, seed=3, view=0)
    cam = case["cam"]
    fwd = cam.world_view_transform[:3, 2]  # view-space z of a point = mu . V[:3, 2] + V[3, 2]
    sc = dict(case["sc"])
    sc["xyz"] = (cam.camera_center[None, :] - (3.0 + torch.rand(P, 1, generator=torch.Generator().manual_seed(4))) * fwd[None, :]
                 + 0.1 * sc["xyz"]).contiguous()
    return dict(case, sc=sc)


def _c_forward(case, flags=0):
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    sc, cam = case["sc"], case["cam"]
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    e = torch.empty(0, device=DEV)
    args = dict(bg=d(case["bg"]), xyz=d(sc["xyz"]), op=d(sc["opacity"]), scl=d(sc["scaling"]), rot=d(sc["rotation"]),
                V=d(cam.world_view_transform), PV=d(cam.full_proj_transform), C=d(cam.camera_center), sh=d(sc["features"]), e=e)
    a = args
    out = _C.rasterize_gaussians(a["bg"], a["xyz"], e, a["op"], a["scl"], a["rot"], 1.0, e, a["V"], a["PV"], case["tfx"],
                                 case["tfy"], case["H"], case["W"], a["sh"], 3, a["C"], False, False, flags=flags)
    return args, out


def _c_backward(case, a, out, G, **kw):
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    R_, color, depth, radii, geom, binning, img = out
    e = a["e"]
    return _C.rasterize_gaussians_backward(a["bg"], a["xyz"], radii, e, a["scl"], a["rot"], 1.0, e, a["V"], a["PV"], case["tfx"],
                                           case["tfy"], G, a["sh"], 3, a["C"], geom, R_, binning, img, False, flags=0, **kw)


def test_nothing_visible_gives_35_exact_zeros():
    case = _behind_camera_case()
    a, out = _c_forward(case)
    assert out[0] == 0 and int((out[3] > 0).sum()) == 0
    pose = torch.full((35,), float("nan"), device=DEV)
    _c_backward(case, a, out, torch.ones(3, case["H"], case["W"], device=DEV), pose_grad_out=pose)
    torch.cuda.synchronize()
    got = pose.cpu().numpy()
    assert got.shape == (35,) and not np.any(got != 0), got  # (NaN != 0: every entry was written, with a zero)


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------
def test_pose_backward_repeats_bit_for_bit_and_leaves_the_table_alone():
    """gsr_pose_backward twice on the accumulator table one blend backward left, between the halves: the same 35 floats bit
    for bit (no float atomics: fixed-order sums), with workspaces that held different garbage, and the table unchanged."""
    from gaussianeditor_amd import _native, options

    case = PH.identity_case()
    sc, H, W = case["sc"], case["H"], case["W"]
    P = sc["xyz"].shape[0]
    a, out = _c_forward(case)
    R_, color, depth, radii, geom, binning, img = out
    assert R_ > 0
    L = _native.lib()
    s = torch.cuda.current_stream().cuda_stream
    G = (seed_gradient(H, W, 19) * H * W).to(DEV).contiguous()
    acc = torch.empty(P * _native.ACC_ROW, device=DEV)
    _native.check("gsr_blend_backward", L.gsr_blend_backward(
        s, P, R_, W, H, a["bg"].data_ptr(), geom.data_ptr(), binning.data_ptr(), img.data_ptr(), G.data_ptr(), acc.data_ptr(), None,
        options.FLAG_CLEAR_GRADS))
    before = acc.clone()
    n = ctypes.c_size_t(0)
    _native.check("gsr_pose_workspace_size", L.gsr_pose_workspace_size(P, ctypes.byref(n)))
    outs = []
    for fill in (0x00, 0xff):
        ws = torch.full((n.value,), fill, dtype=torch.uint8, device=DEV)
        pose = torch.full((35,), float("nan"), device=DEV)
        _native.check("gsr_pose_backward", L.gsr_pose_backward(
            s, P, 3, 16, W, H, a["xyz"].data_ptr(), a["scl"].data_ptr(), 1.0, a["rot"].data_ptr(), None, a["V"].data_ptr(),
            a["PV"].data_ptr(), a["C"].data_ptr(), case["tfx"], case["tfy"], radii.data_ptr(), geom.data_ptr(), acc.data_ptr(),
            ws.data_ptr(), pose.data_ptr(), 0))
        outs.append(pose)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and int((outs[0] != 0).sum()) == 27
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert torch.equal(before.view(torch.int32), acc.view(torch.int32))
    # a state left by a forward-only render is refused, as K8+K9 refuses it
    a2, out2 = _c_forward(case, flags=options.FLAG_FORWARD_ONLY)
    assert L.gsr_pose_backward(s, P, 3, 16, W, H, a2["xyz"].data_ptr(), a2["scl"].data_ptr(), 1.0, a2["rot"].data_ptr(), None,
                               a2["V"].data_ptr(), a2["PV"].data_ptr(), a2["C"].data_ptr(), case["tfx"], case["tfy"],
                               out2[3].data_ptr(), out2[4].data_ptr(), acc.data_ptr(), ws.data_ptr(), pose.data_ptr(), 0) == -1


# ---- 6. plumbing ------------------------------------------------------------------------------------------------------------
def _spy_apply(monkeypatch):
    """Records the number of arguments of every _RasterizeGaussians.apply and the flags of every _C.rasterize_gaussians."""
    import gaussianeditor_amd.diff_gaussian_rasterization as dgr

    seen = SimpleNamespace(arity=[], fwd_flags=[])
    apply, fwd = dgr._RasterizeGaussians.apply, dgr._C.rasterize_gaussians

    def spy_apply(*args):
        seen.arity.append(len(args))
        return apply(*args)

    def spy_fwd(*args, **kw):
        seen.fwd_flags.append(kw.get("flags"))
        return fwd(*args, **kw)
    monkeypatch.setattr(dgr._RasterizeGaussians, "apply", staticmethod(spy_apply))
    monkeypatch.setattr(dgr._C, "rasterize_gaussians", spy_fwd)
    return seen


def _plumbing_regime():
    case = PH.identity_case()
    H, W = case["H"], case["W"]
    return dict(name="plumbing", case=case, D=3, sm=1.0, colors_precomp=None, cov3D_precomp=None,
                G=seed_gradient(H, W, 19) * H * W, GD=None)


def test_flag_off_is_the_call_it_always_was(monkeypatch):
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    seen = _spy_apply(monkeypatch)
    r = _plumbing_regime()
    V, PV, C = _cam_leaves(r["case"]["cam"])
    xyz, m2d, op, kw = _gaussians(r)
    color, radii, depth = GaussianRasterizer(_settings(r["case"], V, PV, C))(xyz, m2d, op, **kw)
    (color * r["G"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert seen.arity == [9]
    assert V.grad is None and PV.grad is None and C.grad is None and xyz.grad is not None


def test_pose_only_optimisation_with_frozen_gaussians(monkeypatch):
    """Gaussians frozen, the camera built from a learnable translation: the gradient arrives at the translation, the forward
    did not run forward-only, and it is the gradient a render with trainable Gaussians gives the camera."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer
    from gaussianeditor_amd.pose import camera_tensors

    seen = _spy_apply(monkeypatch)
    r = _plumbing_regime()
    case, cam = r["case"], r["case"]["cam"]
    wv = cam.world_view_transform.double()
    Rm, T = wv[:3, :3].float().to(DEV), wv[3, :3].float().to(DEV).clone().requires_grad_(True)
    proj = (torch.linalg.inv(wv) @ cam.full_proj_transform.double()).float().to(DEV)
    xyz, m2d, op, kw = _gaussians(r, requires_grad=False)
    with options.override(options.FLAG_POSE_GRAD):
        color, radii, depth = GaussianRasterizer(_settings(case, *camera_tensors(Rm, T, proj)))(xyz, m2d, op, **kw)
    assert color.requires_grad
    (color * r["G"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert seen.arity == [14]
    assert len(seen.fwd_flags) == 1 and not (seen.fwd_flags[0] & options.FLAG_FORWARD_ONLY)
    assert T.grad is not None and torch.isfinite(T.grad).all() and float(T.grad.abs().min()) > 0
    # the same camera with trainable Gaussians: the same accumulator rows up to the order of K7's atomics
    T2 = T.detach().clone().requires_grad_(True)
    xyz2, m2d2, op2, kw2 = _gaussians(r)
    with options.override(options.FLAG_POSE_GRAD):
        color2 = GaussianRasterizer(_settings(case, *camera_tensors(Rm, T2, proj)))(xyz2, m2d2, op2, **kw2)[0]
    (color2 * r["G"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert float((T.grad - T2.grad).abs().max()) <= 1e-4 * float(T2.grad.abs().max())
    # the translation moves the view-space position of every Gaussian: dL/dT = sum_i dL/dt_i, and T = -c A with the
    # identity's c, so dL/dT A^T = sum_i dL/dmu_i
    PH.assert_identity(-(T2.grad.double().cpu() @ wv[:3, :3].T).numpy(), xyz2.grad.cpu().numpy(), "pose-only, through camera_tensors")


class _PC:
    """Duck-typed GaussianModel, frozen."""

    def __init__(self, sc):
        self._sc = {k: v.to(DEV).clone() for k, v in sc.items() if isinstance(v, torch.Tensor) and k != "bg"}
        self.active_sh_degree = self.max_sh_degree = 3

    get_xyz = property(lambda s: s._sc["xyz"])
    get_opacity = property(lambda s: s._sc["opacity"])
    get_scaling = property(lambda s: s._sc["scaling"])
    get_rotation = property(lambda s: s._sc["rotation"])
    get_features = property(lambda s: s._sc["features"])


def test_render_carries_the_gradient_to_a_pose_leaf():
    """render() with a camera object whose three tensors come from pose.camera_tensors: the mirror hands them to the
    rasterizer as they are, so the graph reaches the pose."""
    import gaussianeditor_amd
    from gaussianeditor_amd.gaussian_renderer import render
    from gaussianeditor_amd.pose import camera_tensors

    r = _plumbing_regime()
    case, cam = r["case"], r["case"]["cam"]
    wv = cam.world_view_transform.double()
    Rm = wv[:3, :3].float().to(DEV).clone().requires_grad_(True)
    T = wv[3, :3].float().to(DEV).clone().requires_grad_(True)
    proj = (torch.linalg.inv(wv) @ cam.full_proj_transform.double()).float().to(DEV)
    view, full, center = camera_tensors(Rm, T, proj)
    camera = SimpleNamespace(FoVx=cam.FoVx, FoVy=cam.FoVy, image_height=case["H"], image_width=case["W"],
                             world_view_transform=view, full_proj_transform=full, camera_center=center)
    pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    gaussianeditor_amd.set_pose_grad(True)
    try:
        out = render(camera, _PC(case["sc"]), pipe, case["bg"].to(DEV))
    finally:
        gaussianeditor_amd.set_pose_grad(False)
    (out["render"] * r["G"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    for t in (Rm, T):
        assert t.grad is not None and torch.isfinite(t.grad).all() and float(t.grad.abs().max()) > 0


def test_colour_override_of_a_pose_camera_is_not_served_by_reuse():
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer, _reuse

    r = _plumbing_regime()
    case = r["case"]
    xyz, m2d, op, kw = _gaussians(r, requires_grad=False)
    cols = torch.rand(xyz.shape[0], 3, device=DEV)
    sr = dict(scales=kw["scales"], rotations=kw["rotations"])

    def pair(V, PV, C):
        rast = GaussianRasterizer(_settings(case, V, PV, C))
        rast(xyz, m2d, op, **kw)
        hits = _reuse.stats["hits"]
        image = rast(xyz, m2d, op, colors_precomp=cols, **sr)[0]
        return image, _reuse.stats["hits"] - hits
    with options.override(options.FLAG_POSE_GRAD):
        frozen = [t.detach() for t in _cam_leaves(case["cam"])]
        image0, hits0 = pair(*frozen)
        assert hits0 == 1 and not image0.requires_grad  # (a camera without a gradient: served from the remembered state)
        V, PV, C = _cam_leaves(case["cam"])
        image, hits = pair(V, PV, C)
    assert hits == 0 and image.requires_grad
    assert torch.equal(image, image0)
    (image * r["G"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert V.grad is not None and float(V.grad.abs().max()) > 0 and not bool((C.grad != 0).any())  # (precomputed colours)


def test_persistent_rows_refuse_the_pose_gradient():
    case = PH.identity_case()
    a, out = _c_forward(case)
    P = a["xyz"].shape[0]
    state = torch.zeros(P, dtype=torch.uint8, device=DEV)
    alloc = lambda name, shape, zero: state if name == "row_state" else None  # noqa: E731
    G = torch.ones(3, case["H"], case["W"], device=DEV)
    with pytest.raises(RuntimeError, match="camera gradients are not supported with persistent gradient rows"):
        _c_backward(case, a, out, G, grad_allocator=alloc, pose_grad_out=torch.empty(35, device=DEV))
    for bad in (torch.empty(35, dtype=torch.float64, device=DEV), torch.empty(36, device=DEV), torch.empty(70, device=DEV)[::2],
                torch.empty(35)):
        with pytest.raises(RuntimeError, match="pose_grad_out"):
            _c_backward(case, a, out, G, pose_grad_out=bad)
