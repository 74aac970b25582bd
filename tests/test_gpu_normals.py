"""-m gpu: surface normals (gaussianeditor_amd/normals.py, csrc/gsr_normals.hip) against the float64
restatement of tests/normals_helpers.py with autograd.

The bar of every comparison is the project's rule for fused stages: max(2 x the error of the SAME torch operators run in
float32 against float64, 1e-6 of the tensor's largest entry), per case and per quantity (normals_helpers.bar_of); the
kernels compute in binary64 from the binary32 inputs and round once, so what is measured is the output rounding.
Measured on the MI355X (error / bar, the worst case of each group; every case prints its own figures):

    depth normals: error / bar
    | case | out | d_depth | d_alpha |
    |---|---|---|---|
    | 3x3/alpha | 2.7e-08 / 8.9e-07 | 1.0e-09 / 1.6e-07 | 3.6e-09 / 4.3e-07 |
    | 3x3/noalpha | 8.3e-09 / 9.1e-07 | 6.6e-09 / 1.8e-07 | - |
    | 5x7/alpha | 3.0e-08 / 9.9e-07 | 3.0e-09 / 8.7e-08 | 4.1e-09 / 2.5e-07 |
    | 5x7/holes | 2.7e-08 / 8.8e-07 | 6.0e-09 / 1.4e-07 | 6.2e-09 / 2.5e-07 |
    | 5x7/noalpha | 2.4e-08 / 8.2e-07 | 1.7e-09 / 4.5e-08 | - |
    | 33x17/alpha | 3.0e-08 / 2.2e-06 | 1.4e-09 / 6.2e-08 | 3.5e-09 / 1.4e-07 |
    | 33x17/holes | 3.0e-08 / 2.8e-06 | 1.1e-09 / 9.1e-08 | 2.0e-09 / 2.2e-07 |
    | 33x17/noalpha | 3.0e-08 / 1.0e-06 | 1.6e-09 / 3.2e-08 | - |
    | 64x64/alpha | 3.0e-08 / 5.1e-06 | 4.2e-10 / 3.8e-08 | 9.2e-10 / 1.1e-07 |
    | 64x64/holes | 3.0e-08 / 4.7e-06 | 4.0e-10 / 3.5e-08 | 8.5e-10 / 8.2e-08 |
    | 64x64/noalpha | 3.0e-08 / 2.7e-06 | 2.1e-10 / 6.8e-09 | - |
    | 70x45/alpha | 3.0e-08 / 3.9e-06 | 4.6e-10 / 8.5e-08 | 1.8e-09 / 1.9e-07 |
    | 70x45/holes | 3.0e-08 / 5.5e-06 | 3.4e-10 / 2.7e-08 | 8.5e-10 / 7.5e-08 |
    | 70x45/noalpha | 3.0e-08 / 2.6e-06 | 2.2e-10 / 1.0e-08 | - |
    | 97x131/alpha | 3.0e-08 / 7.9e-06 | 2.2e-10 / 8.9e-08 | 5.3e-10 / 2.1e-07 |
    | 97x131/holes | 3.0e-08 / 9.1e-06 | 2.3e-10 / 1.1e-07 | 8.3e-10 / 2.7e-07 |
    | 97x131/noalpha | 3.0e-08 / 6.6e-06 | 1.9e-10 / 1.1e-08 | - |
    all zero, error 0 / bar 0: 1x1/alpha, 1x1/holes, 1x1/noalpha, 1x5/alpha, 1x5/holes, 1x5/noalpha, 5x1/alpha, 5x1/holes, 5x1/noalpha, 2x2/alpha, 2x2/holes, 2x2/noalpha, 3x3/holes

    loss: error / bar
    | case | loss | d_normals | d_depth | d_alpha |
    |---|---|---|---|---|
    | 3x3/alpha | 8.8e-10 / 6.5e-08 | 3.6e-09 / 1.7e-07 | 2.5e-09 / 9.2e-08 | 6.1e-09 / 2.5e-07 |
    | 5x7/alpha | 1.7e-09 / 8.4e-08 | 1.8e-09 / 4.9e-08 | 2.0e-09 / 1.0e-07 | 8.1e-09 / 2.7e-07 |
    | 5x7/holes | 2.2e-10 / 1.1e-08 | 1.9e-09 / 4.4e-08 | 6.8e-10 / 2.2e-08 | 1.5e-09 / 4.1e-08 |
    | 33x17/alpha | 3.5e-10 / 1.5e-07 | 1.2e-10 / 6.9e-09 | 4.3e-10 / 7.1e-08 | 1.6e-09 / 1.6e-07 |
    | 33x17/holes | 1.9e-09 / 8.6e-08 | 1.2e-10 / 8.7e-09 | 6.4e-10 / 6.1e-08 | 1.8e-09 / 1.5e-07 |
    | 64x64/alpha | 6.9e-10 / 1.6e-07 | 1.5e-11 / 2.2e-09 | 1.2e-10 / 2.2e-08 | 2.7e-10 / 6.6e-08 |
    | 64x64/holes | 2.5e-10 / 8.5e-08 | 1.5e-11 / 2.0e-09 | 1.9e-10 / 2.5e-08 | 3.9e-10 / 7.6e-08 |
    | 70x45/alpha | 5.0e-09 / 1.6e-07 | 2.9e-11 / 2.1e-09 | 2.0e-10 / 3.7e-08 | 4.5e-10 / 8.6e-08 |
    | 70x45/holes | 1.3e-09 / 9.1e-08 | 2.9e-11 / 3.0e-09 | 1.1e-10 / 4.4e-08 | 3.6e-10 / 9.7e-08 |
    | 97x131/alpha | 1.1e-10 / 1.7e-07 | 7.3e-12 / 1.1e-09 | 1.2e-10 / 3.6e-08 | 2.2e-10 / 8.5e-08 |
    | 97x131/holes | 2.6e-09 / 8.8e-08 | 7.3e-12 / 1.3e-09 | 6.2e-11 / 3.4e-08 | 2.2e-10 / 8.4e-08 |
    all zero, error 0 / bar 0: 1x1/alpha, 1x1/holes, 1x5/alpha, 1x5/holes, 5x1/alpha, 5x1/holes, 2x2/alpha, 2x2/holes, 3x3/holes

    gaussian normals: error / bar
    | case | out | d_rotations |
    |---|---|---|
    | P=1 general | 1.7e-08 / 7.5e-07 | 9.7e-08 / 4.9e-06 |
    | P=1 ring0 | 1.4e-08 / 7.8e-07 | 4.3e-08 / 5.4e-06 |
    | P=1 ring2 | 2.0e-08 / 7.8e-07 | 9.5e-08 / 2.2e-06 |
    | P=63 general | 3.0e-08 / 9.9e-07 | 3.9e-07 / 1.6e-05 |
    | P=63 ring0 | 3.0e-08 / 1.0e-06 | 8.3e-07 / 2.0e-05 |
    | P=63 ring2 | 2.9e-08 / 1.0e-06 | 7.9e-07 / 1.8e-05 |
    | P=64 general | 3.0e-08 / 1.0e-06 | 8.8e-07 / 2.5e-05 |
    | P=64 ring0 | 3.0e-08 / 9.9e-07 | 7.8e-07 / 2.0e-05 |
    | P=64 ring2 | 2.9e-08 / 9.9e-07 | 7.1e-07 / 2.7e-05 |
    | P=65 general | 2.9e-08 / 1.0e-06 | 8.3e-07 / 2.9e-05 |
    | P=65 ring0 | 2.9e-08 / 9.9e-07 | 8.4e-07 / 2.6e-05 |
    | P=65 ring2 | 2.9e-08 / 9.9e-07 | 8.8e-07 / 3.0e-05 |
    | P=1000 general | 3.0e-08 / 1.0e-06 | 1.0e-06 / 4.3e-05 |
    | P=1000 ring0 | 3.0e-08 / 1.0e-06 | 1.6e-06 / 4.7e-05 |
    | P=1000 ring2 | 3.0e-08 / 1.0e-06 | 1.2e-06 / 3.6e-05 |
    | P=100003 general | 3.0e-08 / 1.1e-06 | 1.9e-06 / 5.8e-05 |
    | P=100003 ring0 | 3.0e-08 / 1.2e-06 | 1.9e-06 / 6.4e-05 |
    | P=100003 ring2 | 3.0e-08 / 1.1e-06 | 1.9e-06 / 6.5e-05 |

    end to end (64 x 64, 2 000 Gaussians, 1 093 valid pixels, alpha_min 0.4357): dL/dmeans3D 6.2e-08, dL/dscales 7.4e-08,
    dL/drotations 4.9e-08, dL/dopacity 6.4e-08 of each tensor's largest entry (bar 1e-05); half of dL/drotations' largest
    entry comes through the normal image.

Also here: exact zeros at invalid pixels, discrimination (the alpha share and the depth share of the gradient each exceed
ten bars on at least min(100, n / 4) of the n values of the tensor), the same bits on two runs and on a side stream, the
NULL-gradient routes, guard bands around every buffer the module allocates, and render -> loss -> backward end to end
against a composition of the feature, depth and alpha backwards (each held to the oracle by its own tests) with the float64
restatement of the new stage.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import features_helpers as FH
import normals_helpers as NH
from guarded_alloc import GuardedAllocator
from helpers import oracle_forward

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMAGE_CASES = [(n, m) for n in NH.IMAGES for m in NH.MODES]
LOSS_CASES = [(n, m) for n in NH.IMAGES for m in ("alpha", "holes")]


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _f64(t):
    return t.detach().cpu().double().numpy()


def _dev(a, grad=False):
    return None if a is None else torch.tensor(np.array(a)).to(DEV).requires_grad_(grad)


def _kw(case, alpha_min=None):
    fx, fy, cx, cy = case["intrinsics"]
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, alpha_min=case["alpha_min"] if alpha_min is None else alpha_min)


def _depth_normals(case):
    """(out, d_depth, d_alpha | None) tensors of the product for a seeded image case"""
    from gaussianeditor_amd import normals as N

    d, a = _dev(case["depth"], True), _dev(case["alpha"], True)
    out = N.depth_to_normals(d, a, **_kw(case))
    out.backward(_dev(case["dout"]))
    torch.cuda.synchronize()
    return out.detach(), d.grad, None if a is None else a.grad


def _loss(case):
    """(loss, d_normals, d_depth, d_alpha) tensors of the product for a seeded image case"""
    from gaussianeditor_amd import normals as N

    n, d, a = _dev(case["normals"], True), _dev(case["depth"], True), _dev(case["alpha"], True)
    loss = N.normal_consistency_loss(n, d, a, **_kw(case))
    (loss * case["dloss"]).backward()
    torch.cuda.synchronize()
    return loss.detach(), n.grad, d.grad, a.grad


def _rows(case):
    from gaussianeditor_amd import normals as N

    q = _dev(case["rotations"], True)
    out = N.gaussian_normals(q, _dev(case["scales"]), _dev(case["xyz"]), _dev(case["V"]))
    if case["P"]:
        out.backward(_dev(case["dout"]))
    torch.cuda.synchronize()
    return out.detach(), q.grad if q.grad is not None else torch.zeros_like(q)


def _compare(tag, key, got, want, bar):
    err = float(np.abs(_f64(got).reshape(want.shape) - want).max(initial=0.0))
    print(f"  {tag}: {key} error {err:.3e} bar {bar:.3e} (largest entry {float(np.abs(want).max(initial=0.0)):.3e})")
    assert err <= bar, (tag, key, err, bar)
    return err


def _no_valid_neighbour(valid):
    """(H,W) bool: depth pixels none of whose four neighbours is a valid normal -- their gradient is exactly zero"""
    v = np.pad(valid, 1)
    return ~(v[:-2, 1:-1] | v[2:, 1:-1] | v[1:-1, :-2] | v[1:-1, 2:])


def _assert_share(tag, key, want, bar, non_degenerate):
    """the discrimination condition: more than ten bars on at least min(100, n / 4) of the tensor's n values"""
    if not non_degenerate:
        return
    n = want.size
    big = int((np.abs(want) > 10.0 * bar).sum())
    print(f"  {tag}: {key} exceeds ten bars on {big} of {n} values (needed {min(100, n / 4):.1f})")
    assert big >= min(100, n / 4), (tag, key, big, n)


@pytest.mark.parametrize("name,mode", IMAGE_CASES)
def test_depth_normals_and_their_gradients(name, mode):
    case = NH.image_case(name, mode)
    e, bars = NH.image_expectation(name, mode)
    out, d_depth, d_alpha = _depth_normals(case)
    tag = f"depth normals {name}/{mode}"
    _compare(tag, "out", out, e["n_out"], bars["n_out"])
    _compare(tag, "d_depth", d_depth, e["n_d_depth"], bars["n_d_depth"])
    if d_alpha is not None:
        _compare(tag, "d_alpha", d_alpha, e["n_d_alpha"], bars["n_d_alpha"])
    valid = e["n_valid"]
    assert tuple(out.shape) == (3, case["H"], case["W"])
    assert not bool(out.cpu()[:, torch.tensor(~valid)].any()), "an invalid pixel is not exactly zero"
    dead = torch.tensor(_no_valid_neighbour(valid))
    assert not bool(d_depth.cpu()[0][dead].any()) and (d_alpha is None or not bool(d_alpha.cpu()[0][dead].any()))
    if name in NH.DEGENERATE:
        assert not valid.any() and not bool(out.any()) and not bool(d_depth.any())
    live = bool(valid.any())
    _assert_share(tag, "d_depth", e["n_d_depth"], bars["n_d_depth"], live)
    if d_alpha is not None:
        _assert_share(tag, "d_alpha", e["n_d_alpha"], bars["n_d_alpha"], live)


@pytest.mark.parametrize("name,mode", LOSS_CASES)
def test_loss_and_its_three_gradients(name, mode):
    case = NH.image_case(name, mode)
    e, bars = NH.image_expectation(name, mode)
    loss, d_normals, d_depth, d_alpha = _loss(case)
    tag = f"loss {name}/{mode}"
    _compare(tag, "loss", loss, e["l_loss"], bars["l_loss"])
    _compare(tag, "d_normals", d_normals, e["l_d_normals"], bars["l_d_normals"])
    _compare(tag, "d_depth", d_depth, e["l_d_depth"], bars["l_d_depth"])
    _compare(tag, "d_alpha", d_alpha, e["l_d_alpha"], bars["l_d_alpha"])
    valid = e["n_valid"]
    assert not bool(d_normals.cpu()[:, torch.tensor(~valid)].any()), "dL/dN at an invalid pixel is not exactly zero"
    dead = torch.tensor(_no_valid_neighbour(valid))
    assert not bool(d_depth.cpu()[0][dead].any()) and not bool(d_alpha.cpu()[0][dead].any())
    if name in NH.DEGENERATE:
        assert float(loss) == 0.0 and not bool(d_normals.any()) and not bool(d_depth.any()) and not bool(d_alpha.any())
    else:
        assert float(loss) >= 0.0
    live = bool(valid.any())
    _assert_share(tag, "d_depth", e["l_d_depth"], bars["l_d_depth"], live)
    _assert_share(tag, "d_alpha", e["l_d_alpha"], bars["l_d_alpha"], live)


@pytest.mark.parametrize("view", ["general", "ring0", "ring2"])
@pytest.mark.parametrize("P", NH.ROWS)
def test_gaussian_normals_and_the_rotation_gradient(P, view):
    case = NH.rows_case(P, view)
    e, bars = NH.rows_expectation(P, view)
    out, d_rot = _rows(case)
    tag = f"gaussian normals P={P} {view}"
    assert tuple(out.shape) == (P, 3) and tuple(d_rot.shape) == (P, 4)
    if P == 0:
        return
    _compare(tag, "out", out, e["out"], bars["out"])
    _compare(tag, "d_rotations", d_rot, e["d_rotations"], bars["d_rotations"])
    g, q = _f64(d_rot), case["rotations"].astype(np.float64)
    assert (np.abs(g).max(axis=1) > 0).sum() >= P / 2
    # the true gradient is orthogonal to q, so |g . q| = |(g - g_true) . q| <= bar |q|_1
    assert (np.abs((g * q).sum(1)) <= bars["d_rotations"] * np.abs(q).sum(1)).all()
    # every normal is a unit vector that faces the camera
    p_c = case["xyz"].astype(np.float64) @ case["V"].astype(np.float64)[:3, :3] + case["V"].astype(np.float64)[3, :3]
    o = _f64(out)
    assert np.abs(np.linalg.norm(o, axis=1) - 1.0).max() <= 1e-6 and ((o * p_c).sum(1) < 0).all()


def test_the_same_bits_on_two_runs_and_on_a_side_stream():
    img, rows = NH.image_case("97x131", "holes"), NH.rows_case(100_003)
    run = lambda: _depth_normals(img) + _loss(img) + _rows(rows)  # noqa: E731
    want = run()
    again = run()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        side = run()
    s.synchronize()
    for a, b, c in zip(want, again, side):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))


def test_only_what_autograd_needs_is_computed():
    """Through autograd: an input that requires no gradient gets none.  Through the C ABI: a NULL gradient pointer skips that
    output -- a poisoned buffer that was not passed stays poisoned -- and the outputs that were asked for are the bits of
    the full call."""
    from gaussianeditor_amd import _native
    from gaussianeditor_amd import normals as N

    case = NH.image_case("70x45", "holes")
    H, W = case["H"], case["W"]
    full = _loss(case)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        n, d, a = (_dev(case[k], g) for k, g in zip(("normals", "depth", "alpha"), need))
        (N.normal_consistency_loss(n, d, a, **_kw(case)) * case["dloss"]).backward()
        for t, g, f in zip((n, d, a), need, full[1:]):
            assert (t.grad is not None) == g and (not g or np.array_equal(_bits(t.grad), _bits(f)))
    full_dn = _depth_normals(case)
    d, a = _dev(case["depth"], True), _dev(case["alpha"])
    N.depth_to_normals(d, a, **_kw(case)).backward(_dev(case["dout"]))
    assert a.grad is None and np.array_equal(_bits(d.grad), _bits(full_dn[1]))
    with torch.no_grad():
        out = N.depth_to_normals(d, a, **_kw(case))
    assert not out.requires_grad and np.array_equal(_bits(out), _bits(full_dn[0]))

    L = _native.lib()
    s = torch.cuda.current_stream(DEV).cuda_stream
    k = _kw(case)
    view = (H, W, k["fx"], k["fy"], k["cx"], k["cy"], k["alpha_min"])
    n, d, a, dout = (_dev(case[x]) for x in ("normals", "depth", "alpha", "dout"))
    dl = torch.full((1,), case["dloss"], device=DEV)
    poison = lambda c: torch.full((c, H, W), float("nan"), device=DEV)  # noqa: E731
    for mask in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)):
        bufs = [poison(3), poison(1), poison(1)]
        ptrs = [b.data_ptr() if m else None for b, m in zip(bufs, mask)]
        assert L.gsr_normal_loss_backward(s, *view, n.data_ptr(), d.data_ptr(), a.data_ptr(), dl.data_ptr(), *ptrs) == 0
        torch.cuda.synchronize()
        for b, m, f in zip(bufs, mask, full[1:]):
            assert np.array_equal(_bits(b), _bits(f)) if m else bool(torch.isnan(b).all())
    for mask in ((1, 0), (0, 1)):
        bufs = [poison(1), poison(1)]
        ptrs = [b.data_ptr() if m else None for b, m in zip(bufs, mask)]
        assert L.gsr_depth_normals_backward(s, *view, d.data_ptr(), a.data_ptr(), dout.data_ptr(), *ptrs) == 0
        torch.cuda.synchronize()
        for b, m, f in zip(bufs, mask, full_dn[1:]):
            assert np.array_equal(_bits(b), _bits(f)) if m else bool(torch.isnan(b).all())


@pytest.mark.parametrize("name,mode", [("97x131", "holes"), ("33x17", "noalpha"), ("5x7", "alpha"), ("2x2", "alpha")])
def test_outputs_and_the_workspace_keep_their_guard_bands(name, mode):
    """Every buffer the module allocates -- outputs, gradients, the loss's workspace -- between bands of 0xFF (NaN as
    float32): the bands stay, and no output element keeps its poison."""
    img = NH.image_case(name, mode)
    rows = NH.rows_case(1000 if name == "97x131" else 65)
    with GuardedAllocator(0xFF, device=torch.device(DEV, torch.cuda.current_device())) as ga:
        res = list(_depth_normals(img)) + list(_rows(rows))
        if img["alpha"] is not None:
            res += list(_loss(img))
        ga.assert_clean()
        # (out, d_depth [, d_alpha]; out, d_rotations; the loss's workspace, value and three gradients)
        assert len(ga) >= (4 if img["alpha"] is None else 10)
    for t in res:
        assert t is None or not bool(torch.isnan(t).any()), "an output element was not written"


class _Model:
    def __init__(self, sc):
        d = lambda t: t.to(DEV).clone().contiguous().requires_grad_(True)  # noqa: E731
        self._xyz, self._features = d(sc["xyz"]), d(sc["features"])
        self._opacity, self._scaling, self._rotation = d(sc["opacity"]), d(sc["scaling"]), d(sc["rotation"])
        self.active_sh_degree = self.max_sh_degree = 3

    get_xyz = property(lambda s: s._xyz)
    get_features = property(lambda s: s._features)
    get_opacity = property(lambda s: s._opacity)
    get_scaling = property(lambda s: s._scaling)
    get_rotation = property(lambda s: s._rotation)


def _camera(case):
    c = case["cam"]
    return types.SimpleNamespace(FoVx=c.FoVx, FoVy=c.FoVy, image_height=case["H"], image_width=case["W"],
                                 world_view_transform=c.world_view_transform.to(DEV),
                                 full_proj_transform=c.full_proj_transform.to(DEV), camera_center=c.camera_center.to(DEV))


PIPE = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)


def test_render_then_loss_then_backward_end_to_end(oracle):
    """render(return_alpha=True, return_normals=True) under set_depth_grad(True) -> normal_consistency_loss -> backward().
    Expected: the float64 restatement of the loss on the product's three images gives dL/dN, dL/dD, dL/dA; the existing
    feature, depth and alpha backwards (features_helpers.run_hip, each held to the oracle by its own tests) carry them to the
    Gaussians; the float64 restatement of the Gaussian normals carries dL/dfeatures on to the rotations.  1e-5 of each
    tensor's largest entry, the rasterizer's own bar.  alpha_min: the midpoint of the largest gap of the oracle's alpha
    values inside [0.2, 0.8]."""
    import gaussianeditor_amd
    from gaussianeditor_amd import normals as N
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer
    from gaussianeditor_amd.gaussian_renderer import render

    case, _, _, _ = FH.feature_case("p2000")
    H, W, sc = case["H"], case["W"], case["sc"]
    assert (H, W, sc["xyz"].shape[0]) == (64, 64, 2000)
    alpha_min = NH.gap_alpha_min(1.0 - oracle_forward(oracle, case)["final_T"].astype(np.float64))
    cam, bg = _camera(case), case["bg"].to(DEV)
    intr = N.camera_intrinsics(cam)

    before = render(cam, _Model(sc), PIPE, bg)
    m = _Model(sc)
    gaussianeditor_amd.set_depth_grad(True)
    try:
        pkg = render(cam, m, PIPE, bg, return_alpha=True, return_normals=True)
        assert set(pkg) == set(before) | {"alpha", "normals"} and tuple(pkg["normals"].shape) == (3, H, W)
        loss = N.normal_consistency_loss(pkg["normals"], pkg["depth_3dgs"], pkg["alpha"], cam, alpha_min=alpha_min)
        loss.backward()
    finally:
        gaussianeditor_amd.set_depth_grad(False)
    torch.cuda.synchronize()
    got = dict(dL_dmeans3D=m._xyz.grad, dL_dscales=m._scaling.grad, dL_drotations=m._rotation.grad, dL_dopacity=m._opacity.grad)
    got = {k: v.cpu().numpy() for k, v in got.items()}

    # the new stage in float64, on the product's images
    n, d, a = (pkg[k].detach().cpu().double().requires_grad_(True) for k in ("normals", "depth_3dgs", "alpha"))
    assert float((a.detach() - alpha_min).abs().min()) >= NH.ALPHA_GAP, "the largest alpha gap is narrower than the input condition"
    want_loss = NH.normal_loss_ref(n, d, a, intr, alpha_min)
    GN, GD, GA = torch.autograd.grad(want_loss, (n, d, a))
    _, valid = NH.depth_to_normals_ref(d.detach(), a.detach(), intr, alpha_min)
    print(f"  end to end: loss {float(loss.detach()):.6e} (float64 {float(want_loss.detach()):.6e}), {int(valid.sum())} valid pixels, alpha_min {alpha_min:.4f}")
    assert int(valid.sum()) > 500 and abs(float(loss.detach()) - float(want_loss.detach())) <= 1e-6 * abs(float(want_loss.detach()))
    # the Gaussian normals of the view, and the existing backwards
    V = cam.world_view_transform.contiguous()
    nrm = N.gaussian_normals(m._rotation.detach(), m._scaling.detach(), m._xyz.detach(), V)
    want, outs = FH.run_hip(case, GF=GN.float(), feats=nrm.cpu(), GA=GA.float(), GD=GD.float())
    assert np.array_equal(outs["features"], pkg["normals"].detach().cpu().numpy()), "out['normals'] is not the feature image of the normals"
    q = sc["rotation"].double().requires_grad_(True)
    ref_n = NH.gaussian_normals_ref(q, sc["scaling"].double(), sc["xyz"].double(), cam.world_view_transform.cpu().double())
    via_normals, = torch.autograd.grad(ref_n, q, torch.tensor(want["dL_dfeatures"]).double())
    want = {k: want[k].astype(np.float64) for k in got}
    want["dL_drotations"] = want["dL_drotations"] + via_normals.numpy()
    share = float(np.abs(via_normals.numpy()).max() / np.abs(want["dL_drotations"]).max())
    print(f"  end to end: the share of dL/drotations that comes through the normals: {share:.2f} of its largest entry")
    assert share > 0.1
    FH.assert_feature_grads_close(got, want, tol=1e-5, tag="render -> normal loss")

    # user features alongside: C = 1 and C = 253 ride in front of the three normal channels; 254 is refused
    r = GaussianRasterizer(FH.settings(case, DEV))
    leaves = lambda: (m._xyz.detach(), torch.zeros_like(m._xyz), m._opacity.detach())  # noqa: E731
    kw = dict(shs=m._features.detach(), scales=m._scaling.detach(), rotations=m._rotation.detach())
    only = r(*leaves(), features=nrm, **kw)[-1]
    assert np.array_equal(_bits(only), _bits(pkg["normals"]))
    for C in (1, 253):
        feats = FH.make_features(2000, C).to(DEV)
        outs = r(*leaves(), features=feats, return_alpha=True, return_normals=True, **kw)
        assert len(outs) == 6 and tuple(outs[4].shape) == (C, H, W) and tuple(outs[5].shape) == (3, H, W)
        assert np.array_equal(_bits(outs[5]), _bits(pkg["normals"])) and np.array_equal(_bits(outs[3]), _bits(pkg["alpha"]))
        assert np.array_equal(_bits(outs[4]), _bits(r(*leaves(), features=feats, **kw)[-1]))
    with pytest.raises(RuntimeError, match="at most 253 with it, got 254"):
        r(*leaves(), features=torch.zeros(2000, 254, device=DEV), return_normals=True, **kw)
    after = render(cam, _Model(sc), PIPE, bg)
    for k in ("render", "depth_3dgs", "radii"):
        assert np.array_equal(_bits(after[k]), _bits(before[k])), k
