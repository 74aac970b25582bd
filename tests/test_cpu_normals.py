"""CPU: surface normals without a device -- the float64 restatement of tests/normals_helpers.py
against closed forms, the input conditions of the seeded cases (0 offenders), header and symbols, every refusal of the seven
entry points, the Python layer's refusals by name, and render() without the keyword."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import normals_helpers as NH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
ONE = ctypes.c_void_p(256)  # never dereferenced
NAMES = ("gsr_gaussian_normals_forward", "gsr_gaussian_normals_backward", "gsr_depth_normals_forward",
         "gsr_depth_normals_backward", "gsr_normal_loss_workspace_size", "gsr_normal_loss_forward", "gsr_normal_loss_backward")


# ---- the restatement against closed forms -------------------------------------------------------------------------------
def _plane_depth(n, d, H, W, intr):
    """z(x,y) of the plane n . p = d along the ray of every pixel: z = d / (n . r)"""
    fx, fy, cx, cy = intr
    rx = (torch.arange(W, dtype=F64) - cx) / fx
    ry = (torch.arange(H, dtype=F64) - cy) / fy
    return (d / (n[0] * rx[None, :] + n[1] * ry[:, None] + n[2]))[None]


@pytest.mark.parametrize("n", [(0.0, 0.0, -1.0), (0.3, -0.2, -0.9), (-0.5, 0.4, -0.7)])
def test_a_plane_under_perspective_gives_its_normal_exactly(n):
    """Central differences of the back-projected points are exact on a plane: every interior pixel gives n (camera facing,
    n . p < 0) to rounding (measured 2e-15; the bar is 1e-12), the border exactly zero."""
    H, W = 9, 11
    intr = NH.intrinsics_for(H, W)
    n = torch.tensor(n, dtype=F64)
    n = n / n.norm()
    depth = _plane_depth(n, -3.0, H, W, intr)  # n . p = -3: in front of the camera, n towards it
    assert float(depth.min()) > 0.5
    out, valid = NH.depth_to_normals_ref(depth, None, intr)
    assert bool(valid[1:-1, 1:-1].all()) and not bool(valid[0].any() | valid[-1].any() | valid[:, 0].any() | valid[:, -1].any())
    err = float((out[:, 1:-1, 1:-1] - n[:, None, None]).abs().max())
    print(f"plane {n.tolist()}: {err:.2e}")
    assert err <= 1e-12
    border = out.clone()
    border[:, 1:-1, 1:-1] = 0
    assert not bool(border.any()) and torch.equal(out[:, 0], torch.zeros(3, W, dtype=F64))
    if n[0] == 0 and n[1] == 0:  # fronto-parallel: (0, 0, -1)
        assert float((out[:, 1:-1, 1:-1] - torch.tensor([0.0, 0.0, -1.0], dtype=F64)[:, None, None]).abs().max()) <= 1e-12
    # with an alpha image the unnormalised depth z A gives the same normals
    A = torch.rand(1, H, W, dtype=F64, generator=torch.Generator().manual_seed(1)) * 0.4 + 0.6
    out2, _ = NH.depth_to_normals_ref(depth * A, A, intr)
    assert float((out2 - out).abs().max()) <= 1e-12


def test_gaussian_normal_of_an_axis_aligned_disk_and_the_flip_rule():
    """Identity rotation, smallest scale along z: n_w = (0,0,1); in the identity camera in front of it (p_c.z > 0) the normal
    n_c . p_c > 0 flips to (0,0,-1); behind the camera plane it stays (0,0,1).  A raw quaternion of norm 7 gives the same."""
    V = torch.eye(4, dtype=F64)
    q = torch.tensor([[1.0, 0, 0, 0], [7.0, 0, 0, 0]], dtype=F64)
    s = torch.tensor([[0.3, 0.2, 0.01]] * 2, dtype=F64)
    front, behind = torch.tensor([[0.1, 0.2, 4.0]] * 2, dtype=F64), torch.tensor([[0.1, 0.2, -4.0]] * 2, dtype=F64)
    assert torch.equal(NH.gaussian_normals_ref(q, s, front, V), torch.tensor([[0.0, 0, -1]] * 2, dtype=F64))
    assert torch.equal(NH.gaussian_normals_ref(q, s, behind, V), torch.tensor([[0.0, 0, 1]] * 2, dtype=F64))
    # the disk seen edge on but slightly from the side the normal points to keeps its sign
    assert torch.equal(NH.gaussian_normals_ref(q[:1], s[:1], torch.tensor([[3.0, 0.0, -0.01]], dtype=F64), V),
                       torch.tensor([[0.0, 0, 1]], dtype=F64))
    # shortest axis x or y: the first and second column
    assert torch.equal(NH.gaussian_normals_ref(q[:1], torch.tensor([[0.01, 0.2, 0.3]], dtype=F64), torch.tensor([[-2.0, 0, 1]], dtype=F64), V),
                       torch.tensor([[1.0, 0, 0]], dtype=F64))
    # a camera that looks along world +x (its z axis): the world normal (0,0,1) becomes camera (.,.,.) = n_w V[:3,:3]
    Vx = torch.zeros(4, 4, dtype=F64)
    Vx[0, 2], Vx[1, 0], Vx[2, 1], Vx[3, 3] = 1.0, 1.0, 1.0, 1.0  # p_c = (p_w.y, p_w.z, p_w.x)
    out = NH.gaussian_normals_ref(q[:1], s[:1], torch.tensor([[5.0, 0.0, 1.0]], dtype=F64), Vx)
    assert torch.equal(out, torch.tensor([[0.0, -1.0, 0.0]], dtype=F64))  # n_c = (0,1,0), p_c = (0,1,5): flipped


def test_the_tie_rule_takes_the_lowest_index():
    s = torch.tensor([[0.1, 0.1, 0.2], [0.2, 0.1, 0.1], [0.1, 0.2, 0.1], [0.1, 0.1, 0.1], [0.3, 0.2, 0.1]], dtype=F64)
    assert NH.shortest_axis(s).tolist() == [0, 1, 0, 0, 2]


def test_the_gradient_is_orthogonal_to_the_raw_quaternion():
    c = NH.rows_case(1000)
    e, _ = NH.rows_expectation(1000)
    dots = np.abs((e["d_rotations"] * c["rotations"].astype(np.float64)).sum(1))
    assert dots.max() <= 1e-12 * max(1.0, np.abs(e["d_rotations"]).max()) and (np.abs(e["d_rotations"]).max(1) > 0).mean() > 0.99


def test_every_loss_term_is_nonnegative_when_the_normal_image_is_bounded_by_alpha():
    for mode in ("alpha", "holes"):
        c = NH.image_case("33x17", mode)
        n, d, a = (torch.tensor(c[k], dtype=F64) for k in ("normals", "depth", "alpha"))
        assert float((n.norm(dim=0) - a[0]).max()) <= 0.0
        n_d, valid = NH.depth_to_normals_ref(d, a, c["intrinsics"])
        term = a[0] - (n * n_d).sum(0)
        assert float(term[valid].min()) >= 0.0 and int(valid.sum()) > 50
        # ... and equals 2DGS's A (1 - <N / A, n_d>)
        assert float((term - a[0] * (1 - ((n / a) * n_d).sum(0)))[valid].abs().max()) <= 1e-12
        assert float(NH.normal_loss_ref(n, d, a, c["intrinsics"])) == pytest.approx(float(term[valid].sum()) / (33 * 17), rel=1e-12)


def test_the_footprint_of_one_depth_pixel_is_its_four_neighbours():
    """d normals / d depth[y, x] is non-zero at (y-1,x), (y+1,x), (y,x-1), (y,x+1) and nowhere else -- not at (y,x) itself."""
    c = NH.image_case("5x7", "alpha")
    d, a = torch.tensor(c["depth"], dtype=F64), torch.tensor(c["alpha"], dtype=F64)
    y, x = 2, 3
    J = torch.autograd.functional.jacobian(lambda t: NH.depth_to_normals_ref(t, a, c["intrinsics"])[0], d)  # (3,H,W,1,H,W)
    touched = (J[:, :, :, 0, y, x].abs().sum(0) > 0)
    want = torch.zeros(5, 7, dtype=torch.bool)
    want[y - 1, x] = want[y + 1, x] = want[y, x - 1] = want[y, x + 1] = True
    assert torch.equal(touched, want)


def test_the_seeded_cases_meet_the_input_conditions_themselves():
    """The excluded share is 0: no pixel within 1e-3 of alpha_min, no |c| below 1e-6 of its median, every valid tap deeper
    than 0.05; no row whose two smallest scales lie within 1e-3 relative, none within 1e-3 of perpendicular."""
    for name in NH.IMAGES:
        for mode in NH.MODES:
            c = NH.image_case(name, mode)
            assert NH.image_violations(c) == dict(alpha=0, length=0, z=0), (name, mode)
            e, _ = NH.image_expectation(name, mode)
            if name in NH.DEGENERATE:
                assert not e["n_valid"].any() and not np.any(e["n_out"]) and not np.any(e["n_d_depth"])
            elif mode != "alpha" and name not in ("3x3", "5x7"):  # valid and invalid pixels interleave
                inner = e["n_valid"][1:-1, 1:-1]
                assert 0.2 < inner.mean() < 0.9, (name, mode, inner.mean())
    for view in NH.views():
        for P in NH.ROWS:
            c = NH.rows_case(P, view)
            close, side = NH.rows_violations(c["rotations"], c["scales"], c["xyz"], c["V"]) if P else (np.zeros(0, bool),) * 2
            assert not close.any() and not side.any(), (P, view)
            if P:
                norms = np.linalg.norm(c["rotations"].astype(np.float64), axis=1)
                assert 0.099 < norms.min() and norms.max() < 10.01 and (P < 100 or (norms.min() < 0.2 and norms.max() > 5.0))


def test_gap_alpha_min_is_the_midpoint_of_the_largest_gap():
    assert NH.gap_alpha_min([0.0, 0.1, 0.25, 0.3, 0.7, 0.9]) == pytest.approx(0.5)
    assert NH.gap_alpha_min([0.0, 1.0]) == pytest.approx(0.5) and NH.gap_alpha_min([0.21, 0.22, 0.5]) == pytest.approx(0.65)


# ---- header, symbols, refusals ------------------------------------------------------------------------------------------
def test_header_and_symbols():
    from gaussianeditor_amd import _native

    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "#define GSR_ABI_VERSION 6" in hdr
    L = _native.lib()
    assert L.gsr_abi_version() == 6
    for name in NAMES:
        assert f"int {name}(" in hdr and name in _native.SIGNATURES and hasattr(L, name)
    assert "lowest index" in hdr and "1e-30" in hdr and "not the number of valid pixels" in hdr


def test_every_refusal_comes_back_before_the_device_is_touched():
    """GSR_ERR_BAD_ARGUMENT (-1) on a machine without a GPU; the empty calls return GSR_OK without a launch."""
    from gaussianeditor_amd import _native

    L = _native.lib()
    odd = ctypes.c_void_p(258)
    # (a) rows: P = 0 is valid whatever the pointers; P < 0, P > 2^31 - 1, a NULL or misaligned pointer are refused
    fwd, bwd = L.gsr_gaussian_normals_forward, L.gsr_gaussian_normals_backward
    assert fwd(None, 0, None, None, None, None, None) == 0 and bwd(None, 0, None, None, None, None, None, None) == 0
    assert fwd(None, -1, ONE, ONE, ONE, ONE, ONE) == -1 and fwd(None, 1 << 31, ONE, ONE, ONE, ONE, ONE) == -1
    assert bwd(None, -1, ONE, ONE, ONE, ONE, ONE, ONE) == -1 and bwd(None, 1 << 31, ONE, ONE, ONE, ONE, ONE, ONE) == -1
    for i in range(5):
        for bad in (None, odd):
            a = [ONE] * 5
            a[i] = bad
            assert fwd(None, 10, *a) == -1, (i, bad)
    for i in range(6):
        for bad in (None, odd):
            a = [ONE] * 6
            a[i] = bad
            assert bwd(None, 10, *a) == -1, (i, bad)
    # (b), (c) images
    K = (50.0, 60.0, 31.5, 23.5, 0.5)
    bad_views = [dict(H=0), dict(W=0), dict(H=-3), dict(W=-1), dict(H=1 << 16, W=1 << 16), dict(H=524_281, W=1),
                 dict(fx=0.0), dict(fy=-1.0), dict(fx=math.nan), dict(fy=math.inf), dict(cx=math.nan), dict(cy=math.inf),
                 dict(alpha_min=math.nan)]

    def view(H=48, W=64, fx=K[0], fy=K[1], cx=K[2], cy=K[3], alpha_min=K[4]):
        return (H, W, fx, fy, cx, cy, alpha_min)

    def dn_f(depth=ONE, alpha=ONE, out=ONE, **v):
        return L.gsr_depth_normals_forward(None, *view(**v), depth, alpha, out)

    def dn_b(depth=ONE, alpha=ONE, dout=ONE, dd=None, da=None, **v):
        return L.gsr_depth_normals_backward(None, *view(**v), depth, alpha, dout, dd, da)

    def nl_f(normals=ONE, depth=ONE, alpha=ONE, work=ONE, out=ONE, **v):
        return L.gsr_normal_loss_forward(None, *view(**v), normals, depth, alpha, work, out)

    def nl_b(normals=ONE, depth=ONE, alpha=ONE, dl=ONE, dn=None, dd=None, da=None, **v):
        return L.gsr_normal_loss_backward(None, *view(**v), normals, depth, alpha, dl, dn, dd, da)

    for call in (dn_f, dn_b, nl_f, nl_b):
        for v in bad_views:
            assert call(**v) == -1, (call.__name__, v)
    assert dn_f(depth=None) == -1 and dn_f(out=None) == -1
    assert dn_b() == 0 and dn_b(alpha=None) == 0  # no gradient asked for: nothing is launched
    assert dn_b(depth=None, dd=ONE) == -1 and dn_b(dout=None, dd=ONE) == -1
    assert dn_b(alpha=None, da=ONE) == -1  # dL_dalpha without alpha
    for k in ("normals", "depth", "alpha", "work", "out"):
        assert nl_f(**{k: None}) == -1, k
    assert nl_f(work=ctypes.c_void_p(260)) == -1  # the workspace holds doubles
    assert nl_b() == 0
    for k in ("normals", "depth", "alpha", "dl"):
        assert nl_b(dn=ONE, **{k: None}) == -1, k
    # the workspace: one double per 32 x 8 tile
    sz = ctypes.c_size_t(0)
    ws = L.gsr_normal_loss_workspace_size
    assert ws(1080, 1920, ctypes.byref(sz)) == 0 and sz.value == 8 * 60 * 135
    assert ws(1, 1, ctypes.byref(sz)) == 0 and sz.value == 8 and ws(9, 33, ctypes.byref(sz)) == 0 and sz.value == 8 * 2 * 2
    assert ws(0, 5, ctypes.byref(sz)) == -1 and ws(5, -1, ctypes.byref(sz)) == -1 and ws(5, 5, None) == -1
    assert ws(1 << 16, 1 << 16, ctypes.byref(sz)) == -1


def test_the_python_layer_refuses_by_name_before_any_launch():
    from gaussianeditor_amd import normals as N

    P, H, W = 5, 6, 7
    q, s, x, V = torch.randn(P, 4), torch.rand(P, 3), torch.randn(P, 3), torch.eye(4)
    d, a, n = torch.rand(1, H, W), torch.rand(1, H, W), torch.rand(3, H, W)
    K = dict(fx=5.0, fy=5.0, cx=3.0, cy=2.5)
    with pytest.raises(RuntimeError, match="gaussian_normals: rotations must live on the ROCm GPU.*no CPU fallback"):
        N.gaussian_normals(q, s, x, V)
    for name, args in (("rotations", (q.double(), s, x, V)), ("scales", (q, s.half(), x, V)), ("means3D", (q, s, x.double(), V)),
                       ("viewmatrix", (q, s, x, V.double()))):
        with pytest.raises(RuntimeError, match=f"gaussian_normals: {name} has dtype"):
            N.gaussian_normals(*args)
    for name, args in (("rotations", (q[:, :3], s, x, V)), ("scales", (q, s[:4], x, V)), ("means3D", (q, s, x[:, :2], V)),
                       ("viewmatrix", (q, s, x, V[:3]))):
        with pytest.raises(RuntimeError, match=f"gaussian_normals: {name} has shape"):
            N.gaussian_normals(*args)
    with pytest.raises(RuntimeError, match="gaussian_normals: viewmatrix must be contiguous"):
        N.gaussian_normals(q, s, x, V.t())
    with pytest.raises(TypeError, match="gaussian_normals: scales must be a tensor"):
        N.gaussian_normals(q, None, x, V)
    with pytest.raises(RuntimeError, match="depth_to_normals: depth must live on the ROCm GPU"):
        N.depth_to_normals(d, a, **K)
    with pytest.raises(RuntimeError, match="depth_to_normals: depth has shape"):
        N.depth_to_normals(d[0], a, **K)
    with pytest.raises(RuntimeError, match="depth_to_normals: depth has dtype"):
        N.depth_to_normals(d.double(), a, **K)
    with pytest.raises(RuntimeError, match="depth_to_normals: depth must be contiguous"):
        N.depth_to_normals(torch.rand(1, W, H).transpose(1, 2), None, **K)
    with pytest.raises(RuntimeError, match="normal_consistency_loss: normals must live on the ROCm GPU"):
        N.normal_consistency_loss(n, d, a, **K)
    with pytest.raises(RuntimeError, match="normal_consistency_loss: normals has shape"):
        N.normal_consistency_loss(n[:2], d, a, **K)
    with pytest.raises(RuntimeError, match="normal_consistency_loss: normals has dtype"):
        N.normal_consistency_loss(n.double(), d, a, **K)
    with pytest.raises(TypeError, match="normal_consistency_loss: alpha must be a tensor"):
        N.normal_consistency_loss(n, d, None, **K)
    # what follows the tensor checks is refused on a meta-device stand-in: nothing here can reach a kernel
    fake = lambda *shape: _FakeCuda(torch.zeros(*shape))  # noqa: E731
    with pytest.raises(RuntimeError, match="depth_to_normals: alpha has shape"):
        N.depth_to_normals(fake(1, H, W), fake(1, H, W + 1), **K)
    with pytest.raises(RuntimeError, match="normal_consistency_loss: depth has shape"):
        N.normal_consistency_loss(fake(3, H, W), fake(1, H + 1, W), fake(1, H, W), **K)
    with pytest.raises(ValueError, match="depth_to_normals: give a camera"):
        N.depth_to_normals(fake(1, H, W), None, fx=5.0)
    with pytest.raises(ValueError, match="depth_to_normals: fx and fy must be positive"):
        N.depth_to_normals(fake(1, H, W), None, fx=0.0, fy=5.0, cx=1.0, cy=1.0)
    with pytest.raises(ValueError, match="normal_consistency_loss: alpha_min must be finite"):
        N.normal_consistency_loss(fake(3, H, W), fake(1, H, W), fake(1, H, W), alpha_min=math.nan, **K)
    cam = _Cam(W + 1, H)
    with pytest.raises(ValueError, match="depth_to_normals: the camera is"):
        N.depth_to_normals(fake(1, H, W), None, cam)


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: gets past the device check so that the checks behind it can be reached."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    is_cuda = property(lambda self: True)


class _Cam:
    def __init__(self, W, H, fovx=1.0, fovy=0.8):
        self.image_width, self.image_height, self.FoVx, self.FoVy = W, H, fovx, fovy


def test_camera_intrinsics_are_what_ndc2pix_implies():
    import gaussianeditor_amd
    from gaussianeditor_amd import normals as N
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizationSettings

    fx, fy, cx, cy = N.camera_intrinsics(_Cam(640, 480, 1.0, 0.8))
    assert fx == pytest.approx(640 / (2 * math.tan(0.5))) and fy == pytest.approx(480 / (2 * math.tan(0.4)))
    assert (cx, cy) == (319.5, 239.5)
    # ndc2Pix: pixel = ((ndc + 1) W - 1) / 2 with ndc = x / (z tanfovx)  =>  pixel = fx x / z + (W - 1) / 2
    x_over_z, tx = 0.3, math.tan(0.5)
    assert ((x_over_z / tx + 1.0) * 640 - 1.0) * 0.5 == pytest.approx(fx * x_over_z + cx)
    rs = GaussianRasterizationSettings(480, 640, math.tan(0.5), math.tan(0.4), None, 1.0, None, None, 0, None, False, False)
    assert N.camera_intrinsics(rs) == pytest.approx((fx, fy, cx, cy))
    for name in ("gaussian_normals", "depth_to_normals", "normal_consistency_loss", "camera_intrinsics"):
        assert getattr(gaussianeditor_amd, name) is getattr(N, name)
    assert N.TILE == (32, 8) and N.ROWS_PER_BLOCK == 256


def test_render_without_the_keyword_returns_the_keys_it_returns_today(oracle, monkeypatch):
    import features_helpers as FH

    dgr, be = FH.install(monkeypatch)
    from gaussianeditor_amd.gaussian_renderer import render
    from test_cpu_host_api import _PC, PIPE

    case, G, GF, feats = FH.feature_case("p600", C=5)
    base = {"render", "viewspace_points", "visibility_filter", "radii", "depth_3dgs"}
    assert set(render(case["cam"], _PC(case["sc"]), PIPE, case["bg"])) == base
    assert set(render(case["cam"], _PC(case["sc"]), PIPE, case["bg"], return_alpha=True, features=feats)) == base | {"alpha", "features"}
    assert set(render(case["cam"], _PC(case["sc"]), PIPE, case["bg"], return_normals=False)) == base
    assert be.feature_images == 1
    # the rasterizer's arity depends on the keyword alone
    sc = case["sc"]
    rs = FH.settings(case, "cpu")
    outs = dgr.GaussianRasterizer(rs)(sc["xyz"], torch.zeros_like(sc["xyz"]), sc["opacity"], shs=sc["features"], scales=sc["scaling"],
                                      rotations=sc["rotation"], return_normals=False)
    assert len(outs) == 3


def test_return_normals_refusals_need_no_gpu():
    """More than 253 feature channels alongside, and a precomputed covariance, are refused before anything is computed."""
    import features_helpers as FH
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    case, *_ = FH.feature_case("p600", C=5)
    sc = case["sc"]
    P = sc["xyz"].shape[0]
    r = GaussianRasterizer(FH.settings(case, "cpu"))
    kw = dict(shs=sc["features"], scales=sc["scaling"], rotations=sc["rotation"])
    with pytest.raises(RuntimeError, match="at most 253 with it, got 254"):
        r(sc["xyz"], torch.zeros(P, 3), sc["opacity"], features=torch.zeros(P, 254), return_normals=True, **kw)
    with pytest.raises(RuntimeError, match="`return_normals` needs scales and rotations"):
        r(sc["xyz"], torch.zeros(P, 3), sc["opacity"], shs=sc["features"], cov3D_precomp=torch.zeros(P, 6), return_normals=True)
    # 253 is accepted by this check: the call goes on to the normals and stops there only because these tensors are on the CPU
    with pytest.raises(RuntimeError, match="gaussian_normals: rotations must live on the ROCm GPU"):
        r(sc["xyz"], torch.zeros(P, 3), sc["opacity"], features=torch.zeros(P, 253), return_normals=True, **kw)
