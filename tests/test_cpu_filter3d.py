"""CPU: Mip-Splatting's 3D filter without a device -- the restatement of tests/filter3d_helpers.py
against closed forms and at the float32 neighbours of every threshold, the input condition of the seeded sweep cases (0
offenders), the apply's identities against autograd, header and symbols, every refusal of the four entry points, the Python
layer's refusals by name, the packed record, and the scene files."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import filter3d_helpers as FH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
ONE = ctypes.c_void_p(256)  # never dereferenced
NAMES = ("gsr_filter3d_workspace_size", "gsr_filter3d_sweep", "gsr_filter3d_apply_forward", "gsr_filter3d_apply_backward")


def _f32(v):
    return np.float32(v)


# ---- the restatement of the sweep against closed forms ------------------------------------------------------------------
def test_one_identity_camera_and_a_point_on_the_axis():
    cam = FH.identity_camera(W=640, H=480, fovx=1.0, fovy=0.8)
    fx = 640 / (2 * math.tan(0.5))
    for z in (0.5, 2.0, 37.25):
        f, valid = FH.sweep_ref(np.array([[0.0, 0.0, z]], dtype=np.float32), [cam])
        assert valid.tolist() == [True] and f.dtype == np.float32 and f.shape == (1, 1)
        assert f[0, 0] == _f32(z / fx * math.sqrt(0.2))


def test_the_nearer_of_two_cameras_wins_and_f_max_comes_from_a_camera_that_sees_nothing():
    near, far = FH.identity_camera(t=(0, 0, -1.0)), FH.identity_camera(t=(0, 0, 3.0))  # zc = z - 1 and z + 3
    p = np.array([[0.0, 0.0, 4.0]], dtype=np.float32)
    fx = 640 / (2 * math.tan(0.5))
    for cams in ([near, far], [far, near]):
        f, _ = FH.sweep_ref(p, cams)
        assert f[0, 0] == _f32(3.0 / fx * math.sqrt(0.2))
    # a camera that looks away (zc = -z - 1 < 0) with four times the focal length: it sees nothing and sets f_max
    M = np.eye(4)
    M[2, 2], M[0, 0], M[3, 2] = -1.0, -1.0, -1.0
    blind = FH.Cam(M, 2560, 480, 1.0, 0.8)
    f, valid = FH.sweep_ref(p, [near, blind])
    assert valid.tolist() == [True] and f[0, 0] == _f32(3.0 / (4 * fx) * math.sqrt(0.2))
    assert not FH.sees(p, FH.camera_table([blind])[0])[0].any()


def test_an_unseen_row_takes_the_largest_seen_depth_and_nothing_seen_gives_100000():
    cam = FH.identity_camera()
    fx = 640 / (2 * math.tan(0.5))
    xyz = np.array([[0, 0, 1.5], [0, 0, 6.0], [0, 0, -2.0], [500.0, 0, 2.0], [0, 0, 3.0]], dtype=np.float32)
    f, valid = FH.sweep_ref(xyz, [cam])
    assert valid.tolist() == [True, True, False, False, True]
    want = [1.5, 6.0, 6.0, 6.0, 3.0]
    assert f[:, 0].tolist() == [_f32(d / fx * math.sqrt(0.2)) for d in want]
    f, valid = FH.sweep_ref(xyz[2:4], [cam])
    assert not valid.any() and f[:, 0].tolist() == [_f32(100000.0 / fx * math.sqrt(0.2))] * 2


def test_the_float32_neighbours_of_every_threshold_fall_on_opposite_sides():
    """Identity-rotation cameras: p = xyz exactly.  At the near plane 0.2f itself and its predecessor are not seen (the
    comparison is strict), its successor is; at each of the four screen bounds (inclusive) the last float32 inside is seen
    and its neighbour is not -- asserted of the restatement, which the kernel is then held to bit for bit."""
    for cam in (FH.identity_camera(), FH.identity_camera(W=701, H=333, fovx=0.6, fovy=1.1)):
        xyz, want, names = FH.boundary_rows(cam)
        t = FH.camera_table([cam])[0]
        seen, _ = FH.sees(xyz, t)
        assert seen.tolist() == want.tolist(), list(zip(names, seen))
        assert len(names) == 11 and want.sum() == 5
        # the pairs are neighbours in float32, and the screen pairs straddle the bound in u / v
        for i in range(3, 11, 2):
            axis = 0 if names[i][0] == "u" else 1
            a, b = xyz[i, axis], xyz[i + 1, axis]
            assert np.nextafter(a, b) == b, names[i]
            lo_hi = FH.bounds(t)[2 * axis + (1 if "hi" in names[i] else 0)]
            vals = [FH.project(xyz[j:j + 1], t)[1 + axis][0] for j in (i, i + 1)]
            assert min(vals) <= lo_hi <= max(vals) and vals[0] != vals[1], names[i]
        assert xyz[1, 2] == np.float32(0.2) and np.nextafter(xyz[0, 2], np.float32(1)) == xyz[1, 2]
        _, valid = FH.sweep_ref(xyz, [cam])
        assert valid.tolist() == want.tolist()


def test_the_seeded_cases_have_no_decision_near_a_threshold():
    """0 offenders: no (row, camera) decision within 1e-9 relative of its threshold -- a condition on the inputs."""
    mixed = 0
    for P, V in FH.SWEEP_CASES:
        c = FH.sweep_case(P, V)
        assert FH.sweep_offenders(c["xyz"], c["cameras"]) == 0, (P, V)
        _, valid = FH.sweep_expectation(P, V)
        mixed += bool(valid.any() and not valid.all())
    assert mixed >= len(FH.SWEEP_CASES) // 2  # seen and unseen rows in the same case
    _, valid = FH.sweep_expectation(1000, 1)
    assert 0.02 < valid.mean() < 0.98
    # general cameras: roll, unequal focal lengths, sizes that are multiples of nothing
    t = FH.camera_table(FH.seeded_cameras(FH.CHUNK + 1))
    assert all(abs(c["fx"] / c["fy"] - 1.0) > 1e-3 for c in t) and any(c["W"] % 2 for c in t) and any(c["H"] % 2 for c in t)
    assert all(abs(c["M"][0, 1]) > 1e-6 for c in t)
    # the camera-model cameras of tests/camera_cases.py go through the same table
    import camera_cases as CC
    from gaussianeditor_amd.synth import ring_cameras

    base = ring_cameras(3, 97, 61)[1]
    cams = [CC.general_camera(base, 97, 61, *CC.CAMERAS[n]) for n in CC.NAMES]
    xyz = FH.sweep_case(1000, 2)["xyz"] / 3.0
    assert FH.sweep_offenders(xyz, cams) == 0
    f, valid = FH.sweep_ref(xyz, cams)
    assert 0.05 < valid.mean() < 1.0 and np.isfinite(f).all()


def test_the_packed_record_is_the_layout_of_the_header():
    from gaussianeditor_amd import filter3d as F3

    assert F3.CAMERAS_PER_CHUNK == FH.CHUNK and F3.ROWS_PER_BLOCK == FH.ROWS and F3.CAMERA_DOUBLES == 20
    cams = FH.seeded_cameras(5)
    rec, f_max = F3.camera_records(cams)
    table = FH.camera_table(cams)
    assert rec.shape == (5, 20) and rec.dtype == np.float64 and f_max == max(c["fx"] for c in table)
    for r, c in zip(rec, table):
        assert np.array_equal(r[:12].reshape(4, 3), c["M"][:, :3])
        assert r[12:].tolist() == [c["fx"], c["fy"], 0.5 * c["W"], 0.5 * c["H"], *FH.bounds(c)]
    packed = F3.pack_cameras(cams, "cpu")
    assert len(packed) == 5 and packed.f_max == f_max and np.array_equal(packed.records.numpy(), rec)
    import gaussianeditor_amd

    for name in ("pack_cameras", "compute_3d_filter", "apply_3d_filter", "bake_3d_filter"):
        assert getattr(gaussianeditor_amd, name) is getattr(F3, name)


# ---- the apply ----------------------------------------------------------------------------------------------------------
def _case64(P, from_raw, grad=True):
    c = FH.apply_case(P, from_raw)
    return c, {k: torch.tensor(c[k]).double().requires_grad_(grad and k in ("scales", "opacity")) for k in
               ("scales", "opacity", "filter", "g_s", "g_o")}


def test_a_zero_filter_is_the_identity_on_values_and_gradients():
    for from_raw in (False, True):
        c, t = _case64(1000, from_raw)
        zero = torch.zeros_like(t["filter"])
        s_eff, o_eff = FH.apply_ref(t["scales"], t["opacity"], zero, from_raw)
        s = torch.exp(t["scales"]) if from_raw else t["scales"]
        o = torch.sigmoid(t["opacity"]) if from_raw else t["opacity"]
        assert float((s_eff - s).detach().abs().max()) <= 1e-15 * float(s.detach().abs().max())
        assert float((o_eff - o).detach().abs().max()) <= 1e-15
        gs, go = torch.autograd.grad([s_eff, o_eff], [t["scales"], t["opacity"]], [t["g_s"], t["g_o"]])
        ws, wo = torch.autograd.grad([s, o], [t["scales"], t["opacity"]], [t["g_s"], t["g_o"]]) if from_raw else (t["g_s"], t["g_o"])
        assert float((gs - ws).abs().max()) <= 1e-12 * float(ws.abs().max()) and float((go - wo).abs().max()) <= 1e-12


def test_from_raw_is_the_activation_followed_by_the_activated_route():
    c, t = _case64(1000, True)
    a = FH.apply_ref(t["scales"], t["opacity"], t["filter"], True)
    b = FH.apply_ref(torch.exp(t["scales"]), torch.sigmoid(t["opacity"]), t["filter"], False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ga = torch.autograd.grad(list(a), [t["scales"], t["opacity"]], [t["g_s"], t["g_o"]], retain_graph=True)
    gb = torch.autograd.grad(list(b), [t["scales"], t["opacity"]], [t["g_s"], t["g_o"]])
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])


def test_the_gradient_identities_hold_against_autograd():
    """d s_eff_k / d s_k = s_k / s_eff_k;  d o_eff / d o = coef;  d o_eff / d s_k = o coef f^2 / (s_k s_eff_k^2), written as
    the header writes them (no 0 / 0 at f = 0), against autograd of the torch operators: 1e-12 relative, float64 rounding
    of ten operators."""
    c, t = _case64(1000, False)
    s, o, f = t["scales"], t["opacity"], t["filter"]
    s_eff, o_eff = FH.apply_ref(s, o, f, False)
    gs, go = torch.autograd.grad([s_eff, o_eff], [s, o], [t["g_s"], t["g_o"]])
    with torch.no_grad():
        e = s * s + f * f
        coef = torch.sqrt(((s * s) / e).prod(dim=1, keepdim=True))
        want_o = t["g_o"] * coef
        cross = t["g_o"] * (o * coef) * ((f * f) / (s * e))
        want_s = t["g_s"] * (s / torch.sqrt(e)) + cross
    assert float((gs - want_s).abs().max()) <= 1e-12 * float(want_s.abs().max())
    assert float((go - want_o).abs().max()) <= 1e-12 * float(want_o.abs().max())
    assert np.allclose(FH.cross_term(c), cross.numpy(), rtol=1e-10, atol=1e-12 * float(cross.abs().max()))
    assert not bool(cross[(f == 0).expand_as(cross)].any()) and bool(torch.isfinite(want_s).all())
    assert int((f == 0).sum()) > 50


def test_the_cross_term_exceeds_ten_bars_on_enough_rows_of_every_case():
    """The discrimination condition, a property of the inputs: a backward without d o_eff / d s could not pass."""
    for from_raw in (False, True):
        for P in FH.LADDER:
            _, bars = FH.apply_expectation(P, from_raw)
            big = int((np.abs(FH.cross_term(FH.apply_case(P, from_raw))).max(axis=1) > 10.0 * bars["d_scales"]).sum())
            assert big >= min(100, P / 4), (from_raw, P, big)


# ---- header, symbols, refusals ------------------------------------------------------------------------------------------
def test_header_and_symbols():
    from gaussianeditor_amd import _native

    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "#define GSR_ABI_VERSION 6" in hdr and "#define GSR_FILTER3D_CAMERA_DOUBLES 20" in hdr
    L = _native.lib()
    for name in NAMES:
        assert f"int {name}(" in hdr and name in _native.SIGNATURES and hasattr(L, name)
    assert "(double)0.2f" in hdr and "100000" in hdr and "whether they saw anything or not" in hdr
    mk = open(os.path.join(ROOT, "gaussianeditor_amd", "csrc", "Makefile")).read()
    assert "gsr_filter3d.hip" in mk


def test_every_refusal_comes_back_before_the_device_is_touched():
    """GSR_ERR_BAD_ARGUMENT (-1) on a machine without a GPU; the empty calls return GSR_OK without a launch."""
    from gaussianeditor_amd import _native

    L = _native.lib()
    odd, odd8 = ctypes.c_void_p(258), ctypes.c_void_p(260)
    sz = ctypes.c_size_t(0)
    ws = L.gsr_filter3d_workspace_size
    assert ws(0, ctypes.byref(sz)) == 0 and ws(1_000_000, ctypes.byref(sz)) == 0 and sz.value == 8
    assert ws(-1, ctypes.byref(sz)) == -1 and ws(1 << 31, ctypes.byref(sz)) == -1 and ws(5, None) == -1

    def sweep(P=10, V=3, xyz=ONE, cams=ONE, f_max=500.0, coef=0.4, work=ONE, out=ONE, valid=ONE):
        return L.gsr_filter3d_sweep(None, P, V, xyz, cams, f_max, coef, work, out, valid)

    assert sweep(P=0) == 0 and sweep(P=0, xyz=None, work=None, out=None, valid=None) == 0
    for bad in (dict(P=-1), dict(P=1 << 31), dict(V=0), dict(V=-2), dict(P=0, V=0), dict(xyz=None), dict(cams=None),
                dict(P=0, cams=None), dict(work=None), dict(out=None), dict(valid=None), dict(xyz=odd), dict(out=odd),
                dict(cams=odd8), dict(work=odd8), dict(f_max=0.0), dict(f_max=-1.0), dict(f_max=math.nan), dict(f_max=math.inf),
                dict(coef=math.nan)):
        assert sweep(**bad) == -1, bad

    fwd, bwd = L.gsr_filter3d_apply_forward, L.gsr_filter3d_apply_backward
    assert fwd(None, 0, 0, None, None, None, None, None) == 0 and bwd(None, 0, 1, None, None, None, None, None, None, None) == 0
    for raw in (0, 1):
        assert fwd(None, -1, raw, ONE, ONE, ONE, ONE, ONE) == -1 and fwd(None, 1 << 31, raw, ONE, ONE, ONE, ONE, ONE) == -1
        assert bwd(None, -1, raw, ONE, ONE, ONE, ONE, ONE, ONE, ONE) == -1
        for i in range(5):
            for bad in (None, odd):
                a = [ONE] * 5
                a[i] = bad
                assert fwd(None, 10, raw, *a) == -1, (i, bad)
        for i in range(3):  # the inputs are required; the four gradients may be NULL
            for bad in (None, odd):
                a = [ONE] * 7
                a[i] = bad
                assert bwd(None, 10, raw, *a) == -1, (i, bad)
        for i in range(3, 7):
            a = [ONE] * 7
            a[i] = odd
            assert bwd(None, 10, raw, *a) == -1, i
        # no gradient asked for: nothing is launched, whatever the upstream pointers are
        assert bwd(None, 10, raw, ONE, ONE, ONE, ONE, ONE, None, None) == 0
        assert bwd(None, 10, raw, ONE, ONE, ONE, None, None, None, None) == 0
    assert fwd(None, 10, 2, ONE, ONE, ONE, ONE, ONE) == -1 and bwd(None, 10, -1, ONE, ONE, ONE, ONE, ONE, ONE, ONE) == -1


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: gets past the device check so that the checks behind it can be reached."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    is_cuda = property(lambda self: True)


def test_the_python_layer_refuses_by_name_before_any_launch():
    from gaussianeditor_amd import filter3d as F3

    P = 5
    xyz, s, o, f = torch.randn(P, 3), torch.rand(P, 3), torch.rand(P, 1), torch.rand(P, 1)
    cams = list(FH.seeded_cameras(2))
    with pytest.raises(RuntimeError, match="compute_3d_filter: means3D must live on the ROCm GPU.*no CPU fallback"):
        F3.compute_3d_filter(xyz, cams)
    with pytest.raises(RuntimeError, match="compute_3d_filter: means3D has dtype"):
        F3.compute_3d_filter(xyz.double(), cams)
    with pytest.raises(RuntimeError, match="compute_3d_filter: means3D has shape"):
        F3.compute_3d_filter(xyz[:, :2], cams)
    with pytest.raises(RuntimeError, match="compute_3d_filter: means3D must be contiguous"):
        F3.compute_3d_filter(torch.randn(3, P).t(), cams)
    with pytest.raises(TypeError, match="compute_3d_filter: means3D must be a tensor"):
        F3.compute_3d_filter(None, cams)
    fake = _FakeCuda(xyz)
    with pytest.raises(ValueError, match="compute_3d_filter: cameras is empty"):
        F3.compute_3d_filter(fake, [])
    with pytest.raises(ValueError, match="pack_cameras: cameras is empty"):
        F3.pack_cameras([], "cpu")
    for kw, what in ((dict(fovx=0.0), "FoVx 0.0"), (dict(fovy=-0.3), "FoVy -0.3"), (dict(fovx=math.pi), "FoVx"),
                     (dict(W=0), "image size 0 x"), (dict(H=-4), "image size 640 x -4")):
        with pytest.raises(ValueError, match=f"pack_cameras: camera 1 has .*{what}"):
            F3.pack_cameras([cams[0], FH.identity_camera(**kw)], "cpu")
    with pytest.raises(ValueError, match="compute_3d_filter: camera 0 has FoVx"):
        F3.compute_3d_filter(fake, [FH.identity_camera(fovx=-1.0)])
    bad = FH.identity_camera()
    bad.world_view_transform = torch.eye(3)
    with pytest.raises(ValueError, match=r"pack_cameras: camera 0 has no \(4, 4\) world_view_transform"):
        F3.pack_cameras([bad], "cpu")
    packed = F3.pack_cameras(cams, "cpu")
    with pytest.raises(RuntimeError, match="compute_3d_filter: cameras is on meta"):  # (not on the device of means3D)
        F3.compute_3d_filter(fake, F3.PackedCameras(packed.records.to("meta"), packed.f_max))
    with pytest.raises(RuntimeError, match=r"compute_3d_filter: cameras.records must be a contiguous \(V, 20\) float64"):
        F3.compute_3d_filter(fake, F3.PackedCameras(packed.records.float(), packed.f_max))
    with pytest.raises(RuntimeError, match=r"compute_3d_filter: cameras.records must be a contiguous \(V, 20\) float64"):
        F3.compute_3d_filter(fake, F3.PackedCameras(packed.records[:, :19].contiguous(), packed.f_max))

    with pytest.raises(RuntimeError, match="apply_3d_filter: scales must live on the ROCm GPU.*no CPU fallback"):
        F3.apply_3d_filter(s, o, f)
    for name, args in (("scales", (s.double(), o, f)), ("opacity", (s, o.half(), f)), ("filter_3D", (s, o, f.double()))):
        with pytest.raises(RuntimeError, match=f"apply_3d_filter: {name} has dtype"):
            F3.apply_3d_filter(*args)
    for name, args in (("scales", (s[:, :2], o, f)), ("opacity", (s, o[:, 0], f)), ("filter_3D", (s, o, f[:4])),
                       ("opacity", (s, o[:3], f))):
        with pytest.raises(RuntimeError, match=f"apply_3d_filter: {name} has shape"):
            F3.apply_3d_filter(*args)
    with pytest.raises(RuntimeError, match="apply_3d_filter: scales must be contiguous"):
        F3.apply_3d_filter(torch.rand(3, P).t(), o, f)
    with pytest.raises(TypeError, match="apply_3d_filter: filter_3D must be a tensor"):
        F3.apply_3d_filter(s, o, None)
    with pytest.raises(RuntimeError, match="apply_3d_filter: scales must live on the ROCm GPU"):
        F3.bake_3d_filter(s, o, f)


# ---- scene files --------------------------------------------------------------------------------------------------------
def _raw_scene(P=37):
    g = torch.Generator().manual_seed(5)
    r = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    return dict(xyz=r(P, 3), f_dc=r(P, 1, 3), f_rest=r(P, 15, 3), opacity=r(P, 1), scaling=r(P, 3), rotation=r(P, 4))


def test_scene_files_carry_the_filter_and_are_todays_bytes_without_it(tmp_path):
    from gaussianeditor_amd import scene_ply

    raw = _raw_scene()
    filt = torch.rand(37, 1, generator=torch.Generator().manual_seed(6))
    plain, again, with_f = (str(tmp_path / n) for n in ("plain.ply", "again.ply", "filter.ply"))
    scene_ply.save_gaussians_ply(plain, **raw)
    scene_ply.save_gaussians_ply(again, **raw, filter_3D=None)
    scene_ply.save_gaussians_ply(with_f, **raw, filter_3D=filt)
    a, b, c = (open(p, "rb").read() for p in (plain, again, with_f))
    assert a == b and b"filter_3D" not in a
    # today's bytes: the header lists the reference's properties and ends at rot_3; 62 float32 columns per row
    head, body = a.split(b"end_header\n")
    props = [ln.split()[-1] for ln in head.decode().splitlines() if ln.startswith("property")]
    assert props[:6] == ["x", "y", "z", "nx", "ny", "nz"] and props[-1] == "rot_3" and len(props) == 62 and len(body) == 37 * 62 * 4
    # with the filter: one more property, after the rotation columns, and the same bytes in front of it in every row
    head_c, body_c = c.split(b"end_header\n")
    props_c = [ln.split()[-1] for ln in head_c.decode().splitlines() if ln.startswith("property")]
    assert props_c == props + ["filter_3D"] and len(body_c) == 37 * 63 * 4
    rows, rows_c = np.frombuffer(body, "<f4").reshape(37, 62), np.frombuffer(body_c, "<f4").reshape(37, 63)
    assert np.array_equal(rows, rows_c[:, :62]) and np.array_equal(rows_c[:, 62], filt[:, 0].numpy())
    back = scene_ply.load_gaussians_ply(with_f)
    assert tuple(back["filter_3D"].shape) == (37, 1) and torch.equal(back["filter_3D"], filt)
    for k in raw:
        assert torch.equal(back[k], raw[k]), k
    assert "filter_3D" not in scene_ply.load_gaussians_ply(plain) and back["max_sh_degree"] == 3
