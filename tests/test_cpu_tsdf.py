"""CPU: TSDF fusion and mesh extraction (gaussianeditor_amd/tsdf.py) -- what needs no GPU.

  * the numpy restatement's own properties (tests/tsdf_helpers.py), on an analytic sphere at 12^3 and 20^3 (radius 0.4 of the
    lattice): every undirected edge in exactly two faces, every directed edge once, V - E + F = 2, signed volume and area
    within 5 % (12^3) and 1 % (20^3) of the sphere's (measured 0.974 / 0.987 and 0.991 / 0.996), radial vertex error at most
    0.11 voxel (measured 0.084 and 0.049), every vertex referenced; the orientation table; a V-view restatement equals V
    one-view restatements; the seeded integration cases reach every branch they are meant to reach;
  * every refusal of tsdf.py, by name, before anything is launched; the argument checks of the C entry points;
  * a PLY write -> load -> write round trip, byte for byte.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tsdf_helpers as TH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_constants_are_the_kernel_files():
    from gaussianeditor_amd import tsdf as T

    src = open(os.path.join(ROOT, "gaussianeditor_amd", "csrc", "gsr_tsdf.hip")).read()
    m = re.search(r"TS_BX = (\d+), TS_BY = (\d+), TS_BZ = (\d+);", src)
    assert tuple(int(g) for g in m.groups()) == T.BLOCK_DIMS == TH.BLOCK
    assert int(re.search(r"TS_CHUNK = (\d+);", src).group(1)) == T.CAMERAS_PER_CHUNK == TH.CHUNK
    assert int(re.search(r"MT_ROWS = (\d+);", src).group(1)) == T.MESH_ROWS_PER_BLOCK == TH.MESH_ROWS
    assert 7 * T.MAX_MESH_POINTS < 2 ** 31 <= 7 * (T.MAX_MESH_POINTS + 1)
    import gaussianeditor_amd

    assert gaussianeditor_amd.TSDFVolume is T.TSDFVolume and gaussianeditor_amd.extract_mesh is T.extract_mesh


# ---- the restatement ----------------------------------------------------------------------------------------------------
def test_the_orientation_table_depends_on_tetrahedron_and_case_only():
    flip = TH.flip_table()
    assert flip.shape == (6, 16) and not flip[:, 0].any() and not flip[:, 15].any()
    for t in range(6):
        for case in range(1, 15):
            if bin(case).count("1") != 2:  # (the same three edges in the same order: swapping the sides turns the triangle round)
                assert flip[t, case] != flip[t, 15 - case]
    # even and odd permutations mirror one another
    assert all((flip[t, 1:15] != flip[0, 1:15]).all() or (flip[t, 1:15] == flip[0, 1:15]).all() for t in range(6))
    assert [TH.tet_path(0)[1], TH.tet_path(0)[2]] == [(1, 0, 0), (1, 1, 0)] and TH.tet_path(5)[1:3] == ((0, 0, 1), (0, 1, 1))


@pytest.mark.parametrize("n,tol", [(12, 0.05), (20, 0.01)])
def test_sphere_properties_of_the_restatement(n, tol):
    tsdf, weight, centre, radius = TH.sphere_field(n)
    v, f, _ = TH.extract_ref(tsdf, weight, (0.0, 0.0, 0.0), 1.0)
    r = TH.sphere_report(n, v, f, centre, radius)
    print(f"  sphere {n}^3: {len(v)} vertices, {len(f)} faces, {r}")
    assert r["directed_max"] == 1 and r["undirected_min"] == 2 and r["undirected_max"] == 2 and r["euler"] == 2
    assert abs(r["volume_ratio"] - 1.0) <= tol and abs(r["area_ratio"] - 1.0) <= tol
    assert r["radial_max"] <= 0.11 and r["referenced"]
    # colours ride on the same t: a colour field linear in x reproduces the vertices' x
    g = np.broadcast_to(np.arange(n, dtype=np.float32)[:, None, None], (n, n, n))
    c = TH.extract_ref(tsdf, weight, (0.0, 0.0, 0.0), 1.0, np.stack([g, g, g]))[2]
    assert np.abs(c[:, 0] - v[:, 0]).max() < 1e-5


def test_an_unobserved_point_opens_the_mesh_and_an_empty_field_gives_none():
    tsdf, weight, _, _ = TH.sphere_field(12)
    weight = weight.copy()
    weight[6, 6, 1:3] = 0.0
    v, f, _ = TH.extract_ref(tsdf, weight, (0.0, 0.0, 0.0), 1.0)
    full = TH.extract_ref(tsdf, np.ones_like(weight), (0.0, 0.0, 0.0), 1.0)
    assert 0 < len(f) < len(full[1]) and TH.edge_counts(f)[1] == 1 and len(np.unique(f)) == len(v)
    v, f, c = TH.extract_ref(np.abs(tsdf) + 1, weight, (0.0, 0.0, 0.0), 1.0, np.zeros((3, 12, 12, 12), dtype=np.float32))
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3) and f.dtype == np.int32
    assert TH.extract_ref(tsdf[:1], weight[:1], (0.0, 0.0, 0.0), 1.0)[1].shape == (0, 3)


def test_the_seeded_cases_reach_their_branches_and_views_compose():
    C = TH.CHUNK
    case = TH.integrate_case((3, 5, 33), C + 1)
    table = TH.FH.camera_table(case["cameras"])
    origin, vs = case["origin"], case["voxel_size"]
    pts = np.stack(np.meshgrid(*[np.float32(o) + np.float64(np.float32(vs)) * np.arange(n) for o, n in zip(origin, case["dims"])],
                               indexing="ij"), axis=-1).reshape(-1, 3)
    behind = outside = 0
    for cam in table:
        p = pts @ cam["M"][:3, :3] + cam["M"][3, :3]
        behind += int((p[:, 2] <= TH.NEAR).sum())
        u = p[:, 0] / p[:, 2] * cam["fx"] + (TH.IMG_W - 1) / 2
        outside += int(((p[:, 2] > TH.NEAR) & ((u < -0.5) | (u >= TH.IMG_W - 0.5))).sum())
    assert behind > 100 and outside > 100
    assert (case["depth"] == 0).sum() > 100
    half = np.float32(0.5)
    assert (case["alpha"] == half).any() and (case["alpha"] == np.nextafter(half, np.float32(0))).any() and (case["alpha"] < 0.4).any()
    full = TH.run_case_ref(case, 3.0)
    assert float(full[1].max()) == 3.0 and (full[0] == 1.0).any() and (full[0] < 0).any() and (full[0] > 0).any()
    one = TH.run_case_ref(TH.integrate_case((5, 7, 9), 1))
    assert set(np.unique(one[1])) == {0.0, 1.0}
    # V views in one go = one view at a time
    state = None
    for v in range(C + 1):
        state = TH.run_case_ref(case, 3.0, state=state, views=[v])
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(state, full))
    # the plane across the image edges: exactly the points that round into the image
    edge = TH.run_case_ref(TH.edge_case())
    assert edge[1].sum() == (4 * TH.IMG_W) * (4 * TH.IMG_H) and not edge[1][:4].any() and not edge[1][:, :4].any()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _cam(W=8, H=6):
    return TH.FH.Cam(np.eye(4), W, H, 0.9, 0.7)


def test_every_refusal_of_the_volume_by_name():
    from gaussianeditor_amd import tsdf as T

    ok = dict(origin=(0, 0, 0), voxel_size=0.1, dims=(3, 4, 5), trunc=0.3, device="cpu")
    for bad, match in ((dict(dims=(3, 4)), "dims"), (dict(dims=(3, 0, 5)), "dims"), (dict(dims=(3, 4.5, 5)), "dims"),
                       (dict(dims=(2048, 2048, 2048)), "2\\^31"), (dict(origin=(0, 0)), "origin"), (dict(origin=(0, float("nan"), 0)), "origin"),
                       (dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=float("inf")), "voxel_size"), (dict(voxel_size="a"), "voxel_size"),
                       (dict(trunc=-1.0), "trunc"), (dict(trunc=float("nan")), "trunc")):
        with pytest.raises(ValueError, match=match):
            T.TSDFVolume(**{**ok, **bad})
    vol = T.TSDFVolume(**ok)
    assert vol.tsdf.shape == (3, 4, 5) and bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all()) and vol.color.shape == (3, 3, 4, 5)
    assert vol.origin == (0.0, 0.0, 0.0) and vol.voxel_size == float(np.float32(0.1))
    assert T.TSDFVolume(**ok, with_color=False).color is None
    vol.tsdf.fill_(0.5)
    vol.reset()
    assert bool((vol.tsdf == 1).all())


def test_every_refusal_of_integrate_by_name():
    from gaussianeditor_amd import tsdf as T
    from gaussianeditor_amd.filter3d import PackedCameras

    vol = T.TSDFVolume((0, 0, 0), 0.1, (3, 4, 5), 0.3, device="cpu")
    plain = T.TSDFVolume((0, 0, 0), 0.1, (3, 4, 5), 0.3, with_color=False, device="cpu")
    d, a, c = torch.ones(2, 1, 6, 8), torch.ones(2, 1, 6, 8), torch.ones(2, 3, 6, 8)
    cams = [_cam(), _cam()]
    what = "TSDFVolume.integrate"
    cases = [
        (vol, dict(depth=d.numpy()), TypeError, "depth must be a tensor"),
        (vol, dict(depth=d[0, 0]), RuntimeError, "depth has shape"),
        (vol, dict(depth=d.double()), RuntimeError, "depth has dtype"),
        (vol, dict(depth=torch.ones(2, 2, 6, 8)), RuntimeError, "depth has shape"),
        (vol, dict(depth=d.transpose(2, 3).contiguous().transpose(2, 3)), RuntimeError, "depth must be contiguous"),
        (vol, dict(depth=torch.ones(0, 1, 6, 8), color=torch.ones(0, 3, 6, 8), alpha=None), RuntimeError, "at least one view"),
        (vol, dict(alpha=a[:1]), RuntimeError, "alpha has shape"),
        (vol, dict(alpha=a.half()), RuntimeError, "alpha has dtype"),
        (vol, dict(color=c[:, :2]), RuntimeError, "color has shape"),
        (vol, dict(color=None), RuntimeError, "color must be given exactly when"),
        (plain, dict(), RuntimeError, "color must be given exactly when"),
        (vol, dict(alpha_min=0.0), ValueError, "alpha_min"),
        (vol, dict(alpha_min=float("nan")), ValueError, "alpha_min"),
        (vol, dict(max_weight=-1.0), ValueError, "max_weight"),
        (vol, dict(max_weight=float("inf")), ValueError, "max_weight"),
        (vol, dict(cameras=cams[:1]), RuntimeError, "1 cameras for 2 views"),
        (vol, dict(cameras=[_cam(), _cam(W=9)]), RuntimeError, "camera 1 has image size 9 x 6"),
        (vol, dict(cameras=PackedCameras(torch.zeros(3, 20, dtype=torch.float64), 1.0)), RuntimeError, "3 cameras for 2 views"),
        (vol, dict(cameras=PackedCameras(torch.zeros(2, 20), 1.0)), RuntimeError, "cameras.records must be"),
        (vol, dict(cameras=PackedCameras(torch.zeros(2, 19, dtype=torch.float64), 1.0)), RuntimeError, "cameras.records must be"),
        (vol, dict(), RuntimeError, "no CPU fallback"),
        (vol, dict(cameras=PackedCameras(torch.zeros(2, 20, dtype=torch.float64), 1.0)), RuntimeError, "no CPU fallback"),
        (vol, dict(depth=d[0], alpha=a[0], color=c[0], cameras=_cam()), RuntimeError, "no CPU fallback"),
    ]
    for v, over, exc, match in cases:
        kw = {**dict(depth=d, cameras=cams, alpha=a, color=c), **over}
        with pytest.raises(exc, match=match) as e:
            v.integrate(kw.pop("depth"), kw.pop("cameras"), **kw)
        assert what in str(e.value), (over, str(e.value))
    # a state that was assigned wrongly is refused by name too
    vol.tsdf = torch.ones(3, 4, 6)
    with pytest.raises(RuntimeError, match="tsdf has shape"):
        vol.integrate(d, cams, alpha=a, color=c)
    vol.reset()
    vol.weight = vol.weight.double()
    with pytest.raises(RuntimeError, match="weight has dtype"):
        vol.integrate(d, cams, alpha=a, color=c)
    vol.reset()
    # integrate_renders
    pk = dict(depth_3dgs=d[0], alpha=a[0], render=c[0])
    with pytest.raises(ValueError, match="render_pkgs is empty"):
        vol.integrate_renders([], cams)
    with pytest.raises(RuntimeError, match="package 1 has no tensor 'alpha'.*return_alpha=True"):
        vol.integrate_renders([pk, dict(depth_3dgs=d[0], render=c[0])], cams)
    with pytest.raises(RuntimeError, match="package 0 has no tensor 'render'"):
        vol.integrate_renders(dict(depth_3dgs=d[0], alpha=a[0]), cams[:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.integrate_renders([pk, pk], cams)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plain.integrate_renders(dict(depth_3dgs=d[0], alpha=a[0]), cams[0])


def test_every_refusal_of_extract_mesh_by_name():
    from gaussianeditor_amd import tsdf as T

    t, w, c = torch.ones(3, 4, 5), torch.ones(3, 4, 5), torch.ones(3, 3, 4, 5)
    ok = dict(tsdf=t, weight=w, origin=(0, 0, 0), voxel_size=0.1, color=c)
    for over, exc, match in ((dict(tsdf=t.numpy()), TypeError, "tsdf must be a tensor"), (dict(tsdf=t[0]), RuntimeError, "tsdf has shape"),
                             (dict(tsdf=torch.ones(3, 0, 5)), RuntimeError, "every extent at least 1"),
                             (dict(tsdf=t.double()), RuntimeError, "tsdf has dtype"), (dict(weight=w[:2]), RuntimeError, "weight has shape"),
                             (dict(weight=w.transpose(0, 1).contiguous().transpose(0, 1)[:3, :4]), RuntimeError, "weight"),
                             (dict(color=c[:2]), RuntimeError, "color has shape"), (dict(origin=(0, 0)), ValueError, "origin"),
                             (dict(voxel_size=-1), ValueError, "voxel_size"), (dict(), RuntimeError, "no CPU fallback"),
                             (dict(color=None), RuntimeError, "no CPU fallback")):
        with pytest.raises(exc, match=match) as e:
            T.extract_mesh(**{**ok, **over})
        assert "extract_mesh" in str(e.value)
    # 7 nx ny nz >= 2^31 is refused before anything is allocated for it (a tensor that only pretends to be that large)
    big = torch.ones(1).expand(677, 677, 677)
    assert 7 * 677 ** 3 >= 2 ** 31 > 7 * 674 ** 3
    with pytest.raises((RuntimeError, ValueError), match="contiguous|2\\^31"):
        T.extract_mesh(big, big, (0, 0, 0), 1.0)
    with pytest.raises(ValueError, match="2\\^31"):
        T._check_mesh_points("extract_mesh", (677, 677, 677))
    T._check_mesh_points("extract_mesh", (674, 674, 674))
    vol = T.TSDFVolume((0, 0, 0), 0.1, (3, 4, 5), 0.3, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.extract_mesh()


def test_the_entry_points_check_their_arguments_without_a_gpu():
    from gaussianeditor_amd import _native

    L = _native.lib()
    one = ctypes.c_void_p(256)  # never dereferenced
    integ = lambda **k: L.gsr_tsdf_integrate(*[{**dict(s=None, nx=3, ny=4, nz=5, ox=0.0, oy=0.0, oz=0.0, vs=0.1, V=2, H=6, W=8, depth=one,  # noqa: E731
                                                       alpha=one, color=one, cams=one, trunc=0.3, amin=0.5, mw=0.0, tsdf=one, weight=one,
                                                       vcol=one), **k}[n] for n in
                                               ("s", "nx", "ny", "nz", "ox", "oy", "oz", "vs", "V", "H", "W", "depth", "alpha", "color", "cams",
                                                "trunc", "amin", "mw", "tsdf", "weight", "vcol")])
    for bad in (dict(nx=0), dict(nz=-1), dict(nx=2048, ny=2048, nz=2048), dict(vs=0.0), dict(vs=float("nan")), dict(ox=float("inf")),
                dict(V=0), dict(H=0), dict(W=-3), dict(V=1 << 20, H=1 << 10, W=1 << 10), dict(trunc=0.0), dict(amin=0.0),
                dict(amin=float("nan")), dict(mw=-1.0), dict(depth=None), dict(cams=None), dict(tsdf=None), dict(weight=None),
                dict(color=None), dict(vcol=None), dict(depth=ctypes.c_void_p(258)), dict(cams=ctypes.c_void_p(260)),
                dict(alpha=ctypes.c_void_p(257))):
        assert integ(**bad) == -1, bad
    sz = ctypes.c_size_t(0)
    assert L.gsr_tsdf_mesh_workspace_size(3, 4, 5, ctypes.byref(sz)) == 0 and sz.value >= 256 + 60 * 6
    assert L.gsr_tsdf_mesh_workspace_size(3, 4, 5, None) == -1 and L.gsr_tsdf_mesh_workspace_size(0, 4, 5, ctypes.byref(sz)) == -1
    assert L.gsr_tsdf_mesh_workspace_size(674, 674, 674, ctypes.byref(sz)) == 0 and sz.value > 6 * 674 ** 3
    assert L.gsr_tsdf_mesh_workspace_size(677, 677, 677, ctypes.byref(sz)) == -3  # GSR_ERR_TOO_MANY: 7 N >= 2^31
    counts = (ctypes.c_int64 * 2)(7, 7)
    assert L.gsr_tsdf_mesh_count(None, 677, 677, 677, one, one, one, counts) == -3 and counts[0] == 0 and counts[1] == 0
    assert L.gsr_tsdf_mesh_count(None, 3, 4, 5, one, one, one, None) == -1
    assert L.gsr_tsdf_mesh_count(None, 3, 4, 5, None, one, one, counts) == -1
    assert L.gsr_tsdf_mesh_count(None, 3, 4, 5, one, one, ctypes.c_void_p(128), counts) == -1  # workspace 256-byte aligned
    emit = lambda *a: L.gsr_tsdf_mesh_emit(None, 3, 4, 5, 0.0, 0.0, 0.0, 0.1, *a)  # noqa: E731
    assert emit(one, one, one, one, 0, 0, None, None, None) == 0  # an empty mesh: nothing to do
    assert emit(one, one, one, one, -1, 0, one, one, one) == -1 and emit(one, one, one, one, 3, 1, None, one, one) == -1
    assert emit(one, one, None, one, 3, 1, one, one, one) == -1  # colours asked for without a colour volume
    assert emit(one, one, one, one, 7 * 60 + 1, 1, one, one, one) == -1 and emit(one, one, one, None, 3, 1, one, one, one) == -1
    assert L.gsr_tsdf_mesh_emit(None, 677, 677, 677, 0.0, 0.0, 0.0, 0.1, one, one, one, one, 3, 1, one, one, one) == -3


# ---- PLY ----------------------------------------------------------------------------------------------------------------
def test_ply_round_trip_is_byte_exact(tmp_path):
    from gaussianeditor_amd import tsdf as T

    tsdf, weight, _, _ = TH.sphere_field(12)
    v, f, _ = TH.extract_ref(tsdf, weight, (0.5, -1.0, 2.0), 0.25)
    rng = np.random.default_rng(1)
    c = (rng.integers(0, 256, size=v.shape) / 255.0).astype(np.float32)
    for colors in (c, None):
        a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
        T.save_mesh_ply(a, torch.tensor(v), torch.tensor(f), None if colors is None else torch.tensor(colors))
        lv, lf, lc = T.load_mesh_ply(a)
        assert lv.dtype == np.float32 and lf.dtype == np.int32 and lv.tobytes() == v.tobytes() and lf.tobytes() == f.tobytes()
        assert (lc is None) == (colors is None) and (colors is None or lc.tobytes() == colors.tobytes())
        T.save_mesh_ply(b, lv, lf, lc)
        raw = open(a, "rb").read()
        assert raw == open(b, "rb").read()
        head = raw[:raw.index(b"end_header\n")].decode().split("\n")
        assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
        assert "property list uchar int vertex_indices" in head and f"element face {len(f)}" in head
        assert len(raw) == raw.index(b"end_header\n") + 11 + len(v) * (12 + (3 if colors is not None else 0)) + len(f) * 13
    T.save_mesh_ply(str(tmp_path / "e.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    ev, ef, ec = T.load_mesh_ply(str(tmp_path / "e.ply"))
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and ec is None
    for bad, match in (((v.astype(np.float64), f, None), "vertices"), ((v, f.astype(np.int64), None), "faces"), ((v, f + len(v), None), "outside"),
                       ((v, f, c[:-1]), "colors")):
        with pytest.raises(ValueError, match=match):
            T.save_mesh_ply(str(tmp_path / "x.ply"), *bad)
    open(tmp_path / "t.ply", "wb").write(open(tmp_path / "a.ply", "rb").read()[:-5])
    with pytest.raises(ValueError, match="bytes of data"):
        T.load_mesh_ply(str(tmp_path / "t.ply"))
    open(tmp_path / "n.ply", "wb").write(b"not a ply")
    with pytest.raises(ValueError, match="not a PLY"):
        T.load_mesh_ply(str(tmp_path / "n.ply"))
