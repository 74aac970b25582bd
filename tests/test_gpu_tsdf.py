"""-m gpu: TSDF fusion and mesh extraction (gaussianeditor_amd/tsdf.py, csrc/gsr_tsdf.hip) against
the numpy restatements of tests/tsdf_helpers.py.

Integration is held BIT FOR BIT -- tsdf, weight and colour -- to the restatement: add, multiply, divide, floor and compare
in binary64, and add, multiply, divide in binary32, without contraction, are exact IEEE operations on both sides.  Grids
(1,1,1), (5,7,9) and three grids that put every extent at the block size - 1, the block size and the block size + 1; V in
{1, 2, C - 1, C, C + 1}, C = CAMERAS_PER_CHUNK; images of 37 x 23; general rolled cameras, some close enough that lattice
points lie behind the near plane; zero depths; alpha under, at and over alpha_min; sdf on both sides of -trunc and +trunc;
max_weight reached; a plane of points whose projections step by a quarter pixel across every image edge; a fused V-view call
against V one-view calls.

Extraction is held EXACTLY to the restatement: the same faces, the same vertex and colour bits.  A 2 x 2 x 2 grid under all
256 sign patterns, the same with one corner unobserved, a (5,7,9) smooth random field with unobserved points and colours, a
(103,101,102) grid whose surface straddles blocks of MESH_ROWS_PER_BLOCK points and the scan's chunk of 1024 blocks, an
all-positive field, grids with an extent of 1.  On the device output of a 20^3 sphere: every undirected edge in exactly two
faces, every directed edge once, V - E + F = 2, volume and area within 1 %, radial error at most 0.11 voxel, every vertex
referenced.

Also here: the same bits on two runs and on a side stream (tests/stream_order.py), guard bands around every buffer the
module allocates or is handed (tests/guarded_alloc.py), and render -> integrate_renders -> extract_mesh end to end (4 000
Gaussians on a sphere, 8 ring cameras at 64 x 64, a 32^3 volume), equal to the restatement fed the same images; it prints
the radial error of the vertices and does not assert it.

Measured on the MI355X: every integration case 0 differing bits, every extraction 0 differing indices and values; the 20^3
sphere on the device 3 230 vertices, 6 456 faces, volume 0.9913, area 0.9955, radial error 0.049 voxel; the side-stream cell
clean and conclusive, outputs on the host 7.9 ms into a 201 ms sleep; end to end 15 934 of 32 768 lattice points observed,
7 359 vertices, 14 225 faces, radial error of the vertices median 0.109, largest 0.321 at a voxel of 0.097 (the splats are
blobs of sigma 0.05 around the sphere: the rendered depth lies in front of it).  The file takes 3.3 s.
"""
import numpy as np
import pytest
import torch

import stream_order as SO
import tsdf_helpers as TH
from guarded_alloc import GuardedAllocator

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = TH.CHUNK
BX, BY, BZ = TH.BLOCK
GRIDS = [(1, 1, 1), (5, 7, 9), (BX - 1, BY, BZ + 1), (BX, BY + 1, BZ - 1), (BX + 1, BY - 1, BZ)]
VIEWS = [1, 2, C - 1, C, C + 1]


def _dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.int32)


def _volume(case):
    from gaussianeditor_amd import tsdf as T

    return T.TSDFVolume(case["origin"], case["voxel_size"], case["dims"], case["trunc"], with_color=case["image"] is not None, device=DEV)


def _integrate(vol, case, max_weight=0.0, views=None, cameras=None, put=None):
    put = _plain_put if put is None else put
    sel = slice(None) if views is None else list(views)
    pick = lambda a: None if a is None else put(torch.tensor(np.ascontiguousarray(a[sel])))  # noqa: E731
    cams = cameras if cameras is not None else (case["cameras"] if views is None else [case["cameras"][v] for v in views])
    vol.integrate(pick(case["depth"]), cams, alpha=pick(case["alpha"]), color=pick(case["image"]), alpha_min=case["alpha_min"],
                  max_weight=max_weight)


def _assert_state(tag, vol, want):
    torch.cuda.synchronize()
    names = ("tsdf", "weight", "color")
    got = (vol.tsdf, vol.weight, vol.color)
    bad = []
    for name, g, w in zip(names, got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert tuple(g.shape) == w.shape and g.dtype == torch.float32
            bad.append(int((_bits(g) != w.view(np.int32)).sum()))
    touched = int((want[1] > 0).sum())
    print(f"  {tag}: {touched} of {want[1].size} lattice points observed, weights up to {float(want[1].max())}; "
          f"{bad} (tsdf, weight, colour) values differ in their bits")
    assert not any(bad), (tag, bad)


# ---- integration --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", VIEWS)
@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_integration_is_the_restatement_bit_for_bit(dims, V):
    case = TH.integrate_case(dims, V)
    mw = 3.0 if V > 2 else 0.0
    vol = _volume(case)
    _integrate(vol, case, mw)
    _assert_state(f"integrate {dims} V={V} max_weight={mw}", vol, TH.run_case_ref(case, mw))


@pytest.mark.parametrize("V,with_alpha,with_color,mw", [(C + 1, False, True, 0.0), (C + 1, True, False, 5.0), (2, False, False, 1.0),
                                                        (1, False, False, 0.0), (2, True, True, 1.0)])
def test_integration_without_alpha_without_colour_and_at_max_weight(V, with_alpha, with_color, mw):
    case = TH.integrate_case((5, 7, 9), V, with_alpha, with_color)
    want = TH.run_case_ref(case, mw)
    if mw > 0 and V > 1:
        assert float(want[1].max()) == mw and (mw > 1 or int((want[1] == mw).sum()) > 20)  # (the cap is reached)
    vol = _volume(case)
    _integrate(vol, case, mw)
    _assert_state(f"integrate (5,7,9) V={V} alpha={with_alpha} colour={with_color} max_weight={mw}", vol, want)


def test_projections_across_every_image_edge():
    case = TH.edge_case()
    want = TH.run_case_ref(case)
    w = want[1][:, :, 0]
    # a quarter pixel per lattice step: the rows 1.375 .. 0.625 pixels outside stay fresh, from 0.375 outside on they round in
    assert not w[:4].any() and not w[-4:].any() and not w[:, :4].any() and not w[:, -4:].any()
    assert w[4:4 + 4 * TH.IMG_W, 4:4 + 4 * TH.IMG_H].all() and w.sum() == (TH.IMG_W * 4) * (TH.IMG_H * 4)
    vol = _volume(case)
    _integrate(vol, case)
    _assert_state("image edges", vol, want)


def test_a_fused_call_is_the_one_view_calls_and_a_packed_table_is_the_list():
    from gaussianeditor_amd import filter3d as F3

    dims, V, mw = (BX + 1, BY + 1, BZ + 1), C + 1, 3.0
    case = TH.integrate_case(dims, V)
    want = TH.run_case_ref(case, mw)
    fused, single, packed = _volume(case), _volume(case), _volume(case)
    _integrate(fused, case, mw)
    for v in range(V):
        if v % 2:
            _integrate(single, case, mw, views=[v])
        else:  # (one view without the leading dimension)
            single.integrate(_dev(case["depth"][v]), case["cameras"][v], alpha=_dev(case["alpha"][v]), color=_dev(case["image"][v]),
                             alpha_min=case["alpha_min"], max_weight=mw)
    _integrate(packed, case, mw, cameras=F3.pack_cameras(case["cameras"], DEV))
    _assert_state("fused", fused, want)
    _assert_state("V one-view calls", single, want)
    _assert_state("packed camera table", packed, want)
    # and a second fused call continues from the stored state
    _integrate(fused, case, mw, views=range(3))
    _assert_state("continued", fused, TH.run_case_ref(case, mw, state=want, views=range(3)))


# ---- extraction ---------------------------------------------------------------------------------------------------------
def _extract(tsdf, weight, origin, vs, color=None):
    from gaussianeditor_amd import tsdf as T

    v, f, c = T.extract_mesh(_dev(tsdf), _dev(weight), origin, vs, _dev(color))
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.ndim == 2 and v.shape[1] == 3 and f.ndim == 2 and f.shape[1] == 3
    assert (c is None) == (color is None) and (c is None or tuple(c.shape) == tuple(v.shape))
    return v.cpu().numpy(), f.cpu().numpy(), None if c is None else c.cpu().numpy()


def _assert_mesh(tag, got, want, quiet=False):
    (v, f, c), (wv, wf, wc) = got, want
    assert v.shape == wv.shape and f.shape == wf.shape, (tag, v.shape, wv.shape, f.shape, wf.shape)
    bad_f = int((f != wf).sum())
    bad_v = int((v.view(np.int32) != wv.view(np.int32)).sum())
    bad_c = 0 if wc is None else int((c.view(np.int32) != wc.view(np.int32)).sum())
    if not quiet:
        print(f"  {tag}: {len(wv)} vertices, {len(wf)} faces; {bad_f} face indices, {bad_v} vertex and {bad_c} colour values differ")
    assert bad_f == 0 and bad_v == 0 and bad_c == 0, (tag, bad_f, bad_v, bad_c)
    if len(wf):
        assert len(np.unique(f)) == len(v)  # every vertex is referenced by a face


@pytest.mark.parametrize("unobserved", [False, True], ids=["observed", "one-corner-unobserved"])
def test_all_256_sign_patterns_of_one_cube(unobserved):
    rng = np.random.default_rng(5)
    origin, vs = (0.25, -1.5, 3.0), 0.37
    faces = 0
    for pattern in range(256):
        mag = rng.uniform(0.1, 1.0, size=8).astype(np.float32)
        sign = np.array([-1.0 if (pattern >> b) & 1 else 1.0 for b in range(8)], dtype=np.float32)
        tsdf = (mag * sign).reshape(2, 2, 2)
        weight = np.ones((2, 2, 2), dtype=np.float32)
        if unobserved:
            weight.reshape(-1)[pattern % 8] = 0.0
        color = rng.uniform(size=(3, 2, 2, 2)).astype(np.float32)
        want = TH.extract_ref(tsdf, weight, origin, vs, color)
        _assert_mesh(f"pattern {pattern}", _extract(tsdf, weight, origin, vs, color), want, quiet=True)
        faces += len(want[1])
    print(f"  256 patterns, {'one corner unobserved' if unobserved else 'all observed'}: {faces} faces in all, all equal")
    assert faces > 256


def test_a_smooth_random_field_with_unobserved_points_and_colours():
    tsdf, weight, color = TH.smooth_field((5, 7, 9))
    assert (tsdf < 0).any() and (tsdf > 0).any() and (weight == 0).any()
    origin, vs = (-0.3, 0.2, 1.1), 0.21
    want = TH.extract_ref(tsdf, weight, origin, vs, color)
    assert len(want[1]) > 50
    _assert_mesh("smooth (5,7,9)", _extract(tsdf, weight, origin, vs, color), want)
    _assert_mesh("smooth (5,7,9), no colour", _extract(tsdf, weight, origin, vs), TH.extract_ref(tsdf, weight, origin, vs))


def test_a_surface_across_blocks_and_across_the_chunk_of_the_scan():
    """(103,101,102) = 1 061 106 lattice points = 1 037 blocks of 1 024: the scan of the block counts takes two chunks.  A
    sphere of radius 7.3 about (95.2, 50.1, 50.3) has vertices on both sides of lattice point 1 024 x 1 024 (x = 101, y = 79)
    and is cut open by the end of the lattice."""
    dims = (103, 101, 102)
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing="ij"), axis=-1)
    tsdf = (np.linalg.norm(g - np.array([95.2, 50.1, 50.3]), axis=-1) - 7.3).astype(np.float32)
    weight = np.ones(dims, dtype=np.float32)
    want = TH.extract_ref(tsdf, weight, (0.0, 0.0, 0.0), 1.0)
    rows = TH.MESH_ROWS
    lower_x = want[0][:, 0]
    assert np.prod(dims) > rows * 1024 and (lower_x < 101.0).any() and (lower_x >= 102.0).any() and len(want[1]) > 2000
    _assert_mesh("two scan chunks", _extract(tsdf, weight, (0.0, 0.0, 0.0), 1.0), want)


@pytest.mark.parametrize("dims", [(6, 5, 4), (1, 5, 5), (5, 1, 5), (5, 5, 1), (1, 1, 1)], ids=lambda d: "x".join(map(str, d)))
def test_empty_meshes(dims):
    """an all-positive field; grids with an extent of 1 have no cubes, whatever the signs"""
    tsdf, weight, color = TH.smooth_field(dims)
    if min(dims) > 1:
        tsdf = np.abs(tsdf) + np.float32(0.01)
    else:
        assert (tsdf < 0).any() or dims == (1, 1, 1)
    v, f, c = _extract(tsdf, np.ones(dims, dtype=np.float32), (0, 0, 0), 1.0, color)
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)
    # an unobserved volume is empty too
    tsdf, _, _ = TH.smooth_field((5, 7, 9))
    v, f, _ = _extract(tsdf, np.zeros((5, 7, 9), dtype=np.float32), (0, 0, 0), 1.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_sphere_properties_of_the_device_mesh():
    n = 20
    tsdf, weight, centre, radius = TH.sphere_field(n)
    v, f, _ = _extract(tsdf, weight, (0.0, 0.0, 0.0), 1.0)
    r = TH.sphere_report(n, v, f, centre, radius)
    print(f"  sphere {n}^3 on the device: {len(v)} vertices, {len(f)} faces, {r}")
    assert r["directed_max"] == 1 and r["undirected_min"] == 2 and r["undirected_max"] == 2 and r["euler"] == 2
    assert abs(r["volume_ratio"] - 1.0) <= 0.01 and abs(r["area_ratio"] - 1.0) <= 0.01 and r["volume_ratio"] > 0
    assert r["radial_max"] <= 0.11 and r["referenced"]


# ---- robustness ---------------------------------------------------------------------------------------------------------
_CELL_DIMS, _CELL_V = (BX + 1, BY + 1, BZ + 1), C + 1


def _cell(put):
    """integrate (fused) and extract a sphere's mesh with colours on whatever stream is current"""
    from gaussianeditor_amd import filter3d as F3
    from gaussianeditor_amd import tsdf as T

    case = TH.integrate_case(_CELL_DIMS, _CELL_V)
    vol = _volume(case)
    rec, f_max = F3.camera_records(case["cameras"])
    _integrate(vol, case, 3.0, cameras=F3.PackedCameras(put(torch.from_numpy(rec)), f_max), put=put)
    tsdf, weight, _, _ = TH.sphere_field(20)
    color = TH.smooth_field((20, 20, 20))[2]
    v, f, c = T.extract_mesh(put(torch.tensor(tsdf)), put(torch.tensor(weight)), (0.5, 0.25, -1.0), 0.125, put(torch.tensor(color)))
    return dict(tsdf=vol.tsdf, weight=vol.weight, color=vol.color, vertices=v, faces=f, colors=c), None


def _plain_put(t):
    return t.detach().to(DEV)


def test_the_same_bits_on_two_runs_and_on_a_side_stream():
    det, _ = _cell(_plain_put)
    torch.cuda.synchronize()
    want = SO.host(det)
    det, _ = _cell(_plain_put)
    torch.cuda.synchronize()
    again = SO.host(det)
    assert again.keys() == want.keys() and all(SO.same_bits(again[k], want[k]) for k in want)
    out, side = SO.run_cell(_cell, SO.SLEEP_FLOOR_MS, allocator=lambda: GuardedAllocator(0x5A))
    v = SO.verdict(out[0], want, side)
    print(f"  tsdf cell: {v}; {SO.report(side)}")
    assert v == "clean"
    ref = TH.run_case_ref(TH.integrate_case(_CELL_DIMS, _CELL_V), 3.0)
    assert np.array_equal(want["tsdf"].view(np.int32), ref[0].view(np.int32)) and len(want["faces"]) > 1000


@pytest.mark.parametrize("dims,V", [((BX + 1, BY + 1, BZ + 1), C + 1), ((5, 7, 9), 2), ((1, 1, 1), 1)], ids=["blocks", "5x7x9", "1x1x1"])
def test_every_buffer_keeps_its_guard_bands(dims, V):
    """The volume, the images, the camera table, the mesh workspace and the mesh between bands of 0xFF (NaN as float32, -1 as
    int32): the bands stay, and no output element keeps its poison."""
    from gaussianeditor_amd import filter3d as F3
    from gaussianeditor_amd import tsdf as T

    case = TH.integrate_case(dims, V)
    rec, f_max = F3.camera_records(case["cameras"])
    field = TH.sphere_field(20)[:2] + (TH.smooth_field((20, 20, 20))[2],) if V > 2 else TH.smooth_field((5, 7, 9))
    with GuardedAllocator(0xFF, device=torch.device(DEV, torch.cuda.current_device())) as ga:
        vol = _volume(case)
        _integrate(vol, case, 3.0, cameras=F3.PackedCameras(ga.place(torch.from_numpy(rec)), f_max), put=ga.place)
        v, f, c = T.extract_mesh(*(ga.place(torch.tensor(a)) for a in field[:2]), (0.0, 0.0, 0.0), 1.0, ga.place(torch.tensor(field[2])))
        ga.assert_clean()
        # the volume's three tensors; depth, alpha, image, cameras; tsdf, weight, colour; workspace, vertices, faces, colours
        assert len(ga) >= 3 + 4 + 3 + 4
    _assert_state("guarded integrate", vol, TH.run_case_ref(case, 3.0))
    got = (v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy())
    _assert_mesh("guarded extract", got, TH.extract_ref(field[0], field[1], (0.0, 0.0, 0.0), 1.0, field[2]))
    assert len(f) > 50 and not np.isnan(got[0]).any() and not np.isnan(got[2]).any() and int(got[1].min()) >= 0


# ---- end to end ---------------------------------------------------------------------------------------------------------
class _Model:
    def __init__(self, sc):
        d = lambda t: t.to(DEV).clone().contiguous()  # noqa: E731
        self._xyz, self._features, self._rotation = d(sc["xyz"]), d(sc["features"]), d(sc["rotation"])
        self._scaling, self._opacity = d(sc["scaling"]), d(sc["opacity"])
        self.active_sh_degree = self.max_sh_degree = 3

    get_xyz = property(lambda s: s._xyz)
    get_features = property(lambda s: s._features)
    get_opacity = property(lambda s: s._opacity)
    get_scaling = property(lambda s: s._scaling)
    get_rotation = property(lambda s: s._rotation)


def test_render_then_fuse_then_mesh_end_to_end():
    """4 000 Gaussians on the unit sphere, 8 ring cameras at 64 x 64: render with alpha -> integrate_renders into 32^3 ->
    extract_mesh.  Equal to the restatement fed the same images, and not empty.  The radial error of the vertices is printed,
    not asserted: it depends on the splats."""
    import types

    from gaussianeditor_amd import tsdf as T
    from gaussianeditor_amd.gaussian_renderer import render
    from gaussianeditor_amd.synth import ring_cameras, synth_scene

    H = W = 64
    sc = synth_scene(4000, seed=11, s0=0.05)
    sc["xyz"] = torch.nn.functional.normalize(sc["xyz"] + 1e-3, dim=-1).contiguous()
    sc["opacity"] = torch.full_like(sc["opacity"], 0.95)
    cams = ring_cameras(8, W, H)
    model = _Model(sc)
    pipe = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        pkgs = [render(c.to(DEV), model, pipe, bg, return_alpha=True) for c in cams]
    n, lo, hi = 32, -1.5, 1.5
    vs = (hi - lo) / (n - 1)
    vol = T.TSDFVolume((lo, lo, lo), vs, (n, n, n), 4.0 * vs, device=DEV)
    vol.integrate_renders(pkgs, cams)
    v, f, c = vol.extract_mesh()
    torch.cuda.synchronize()
    stack = lambda k: torch.stack([p[k] for p in pkgs]).float().cpu().numpy()  # noqa: E731
    state = TH.integrate_ref(TH.fresh((n, n, n)), (lo, lo, lo), vs, cams, 4.0 * vs, stack("depth_3dgs"), stack("alpha"), stack("render"))
    _assert_state("end to end", vol, state)
    want = TH.extract_ref(state[0], state[1], (lo, lo, lo), vs, state[2])
    _assert_mesh("end to end", (v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy()), want)
    assert len(f) > 500 and len(v) > 250
    radial = np.abs(np.linalg.norm(v.cpu().numpy().astype(np.float64), axis=1) - 1.0)
    print(f"  end to end: {len(v)} vertices, {len(f)} faces; radial error of the vertices against the unit sphere: median "
          f"{np.median(radial):.4f}, largest {radial.max():.4f} (voxel {vs:.4f}); not asserted")
