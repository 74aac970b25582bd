"""-m gpu: antialiased rendering (GSR_FLAG_ANTIALIAS) of the product.

  1. the forward under the flag IS the plain forward at the effective opacities rec0.w, bit for bit, in both tile-bound
     modes; rec0.w agrees with float64 opacity * h;
  2. the flag changes the picture where it should (sub-pixel Gaussians), and keeps a sparse scene's mass across resolutions;
  3. the backward matches float64 autograd of render_f64(opacities = o * h) on every case of the regime matrix
     (tests/f64_regimes.py) and on three regimes of its own (tests/aa_helpers.py), also with forced list segments;
  4. the same through the direct, rgb and persistent-rows GradBucket routes;
  5. view reuse serves an antialiased override render only from an antialiased full render;
  6. apply_weights under the flag is apply_weights of the plain render at rec0.w;
  7. the accumulator table kept across backwards is zero again after antialiased backwards."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import aa_helpers as A
import f64_regimes as R
from helpers import assert_grads_close, hip_state, oracle_forward, rel_err, settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = R.CASES + A.NEW_CASES


def _aa():
    from gaussianeditor_amd import options

    return options.FLAG_ANTIALIAS


def _render(case, flags, opacity=None, D=3, colors_precomp=None, cov3D_precomp=None, sm=1.0):
    """_C.rasterize_gaussians of a case -> (R, color, depth, radii, geom, binning, img)."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    sc, cam = case["sc"], case["cam"]
    d = lambda t: torch.as_tensor(t).to(DEV).contiguous()  # noqa: E731
    e = torch.empty(0, device=DEV)
    op = sc["opacity"] if opacity is None else torch.as_tensor(opacity, dtype=torch.float32).reshape(-1, 1)
    return _C.rasterize_gaussians(
        d(case["bg"]), d(sc["xyz"]), e if colors_precomp is None else d(colors_precomp), d(op),
        e if cov3D_precomp is not None else d(sc["scaling"]), e if cov3D_precomp is not None else d(sc["rotation"]), sm,
        e if cov3D_precomp is None else d(cov3D_precomp), d(cam.world_view_transform), d(cam.full_proj_transform),
        case["tfx"], case["tfy"], case["H"], case["W"], d(sc["features"]) if colors_precomp is None else e, D,
        d(cam.camera_center), False, False, flags=flags)


def _rec0w(case, flags=0, **kw):
    """The product's effective opacities (rec0.w of the geometry state; 0 for Gaussians binned into no tile)."""
    R_, _, _, _, geom, binning, img = _render(case, flags | _aa(), **kw)
    P = case["sc"]["xyz"].shape[0]
    return hip_state(P, R_, case["W"], case["H"], geom, binning, img)["conic_opacity"][:, 3].copy()


# ---- 1. forward identity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", ["reference", "alpha"])
@pytest.mark.parametrize("name", ["sub_pixel", "floor", "off_cone"])
def test_forward_is_the_plain_forward_at_rec0w(name, bounds):
    _check_forward_at_rec0w(name, bounds)


def _check_forward_at_rec0w(name, bounds, camera=None):
    from gaussianeditor_amd import options

    r = A.regime(name, camera=camera)
    case = r["case"]
    P, W, H = case["sc"]["xyz"].shape[0], case["W"], case["H"]
    tb = options.FLAG_TILE_BOUNDS_ALPHA if bounds == "alpha" else 0
    out_aa = _render(case, tb | _aa())
    st_aa = hip_state(P, out_aa[0], W, H, *out_aa[4:])
    ow = st_aa["conic_opacity"][:, 3].copy()
    out_pl = _render(case, tb, opacity=ow)
    st_pl = hip_state(P, out_pl[0], W, H, *out_pl[4:])
    assert out_aa[0] == out_pl[0]
    for i, what in ((1, "image"), (2, "depth"), (3, "radii")):
        assert torch.equal(out_aa[i], out_pl[i]), what
    for k in ("n_contrib", "final_T", "point_list", "conic_opacity", "means2D", "depths", "rgb"):
        assert np.array_equal(st_aa[k], st_pl[k]), k
    # rec0.w against float64 o * h (reference bounds: every visible Gaussian has a record)
    if bounds == "reference":
        h, ratio, x, y, z = A.h_of_case(case)
        vis = out_aa[3].cpu().numpy() > 0
        want = case["sc"]["opacity"].double().numpy().reshape(-1) * h
        det = x * y - z * z
        cond = np.where(det > 0, x * y / np.maximum(det, 1e-300), np.inf)  # how much float32's x y - z^2 amplifies rounding
        rel = np.abs(ow.astype(np.float64) - want) / np.abs(want)
        # float32 K1: x, y, z within a few ulp of float64, then x y - z^2 (its rounding amplified by cond), one division, a
        # square root.  Well-conditioned footprints (cond <= 20): 1e-5.  The others: the same error scaled by cond,
        # 1e-5 + 2e-6 cond, above the floor; on the floor h is a constant.  Counted, bounded, and h stays in [floor, 1].
        good = vis & (cond <= 20)
        assert rel[good].max() <= 1e-5, float(rel[good].max())
        rest = vis & ~good & (ratio > 2 * A.FLOOR)
        assert np.all(rel[rest] <= 1e-5 + 2e-6 * cond[rest]), float((rel[rest] / (1e-5 + 2e-6 * cond[rest])).max())
        print(f"  [{name}] rec0.w vs float64: {int(good.sum())} rows within {rel[good].max():.1e}, {int(rest.sum())} "
              f"worse-conditioned rows (max rel {rel[rest].max() if rest.any() else 0:.1e})")
        o = case["sc"]["opacity"].numpy().reshape(-1)
        assert np.all(ow[vis] <= o[vis] * 1.000001) and np.all(ow[vis] >= o[vis] * 0.999 * np.sqrt(A.FLOOR))


# ---- 2. the flag changes the picture --------------------------------------------------------------------------------
def test_antialiasing_changes_sub_pixel_images_and_keeps_their_mass():
    r = A.regime("sub_pixel")
    plain, aa = _render(r["case"], 0)[1], _render(r["case"], _aa())[1]
    diff = float((plain - aa).abs().max())
    assert diff > 0.05, diff
    # the intent check of test_cpu_antialias on the product: a sparse sub-pixel scene's mass at 1/4 resolution
    cov = {}
    for flags in (0, _aa()):
        for W in (512, 128):
            c = A.sparse_case(W, W)
            cols = torch.ones(c["sc"]["xyz"].shape[0], 3)
            out = _render(c, flags, colors_precomp=cols, D=0)
            st = hip_state(c["sc"]["xyz"].shape[0], out[0], W, W, *out[4:])
            cov[flags, W] = A.coverage(st["final_T"], W, W)
    plain_ratio, aa_ratio = cov[0, 128] / cov[0, 512], cov[_aa(), 128] / cov[_aa(), 512]
    print(f"  mass at 1/4 resolution over full resolution: plain {plain_ratio:.3f}, antialiased {aa_ratio:.3f}")
    assert plain_ratio > 3.0
    assert abs(aa_ratio - 1.0) < 0.15


# ---- 3. / 4. backward against float64 autograd ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _expectation(name, camera=None):
    """-> (regime, float32 oracle forward at the product's rec0.w, float64 gradients, stats, masked rows)."""
    from oracle import cpu

    cpu.build()
    r = A.regime(name, camera=camera)
    ow = _rec0w(r["case"], D=r["D"], colors_precomp=r["colors_precomp"], cov3D_precomp=r["cov3D_precomp"], sm=r["sm"])
    sc = dict(r["case"]["sc"], opacity=torch.from_numpy(ow).reshape(-1, 1))
    f = oracle_forward(cpu, dict(r["case"], sc=sc), colors_precomp=r["colors_precomp"], cov3D_precomp=r["cov3D_precomp"],
                       D=r["D"], scale_modifier=r["sm"])
    want, stats, _, geom = A.f64_run_aa(f, r)
    masked, counts = A.masked_rows_aa(r, f, stats, geom)
    print(f"[{name}] masked rows: {counts}")
    return r, f, want, stats, masked, geom


def _check(name, route, camera=None):
    from gaussianeditor_amd import options
    from test_gpu_f64_regimes import _bucket, _l1

    r, f, want, stats, masked, geom = _expectation(name, camera)
    with options.override(options.current_flags() | _aa()):
        got = _l1(r) if route == "l1" else _bucket(r, route)
    assert all(np.isfinite(v).all() for v in got.values()), (name, route, "a gradient entry was never written")
    if A.aa_regime_count(r, f, geom) is None:
        R.regime_count(r, f, want, stats, got=got)
    worst = assert_grads_close(got, want, tol=R.TOL, tag=f"antialiased product[{route}] vs float64 [{name}]", masked=masked,
                               keys=R.grad_keys(r))
    print(f"  antialiased product[{route}] vs float64 [{name}]: worst tensor-wide error {worst:.2e}, "
          f"masked rows {int(masked.sum())}")


@pytest.mark.parametrize("name", ALL_CASES)
def test_l1_backward_antialiased_matches_float64(name):
    _check(name, "l1")


@pytest.mark.parametrize("route", ["direct", "rgb", "persistent"])
@pytest.mark.parametrize("name", ["sub_pixel", "floor", "off_cone", "sh_D1"])
def test_view_grads_backward_antialiased_matches_float64(name, route):
    _check(name, route)


def test_l1_backward_antialiased_matches_float64_with_forced_list_segments():
    """The edit view and the sub-pixel case again in a fresh process whose backward cuts every tile's list into segments
    that start from the forward's checkpoints (GSR_BWD_SEG=1, a checkpoint every 256 list positions)."""
    env = dict(os.environ, GSR_CK_CHUNKS="4", GSR_BWD_SEG="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "test_l1_backward_antialiased_matches_float64 and not forced and (edit_view or sub_pixel)"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "2 passed" in p.stdout, p.stdout[-2000:]


# ---- 5. view reuse --------------------------------------------------------------------------------------------------
def test_view_reuse_serves_antialiased_renders_only_from_antialiased_ones():
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer, _reuse

    r = A.regime("sub_pixel")
    case = r["case"]
    sc = case["sc"]
    rs = settings(case, DEV)
    d = {k: sc[k].to(DEV) for k in ("xyz", "opacity", "features", "scaling", "rotation")}
    m2d = torch.zeros_like(d["xyz"])
    over = torch.rand(d["xyz"].shape[0], 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    rast = GaussianRasterizer(rs)

    def full(flags):
        with options.override(flags), torch.no_grad():
            return rast(d["xyz"], m2d, d["opacity"], shs=d["features"], scales=d["scaling"], rotations=d["rotation"])

    def override(flags):
        with options.override(flags), torch.no_grad():
            return rast(d["xyz"], m2d, d["opacity"].clone(), colors_precomp=over, scales=d["scaling"].clone(),
                        rotations=d["rotation"].clone())
    was = _reuse.view_reuse()
    try:
        _reuse.set_view_reuse(True)
        full(_aa())
        h0 = _reuse.stats["hits"]
        served = override(_aa())
        assert _reuse.stats["hits"] == h0 + 1
        _reuse.set_view_reuse(False)
        whole = override(_aa())
        for a, b in zip(served, whole):
            assert torch.equal(a, b)
        _reuse.set_view_reuse(True)
        # mixing the flag misses, both ways
        for first, second in ((_aa(), 0), (0, _aa())):
            full(first)
            h0, m0 = _reuse.stats["hits"], _reuse.stats["misses"]
            override(second)
            assert _reuse.stats["hits"] == h0 and _reuse.stats["misses"] == m0 + 1
    finally:
        _reuse.set_view_reuse(was)


# ---- 6. apply_weights -----------------------------------------------------------------------------------------------
def test_apply_weights_antialiased_is_apply_weights_at_rec0w():
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    r = A.regime("sub_pixel")
    case = r["case"]
    sc = case["sc"]
    P, W, H = sc["xyz"].shape[0], case["W"], case["H"]
    rs = settings(case, DEV)
    ow = torch.from_numpy(_rec0w(case)).reshape(-1, 1).to(DEV)
    mask = torch.rand(1, H, W, generator=torch.Generator().manual_seed(9)).to(DEV)
    res = {}
    for tag, flags, op in (("aa", _aa(), sc["opacity"].to(DEV)), ("plain", 0, ow)):
        wts = torch.zeros(P, 1, device=DEV)
        cnt = torch.zeros(P, dtype=torch.int32, device=DEV)
        with options.override(flags):
            GaussianRasterizer(rs).apply_weights(sc["xyz"].to(DEV), torch.zeros(P, 3, device=DEV), op,
                                                 scales=sc["scaling"].to(DEV), rotations=sc["rotation"].to(DEV),
                                                 weights=wts, cnt=cnt, image_weights=mask)
        torch.cuda.synchronize()
        res[tag] = (wts.cpu().numpy(), cnt.cpu().numpy())
    assert np.array_equal(res["aa"][1], res["plain"][1])
    assert int(res["aa"][1].sum()) > 0
    # (float atomics add the pixels' contributions in another order on every run)
    assert rel_err(res["aa"][0], res["plain"][0]) <= 1e-5


# ---- 7. the kept accumulator table ----------------------------------------------------------------------------------
def test_accumulator_table_is_zero_after_antialiased_backwards():
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    if not _C._ACC_PERSIST:
        pytest.skip("GSR_ACC_PERSIST=0: no table is kept")
    from test_gpu_f64_regimes import _l1

    for name in ("sub_pixel", "floor"):
        with options.override(_aa()):
            _l1(A.regime(name))
            _l1(dict(A.regime(name), GD=R.seed_gradient(A.regime(name)["case"]["H"], A.regime(name)["case"]["W"], 5)[:1]))
    torch.cuda.synchronize()
    assert _C._ACC_TABLES
    for t in _C._ACC_TABLES.values():
        assert float(t.abs().max()) == 0.0
