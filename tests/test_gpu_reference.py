"""-m gpu: parity against THE REFERENCE ITSELF -- its own .cu sources compiled for gfx950
(oracle/_ref, built by oracle/ref_build/Makefile in the dev container; the .so files travel to the
GPU box).  Two roles:
  1. pin the CPU oracle: oracle == reference(-ffp-contract=off) bit-for-bit on every integer/index
     output and on the per-Gaussian floats; images within the expf difference (the reference calls the
     device libm exp, the oracle the exactly specified gsr_expf);
  2. pin the product: HIP path vs the reference in its natural (FMA-contracting) build.
"""
import numpy as np
import pytest
import torch

from helpers import hip_state, make_case, oracle_forward, rel_err, seed_gradient, settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ref(variant):
    from helpers import require_ref

    return require_ref(variant).Reference(variant, DEV)


def _ref_forward(R, case, **kw):
    sc, cam = case["sc"], case["cam"]
    return R.forward(sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], sc["features"], None, None,
                     cam.world_view_transform, cam.full_proj_transform, cam.camera_center, case["bg"], case["W"], case["H"],
                     case["tfx"], case["tfy"], 1.0, case["D"])


def _np(t):
    return t.detach().cpu().numpy()


CASES = [(10000, 256, 256, 0.03, 1), (3000, 250, 131, 0.05, 2), (20000, 512, 512, 0.02, 4)]


@pytest.mark.parametrize("P,W,H,s0,seed", CASES)
def test_oracle_is_pinned_by_reference_nofma(oracle, P, W, H, s0, seed):
    _check_oracle_is_pinned(oracle, make_case(P, W, H, seed=seed, s0=s0))


def _check_oracle_is_pinned(oracle, case):
    f = oracle_forward(oracle, case)
    r = _ref_forward(_ref("nofma"), case)
    vis = f["radii"] > 0
    # integers / indices: bit exact
    assert r["num_rendered"] == f["num_rendered"]
    assert np.array_equal(_np(r["radii"]), f["radii"])
    assert np.array_equal(_np(r["tiles_touched"]).view(np.uint32), f["tiles_touched"])
    assert np.array_equal(_np(r["point_offsets"]).view(np.uint32), f["point_offsets"])
    assert np.array_equal(_np(r["keys"]).view(np.uint64), f["keys"])
    assert np.array_equal(_np(r["point_list"]).view(np.uint32), f["point_list"])
    assert np.array_equal(_np(r["ranges"]).view(np.uint32), f["ranges"])
    assert np.array_equal(_np(r["clamped"])[vis], f["clamped"][vis])
    # per-Gaussian floats: same IEEE operations in the same order => bit exact
    for k in ("means2D", "depths", "cov3D", "conic_opacity", "rgb"):
        assert np.array_equal(_np(r[k])[vis], f[k][vis]), k
    # images: the reference's exp is the device libm's, ours the specified polynomial (<= 3e-7 apart);
    # discrete per-pixel decisions can flip only where a value sits within that distance of a threshold
    nc_ref = _np(r["n_contrib"]).view(np.uint32)
    mism = float((nc_ref != f["n_contrib"]).mean())
    dc = np.abs(_np(r["color"]) - f["color"])
    print(f"n_contrib mismatch fraction {mism:.2e}; colour max diff {dc.max():.2e}, p99.99 {np.quantile(dc, 0.9999):.2e}")
    assert mism < 1e-3
    assert np.quantile(dc, 0.9999) <= 1e-5
    assert dc.max() < 1e-2  # a flipped 1/255 decision moves a pixel by at most alpha * T * colour


@pytest.mark.parametrize("P,W,H,s0,seed", CASES)
def test_product_vs_reference_fma(P, W, H, s0, seed):
    """The HIP path against the reference as hipcc builds it by default (contraction on)."""
    _check_product_vs_reference_fma(make_case(P, W, H, seed=seed, s0=s0), seed)


def _check_product_vs_reference_fma(case, seed):
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    sc, P, W, H = case["sc"], case["sc"]["xyz"].shape[0], case["W"], case["H"]
    r = _ref_forward(_ref("fma"), case)
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)  # noqa: E731
    xyz, op, sh, scl, rot = leaf(sc["xyz"]), leaf(sc["opacity"]), leaf(sc["features"]), leaf(sc["scaling"]), leaf(sc["rotation"])
    m2d = torch.zeros_like(xyz, requires_grad=True)
    color, radii, depth = GaussianRasterizer(settings(case, DEV))(xyz, m2d, op, shs=sh, scales=scl, rotations=rot)
    rad_mism = int((radii != r["radii"]).sum())
    dc = (color.detach() - r["color"]).abs()
    print(f"radii differing (FMA contraction in the reference build): {rad_mism}/{P}; R {r['num_rendered']}; "
          f"colour max {float(dc.max()):.2e} p99.99 {float(torch.quantile(dc.flatten()[:4_000_000], 0.9999)):.2e}")
    assert rad_mism <= max(2, P // 2000)
    assert float(torch.quantile(dc.flatten()[:4_000_000], 0.9999)) <= 1e-5
    # depth image (forward.cu:359, 377), same bar as the colour: the FMA build flips a few threshold decisions
    dd = (depth.detach() - r["depth"]).abs().flatten() / max(1.0, float(r["depth"].abs().max()))
    print(f"depth max {float(dd.max()):.2e} p99.99 {float(torch.quantile(dd[:4_000_000], 0.9999)):.2e}")
    assert float(torch.quantile(dd[:4_000_000], 0.9999)) <= 1e-5
    assert float(dd.max()) < 1e-2
    # gradients
    G = (seed_gradient(H, W, seed) * (H * W)).to(DEV)
    (color * G).sum().backward()
    g = _ref("fma")
    g.forward(sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], sc["features"], None, None,
              case["cam"].world_view_transform, case["cam"].full_proj_transform, case["cam"].camera_center, case["bg"], W, H,
              case["tfx"], case["tfy"], 1.0, 3)
    gr = g.backward(G)
    for name, t in (("dL_dmeans3D", xyz), ("dL_dopacity", op), ("dL_dsh", sh), ("dL_dscales", scl),
                    ("dL_drotations", rot), ("dL_dmeans2D", m2d)):
        a, b = _np(t.grad).astype(np.float64), _np(gr[name]).reshape(t.shape).astype(np.float64)
        scale = np.abs(b).max()
        err = np.abs(a - b) / scale
        l2 = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        print(f"{name}: max {err.max():.2e}  p99.9 {np.quantile(err, 0.999):.2e}  rel-L2 {l2:.2e}")
        # The reference build contracts a*b+c into FMAs, the product does not: where a pixel's alpha or
        # transmittance sits within one rounding of a threshold (1/255, 1e-4) the two builds take different
        # branches and that pixel's contribution moves by O(alpha).  Such flips are rare (see the colour
        # statistics above); everything else agrees to ~1e-6.
        assert np.quantile(err, 0.999) <= 1e-5, name
        assert l2 <= 1e-3 and err.max() <= 5e-3, name


def test_product_vs_reference_nofma_integers():
    """Against the contraction-free reference build the product's integer outputs are bit-exact."""
    _check_product_vs_reference_nofma_integers(make_case(20000, 512, 512, seed=4, s0=0.02))


def _check_product_vs_reference_nofma_integers(case):
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    sc, cam, P, W, H = case["sc"], case["cam"], case["sc"]["xyz"].shape[0], case["W"], case["H"]
    r = _ref_forward(_ref("nofma"), case)
    e = torch.empty(0, device=DEV)
    d = lambda t: t.to(DEV)  # noqa: E731
    R, color, depth, radii, geom, binning, img = _C.rasterize_gaussians(
        d(case["bg"]), d(sc["xyz"]), e, d(sc["opacity"]), d(sc["scaling"]), d(sc["rotation"]), 1.0, e,
        d(cam.world_view_transform), d(cam.full_proj_transform), case["tfx"], case["tfy"], H, W, d(sc["features"]), 3,
        d(cam.camera_center), False, False)
    st = hip_state(P, R, W, H, geom, binning, img)
    assert R == r["num_rendered"]
    assert torch.equal(radii, r["radii"])
    assert np.array_equal(st["keys"], _np(r["keys"]).view(np.uint64))
    assert np.array_equal(st["point_list"], _np(r["point_list"]).view(np.uint32))
    assert np.array_equal(st["ranges"], _np(r["ranges"]).view(np.uint32))


@pytest.mark.parametrize("P,W,H,s0,C,big", [(6000, 256, 256, 0.04, 1, False), (20000, 512, 512, 0.02, 3, False),
                                            (20000, 512, 512, 0.02, 2, False), (1_000_000, 1920, 1088, 0.01, 1, True),
                                            # the exact workload of bench.py's C3 / C5 entries (round 6): 1 M Gaussians through the
                                            # editor's 512 x 512 image, SPLIT items + list segments together
                                            (1_000_000, 512, 512, 0.01, 1, True)])
def test_apply_weights_vs_reference(oracle, P, W, H, s0, C, big):
    """K11+K12 against the reference's own apply_weights.cu (contraction-free build), C = 1, 2, 3 and at the headline size
    (1088 rows: the reference reads image_weights out of bounds unless both sides are multiples of 16).  `cnt` is an
    integer per Gaussian: it must be IDENTICAL except for the Gaussians blended at a pixel whose threshold decision
    differs between libm's exp (reference) and gsr_expf (here) -- those pixels are found by comparing the two forward
    renders' n_contrib / final_T, counted and bounded; the float weights agree to the atomics' re-association."""
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer
    from helpers import flipped_pixels as _flipped_pixels, gaussians_under as _gaussians_under

    case = make_case(P, W, H, seed=11 if not big else 0, s0=s0, view=0, nviews=8 if big else 4,
                     bg=(0.0, 0.0, 0.0))
    sc, cam = case["sc"], case["cam"]
    mask = (torch.rand(C, H, W, generator=torch.Generator().manual_seed(12)) > 0.5).float()  # 0 / 1: exact sums
    R_ = _ref("nofma")
    w_ref = torch.zeros((P, C), device=DEV)
    c_ref = torch.zeros((P,), dtype=torch.int32, device=DEV)
    R_.apply_weights(sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], cam.world_view_transform,
                     cam.full_proj_transform, cam.camera_center, W, H, case["tfx"], case["tfy"], mask, w_ref, c_ref)
    w = torch.zeros((P, C), device=DEV)
    cnt = torch.zeros((P, 1), dtype=torch.int32, device=DEV)
    GaussianRasterizer(settings(case, DEV, D=0)).apply_weights(sc["xyz"].to(DEV), None, sc["opacity"].to(DEV), None, w,
                                                             sc["scaling"].to(DEV), sc["rotation"].to(DEV), None, cnt,
                                                             mask.to(DEV))
    torch.cuda.synchronize()
    # where may the two differ at all?  pixels whose blend decisions flip between the two exps
    r = _ref_forward(_ref("nofma"), case)
    f = oracle_forward(oracle, case)
    flips = _flipped_pixels(_np(r["n_contrib"]).view(np.uint32), _np(r["final_T"]), f["n_contrib"], f["final_T"])
    masked = _gaussians_under(flips, W, f, _np(r["n_contrib"]).view(np.uint32))
    diff = _np(cnt).reshape(-1) != _np(c_ref)
    print(f"[{P} @ {W}x{H}, C={C}] flipped pixels {flips.size}, Gaussians under them {int(masked.sum())}; cnt differs on "
          f"{int(diff.sum())} Gaussians ({int((diff & ~masked).sum())} outside them); total {int(c_ref.sum())}")
    assert flips.size <= 4 + 2e-4 * W * H
    assert not (diff & ~masked).any()
    assert np.abs(_np(cnt).reshape(-1).astype(np.int64) - _np(c_ref).astype(np.int64))[masked].max(initial=0) <= 4 * C
    dw = (w - w_ref).abs().cpu().numpy()
    assert dw[~masked].max(initial=0.0) <= 1e-5 * max(1.0, float(w_ref.abs().max()))


@pytest.mark.parametrize("P,kind", [(5000, "uniform"), (200000, "uniform"), (100000, "clustered")])
def test_knn_vs_reference_simple_knn(P, kind):
    """distCUDA2 against the reference's own simple_knn.cu compiled for gfx950: bit-identical to the contraction-free
    build (both round dx*dx + dy*dy + dz*dz operation by operation), within one rounding of the default (FMA) build."""
    from gaussianeditor_amd.simple_knn._C import distCUDA2
    from helpers import require_ref

    R = require_ref("nofma", knn=True)
    g = torch.Generator().manual_seed(P)
    pts = torch.rand(P, 3, generator=g) * 2 - 1
    if kind == "clustered":
        pts = pts * 0.01 + torch.randint(0, 5, (P, 3), generator=g).float()
    pts = pts.to(DEV)
    mine = distCUDA2(pts)
    ref_nofma = R.knn_mean_dist2(pts, "nofma")
    assert torch.equal(mine, ref_nofma)
    if R.knn_available("fma"):
        ref_fma = R.knn_mean_dist2(pts, "fma")
        rel = ((mine - ref_fma).abs() / ref_fma.abs().clamp_min(1e-30)).max()
        assert float(rel) <= 1e-6
