"""-m gpu: the PRODUCT's backward directly against float64 autograd on every case of the regime matrix (tests/f64_regimes.py),
not routed through the oracle, through every backward route that takes the case:
  * the L1 GaussianRasterizer (all cases, precomputed colours / covariances included; the depth route for `depth`);
  * render_view_grads into a GradBucket with sh_exchange="direct", with "rgb" (the SH gradient rebuilt from the colour
    gradient by gsr_sh_grad_compose) and with persistent_rows=True (a second backward over rows an earlier view left zero).
Gradient buffers are poisoned with NaN (or the allocator's cache is) before each backward, so that an entry the backward
forgets to write fails the comparison instead of passing on a lucky zero."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import f64_regimes as R
from helpers import assert_grads_close, settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUCKET_KEYS = dict(means3D="dL_dmeans3D", sh="dL_dsh", opacities="dL_dopacity", scales="dL_dscales", rotations="dL_drotations",
                   means2D="dL_dmeans2D")


@functools.lru_cache(maxsize=None)
def _expectation(name, camera=None):
    """-> (regime, float32 oracle forward, float64 gradients, render_f64 stats, masked rows): computed once per case (and
    per camera of camera_cases.CAMERAS; None: the case's ring camera)."""
    from oracle import cpu

    cpu.build()
    r = R.regime(name, camera=camera)
    f, _ = R.oracle_run(cpu, r)
    want, stats, _ = R.f64_run(f, r)
    masked, report = R.masked_rows(r, f, stats)
    print(f"[{name}{'' if camera is None else ', ' + camera}] {report}")
    return r, f, want, stats, masked


def _poison_allocator(nbytes):
    """Leave a NaN-filled block of `nbytes` in the caching allocator's pool: a torch.empty of that size in the backward
    (the binding's dL_dsh) is then handed NaNs rather than whatever zeros a fresh block may hold."""
    t = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    del t


def _l1(r):
    """Product gradients through GaussianRasterizer (and, for the depth case, of <G, C> + <GD, D> with the depth flag)."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    case = r["case"]
    sc = case["sc"]
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)  # noqa: E731
    xyz, op = leaf(sc["xyz"]), leaf(sc["opacity"])
    m2d = torch.zeros_like(xyz, requires_grad=True)
    kw, leaves = {}, dict(dL_dmeans3D=xyz, dL_dopacity=op, dL_dmeans2D=m2d)
    if r["colors_precomp"] is None:
        kw["shs"] = leaves["dL_dsh"] = leaf(sc["features"])
    else:
        kw["colors_precomp"] = leaves["dL_dcolors"] = leaf(r["colors_precomp"])
    if r["cov3D_precomp"] is None:
        kw["scales"] = leaves["dL_dscales"] = leaf(sc["scaling"])
        kw["rotations"] = leaves["dL_drotations"] = leaf(sc["rotation"])
    else:
        kw["cov3D_precomp"] = leaves["dL_dcov3D"] = leaf(r["cov3D_precomp"])
    flags = options.current_flags() | (options.FLAG_DEPTH_GRAD if r["GD"] is not None else 0)
    with options.override(flags):
        color, radii, depth = GaussianRasterizer(settings(case, DEV, D=r["D"], scale_modifier=r["sm"]))(xyz, m2d, op, **kw)
    loss = (color * r["G"].to(DEV)).sum()
    if r["GD"] is not None:
        loss = loss + (depth * r["GD"].to(DEV)).sum()
    _poison_allocator(xyz.shape[0] * R.M * 3 * 4)
    loss.backward()
    torch.cuda.synchronize()
    return {k: v.grad.cpu().numpy() for k, v in leaves.items()}


def _bucket(r, mode):
    """Product gradients through render_view_grads into a GradBucket: "direct", "rgb" or "persistent" (direct, persistent
    rows, after a first backward of another view into the same bucket)."""
    from gaussianeditor_amd.multiview import GradBucket, allreduce_view_grads, render_view_grads
    from gaussianeditor_amd.synth import look_at_camera

    case = r["case"]
    sc = case["sc"]
    P = sc["xyz"].shape[0]
    args = [sc[k].to(DEV) for k in ("xyz", "opacity", "features", "scaling", "rotation")]
    b = GradBucket(P, R.M, DEV, sh_exchange="rgb" if mode == "rgb" else "direct", persistent_rows=mode == "persistent")
    b._buf.fill_(float("nan"))
    if b.rgb is not None:
        b.rgb.fill_(float("nan"))
    b.invalidate_rows()
    if mode == "persistent":
        # another camera of the same scene first, with a pixel gradient on one corner only: most rows get zeros and are
        # marked as holding them, and the case's own backward then skips rewriting those it does not touch either
        other = look_at_camera([3.0, -1.5, 2.5], [0.0, 0.0, 0.0], case["W"], case["H"])
        rs0 = settings(dict(case, cam=other), DEV, D=r["D"], scale_modifier=r["sm"])
        g0 = torch.zeros(3, case["H"], case["W"], device=DEV)
        g0[:, :32, :48] = 1.0
        render_view_grads(rs0, *args, g0, b)
        assert int((b.row_state == 0).sum()) > 0  # the second backward really runs over rows marked as holding zeros
    rs = settings(case, DEV, D=r["D"], scale_modifier=r["sm"])
    _, _, _, grads = render_view_grads(rs, *args, r["G"].to(DEV), b)
    if mode == "rgb":
        assert allreduce_view_grads(b, None) == "local"
        grads["sh"] = b.views["sh"]
    torch.cuda.synchronize()
    return {BUCKET_KEYS[k]: v.cpu().numpy() for k, v in grads.items()}


def _check(name, route, camera=None):
    r, f, want, stats, masked = _expectation(name, camera)
    got = _l1(r) if route == "l1" else _bucket(r, route)
    assert all(np.isfinite(v).all() for v in got.values()), (name, route, "a gradient entry was never written")
    R.regime_count(r, f, want, stats, got=got)
    worst = assert_grads_close(got, want, tol=R.TOL, tag=f"product[{route}] vs float64 [{name}]", masked=masked,
                               keys=R.grad_keys(r))
    print(f"  product[{route}] vs float64 [{name}]: worst tensor-wide error {worst:.2e}, masked rows {int(masked.sum())}")


@pytest.mark.parametrize("name", R.CASES)
def test_l1_backward_matches_float64(name):
    _check(name, "l1")


@pytest.mark.parametrize("route", ["direct", "rgb", "persistent"])
@pytest.mark.parametrize("name", R.SH_CASES)
def test_view_grads_backward_matches_float64(name, route):
    _check(name, route)


def test_l1_backward_matches_float64_with_forced_list_segments():
    """The L1 cases again in a fresh process with the backward cutting every tile's list into segments that start from the
    forward's checkpoints (GSR_BWD_SEG=1, a checkpoint every 256 list positions; tests/test_gpu_round4.py forces them the
    same way)."""
    env = dict(os.environ, GSR_CK_CHUNKS="4", GSR_BWD_SEG="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "test_l1_backward_matches_float64 and not forced"], capture_output=True, text=True, timeout=900,
                       cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert f"{len(R.CASES)} passed" in p.stdout, p.stdout[-2000:]


# ---------------------------------------------------------------------------------------------------------------------
# reference-derived fixtures (tests/golden/make_golden.py): the 3D covariance and the clamped SH colour of the product
GOLD = os.path.join(ROOT, "tests", "golden")


def test_debug_cov3d_matches_reference_fixture():
    """gsr_debug_cov3d (the covariance K1 and K8+K9 both compute) against the reference's build_scaling_rotation /
    strip_symmetric in float64, scaling_modifier 0.5, 1, 1.7: within 1e-6 of each covariance's largest entry."""
    import ctypes

    from gaussianeditor_amd import _native

    g = np.load(os.path.join(GOLD, "cov3d.npz"))
    L = _native.lib()
    scl, rot = torch.from_numpy(g["scaling"]).to(DEV), torch.from_numpy(g["rotation"]).to(DEV)
    P = scl.shape[0]
    s = torch.cuda.current_stream().cuda_stream
    for i, sm in enumerate(g["modifiers"]):
        out = torch.full((P, 6), float("nan"), device=DEV)
        _native.check("debug_cov3d", L.gsr_debug_cov3d(s, P, scl.data_ptr(), ctypes.c_float(float(sm)), rot.data_ptr(),
                                                       out.data_ptr()))
        torch.cuda.synchronize()
        want = g[f"cov3D_{i}"]
        err = np.abs(out.cpu().numpy().astype(np.float64) - want).max(axis=1) / np.abs(want).max(axis=1)
        print(f"  cov3D at scaling_modifier {float(sm)}: max relative error {err.max():.2e}")
        assert err.max() <= 1e-6, (float(sm), float(err.max()))


def test_k1_rgb_and_clamped_match_reference_fixture():
    """K1's exported rgb / clamped (tests/helpers.py hip_state) against clamp_min(eval_sh + 0.5, 0) of the reference's
    renderer, degrees 0..3 with 16 coefficients: rgb within 1e-6 of the largest channel, flags equal except where
    |rgb + 0.5| < 1e-6."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C
    from gaussianeditor_amd.synth import look_at_camera
    from helpers import hip_state

    g = np.load(os.path.join(GOLD, "sh_clamped.npz"))
    shs, dirs = torch.from_numpy(g["shs"]), torch.from_numpy(g["dirs"])
    P, W, H = shs.shape[0], 64, 64
    cam = look_at_camera([0.0, 0.0, -10.0], [0.0, 0.0, 0.0], W, H, fovy_deg=60.0)
    tf = float(np.tan(cam.FoVy / 2))
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    e = torch.empty(0, device=DEV)
    for deg in range(4):
        R_, _, _, radii, geom, binning, img = _C.rasterize_gaussians(
            d(torch.tensor([0.1, 0.2, 0.3])), d(dirs * 3.0), e, d(torch.full((P, 1), 0.5)), d(torch.full((P, 3), 0.01)),
            d(torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1)), 1.0, e, d(cam.world_view_transform), d(cam.full_proj_transform),
            tf, tf, H, W, d(shs), deg, d(torch.zeros(3)), False, False)
        st = hip_state(P, R_, W, H, geom, binning, img)
        assert (radii > 0).all()
        ref, raw = g[f"rgb_clamped_deg{deg}"], g[f"rgb_deg{deg}"] + 0.5
        assert np.abs(st["rgb"] - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())
        differ = st["clamped"].astype(bool) != (raw < 0)
        print(f"  degree {deg}: clamped channels {int((raw < 0).sum())}, flags that differ {int(differ.sum())}")
        assert not differ.any() or np.abs(raw[differ]).max() < 1e-6
