"""Shared test plumbing: scene setup, oracle runs, and extraction of the HIP path's
intermediate state through the debug-export entry points of the C ABI."""
import math

import numpy as np
import torch

from gaussianeditor_amd.synth import ring_cameras, seed_gradient, synth_scene


def make_case(P, W, H, seed=1, s0=0.03, view=0, nviews=4, sh_degree=3, scale_xyz=1.0, bg=(0.1, 0.2, 0.3), camera=None):
    """`camera`: a name of camera_cases.CAMERAS -- the ring camera with unequal focal lengths, roll and / or an off-centre
    principal axis -- or None for the ring camera itself."""
    sc = synth_scene(P, seed=seed, s0=s0, sh_degree=sh_degree)
    sc["xyz"] = (sc["xyz"] * scale_xyz).contiguous()
    cam = ring_cameras(nviews, W, H)[view]
    tfx, tfy = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    if camera is not None:
        from camera_cases import named_camera

        cam, tfx, tfy = named_camera(camera, cam, W, H)
    case = dict(sc=sc, cam=cam, W=W, H=H, tfx=tfx, tfy=tfy, bg=torch.tensor(bg, dtype=torch.float32), D=sh_degree)
    return case


def oracle_forward(O, case, colors_precomp=None, cov3D_precomp=None, D=None, shs=None, scale_modifier=1.0):
    sc, cam = case["sc"], case["cam"]
    shs = sc["features"] if (shs is None and colors_precomp is None) else shs
    return O.forward(sc["xyz"], None if cov3D_precomp is not None else sc["scaling"],
                     None if cov3D_precomp is not None else sc["rotation"], sc["opacity"],
                     None if colors_precomp is not None else shs, colors_precomp, cov3D_precomp,
                     cam.world_view_transform, cam.full_proj_transform, cam.camera_center, case["bg"], case["W"],
                     case["H"], case["tfx"], case["tfy"], scale_modifier, case["D"] if D is None else D)


def oracle_backward(O, case, fwd, G, colors_precomp=None, cov3D_precomp=None, D=None, shs=None, scale_modifier=1.0):
    sc, cam = case["sc"], case["cam"]
    shs = sc["features"] if (shs is None and colors_precomp is None) else shs
    return O.backward(fwd, G, sc["xyz"], None if cov3D_precomp is not None else sc["scaling"],
                      None if cov3D_precomp is not None else sc["rotation"],
                      None if colors_precomp is not None else shs, colors_precomp, cov3D_precomp,
                      cam.world_view_transform, cam.full_proj_transform, cam.camera_center, case["bg"], case["W"],
                      case["H"], case["tfx"], case["tfy"], scale_modifier, case["D"] if D is None else D)


def settings(case, dev, D=None, scale_modifier=1.0, debug=False):
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizationSettings

    cam = case["cam"]
    return GaussianRasterizationSettings(case["H"], case["W"], case["tfx"], case["tfy"], case["bg"].to(dev),
                                         scale_modifier, cam.world_view_transform.to(dev),
                                         cam.full_proj_transform.to(dev), case["D"] if D is None else D,
                                         cam.camera_center.to(dev), False, debug)


def hip_state(P, R, W, H, geom, binning, img, cov_inputs=None):
    """Pull every intermediate out of the opaque scratch buffers (device -> numpy)."""
    from gaussianeditor_amd import _native

    L = _native.lib()
    dev = geom.device
    s = torch.cuda.current_stream(dev).cuda_stream
    T = ((W + 15) // 16) * ((H + 15) // 16)
    f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
    out = dict(means2D=f(P, 2), depths=f(P), cov3D=f(P, 6), rgb=f(P, 3), conic_opacity=f(P, 4),
               tiles_touched=torch.zeros(P, dtype=torch.int32, device=dev),
               clamped=torch.zeros((P, 3), dtype=torch.uint8, device=dev),
               keys=torch.zeros(R, dtype=torch.int64, device=dev),
               point_list=torch.zeros(R, dtype=torch.int32, device=dev),
               ranges=torch.zeros((T, 2), dtype=torch.int32, device=dev), final_T=f(H * W),
               n_contrib=torch.zeros(H * W, dtype=torch.int32, device=dev))
    p = lambda k: out[k].data_ptr()  # noqa: E731
    _native.check("export_geom", L.gsr_debug_export_geom(s, P, geom.data_ptr(), p("means2D"), p("depths"),
                                                         p("rgb"), p("conic_opacity"), p("tiles_touched"), p("clamped")))
    if cov_inputs is not None:  # (scales, rotations, scale_modifier): the 3D covariance both passes compute from them
        import ctypes

        sc_, rot_, mod_ = cov_inputs
        sc_, rot_ = sc_.to(dev).contiguous(), rot_.to(dev).contiguous()
        _native.check("debug_cov3d", L.gsr_debug_cov3d(s, P, sc_.data_ptr(), ctypes.c_float(mod_), rot_.data_ptr(), p("cov3D")))
    else:
        del out["cov3D"]
    if R > 0:
        _native.check("export_binning", L.gsr_debug_export_binning(s, P, R, W, H, geom.data_ptr(), binning.data_ptr(),
                                                                   p("keys"), p("point_list")))
    _native.check("export_image", L.gsr_debug_export_image(s, W, H, img.data_ptr(), p("ranges"), p("final_T"),
                                                           p("n_contrib")))
    torch.cuda.synchronize(dev)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["tiles_touched"] = res["tiles_touched"].view(np.uint32)
    res["keys"] = res["keys"].view(np.uint64)
    res["point_list"] = res["point_list"].view(np.uint32)
    res["ranges"] = res["ranges"].view(np.uint32)
    res["n_contrib"] = res["n_contrib"].view(np.uint32)
    return res


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max())) if a.size else 0.0


def flipped_pixels(nc_a, ft_a, nc_b, ft_b):
    """Pixels whose discrete blend decisions differ between two implementations: a different last contributor, or a
    final transmittance that differs by more than rounding (one skipped / extra alpha >= 1/255 entry moves it by
    >= 0.4 %)."""
    nc_a, nc_b = nc_a.reshape(-1).astype(np.int64), nc_b.reshape(-1).astype(np.int64)
    ft_a, ft_b = ft_a.reshape(-1).astype(np.float64), ft_b.reshape(-1).astype(np.float64)
    rel = np.abs(ft_a - ft_b) / np.maximum(np.maximum(np.abs(ft_a), np.abs(ft_b)), 1e-30)
    return np.nonzero((nc_a != nc_b) | (rel > 1e-4))[0]


def gaussians_under(pixels, W, f, nc_other):
    """Mask of the Gaussians that are blended at one of `pixels` (flat indices) by either implementation: the entries
    of the pixel's tile list up to its last contributor whose alpha there reaches the threshold (with some slack)."""
    P = f["radii"].shape[0]
    mask = np.zeros(P, bool)
    gx = (W + 15) // 16
    nc_a, nc_b = f["n_contrib"].reshape(-1), np.asarray(nc_other).reshape(-1)
    for p in pixels.tolist():
        px, py = p % W, p // W
        lo, hi = (int(v) for v in f["ranges"][(py // 16) * gx + px // 16])
        n = max(int(nc_a[p]), int(nc_b[p]))
        ids = f["point_list"][lo:min(hi, lo + n)].astype(np.int64)
        co, m = f["conic_opacity"][ids].astype(np.float64), f["means2D"][ids].astype(np.float64)
        dx, dy = m[:, 0] - px, m[:, 1] - py
        power = -0.5 * (co[:, 0] * dx * dx + co[:, 2] * dy * dy) - co[:, 1] * dx * dy
        alpha = co[:, 3] * np.exp(np.minimum(power, 0.0))
        mask[ids[(power <= 1e-6) & (alpha >= 0.5 / 255.0)]] = True
    return mask


ROW_REL, ROW_FLOOR, ROW_FRACTION = 1e-3, 1e-7, 1e-3


def assert_grads_close(got, want, tol=1e-5, tag="", masked=None, keys=None):
    """The two bars of every gradient comparison (the tensor-wide bar alone would pass a
    row that is 100 % wrong if it is small).  `got` / `want`: dicts of arrays whose first axis is the Gaussian.
      1. max |a - b| <= tol * max |b|                                   -- north_star's 1e-5, relative to the tensor's largest entry;
      2. per ROW: |a - b| <= ROW_FLOOR * max|b| + ROW_REL * |b_row|     -- a row is a cancelling sum over pixels whose binary32
         value depends on the summation order (wave reductions + atomics here, per-pixel atomics in the reference), so a FEW
         rows may exceed it by rounding alone: at most ROW_FRACTION of the rows that carry a gradient (+ 2) may, and none
         of them by more than bar 1.
    `masked` rows (Gaussians under pixels whose discrete decisions differ between two exp implementations) are reported by
    the caller, not asserted.  Returns the worst tensor-wide error."""
    worst = 0.0
    for k in (keys if keys is not None else got.keys()):
        a = np.asarray(got[k], dtype=np.float64)
        a = a.reshape(a.shape[0], -1) if a.ndim else a.reshape(1, 1)
        b = np.asarray(want[k], dtype=np.float64).reshape(a.shape)
        if a.size == 0:
            continue
        m = np.zeros(a.shape[0], bool) if masked is None else masked
        scale = max(float(np.abs(b).max()), 1e-30)
        d = np.abs(a - b).max(axis=1)
        e_kept = float((d[~m] / scale).max()) if (~m).any() else 0.0
        worst = max(worst, e_kept)
        row = np.abs(b).max(axis=1)
        bad = (d > ROW_FLOOR * scale + ROW_REL * row) & ~m
        live = (row > 0) & ~m
        assert e_kept <= tol, (tag, k, e_kept)
        assert int(bad.sum()) <= ROW_FRACTION * max(1, int(live.sum())) + 2, (tag, k, int(bad.sum()), int(live.sum()))
    return worst


def v2_fuzz_case(seed):
    """Configuration `seed` of tools/fuzz_v2.py: a synth-v2 scene (thin disks on surfaces, bimodal opacity) of random size seen
    through a random small image -> (case, scale_modifier, sh_degree)."""
    from gaussianeditor_amd.synth import synth_scene_v2

    rng = np.random.default_rng(77000 + seed)
    P = int(rng.integers(300, 9000))
    W = int(rng.choice([1, 2, 15, 17, 31]) if seed % 5 == 0 else rng.integers(8, 500))
    H = int(rng.choice([1, 3, 16, 47]) if seed % 7 == 1 else rng.integers(8, 320))
    D = int(rng.integers(0, 4))
    sm = float(rng.choice([0.5, 1.0, 1.7]))
    case = make_case(P, W, H, seed=seed, view=int(rng.integers(0, 8)), nviews=8, sh_degree=D)
    sc = synth_scene_v2(P, seed=seed, sh_degree=D)
    sc["xyz"] = (sc["xyz"] * float(rng.choice([0.5, 1.0, 1.0, 2.0]))).contiguous()
    case["sc"] = sc
    return case, sm, D


__all__ = ["make_case", "oracle_forward", "oracle_backward", "settings", "hip_state", "rel_err", "seed_gradient", "v2_fuzz_case",
           "flipped_pixels", "gaussians_under", "assert_grads_close"]


# ---- the reference's own sources compiled for gfx950 (oracle/_ref): presence is LOUD when asked for ----
REF_BACKED = []  # node ids of the tests that really ran against oracle/_ref (printed in the terminal summary, conftest.py)


def require_ref(variant="nofma", knn=False):
    """-> the `oracle.ref` module, after checking that the reference build `variant` exists.  The binaries are git-ignored
    and reach the GPU box with gpurun's push of the work tree: where one is missing the test is SKIPPED -- unless
    GSR_REQUIRE_REF=1 (tools/gpu_session.sh, tools/gpu_final.sh set it; the round-end driver should too), under which it
    FAILS: a lost push must not turn the strongest parity evidence into green skips."""
    import os

    import pytest

    from oracle import ref

    ok = ref.knn_available(variant) if knn else ref.available(variant)
    if not ok:
        what = f"oracle/_ref ({'knn ' if knn else ''}{variant}) not built / not shipped (needs /root/reference at build time)"
        if os.environ.get("GSR_REQUIRE_REF") == "1":
            pytest.fail("GSR_REQUIRE_REF=1: " + what)
        pytest.skip(what)
    node = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    if node not in REF_BACKED:
        REF_BACKED.append(node)
    return ref
