"""-m gpu: the blend launch layer's dispatch.  The forward (K6) and the trace kernel (K12) are each built once per quadrant
cut (1, 2 or 4 items per quadrant), exp mode and -- the forward -- colour source; which one a call gets is decided on the
host (gsr_blend.hip: launch_blend_forward, launch_trace_weights) and, unlike K7's, counted nowhere.  One small scene rendered
at image sizes on every side of the cut's thresholds, in both exp modes, through the main forward (with and without
GSR_FLAG_FORWARD_ONLY), the auxiliary forward and the trace, each against the CPU oracle.

What a failure here can mean: a combination that launched nothing or was refused, the auxiliary and the main kernel or
two channel counts mixed up, the forward's exact kernel where the fast one was asked for or the reverse.  What it cannot
see: a kernel of another cut -- every cut computes the same image and the same weights, so all of them are held to the
oracle here, but not told apart --, and in the trace an exact kernel in place of the fast one (0 / 1 masks, no flipped
pixel on this scene).  (The checkpointed forward is chosen by process-wide environment knobs; every SEG case of
test_gpu_k7_matrix.py exercises it.)"""
import functools

import numpy as np
import pytest
import torch

from helpers import flipped_pixels, gaussians_under, hip_state, make_case, oracle_forward, settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 5000


def _c():
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    return _C


def forward_split(grid, quads, for_backward):
    """gsr_blend.hip, forward_split(): items a quadrant is cut into, its two rules restated."""
    if for_backward:
        return 1 if quads > grid else (2 if 4 * quads > grid else 4)
    return 1 if quads >= 2 * grid else (2 if quads >= grid else 4)


@functools.lru_cache(None)
def _grid():
    # (blend_grid_size(): CUs x 4 SIMDs x 4 persistent waves)
    return torch.cuda.get_device_properties(DEV).multi_processor_count * 4 * 4


def _size(cut, for_backward):
    """(W, H) of an image of n x n tiles that the rule cuts `cut` ways: the smallest such n, for 4 the largest -- the sizes
    next to the thresholds.  Ragged in both directions (tiles are 16 x 16)."""
    ns = [n for n in range(1, 129) if forward_split(_grid(), 4 * n * n, for_backward) == cut]
    if not ns:
        pytest.skip(f"no square image of up to 128 x 128 tiles is cut {cut} ways on a grid of {_grid()} waves")
    n = max(ns) if cut == 4 else min(ns)
    return 16 * n - 3, 16 * n - 7


@functools.lru_cache(None)
def _case(W, H):
    """The scene, its view and the oracle's main render of it (computed once per size, never written to)."""
    from oracle import cpu as O

    O.build()
    case = make_case(P, W, H, seed=7, s0=0.03)
    return case, oracle_forward(O, case)


@functools.lru_cache(None)
def _aux_colors():
    return torch.rand(P, 3, generator=torch.Generator().manual_seed(8))  # (not the scene's colours)


@functools.lru_cache(None)
def _aux_case(W, H):
    """The oracle's render of the view with the auxiliary colours as colors_precomp."""
    from oracle import cpu as O

    return oracle_forward(O, _case(W, H)[0], colors_precomp=_aux_colors())


@functools.lru_cache(None)
def _trace_case(W, H, C):
    """A 0 / 1 mask image (sums exact in any order) and the oracle's apply_weights of it -> (mask, weights, cnt)."""
    from oracle import cpu as O

    case = _case(W, H)[0]
    sc, cam = case["sc"], case["cam"]
    mask = (torch.rand(C, H, W, generator=torch.Generator().manual_seed(12)) > 0.5).float()
    w_ref, c_ref = np.zeros((P, C), np.float32), np.zeros((P,), np.int32)
    O.apply_weights(sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], None, cam.world_view_transform,
                    cam.full_proj_transform, cam.camera_center, W, H, case["tfx"], case["tfy"], mask, w_ref, c_ref)
    return mask, w_ref, c_ref


def _render(case, flags):
    sc, cam = case["sc"], case["cam"]
    e = torch.empty(0, device=DEV)
    dev = lambda t: t.to(DEV)  # noqa: E731
    return _c().rasterize_gaussians(
        dev(case["bg"]), dev(sc["xyz"]), e, dev(sc["opacity"]), dev(sc["scaling"]), dev(sc["rotation"]), 1.0, e,
        dev(cam.world_view_transform), dev(cam.full_proj_transform), case["tfx"], case["tfy"], case["H"], case["W"],
        dev(sc["features"]), case["D"], dev(cam.camera_center), False, False, flags=flags)


def _assert_image(tag, fast, color, depth, st, f, W, H):
    """Exact exp: colour, depth, n_contrib and final_T bit for bit (test_gpu_parity.py).  GSR_FLAG_FAST_EXP: the bar of
    test_gpu_round2.py::test_fast_exp_flag_parity_and_flag_pinning -- the pixels whose threshold decisions flip counted and
    bounded, the image within 1e-5 outside them and within 2.1 / 255 of the largest colour at them."""
    col, dep = color.cpu().numpy(), depth.cpu().numpy() if depth is not None else None
    if not fast:
        exact = dict(color=np.array_equal(col, f["color"]), n_contrib=np.array_equal(st["n_contrib"], f["n_contrib"]),
                     final_T=np.array_equal(st["final_T"], f["final_T"]))
        if dep is not None:
            exact["depth"] = np.array_equal(dep, f["depth"])
        print(f"  {tag}: bit-exact {exact}")
        assert all(exact.values()), (tag, exact)
        return None
    flips = flipped_pixels(st["n_contrib"], st["final_T"], f["n_contrib"], f["final_T"])
    keep = np.ones(W * H, bool)
    keep[flips] = False
    dc = np.abs(col - f["color"]).reshape(3, -1)
    print(f"  {tag}: flipped pixels {flips.size} of {W * H}; colour max diff outside them {dc[:, keep].max():.2e}, with them "
          f"{dc.max():.2e}")
    assert flips.size <= 4 + 2e-4 * W * H, tag
    assert not np.array_equal(col, f["color"]), tag  # (the hardware's 2^x is not the specified polynomial: the exact kernel ran)
    cmax = max(1.0, float(np.abs(f["colors_used"][f["radii"] > 0]).max()))
    assert dc[:, keep].max() <= 1e-5 and dc.max() <= 2.1 * cmax / 255.0 + 1e-5, tag
    if dep is not None:  # (reported, as there: that test sets the depth image no bar)
        print(f"  {tag}: depth max diff outside the flipped pixels {np.abs(dep - f['depth']).reshape(-1)[keep].max():.2e}")
    return flips


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast_exp"])
@pytest.mark.parametrize("forward_only", [True, False], ids=["forward_only", "for_backward"])
@pytest.mark.parametrize("cut", [1, 2, 4])
def test_main_forward(cut, forward_only, fast):
    from gaussianeditor_amd import options

    W, H = _size(cut, not forward_only)
    case, f = _case(W, H)
    flags = (options.FLAG_FORWARD_ONLY if forward_only else 0) | (options.FLAG_FAST_EXP if fast else 0)
    R, color, depth, radii, geom, binning, img = _render(case, flags)
    assert R == f["num_rendered"] > 0 and np.array_equal(radii.cpu().numpy(), f["radii"])
    st = hip_state(P, R, W, H, geom, binning, img)
    assert np.array_equal(st["point_list"], f["point_list"]) and np.array_equal(st["ranges"], f["ranges"])
    _assert_image(f"cut {cut} {W}x{H} flags {flags}", fast, color, depth, st, f, W, H)


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast_exp"])
@pytest.mark.parametrize("cut", [1, 2, 4])
def test_aux_forward(cut, fast):
    """The auxiliary render takes the forward-only cut (it has no backward) and leaves the main render's state alone."""
    from gaussianeditor_amd import options

    W, H = _size(cut, False)
    case, f = _case(W, H)
    aux, f_aux = _aux_colors(), _aux_case(W, H)
    flags = options.FLAG_FAST_EXP if fast else 0
    R, color, depth, radii, geom, binning, img = _render(case, flags)
    before = hip_state(P, R, W, H, geom, binning, img)
    sem = _c().rasterize_gaussians_aux(case["bg"].to(DEV), aux.to(DEV), R, geom, binning, img, H, W, flags=flags)
    after = hip_state(P, R, W, H, geom, binning, img)
    assert np.array_equal(before["final_T"], after["final_T"]) and np.array_equal(before["n_contrib"], after["n_contrib"])
    assert not np.array_equal(f_aux["color"], f["color"])
    # (the aux kernel writes neither final_T nor n_contrib: its decisions are those of the main render of the same exp mode)
    _assert_image(f"aux cut {cut} {W}x{H} flags {flags}", fast, sem, None, after, f_aux, W, H)


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast_exp"])
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("cut", [1, 2, 4])
def test_trace(cut, C, fast):
    """apply_weights with 0 / 1 masks.  Exact exp: `weights` and `cnt` identical to the oracle's
    (test_gpu_parity.py::test_apply_weights).  GSR_FLAG_FAST_EXP: identical outside the Gaussians blended at a pixel whose
    threshold decision flips, those counted and bounded (test_gpu_reference.py::test_apply_weights_vs_reference)."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    W, H = _size(cut, False)
    case, f = _case(W, H)
    sc = case["sc"]
    mask, w_ref, c_ref = _trace_case(W, H, C)
    assert c_ref.sum() > 0
    flags = options.FLAG_FAST_EXP if fast else 0
    w = torch.zeros((P, C), device=DEV)
    cnt = torch.zeros((P, 1), dtype=torch.int32, device=DEV)
    with options.override(flags):
        GaussianRasterizer(settings(case, DEV, D=0)).apply_weights(
            sc["xyz"].to(DEV), None, sc["opacity"].to(DEV), None, w, sc["scaling"].to(DEV), sc["rotation"].to(DEV), None, cnt,
            mask.to(DEV))
    torch.cuda.synchronize()
    got_w, got_c = w.cpu().numpy(), cnt.cpu().numpy().reshape(-1)
    if not fast:
        assert np.array_equal(got_c, c_ref) and np.array_equal(got_w, w_ref)
        return
    R, color, depth, radii, geom, binning, img = _render(case, flags)
    st = hip_state(P, R, W, H, geom, binning, img)
    flips = flipped_pixels(st["n_contrib"], st["final_T"], f["n_contrib"], f["final_T"])
    masked = gaussians_under(flips, W, f, st["n_contrib"])
    diff = got_c != c_ref
    print(f"  trace cut {cut} C={C}: flipped pixels {flips.size}, Gaussians under them {int(masked.sum())}; cnt differs on "
          f"{int(diff.sum())} ({int((diff & ~masked).sum())} outside them)")
    assert flips.size <= 4 + 2e-4 * W * H
    assert not (diff & ~masked).any()
    assert np.abs(got_c.astype(np.int64) - c_ref.astype(np.int64))[masked].max(initial=0) <= 4 * C
    assert np.abs(got_w - w_ref)[~masked].max(initial=0.0) <= 1e-5 * max(1.0, float(np.abs(w_ref).max()))


def test_trace_four_channels_is_refused():
    from gaussianeditor_amd import _native
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    W, H = _size(4, False)
    case, _ = _case(W, H)
    sc = case["sc"]
    with pytest.raises(_native.GsrError, match="Unsupported number of channels: 4"):
        GaussianRasterizer(settings(case, DEV, D=0)).apply_weights(
            sc["xyz"].to(DEV), None, sc["opacity"].to(DEV), None, torch.zeros(P, 4, device=DEV), sc["scaling"].to(DEV),
            sc["rotation"].to(DEV), None, torch.zeros(P, dtype=torch.int32, device=DEV), torch.zeros(4, H, W, device=DEV))
    # ... and by the library itself, in front of every other check
    assert _native.lib().gsr_trace_weights(None, P, 1, W, H, 4, None, None, None, None, None, None, 0) == -2


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast_exp"])
def test_nothing_to_blend(fast):
    """No Gaussian at all, and none in view, at the smallest size: zeros, and the background over an untouched state."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    W, H = min(_size(4, False), _size(4, True))
    case, _ = _case(W, H)
    flags = options.FLAG_FAST_EXP if fast else 0
    empty = dict(case, sc={k: (v[:0].contiguous() if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == P else v)
                           for k, v in case["sc"].items()})
    R, color, depth, radii, *_ = _render(empty, flags)
    assert R == 0 and radii.numel() == 0 and color.shape == (3, H, W)
    assert float(color.abs().max()) == 0.0 and float(depth.abs().max()) == 0.0
    behind = dict(case, sc=dict(case["sc"], xyz=(case["sc"]["xyz"] * 0.1 + case["cam"].camera_center * 2.0).contiguous()))
    R, color, depth, radii, geom, binning, img = _render(behind, flags)
    assert R == 0 and int(radii.abs().max()) == 0
    assert torch.equal(color, case["bg"].to(DEV)[:, None, None].expand(3, H, W)) and float(depth.abs().max()) == 0.0
    st = hip_state(P, R, W, H, geom, binning, img)
    assert np.array_equal(st["final_T"], np.ones(W * H, np.float32)) and not st["n_contrib"].any()
    sem = _c().rasterize_gaussians_aux(case["bg"].to(DEV), _aux_colors().to(DEV), R, geom, binning, img, H, W, flags=flags)
    assert torch.equal(sem, color)
    w, cnt = torch.zeros((P, 1), device=DEV), torch.zeros((P, 1), dtype=torch.int32, device=DEV)
    sc = behind["sc"]
    with options.override(flags):
        GaussianRasterizer(settings(case, DEV, D=0)).apply_weights(
            sc["xyz"].to(DEV), None, sc["opacity"].to(DEV), None, w, sc["scaling"].to(DEV), sc["rotation"].to(DEV), None, cnt,
            torch.ones(1, H, W, device=DEV))
    assert not w.any() and not cnt.any()
