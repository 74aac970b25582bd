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
test_gpu_k7_matrix.py exercises it.)

The grid of the persistent kernels is compute units x 4 x GSR_BLEND_WAVES_PER_SIMD (4 by default), and the cut's
thresholds move with it: `_grid` reads the knob as the library does, and test_on_other_grid_shapes runs the file, the
feature kernels and the feature cells of the guard-band matrix in a fresh process for 1, 2, 3, 5 and 8 (6.1, 6.5, 7.4, 8.0
and 8.8 s on the MI355X; this process: 5 s without them).  test_back_to_back_launches_of_one_queue_kind is where a launch
that fails to put its queue's cursors back shows, at each of those grids."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import (assert_grads_close, flipped_pixels, gaussians_under, hip_state, make_case, oracle_backward, oracle_forward,
                     rel_err, seed_gradient, settings)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "GSR_BLEND_WAVES_PER_SIMD"
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
def _waves_per_simd():
    """gsr_blend.hip, waves_per_simd(): GSR_BLEND_WAVES_PER_SIMD clamped to 0 .. 8, 0 and unset: 4."""
    e = os.environ.get(KNOB)
    if e is None:
        return 4
    try:
        v = int(e)
    except ValueError:
        v = 0  # (atoi)
    return min(max(v, 0), 8) or 4


@functools.lru_cache(None)
def _grid():
    # (blend_grid_size(): CUs x 4 SIMDs x the persistent waves per SIMD, 4 unless the environment says otherwise: the
    #  image sizes below stay next to the thresholds of the grid that is really launched)
    return torch.cuda.get_device_properties(DEV).multi_processor_count * 4 * _waves_per_simd()


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


# ----------------------------------------------------------------------------------------------------------------------
# back-to-back launches of one queue kind; the other launch grids
# ----------------------------------------------------------------------------------------------------------------------
def test_back_to_back_launches_of_one_queue_kind():
    """The cursors of a queue kind (forward, backward, trace) live in the view's image state, zeroed by the binning and then
    by the workgroup of every launch that retires last (retire_queue): a launch that leaves them standing makes the NEXT
    launch of its kind on that state skip items.  Two renders of one view, two auxiliary forwards and two backwards on the
    second one's state, then a smaller view that reuses nothing: every forward bit-identical to its twin and to the oracle,
    the backwards within the run-to-run bar of test_gpu_parity.py::test_backward_run_to_run_spread (2e-6) of each other and
    within the parity bar of the oracle."""
    from oracle import cpu as O

    c = _c()
    W, H = _size(1, True)  # more quadrant items than persistent waves: the queues are popped
    case, f = _case(W, H)
    sc, cam = case["sc"], case["cam"]
    e = torch.empty(0, device=DEV)
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731
    bg, xyz, op, scl, rot, sh = (dev(t) for t in (case["bg"], sc["xyz"], sc["opacity"], sc["scaling"], sc["rotation"], sc["features"]))
    view, proj, campos = dev(cam.world_view_transform), dev(cam.full_proj_transform), dev(cam.camera_center)

    def render():
        return c.rasterize_gaussians(bg, xyz, e, op, scl, rot, 1.0, e, view, proj, case["tfx"], case["tfy"], H, W, sh, case["D"],
                                     campos, False, False, flags=0)

    first, second = render(), render()
    R, color, depth, radii, geom, binning, img = second
    assert R == first[0] == f["num_rendered"] > 0
    assert torch.equal(first[1], color) and torch.equal(first[2], depth) and torch.equal(first[3], radii)
    _assert_image(f"second render {W}x{H}", False, color, depth, hip_state(P, R, W, H, geom, binning, img), f, W, H)
    aux, f_aux = dev(_aux_colors()), _aux_case(W, H)
    sems = [c.rasterize_gaussians_aux(bg, aux, R, geom, binning, img, H, W, flags=0) for _ in range(2)]
    assert torch.equal(sems[0], sems[1]) and np.array_equal(sems[1].cpu().numpy(), f_aux["color"])
    G = seed_gradient(H, W, 5) * (H * W)
    Gd = dev(G)

    def backward():
        m2, _, dop, m3, _, dsh, dscl, drot = c.rasterize_gaussians_backward(
            bg, xyz, radii, e, scl, rot, 1.0, e, view, proj, case["tfx"], case["tfy"], Gd, sh, case["D"], campos, geom, R, binning,
            img, False, flags=0)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in dict(dL_dmeans2D=m2, dL_dopacity=dop, dL_dmeans3D=m3, dL_dsh=dsh, dL_dscales=dscl,
                                                    dL_drotations=drot).items()}

    a, b = backward(), backward()
    want = oracle_backward(O, case, f, G)
    for k in a:
        spread = rel_err(a[k], b[k])
        print(f"  back to back: {k} run-to-run {spread:.2e}")
        assert spread <= 2e-6, (k, spread)
    for i, g in enumerate((a, b)):
        assert_grads_close(g, want, tag=f"backward {i}", keys=list(g))
    # ... and after the backwards, once more the forward kind on that state
    assert torch.equal(c.rasterize_gaussians_aux(bg, aux, R, geom, binning, img, H, W, flags=0), sems[0])
    W2, H2 = min(_size(4, False), _size(4, True))
    assert W2 * H2 < W * H
    case2, f2 = _case(W2, H2)
    R2, color2, depth2, _, geom2, binning2, img2 = _render(case2, 0)
    assert R2 == f2["num_rendered"] > 0
    _assert_image(f"smaller view {W2}x{H2}", False, color2, depth2, hip_state(P, R2, W2, H2, geom2, binning2, img2), f2, W2, H2)


#: what a child of test_on_other_grid_shapes runs: this file (without that test), the feature forward at every channel count
#: and the feature backward -- grid min(blend grid / 4, 3 x compute units): 1, 2 and 3 slots --, and the feature cells of the
#: guard-band matrix, which also meet the run on a side stream there
CHILD_FILES = ("test_gpu_blend_dispatch.py", "test_gpu_features.py", "test_gpu_guard_bands.py")
CHILD_SELECT = ("(test_gpu_blend_dispatch and not test_on_other_grid_shapes) or channel_counts or backward_with_the_colour_loss "
                "or test_feature_image_and_its_backward")


@pytest.mark.parametrize("waves", ["1", "2", "3", "5", "8"])
def test_on_other_grid_shapes(waves):
    """DESIGN 3.3, "no launch-shape knob changes a result": everything above -- the main forward with and without
    GSR_FLAG_FORWARD_ONLY, the auxiliary forward and the trace in both exp modes at the sizes next to the cut's thresholds
    of THAT grid, the back-to-back launches -- and the feature kernels, in a fresh process per value of
    GSR_BLEND_WAVES_PER_SIMD (read once per process), one at a time, each under its own time limit.  At 8 the single-wave
    kernels launch 8 192 workgroups: 128 retire groups, the last grid retire_queue serves.  Measured on the MI355X: 50 tests
    per child, the children for 1, 2, 3, 5 and 8 take 6.1, 6.5, 7.4, 8.0 and 8.8 s (4.5 to 7.2 s of them in the tests); every
    stream run in them conclusive.  Not reached on a 256-CU device and left untested: the memset fallback of prepare_queue
    (more than 128 retire groups) and units == 0 (a CU count the fold does not divide)."""
    env = {k: v for k, v in os.environ.items() if k != KNOB}
    env[KNOB] = waves
    files = [os.path.join(ROOT, "tests", f) for f in CHILD_FILES]
    r = subprocess.run([sys.executable, "-m", "pytest", *files, "-m", "gpu", "-x", "-q", "-s", "-k", CHILD_SELECT],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print("\n".join(ln for ln in r.stdout.splitlines() if "side stream" in ln or " passed" in ln or " failed" in ln))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:]
