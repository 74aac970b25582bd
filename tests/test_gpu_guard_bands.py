"""-m gpu: guard bands and poison around every caller-owned buffer the kernels touch.

The native library never allocates: every output, the three state buffers and every workspace is a torch allocation of
the Python glue, sized by gsr_scratch_sizes and the gsr_*_workspace_size functions, and the kernels get raw pointers.
The rest of the suite checks what the kernels leave INSIDE those buffers.  Here every matrix cell is driven through the
product's own Python entry points -- under guarded_alloc.GuardedAllocator with pattern 0xFF (NaN as float32,
0xFFFFFFFF as an index or count, 255 as a mask byte), with pattern 0x5A (a large finite float, a large index) and
unpatched -- with the test's own inputs inside guarded interiors too (`place`):

  (a) no guard byte in front of or behind any buffer may have changed, under either pattern;
  (b) every documented output of a deterministic operation is bit-identical between the three runs: nothing may depend on
      what an `empty` buffer or the memory around a buffer held;
  (c) the backward's gradients (summed by float atomics, not bit-stable) meet the bar of
      test_gpu_parity.py::test_backward_vs_oracle against the CPU oracle -- helpers.assert_grads_close at its default
      1e-5 plus the per-tensor 1e-5 -- in every run.  Where the oracle has no counterpart (FLAG_ANTIALIAS and
      FLAG_FAST_EXP change the arithmetic; the absolute gradient, the camera gradient and the "rgb" colour gradient are
      outputs the oracle does not have) the patterned runs are held to the same bar against the unpatched run of the
      product, which the tests of those features pin.

Outputs the API documents as unspecified are cut to their specified part before (b): `dead_idx` beyond n_dead.

A fourth run of every cell, in front of the unpatched one, is off the default stream (stream_order.SideStream): on a
fresh stream, its inputs holding decoys until a sleep on that stream has passed, while the default stream sleeps; its
outputs are copied to the host on that stream and only that stream is waited for.  (b) holds for it unchanged -- every
deterministic output bit-identical to the unpatched run --, (c) through the callers' loops over the runs, and the run must
be conclusive: the outputs on the host while the default stream still sleeps.  A mismatch: the product launched something
on another stream before the side stream's inputs existed, or something had not run when the outputs were read.  Not
conclusive: the product waited for the default stream or the whole device.  The run and its warm-up are under
GuardedAllocator (0x5A, guards unchecked, not in the table below): the buffers are poisoned anew on the side stream, so
that the warm-up's right results, still in the blocks the caching allocator hands back, cannot stand in for a kernel
that never ran.  The drivers' own waits are for the current stream, not the device.

Measured on the MI355X, the stream run: all 56 cells (and the two children's) conclusive and bit-identical.  The first run of
a cell takes 0.3 to 16 ms, except where it loads a code object (rasterizer P1_17x19 165 ms, fused loss tex_5x7 738 ms,
fused Adam aligned n257 569 ms, densify 296 ms, the children's cell 179 ms), so the sleep is the floor of 200 ms in 52
cells and 0.66, 2.95, 2.27, 1.18 and 0.71 s in those.  With `place` sleeping 1 ms per input the outputs are on the host
1.1 ms (simple_knn, 1 input) to 41.5 ms (densify, 37 inputs) after entry, 11.8 ms in the rasterizer cells (11 inputs),
34.2 ms at 4112 x 4096: the sleep is 5.3 times the window where the margin is smallest (the message round trip, 36
inputs: 37.6 ms of 200 ms), 5.8 times at 4112 x 4096 and fused Adam two_launches, 7.7 times or more elsewhere.  The whole
file then runs in 33.5 s (before the stream run: 14.7 s): 52 sleeps of 0.2 s and four longer ones are 17.5 s of that.

Measured on the MI355X before the stream run was added: the whole file, 60 tests in one process plus the two child
processes of the environment regimes, runs in 14.7 s; the slowest tests are the two children (3.7 s each, mostly
interpreter start; 4.5 s with the stream run) and the 4112 x 4096 image (1.6 s; 1.95 s).  Guarded allocations whose guards were checked, both patterns together (`test_zz_allocation_counts` prints the
table); "product": made by an allocation call inside gaussianeditor_amd/, the rest are the tests' own inputs (`place`):

    group                  checked  product
    rasterizer                 574      312
    binning paths               96       52
    flags                      308      166
    saved view                 112       68
    features                   168       90
    trace weights               90       24
    multiview                  300       96
    simple_knn                  18       12
    near                        36       20
    arrays_equal                16        0   (the compare takes pointers and allocates nothing)
    fused loss                  36       24
    fused Adam                 424      160
    row arena                   84       16
    densify                    224      126
    MCMC                       152       82
    detector self-test          16        7
    environment regimes         48       26   (in the two child processes: 24 per pattern and child, 13 the product's)

Every guard was clean and every deterministic output bit-identical under both patterns; the largest gradient error against
the oracle was 2.4e-6 of the tensor's maximum (bar 1e-5).
"""
import collections
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import alpha_helpers as AH
import densify_helpers as dh
import features_helpers as FH
import loss_helpers as LH
import mcmc_helpers as mh
import stream_order as SO
from depth_helpers import depth_expectation
from guarded_alloc import GuardedAllocator
from helpers import assert_grads_close, make_case, oracle_backward, oracle_forward, rel_err, seed_gradient
from stream_order import host as _host, same_bits as _same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = (0xFF, 0x5A)
COUNTS = collections.Counter()   # group -> guarded allocations checked
PRODUCT = collections.Counter()  # group -> those of them made inside gaussianeditor_amd/


# ----------------------------------------------------------------------------------------------------------------------
# the three runs
# ----------------------------------------------------------------------------------------------------------------------
def _plain_put(t):
    out = t.detach().to(DEV).clone()
    return out.requires_grad_(True) if t.requires_grad else out


def _reset_product_state():
    """State the binding keeps across calls: the accumulator tables kept per stream (so that each run allocates its own,
    under its own pattern) and the remembered view of the colour-override reuse."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C, _reuse

    _C._ACC_TABLES.clear()
    _reuse.forget()


def three_runs(group, fn, tag=""):
    """fn(put) -> (deterministic outputs {name: tensor | number}, gradients {name: tensor} | None), run under 0xFF, under
    0x5A, on a side stream with late inputs while the default stream sleeps (stream_order.SideStream) and unpatched; (a) and
    (b) asserted here -> [(outputs, gradients)] as numpy, in that order: the unpatched run last."""
    runs = []
    cell_seconds = None
    for pattern in PATTERNS + (None,):
        _reset_product_state()
        if pattern is None:
            # the stream run: after the patterned runs (code objects loaded, the allocator warm), in front of the unpatched one
            stream_run, side = SO.run_cell(fn, SO.sleep_ms_for(cell_seconds), reset=_reset_product_state,
                                           allocator=lambda: GuardedAllocator(PATTERNS[1]))
            print(f"  {group} {tag}: first run {cell_seconds * 1e3:.0f} ms; {SO.report(side)}")
            runs.append(stream_run)
            _reset_product_state()
            det, grads = fn(_plain_put)
            torch.cuda.synchronize()
        else:
            t0 = time.perf_counter()
            with GuardedAllocator(pattern) as ga:
                det, grads = fn(ga.place)
                torch.cuda.synchronize()
            if cell_seconds is None:
                cell_seconds = time.perf_counter() - t0
            ga.assert_clean()  # (a)
            made = sum(r["site"].startswith("gaussianeditor_amd") for r in ga.records)  # (the rest: the test's own `place`)
            print(f"  {group} {tag}: pattern {pattern:#04x}: {len(ga)} guarded allocations, {made} of them the product's, all clean")
            assert len(ga) > 0
            COUNTS[group] += len(ga)
            PRODUCT[group] += made
        runs.append((_host(det), _host(grads)))
    _reset_product_state()
    plain = runs[-1][0]
    assert plain, (group, tag)
    for pattern, (det, _) in zip(PATTERNS, runs):  # (b)
        assert det.keys() == plain.keys(), (group, tag)
        for name in plain:
            assert _same_bits(det[name], plain[name]), f"{group} {tag}: `{name}` depends on the pattern ({pattern:#04x})"
    # (b) of the stream run: a mismatch -- something ran on another stream before the side stream's inputs existed, or had not
    # run when the outputs were read; not conclusive -- the product waited for the default stream or for the whole device
    v = SO.verdict(stream_run[0], plain, side)
    assert v == "clean", f"{group} {tag}: the run on a side stream: {v}; {SO.report(side)}"
    return runs


def _close(got, want, tag, keys=None):
    """The bar of test_backward_vs_oracle: 1e-5 of the tensor's largest entry, and helpers.assert_grads_close."""
    for k in (keys if keys is not None else got.keys()):
        e = rel_err(got[k], np.asarray(want[k]).reshape(got[k].shape))
        print(f"  {tag}: {k} rel err {e:.2e}")
        assert np.isfinite(np.asarray(got[k], dtype=np.float64)).all(), (tag, k)
        assert e <= 1e-5, (tag, k, e)
    assert_grads_close(got, want, tag=tag, keys=keys)


# ----------------------------------------------------------------------------------------------------------------------
# rasterizer forward and backward
# ----------------------------------------------------------------------------------------------------------------------
def _flags():
    from gaussianeditor_amd import options

    return options


def _settings(put, case, D=None):
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizationSettings

    cam = case["cam"]
    return GaussianRasterizationSettings(case["H"], case["W"], case["tfx"], case["tfy"], put(case["bg"]), 1.0,
                                         put(cam.world_view_transform), put(cam.full_proj_transform),
                                         case["D"] if D is None else D, put(cam.camera_center), False, False)


def _raster(put, case, G, cols=None, cov=None, flags=0, GA=None, GD=None, pose=False, feats=None, GF=None):
    """One render + backward of <G, C> (+ <GA, A>) (+ <GD, D>) (+ <GF, F>) through GaussianRasterizer under
    options.override(flags) -> (deterministic outputs, gradients by the oracle's names)."""
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    O = _flags()
    sc = case["sc"]
    P = sc["xyz"].shape[0]
    rs = _settings(put, case)
    leaf = lambda t: put(t.detach().clone().requires_grad_(True))  # noqa: E731
    cams = None
    if pose:
        cams = dict(pose_view=leaf(case["cam"].world_view_transform), pose_proj=leaf(case["cam"].full_proj_transform),
                    pose_campos=leaf(case["cam"].camera_center))
        rs = rs._replace(viewmatrix=cams["pose_view"], projmatrix=cams["pose_proj"], campos=cams["pose_campos"])
    xyz, op, m2d = leaf(sc["xyz"]), leaf(sc["opacity"]), leaf(torch.zeros(P, 3))
    kw, leaves = {}, dict(dL_dmeans3D=xyz, dL_dopacity=op, dL_dmeans2D=m2d)
    if cols is None:
        kw["shs"] = leaves["dL_dsh"] = leaf(sc["features"])
    else:
        kw["colors_precomp"] = leaves["dL_dcolors"] = leaf(cols)
    if cov is None:
        kw["scales"] = leaves["dL_dscales"] = leaf(sc["scaling"])
        kw["rotations"] = leaves["dL_drotations"] = leaf(sc["rotation"])
    else:
        kw["cov3D_precomp"] = leaves["dL_dcov3D"] = leaf(cov)
    if GA is not None:
        kw["return_alpha"] = True
    if feats is not None:
        kw["features"] = leaves["dL_dfeatures"] = leaf(feats)
    with O.override(flags):
        outs = GaussianRasterizer(rs)(xyz, m2d, op, **kw)
    color, radii, depth = outs[:3]
    det = dict(num_rendered=int(color.grad_fn.num_rendered), color=color, depth=depth, radii=radii)
    loss = (color * put(G)).sum()
    if feats is not None:
        det["features"] = outs[-1]
        loss = loss + (outs[-1] * put(GF)).sum()
    if GA is not None:
        det["alpha"] = outs[-1 - (feats is not None)]
        loss = loss + (det["alpha"] * put(GA)).sum()
    if GD is not None:
        loss = loss + (depth * put(GD)).sum()
    loss.backward()
    torch.cuda.current_stream().synchronize()  # (the product has joined its own streams back; a side stream run stays on its stream)
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v.detach())) for k, v in leaves.items()}
    if flags & O.FLAG_ABS_GRAD:
        grads["absgrad"] = m2d.absgrad
    if pose:
        grads.update({k: v.grad.reshape(-1) for k, v in cams.items()})
    return det, grads


_expect = {}


def _oracle_grads(O, key, case, G, cols=None, cov=None, GA=None, GD=None):
    """The oracle's gradients of a case, computed once -> (gradients, num_rendered)."""
    if key not in _expect:
        f = oracle_forward(O, case, colors_precomp=cols, cov3D_precomp=cov)
        if GA is not None:
            g, _ = AH.alpha_expectation(O, case, G, GA, GD=GD, colors_precomp=cols, cov3D_precomp=cov)
        elif GD is not None:
            g = depth_expectation(O, case, G, GD, colors_precomp=cols, cov3D_precomp=cov)
            g.pop("dL_ddepth", None)
        else:
            g = oracle_backward(O, case, f, G, colors_precomp=cols, cov3D_precomp=cov)
        _expect[key] = (g, int(f["num_rendered"]), f)
    return _expect[key]


def _gradient(case, seed=1):
    return seed_gradient(case["H"], case["W"], seed) * (case["H"] * case["W"])


def _check_raster(O, group, key, case, oracle_ok=True, want_R=None, **kw):
    """(a), (b), (c) of one rasterizer cell.  oracle_ok=False: the flags change the arithmetic, every gradient is held to
    the bar against the unpatched run instead."""
    G = _gradient(case)
    okw = {k: kw.get(k) for k in ("cols", "cov", "GA", "GD")}
    runs = three_runs(group, lambda put: _raster(put, case, G, **kw), tag=key)
    R = runs[-1][0]["num_rendered"]
    plain = runs[-1][1]
    extra = [k for k in plain if k == "absgrad" or k.startswith("pose_") or k == "dL_dfeatures"]
    if oracle_ok:
        want, want_R_oracle, _ = _oracle_grads(O, key, case, G, **okw)
        assert R == want_R_oracle, (key, R, want_R_oracle)
        keys = [k for k in plain if k not in extra]
        assert keys and all(k in want for k in keys), (keys, list(want))
        for i, (_, grads) in enumerate(runs):
            _close(grads, want, f"{key} run {i} vs oracle", keys=keys)
    else:
        extra = list(plain)
    for i, (_, grads) in enumerate(runs[:-1]):
        if extra:
            _close(grads, plain, f"{key} run {i} vs unpatched", keys=extra)
    if want_R is not None:
        assert want_R(R), (key, R)
    return R


RASTER_P = [1, 255, 257, 4097]        # straddle GAUSS_BLOCK = 256 and SORT_KPB = 4096
RASTER_IMAGES = [(17, 19), (130, 66)]  # ragged tiles both ways; one 8 x 8-tile group edge crossed each way


@pytest.mark.parametrize("W,H", RASTER_IMAGES, ids=lambda v: str(v))
@pytest.mark.parametrize("P", RASTER_P)
def test_rasterizer(oracle, P, W, H):
    case = make_case(P, W, H, seed=1, s0=0.1)
    R = _check_raster(oracle, "rasterizer", f"P{P}_{W}x{H}", case)
    assert R > 0


def test_rasterizer_num_rendered_between_one_and_two_sort_blocks(oracle):
    """P = 257 with s0 = 0.6: the CPU oracle gives num_rendered = 6082, inside (4096, 8192) -- a ragged second sort block."""
    case = make_case(257, 130, 66, seed=1, s0=0.6)
    _check_raster(oracle, "rasterizer", "P257_130x66_R6082", case, want_R=lambda R: 4096 < R < 8192)


def _culled_case():
    case = make_case(257, 130, 66, seed=1, s0=0.1)
    sc = dict(case["sc"])
    sc["xyz"] = (2.0 * case["cam"].camera_center.reshape(1, 3) - sc["xyz"]).contiguous()  # mirrored to behind the camera
    return dict(case, sc=sc)


def test_rasterizer_fully_culled(oracle):
    _check_raster(oracle, "rasterizer", "culled", _culled_case(), want_R=lambda R: R == 0)


def test_rasterizer_sh_degree_0(oracle):
    case = make_case(257, 17, 19, seed=2, s0=0.1, sh_degree=0)
    assert case["sc"]["features"].shape[1] == 1
    _check_raster(oracle, "rasterizer", "D0", case)


def test_rasterizer_precomputed_colours_and_covariances(oracle):
    case = make_case(257, 130, 66, seed=3, s0=0.1)
    cols = torch.rand(257, 3, generator=torch.Generator().manual_seed(3))
    cov = torch.from_numpy(oracle_forward(oracle, case)["cov3D"].copy())
    _check_raster(oracle, "rasterizer", "precomp", case, cols=cols, cov=cov)


@pytest.mark.parametrize("W,H,path", [(2200, 2064, "11-bit group pass: 18 x 17 = 306 groups > 256"),
                                      (4112, 4096, "legacy pair sort, 32-bit tile keys: 257 tiles per row > RECT32_EDGE")],
                         ids=["groups306", "tiles257"])
def test_binning_paths(oracle, W, H, path):
    case = make_case(257, W, H, seed=1, s0=0.05)
    R = _check_raster(oracle, "binning paths", f"{W}x{H}", case)
    print(f"  {W}x{H} ({path}): num_rendered {R}")
    assert R > 257


FLAG_CASES = ["antialias", "depth_grad", "abs_grad", "alpha_out", "pose_grad", "fast_exp"]


@pytest.mark.parametrize("name", FLAG_CASES)
def test_flags(oracle, name):
    O = _flags()
    case = make_case(257, 130, 66, seed=4, s0=0.2)
    H, W = case["H"], case["W"]
    kw = dict(antialias=dict(flags=O.FLAG_ANTIALIAS, oracle_ok=False),
              depth_grad=dict(flags=O.FLAG_DEPTH_GRAD, GD=seed_gradient(H, W, 5)[:1].contiguous() * (H * W)),
              abs_grad=dict(flags=O.FLAG_ABS_GRAD),
              alpha_out=dict(flags=O.FLAG_ALPHA_OUT, GA=seed_gradient(H, W, 6)[:1].contiguous() * (H * W)),
              pose_grad=dict(flags=O.FLAG_POSE_GRAD, pose=True),
              fast_exp=dict(flags=O.FLAG_FAST_EXP, oracle_ok=False))[name]
    _check_raster(oracle, "flags", f"flag_{name}", case, **kw)


# ----------------------------------------------------------------------------------------------------------------------
# extensions of a saved view
# ----------------------------------------------------------------------------------------------------------------------
def _forward_args(put, case):
    sc, cam = case["sc"], case["cam"]
    e = torch.empty(0, device=DEV)
    return (put(case["bg"]), put(sc["xyz"]), e, put(sc["opacity"]), put(sc["scaling"]), put(sc["rotation"]), 1.0, e,
            put(cam.world_view_transform), put(cam.full_proj_transform), case["tfx"], case["tfy"], case["H"], case["W"],
            put(sc["features"]), case["D"], put(cam.camera_center), False, False)


@pytest.mark.parametrize("W,H", [(130, 66), (17, 19)], ids=["WxH_divisible_by_4", "WxH_not_divisible_by_4"])
def test_saved_view_extensions(W, H):
    """begin / finish, the auxiliary image, the alpha image (its vec4 path at W * H divisible by 4, the scalar one
    otherwise) and mark_visible, all on the state of one view."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    assert (W * H % 4 == 0) == (W == 130)
    case = make_case(257, W, H, seed=5, s0=0.2)
    aux = torch.rand(257, 3, generator=torch.Generator().manual_seed(8))

    def run(put):
        args = _forward_args(put, case)
        R, color, depth, radii, geom, binning, img = _C.rasterize_gaussians(*args, flags=0)
        R2, color2, depth2, radii2, geom2, binning2, img2 = _C.rasterize_gaussians_finish(_C.rasterize_gaussians_begin(*args, flags=0))
        det = dict(R=R, color=color, depth=depth, radii=radii, R2=R2, color2=color2, depth2=depth2, radii2=radii2,
                   aux=_C.rasterize_gaussians_aux(args[0], put(aux), R, geom, binning, img, H, W, flags=0),
                   aux2=_C.rasterize_gaussians_aux(args[0], put(aux), R2, geom2, binning2, img2, H, W, flags=0),
                   alpha=_C.alpha_image(img, H, W), alpha2=_C.alpha_image(img2, H, W),
                   visible=_C.mark_visible(args[1], args[8], args[9]))
        return det, None

    det = three_runs("saved view", run, tag=f"{W}x{H}")[-1][0]
    assert det["R"] == det["R2"] > 0
    for k in ("color", "depth", "radii", "aux", "alpha"):
        assert _same_bits(det[k], det[k + "2"]), k
    assert 0 < det["alpha"].max() <= 1.0 and det["visible"].any()


@pytest.mark.parametrize("C", [1, 16, 17])
def test_feature_image_and_its_backward(oracle, C):
    """rasterize_features through GaussianRasterizer(features=) and its backward: one partial block, one full 16-channel
    block, one full block and a ragged one."""
    case = make_case(257, 130, 66, seed=6, s0=0.2)
    H, W = case["H"], case["W"]
    G, GF, feats = _gradient(case), FH.feature_gradient(H, W, C), FH.make_features(257, C)
    runs = three_runs("features", lambda put: _raster(put, case, G, feats=feats, GF=GF), tag=f"C{C}")
    want, _, dfeat, slice_max = FH.feature_expectation(oracle, case, G, GF, feats)
    want = dict(want, dL_dfeatures=dfeat)
    for i, (_, grads) in enumerate(runs):
        assert "dL_dfeatures" in grads and all(k in want for k in grads)
        FH.assert_feature_grads_close(grads, want, slice_max=slice_max, tol=1e-5, tag=f"C{C} run {i}", keys=list(grads))
    fimg = FH.oracle_feature_image(oracle, case, feats)
    assert np.abs(runs[-1][0]["features"] - fimg).max() <= 1e-5 * max(1.0, np.abs(fimg).max())


@pytest.mark.parametrize("C", [1, 2, 3])
def test_trace_weights(oracle, C):
    """apply_weights with 0 / 1 image weights: the float sums are exact in any order, so the outputs are deterministic."""
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    P, W, H = 257, 130, 66
    case = make_case(P, W, H, seed=7, s0=0.2)
    sc, cam = case["sc"], case["cam"]
    mask = (torch.rand(C, H, W, generator=torch.Generator().manual_seed(12)) > 0.5).float()

    def run(put):
        w, cnt = put(torch.zeros(P, C)), put(torch.zeros(P, 1, dtype=torch.int32))
        GaussianRasterizer(_settings(put, case, D=0)).apply_weights(
            put(sc["xyz"]), None, put(sc["opacity"]), None, w, put(sc["scaling"]), put(sc["rotation"]), None, cnt, put(mask))
        return dict(weights=w, cnt=cnt), None

    det = three_runs("trace weights", run, tag=f"C{C}")[-1][0]
    w_ref, c_ref = np.zeros((P, C), np.float32), np.zeros((P,), np.int32)
    oracle.apply_weights(sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], None, cam.world_view_transform,
                         cam.full_proj_transform, cam.camera_center, W, H, case["tfx"], case["tfy"], mask, w_ref, c_ref)
    assert np.array_equal(det["weights"], w_ref) and np.array_equal(det["cnt"].reshape(-1), c_ref) and c_ref.sum() > 0


# ----------------------------------------------------------------------------------------------------------------------
# multiview, single process
# ----------------------------------------------------------------------------------------------------------------------
_MV_NAMES = dict(means3D="dL_dmeans3D", sh="dL_dsh", opacities="dL_dopacity", scales="dL_dscales", rotations="dL_drotations",
                 means2D="dL_dmeans2D")


@pytest.mark.parametrize("mode", ["direct", "rgb", "persistent_rows"])
def test_render_view_grads_into_a_bucket(oracle, mode):
    from gaussianeditor_amd.multiview import GradBucket, render_view_grads

    P = 257
    case = make_case(P, 130, 66, seed=8, s0=0.2)
    sc = case["sc"]
    G = _gradient(case)

    def run(put):
        b = GradBucket(P, 16, DEV, sh_exchange="rgb" if mode == "rgb" else "direct", persistent_rows=mode == "persistent_rows")
        args = [put(sc[k]) for k in ("xyz", "opacity", "features", "scaling", "rotation")]
        rs, g = _settings(put, case), put(G)
        for _ in range(2 if mode == "persistent_rows" else 1):  # (the second backward leaves the rows that are zero again)
            color, radii, depth, grads = render_view_grads(rs, *args, g, b)
        out = {_MV_NAMES[k]: v for k, v in grads.items() if v is not None}
        if mode == "rgb":
            out["rgb"] = b.rgb
        det = dict(color=color, depth=depth, radii=radii)
        if b.row_state is not None:
            det["row_state"] = b.row_state
        return det, out

    runs = three_runs("multiview", run, tag=mode)
    want, _, _ = _oracle_grads(oracle, "mv", case, G)
    for i, (_, grads) in enumerate(runs):
        _close(grads, want, f"{mode} run {i} vs oracle", keys=[k for k in grads if k != "rgb"])
        if mode == "rgb":
            assert "dL_dsh" not in grads
            _close(grads, runs[-1][1], f"{mode} run {i} vs unpatched", keys=["rgb"])


@pytest.mark.parametrize("P", [257, 1025])
def test_view_message_round_trip(P):
    """Plan, pack and accumulate (test_gpu_parity.py::test_touched_rows_exchange_kernels) on fixed per-view gradients, so
    that every output is deterministic; P on each side of one 1024-row compact block."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    views, M, D = 3, 16, 3
    gen = torch.Generator().manual_seed(P)
    widths = (3, 3, 4, 3, 1)
    rows = [torch.rand(P, generator=gen) < 0.4 for _ in range(views)]
    some = lambda r, k: torch.where(r[:, None], torch.randn(P, k, generator=gen), torch.zeros(P, k))  # noqa: E731
    grads = [[some(r, k) for k in widths] for r in rows]
    rgbs = [some(r, 3) for r in rows]
    cams = [torch.randn(3, generator=gen) for _ in range(views)]
    m3 = torch.randn(P, 3, generator=gen)

    def run(put):
        g5 = [[put(t) for t in g] for g in grads]
        rgb, cam, means = [put(t) for t in rgbs], [put(t) for t in cams], put(m3)
        plans = [_C.view_message_plan(g5[v], rgb[v]) for v in range(views)]
        counts = [c for _, c in plans]
        cap = max(counts) + 5
        words = _C.view_message_words(P, cap)
        messages = put(torch.full((views, words), float("nan")))
        for v in range(views):
            _C.view_message_pack(plans[v][0], g5[v], rgb[v], cam[v], cap, messages[v])
        dense = [put(torch.full((P, k), float("nan"))) for k in widths] + [put(torch.full((P, M, 3), float("nan")))]
        _C.view_messages_accumulate(messages, P, cap, D, M, means, dense)
        sparse = [put(torch.full((P, k), 7.0)) for k in widths] + [put(torch.full((P, M, 3), 7.0))]
        valid = put(torch.full((P,), 7, dtype=torch.uint8))
        _C.view_messages_accumulate(messages, P, cap, D, M, means, sparse, row_valid=valid)
        det = dict(valid=valid, composed=_C.sh_grad_compose(means, torch.stack(cam), torch.stack(rgb), D, M))
        for v in range(views):
            det[f"count{v}"] = counts[v]
            det[f"head{v}"] = messages[v, :4].clone()
        for i, (a, b) in enumerate(zip(dense, sparse)):
            det[f"dense{i}"], det[f"sparse{i}"] = a, b
        return det, None

    det = three_runs("multiview", run, tag=f"messages P{P}")[-1][0]
    any_row = np.zeros(P, bool)
    for v in range(views):
        nz = np.concatenate([g.numpy() for g in grads[v]] + [rgbs[v].numpy()], axis=1).any(axis=1)
        assert det[f"count{v}"] == int(nz.sum()) > 0
        any_row |= nz
    assert np.array_equal(det["valid"].astype(bool), any_row) and not any_row.all()
    for i in range(5):
        seq = grads[0][i] + grads[1][i] + grads[2][i]  # (0 + g0) + g1 + g2, as the kernel adds them
        assert np.array_equal(det[f"dense{i}"], seq.numpy()), i
        assert np.array_equal(det[f"sparse{i}"][any_row], seq.numpy()[any_row]) and (det[f"sparse{i}"][~any_row] == 7.0).all(), i
    assert np.array_equal(det["dense5"], det["composed"])


# ----------------------------------------------------------------------------------------------------------------------
# simple_knn, near points, arrays_equal
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 257, 4097])
def test_knn(oracle, P):
    from gaussianeditor_amd.simple_knn._C import distCUDA2

    pts = torch.rand(P, 3, generator=torch.Generator().manual_seed(P))
    det = three_runs("simple_knn", lambda put: (dict(dist2=distCUDA2(put(pts))), None), tag=f"P{P}")[-1][0]
    want = oracle.knn_mean_dist2(pts.numpy())
    assert np.array_equal(det["dist2"].view(np.uint32), want.view(np.uint32))  # (the bar of test_knn_bit_exact_vs_oracle)


@pytest.mark.parametrize("return_dist", [False, True], ids=["mask", "mask_and_dist"])
@pytest.mark.parametrize("n_query", [1, 300])
def test_near_points(oracle, n_query, return_dist):
    from gaussianeditor_amd.near import near_points

    gen = torch.Generator().manual_seed(n_query)
    ref, qry = torch.rand(257, 3, generator=gen), torch.rand(n_query, 3, generator=gen)
    qry[0] = ref[5] + 0.01

    def run(put):
        out = near_points(put(ref), put(qry), 0.08, return_dist=return_dist)
        return (dict(near=out[0], dist=out[1]) if return_dist else dict(near=out)), None

    det = three_runs("near", run, tag=f"q{n_query}")[-1][0]
    d = torch.cdist(qry.double(), ref.double()).min(dim=1).values.numpy()
    sure = np.abs(d - 0.08) > 1e-6
    assert np.array_equal(det["near"].astype(bool)[sure], (d <= 0.08)[sure]) and det["near"][0]
    if n_query > 1:
        assert det["near"].any() and not det["near"].all()
    if return_dist:
        near = det["near"].astype(bool)
        assert np.abs(det["dist"][near] - d[near]).max() <= 1e-6 and np.isinf(det["dist"][~near & sure]).all()


def test_arrays_equal():
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    gen = torch.Generator().manual_seed(1)
    a, b = torch.randn(257, 3, generator=gen), torch.randint(0, 99, (1025,), generator=gen, dtype=torch.int32)
    a2 = a.clone()
    a2[256, 2] += 1.0  # the very last element differs

    def run(put):
        same = _C.arrays_equal([(put(a), put(a)), (put(b), put(b))])
        differ = _C.arrays_equal([(put(a), put(a2)), (put(b), put(b))])
        return dict(same=same, differ=differ), None

    det = three_runs("arrays_equal", run)[-1][0]
    assert det["same"] is True and det["differ"] is False


# ----------------------------------------------------------------------------------------------------------------------
# fused loss
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tex_5x7", "flat_45x70", "tex_batch"])
def test_fused_loss(name):
    from gaussianeditor_amd.losses import photometric_loss

    fx = LH.fixture()
    x, y = torch.from_numpy(fx[f"{name}/x"].copy()), torch.from_numpy(fx[f"{name}/y"].copy())

    def run(put):
        img = put(x.clone().requires_grad_(True))
        loss, l1, ssim = photometric_loss(img, put(y), LH.LAMBDA, return_terms=True)
        loss.backward()
        return dict(loss=loss, l1=l1, ssim=ssim, grad=img.grad), None

    det = three_runs("fused loss", run, tag=name)[-1][0]
    bar, e = LH.fixture_bar(name), LH.expectation(name)
    for k in ("loss", "l1", "ssim"):
        assert abs(float(det[k]) - e[k]) <= bar[k], (name, k)
    assert np.abs(det["grad"].astype(np.float64) - e["grad"]).max() <= bar["grad"], name


# ----------------------------------------------------------------------------------------------------------------------
# fused Adam
# ----------------------------------------------------------------------------------------------------------------------
def _adam_state(opt, params):
    det = {}
    for k, p in params.items():
        st = opt.state[p]
        det[k], det[k + ".m"], det[k + ".v"] = p.detach(), st["exp_avg"], st["exp_avg_sq"]
    return det


def _adam_steps(put, opt, params, grads):
    for step_grads in grads:
        for k, p in params.items():
            p.grad = put(step_grads[k])
        opt.step()


def _adam_oracle(oracle, init, grads, lrs, steps_mask=None):
    out = {}
    for k, p0 in init.items():
        p, m, v = p0.numpy().copy(), np.zeros(p0.shape, np.float32), np.zeros(p0.shape, np.float32)
        for step, g in enumerate(grads, 1):
            kw = {} if steps_mask is None else dict(row_mask=steps_mask, masked=True)
            oracle.adam_step(p, g[k].numpy(), m, v, lrs[k], step, eps=1e-15, **kw)
        out[k], out[k + ".m"], out[k + ".v"] = p, m, v
    return out


ADAM_SHAPES = dict(aligned=lambda n: [(n, 3), (n, 15, 3), (n, 1), (n, 4)],
                   two_launches=lambda n: [(n, 3), (n, 1), (n, 4), (n, 15, 3), (n, 1, 3), (n, 7), (n, 3), (n,), (n, 2), (n, 4), (n, 5)],
                   masked=lambda n: [(n, 3), (n, 1), (n, 4)])


@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("kind", ["aligned", "two_launches", "masked"])
def test_fused_adam(oracle, kind, n):
    """One aligned tensor set (the float4 path with its scalar tail), eleven tensors (a launch of 8 and one of 3), and a
    masked row step; two steps each, against oracle.adam_step bit for bit."""
    from gaussianeditor_amd.optim import FusedMaskedAdam

    gen = torch.Generator().manual_seed(n)
    shapes = ADAM_SHAPES[kind](n)
    init = {f"t{i}": torch.randn(s, generator=gen) for i, s in enumerate(shapes)}
    lrs = {k: 1e-3 * (i + 1) for i, k in enumerate(init)}
    grads = [{k: torch.randn(t.shape, generator=gen) * (10.0 if step else 0.1) for k, t in init.items()} for step in range(2)]
    mask = (torch.rand(n, generator=gen) > 0.5) if kind == "masked" else None

    def run(put):
        params = {k: torch.nn.Parameter(put(t)) for k, t in init.items()}
        opt = FusedMaskedAdam([{"params": [p], "lr": lrs[k], "name": k, "masked": kind == "masked"} for k, p in params.items()],
                              lr=0.0, eps=1e-15)
        if mask is not None:
            opt.set_row_mask(put(mask))
        _adam_steps(put, opt, params, grads)
        return _adam_state(opt, params), None

    det = three_runs("fused Adam", run, tag=f"{kind} n{n}")[-1][0]
    want = _adam_oracle(oracle, init, grads, lrs, None if mask is None else mask.numpy())
    for k in want:
        assert np.array_equal(det[k], want[k]), (kind, n, k)


@pytest.mark.parametrize("n", [257, 1025])
def test_fused_adam_unaligned_pointers(oracle, n):
    """The tensor set of test_fused_adam_unaligned_pointers_take_the_scalar_path: `a` with the unaligned parameter (rows 5.. of
    an (n + 5, 3) tensor: 60 bytes in), `b` with the unaligned moments, `c` aligned throughout in the same launch."""
    from gaussianeditor_amd.optim import FusedMaskedAdam

    gen = torch.Generator().manual_seed(n)
    big_a = torch.randn(n + 5, 3, generator=gen)
    big_m = torch.zeros(n + 5, 3)
    big_m[:5] = 7.0
    init = dict(a=big_a[5:].clone(), b=torch.randn(n, 3, generator=gen), c=torch.randn(n, 3, generator=gen))
    lrs = dict(a=1.6e-4, b=5e-2, c=5e-3)
    grads = [{k: torch.randn(n, 3, generator=gen) * (10.0 if step else 0.1) for k in init} for step in range(2)]

    def run(put):
        ga, gm, gv = put(big_a), put(big_m), put(big_m)
        params = dict(a=torch.nn.Parameter(ga[5:]), b=torch.nn.Parameter(put(init["b"])), c=torch.nn.Parameter(put(init["c"])))
        assert params["a"].data_ptr() % 16 != 0 and params["a"].is_contiguous() and gm[5:].data_ptr() % 16 != 0
        opt = FusedMaskedAdam([{"params": [p], "lr": lrs[k], "name": k} for k, p in params.items()], lr=0.0, eps=1e-15)
        opt.state[params["b"]] = {"step": torch.tensor(0.0, dtype=torch.float32), "exp_avg": gm[5:], "exp_avg_sq": gv[5:]}
        _adam_steps(put, opt, params, grads)
        det = _adam_state(opt, params)
        det.update(head_a=ga[:5], head_m=gm[:5], head_v=gv[:5])
        return det, None

    det = three_runs("fused Adam", run, tag=f"unaligned n{n}")[-1][0]
    want = _adam_oracle(oracle, init, grads, lrs)
    for k in want:
        assert np.array_equal(det[k], want[k]), (n, k)
    assert np.array_equal(det["head_a"], big_a[:5].numpy()) and (det["head_m"] == 7.0).all() and (det["head_v"] == 7.0).all()


# ----------------------------------------------------------------------------------------------------------------------
# row arena, densify, MCMC
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [257, 1025])
def test_row_arena_compact_and_append(P):
    """Compaction at keep fractions 1, about 0.5 and 0, appends of 1 and 257 rows, against tensor[mask] / torch.cat."""
    from gaussianeditor_amd.arena import RowArena

    gen = torch.Generator().manual_seed(P)
    t = dict(xyz=torch.randn(P, 3, generator=gen), f_rest=torch.randn(P, 15, 3, generator=gen),
             opacity=torch.randn(P, 1, generator=gen), rot=torch.randn(P, 4, generator=gen),
             radii=torch.randint(0, 99, (P,), generator=gen, dtype=torch.int32), mask=torch.rand(P, generator=gen) > 0.5)
    half = torch.rand(P + 1, generator=gen) > 0.5
    ext = {n: dict(xyz=torch.randn(n, 3, generator=gen), f_rest=torch.randn(n, 15, 3, generator=gen),
                   rot=torch.randn(n, 4, generator=gen), mask=torch.rand(n, generator=gen) > 0.5) for n in (1, 257)}
    steps = [("keep_all", lambda A, put: A.compact(put(torch.ones(A.P, dtype=torch.bool)))),
             ("append_1", lambda A, put: A.append({k: put(v) for k, v in ext[1].items()}, n=1)),
             ("keep_half", lambda A, put: A.compact(put(half[:A.P]))),
             ("append_257", lambda A, put: A.append({k: put(v) for k, v in ext[257].items()}, n=257)),
             ("keep_none", lambda A, put: A.compact(put(torch.zeros(A.P, dtype=torch.bool))))]

    def run(put):
        A = RowArena({k: put(v) for k, v in t.items()})
        det = {}
        for name, step in steps:
            step(A, put)
            det[f"{name}.P"] = A.P
            for k in A.names:
                if A.P:
                    det[f"{name}.{k}"] = A[k].clone()
        assert A.allocations == 1
        return det, None

    det = three_runs("row arena", run, tag=f"P{P}")[-1][0]
    want = {k: v.clone() for k, v in t.items()}
    zeros = lambda v, n: torch.zeros((n,) + tuple(v.shape[1:]), dtype=v.dtype)  # noqa: E731
    for name, op in (("keep_all", None), ("append_1", 1), ("keep_half", "half"), ("append_257", 257)):
        if op == "half":
            keep = half[:want["xyz"].shape[0]]
            want = {k: v[keep] for k, v in want.items()}
        elif op is not None:
            want = {k: torch.cat((v, ext[op][k] if k in ext[op] else zeros(v, op))) for k, v in want.items()}
        assert det[f"{name}.P"] == want["xyz"].shape[0]
        for k, v in want.items():
            assert _same_bits(det[f"{name}.{k}"], _host(dict(x=v))["x"]), (name, k)
    assert det["keep_none.P"] == 0


def _model(P, seed, dead_every=None):
    """The six raw parameter tensors of a Gaussian model (host), as tests/test_gpu_mcmc.py and test_gpu_densify_policy.py
    build them."""
    sc = make_case(P, 64, 64, seed=seed, s0=0.03)["sc"]
    f = sc["features"]
    opacity = sc["opacity"].reshape(-1, 1).clamp(0.01, 0.99).clone()
    if dead_every:
        opacity[::dead_every] = 0.003
    return dict(xyz=sc["xyz"].clone(), f_dc=f[:, :1].contiguous(), f_rest=f[:, 1:].contiguous(), opacity=torch.logit(opacity),
                scaling=torch.log(sc["scaling"]), rotation=(sc["rotation"] * 1.7).contiguous())


def _optimizer(put, par, names, seed=3):
    """torch.optim.Adam over the six named groups with non-zero moments (two steps on fixed gradients)."""
    par = {k: torch.nn.Parameter(put(v)) for k, v in par.items()}
    opt = torch.optim.Adam([dict(params=[par[k]], lr=1e-4, name=k) for k in names], lr=0.0, eps=1e-15)
    g = torch.Generator().manual_seed(seed)
    for _ in range(2):
        for p in par.values():
            p.grad = put(torch.randn(p.shape, generator=g) * 1e-3)
        opt.step()
    opt.zero_grad(set_to_none=True)
    return opt


def _opt_state(opt, prefix):
    det = {}
    for g in opt.param_groups:
        p = g["params"][0]
        det[f"{prefix}.{g['name']}"] = p.detach().clone()
        det[f"{prefix}.{g['name']}.m"] = opt.state[p]["exp_avg"].clone()
        det[f"{prefix}.{g['name']}.v"] = opt.state[p]["exp_avg_sq"].clone()
    return det


def test_densify_round():
    """Statistics, selection, split positions, keep mask and the whole densify_and_prune on P = 1025."""
    from gaussianeditor_amd import densify

    P = 1025
    par = _model(P, 11)
    par["opacity"][::50] = float(torch.logit(torch.tensor(0.006)))
    gen = torch.Generator().manual_seed(3)
    stats = [([torch.randn(P, 3, generator=gen) * 4e-4 for _ in range(2)],
              [torch.randint(-1, 30, (P,), generator=gen, dtype=torch.int32) for _ in range(2)]) for _ in range(3)]
    mask = torch.rand(P, generator=gen) < 0.5
    smax = torch.exp(par["scaling"]).max(dim=1).values
    kw = dict(max_grad=dh.MAX_GRAD, max_densify_percent=0.3, percent_dense=float(smax.median()) / dh.EXTENT, extent=dh.EXTENT)

    def run(put):
        opt = _optimizer(put, par, dh.NAMES)
        extra = dict(xyz_gradient_accum=put(torch.zeros(P, 1)), denom=put(torch.zeros(P, 1)), max_radii2D=put(torch.zeros(P)),
                     mask=put(mask), generation=put(torch.zeros(P, dtype=torch.int64)))
        for grads, radii in stats:
            densify.add_densification_stats(extra["xyz_gradient_accum"], extra["denom"], extra["max_radii2D"],
                                            [put(g) for g in grads], [put(r) for r in radii])
        det = {k: extra[k].clone() for k in ("xyz_gradient_accum", "denom", "max_radii2D")}
        now = {g["name"]: g["params"][0].detach() for g in opt.param_groups}
        scaling = torch.exp(now["scaling"])
        sel = densify.select_densification(extra["xyz_gradient_accum"], extra["denom"], extra["mask"], scaling, **kw)
        det.update(clone_sel=sel.clone_sel, split_sel=sel.split_sel, nonzero=sel.nonzero, n_clone=sel.n_clone, n_split=sel.n_split,
                   threshold=sel.threshold)
        noise = torch.randn(2 * sel.n_split, 3, generator=torch.Generator().manual_seed(9))
        det["split_xyz"] = densify.split_positions(now["xyz"], scaling, now["rotation"], sel, put(noise), 2)
        det["split_xyz_mask"] = densify.split_positions(now["xyz"], scaling, now["rotation"], sel.split_sel, put(noise), 2)
        det["keep"] = densify.prune_keep_mask(torch.sigmoid(now["opacity"]).reshape(-1), scaling, extra["mask"], min_opacity=0.02,
                                              max_screen_size=20.0, extent=dh.EXTENT, max_radii2D=extra["max_radii2D"],
                                              drop=sel.split_sel)
        new_par, new_extra, counts = densify.densify_and_prune(
            opt, extra, min_opacity=0.02, max_screen_size=20, N=2, generation_num=1,
            generator=torch.Generator(device=DEV).manual_seed(1234), max_grad=kw["max_grad"],
            max_densify_percent=kw["max_densify_percent"], percent_dense=kw["percent_dense"], extent=kw["extent"])
        det["counts"] = tuple(int(c) for c in counts)
        det.update(_opt_state(opt, "after"))
        det.update({f"extra.{k}": v.clone() for k, v in new_extra.items() if isinstance(v, torch.Tensor)})
        return det, None

    det = three_runs("densify", run)[-1][0]
    before, n_clone, n_split, n_pruned = det["counts"]
    print(f"  densify round: (before, n_clone, n_split, n_pruned) = {det['counts']}")
    assert before == P and min(n_clone, n_split, n_pruned) > 0 and (det["n_clone"], det["n_split"]) == (n_clone, n_split)
    assert det["after.xyz"].shape[0] == before + n_clone + n_split * (2 - 1) - n_pruned  # (the split parents leave: N - 1 each)
    assert _same_bits(det["split_xyz"], det["split_xyz_mask"])
    # the statistics against the numpy restatement of the reference lines, bit for bit
    acc, den, rad = np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32)
    for grads, radii in stats:
        acc, den, rad, _ = dh.stats_np(acc, den, rad, [g.numpy() for g in grads], [r.numpy() for r in radii])
    assert np.array_equal(det["xyz_gradient_accum"].reshape(-1), acc) and np.array_equal(det["denom"].reshape(-1), den)
    assert np.array_equal(det["max_radii2D"], rad)


def test_mcmc_round():
    """Noise, sampling, relocation values and both scatters (relocate, add_new) on P = 1025 with fixed uniform and normal
    numbers."""
    from gaussianeditor_amd import mcmc

    P, MIN_OPACITY, n_new = 1025, 0.005, 51
    par = _model(P, 21, dead_every=7)
    gen = torch.Generator().manual_seed(5)
    noise, u, u2 = torch.randn(P, 3, generator=gen), torch.rand(P, generator=gen), torch.rand(n_new, generator=gen)
    mask = torch.rand(P, generator=gen) < 0.8

    def run(put):
        opt = _optimizer(put, par, mh.NAMES)
        now = {g["name"]: g["params"][0].detach() for g in opt.param_groups}
        m = put(mask)
        mcmc.inject_noise(now["xyz"], now["scaling"], now["rotation"], now["opacity"], put(noise), scaler=5e-3, mask=m)
        det = dict(xyz_noised=now["xyz"].clone())
        opacity = torch.sigmoid(now["opacity"]).reshape(-1).contiguous()
        s = mcmc.classify_and_sample(opacity, put(u), min_opacity=MIN_OPACITY, mask=m)
        n = s.n_draws
        det.update(opacity=opacity, dead_sel=s.dead_sel, dead_idx=s.dead_idx[:s.n_dead].clone(), src=s.src, count=s.count, ratio=s.ratio,
                   n_dead=s.n_dead, n_alive=s.n_alive, n_draws=n, total=s.total)
        src, ratio = s.src[:n].contiguous(), s.ratio[:n].contiguous()
        new_o, new_s = mcmc.relocation_values(opacity, now["scaling"], src, ratio, min_opacity=MIN_OPACITY)
        det.update(new_o=new_o, new_s=new_s)
        mcmc.relocate(opt, s.dead_idx[:n].contiguous(), src, new_o, new_s)
        det.update(_opt_state(opt, "relocated"))
        opacity = torch.sigmoid(opt.param_groups[mh.NAMES.index("opacity")]["params"][0].detach()).reshape(-1).contiguous()
        s2 = mcmc.classify_and_sample(opacity, put(u2), min_opacity=MIN_OPACITY, mask=m, n_draws=n_new)
        scaling = opt.param_groups[mh.NAMES.index("scaling")]["params"][0].detach()
        o2, sc2 = mcmc.relocation_values(opacity, scaling, s2.src, s2.ratio, min_opacity=MIN_OPACITY)
        det.update(src2=s2.src, ratio2=s2.ratio, count2=s2.count, new_o2=o2, new_s2=sc2)
        _, extra = mcmc.add_new(opt, dict(mask=m, denom=put(torch.ones(P, 1))), s2.src, o2, sc2, generation_num=2)
        det.update(_opt_state(opt, "grown"))
        det.update(extra_mask=extra["mask"], extra_denom=extra["denom"])
        return det, None

    det = three_runs("MCMC", run)[-1][0]
    assert det["n_dead"] > 0 and det["n_draws"] == det["n_dead"] and det["total"] > 0
    assert det["grown.xyz"].shape[0] == P + n_new and det["relocated.xyz"].shape[0] == P
    # the draws against the integer restatement, bit for bit
    want = mh.sample_int(det["opacity"], u.numpy(), MIN_OPACITY, mask=mask.numpy())  # (the opacities after the two Adam steps)
    assert want["record"] == (det["n_dead"], det["n_alive"], det["n_draws"], det["total"])
    assert np.array_equal(det["src"][:det["n_draws"]], want["src"][:det["n_draws"]]) and np.array_equal(det["count"], want["count"])
    assert np.array_equal(det["dead_idx"], want["dead_idx"]) and np.array_equal(det["dead_sel"].astype(bool), want["dead_sel"])


# ----------------------------------------------------------------------------------------------------------------------
# the detector sees a real kernel's stores
# ----------------------------------------------------------------------------------------------------------------------
def test_detector_sees_the_alpha_kernels_stores():
    """alpha_image for a 130 x 66 view with understate(4) armed for its output: the kernel writes exactly the bytes the
    tensor has -- all inside the allocation --, the record says the last 4 are guard: 4 changed bytes at `back`, of that
    site, and nothing else."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    W, H = 130, 66
    case = make_case(257, W, H, seed=5, s0=0.6)
    _reset_product_state()
    with GuardedAllocator(0xFF) as ga:
        state = _C.rasterize_gaussians(*_forward_args(ga.place, case), flags=0)
        torch.cuda.synchronize()
        assert ga.check() == []
        ga.understate(4)
        alpha = _C.alpha_image(state[6], H, W)
        got = ga.check()
    print("  understate(4):", got)
    assert len(got) == 1, got
    v = got[0]
    assert (v["side"], v["offset"], v["count"], tuple(v["shape"]), v["dtype"]) == ("back", 0, 4, (1, H, W), torch.float32)
    assert v["site"].startswith(os.path.join("gaussianeditor_amd", "diff_gaussian_rasterization", "_C.py") + ":")
    assert bool(torch.isfinite(alpha).all())
    COUNTS["detector self-test"] += len(ga)
    PRODUCT["detector self-test"] += sum(r["site"].startswith("gaussianeditor_amd") for r in ga.records)


# ----------------------------------------------------------------------------------------------------------------------
# regimes the library reads from the environment once per process
# ----------------------------------------------------------------------------------------------------------------------
REGIMES = {"legacy_16bit_keys": dict(GSR_BIN_LEGACY="1"), "list_segments": dict(GSR_CK_CHUNKS="1", GSR_CK_DEBUG="1")}


@pytest.mark.parametrize("regime", list(REGIMES))
def test_environment_regimes(regime):
    """One forward and backward cell (P = 257, 130 x 66, num_rendered 6082) with the same three assertions in a fresh
    process per regime, one at a time, each under its own time limit.  With GSR_CK_CHUNKS=1 the lists are cut into
    segments and the checkpoint pool is the last section of the image scratch."""
    env = {k: v for k, v in os.environ.items() if k not in ("GSR_BIN_LEGACY", "GSR_CK_CHUNKS", "GSR_CK_DEBUG", "GSR_BWD_SEG", "GSR_SORT_THREADS")}
    env.update(REGIMES[regime])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-s", "-k",
                        "test_rasterizer_num_rendered_between_one_and_two_sort_blocks"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and "failed" not in r.stdout and "all clean" in r.stdout


def test_zz_allocation_counts():
    """The number of guarded allocations each group checked (the table of the module docstring)."""
    for group, n in COUNTS.items():
        print(f"  {group:<22} {n:>6} {PRODUCT[group]:>6}")
        assert n > 0, group
