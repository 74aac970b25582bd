"""-m gpu: the work queues of K7's siblings -- feature_backward_kernel and distortion_backward_kernel (their own work list,
assigned first items, pops of `base + atomic` from the per-XCD cursors, their own decoding of whole and half items,
retire_queue), their forwards and trace_contributions_kernel (run_work_queue<1>), gsr_blend.hip -- at the sizes where an item
is really popped and a workgroup runs a second item on the LDS buffers its first one left.  Every other test of these
kernels uses images of at most 16 tiles: no pop of theirs ever handed out work.

Scenes (tests/sibling_helpers.py; their shape is asserted from the oracle forward): "wide", 640 x 480 = 1 200 tiles, and
"narrow", 320 x 240 = 300 tiles; a sparse background under 64 entries a tile and >= 8 tiles of several hundred entries.
Expectations and bars are the existing ones: the slice builder of features_helpers at helpers.assert_grads_close's defaults
(1e-5, the per-row rule) with the share rule; distortion_helpers.f64_distortion at distortion_helpers.TOL (2e-5) with
f64_regimes.masked_rows (at most 2 % of the rows on "wide", none on "narrow"; CPU: 0 of 3 223 and 0 of 3 700); the exhaustive
reference of contrib_helpers bit for bit.  The step with all four losses is held to the SUM of the oracle's colour, alpha
and slice backwards and the float64 distortion share: the tensors that hold a float64 share at that share's bar, 2e-5 with
the masked rows, on the scale of the share rule; dL_dsh and dL_dfeatures, which hold none, at 1e-5.

Work lists (k7_matrix_helpers.work_items after each sibling backward; asserted): no segment items, tiles < items < 2 tiles
(whole AND half items), and more items than workgroups wherever the grid in use says so -- "wide" at up to 4 waves per SIMD,
"narrow" at 1.  test_on_other_grid_shapes runs the file in fresh processes with GSR_BLEND_WAVES_PER_SIMD = 1, 2, 3, 5, 8 on
the parent's expectations (an .npz in tmp_path).

Measured on the MI355X (256 compute units), default grid: "wide" 1 200 tiles, 1 216 items for the feature backward's 768
workgroups and 1 217 for the distortion backward's 1 024; "narrow" 300 tiles, 353 items.  With one wave per SIMD: 1 216 and 314
items for 256 workgroups.  Worst errors: features 2.2e-6 (bar 1e-5), distortion 1.1e-5 (bar 2e-5; image 3.2e-6), the step with
every loss 4.6e-6; the trace identical in all 3 223 rows and both pixel images.  Times: features 1.2 / 0.5 s ("wide" /
"narrow"), distortion 2.6 and 1.9 / 0.5 s, the step twice 0.7 / 0.4 s, the trace 1.7 s (most of each: the CPU expectation,
computed once); each child 4.2 to 4.7 s (its nine tests 2.7 s); the file 34 s.
With `run_tile(x + 8u * q)` of both backwards guarded by `q < base` in a scratch build -- every popped item skipped --
test_feature_image_and_backward and test_distortion_image_and_backward fail on "wide" (dL_dmeans3D off by 0.82 and 0.29 of
its maximum; "narrow" has no popped item at the default grid)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distortion_helpers as DH
import features_helpers as FH
import k7_matrix_helpers as K
import sibling_helpers as S
from helpers import assert_grads_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "GSR_BLEND_WAVES_PER_SIMD"
SCENES = ["wide", "narrow"]
FEAT_BWD_WAVES_PER_SIMD = 3  # gsr_blend.hip


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def _grids():
    """(workgroups of the distortion backward, of the feature backward): blend_grid_size() / 4 waves, the feature backward's
    capped at 3 per compute unit -- the grid as test_gpu_blend_dispatch._grid reads it."""
    from test_gpu_blend_dispatch import _grid

    cus = torch.cuda.get_device_properties(DH.DEV).multi_processor_count
    return _grid() // 4, min(_grid() // 4, cus * FEAT_BWD_WAVES_PER_SIMD)


def _check_items(name, what, items, workgroups):
    """The list a sibling backward left: no segment items, whole and half items, and popped items where the grid says so."""
    tiles = S.tile_shape(name, S.forward(name))["tiles"]
    cus = torch.cuda.get_device_properties(DH.DEV).multi_processor_count
    print(f"  {name} {what}: items {items[0]} (segment items {items[1]}), tiles {tiles}, workgroups {workgroups}")
    assert items[1] == 0, (name, what, items)
    assert tiles < items[0] < 2 * tiles, (name, what, items, tiles)
    from test_gpu_blend_dispatch import _waves_per_simd

    waves = _waves_per_simd()
    if KNOB not in os.environ:
        assert workgroups in (cus * 4, cus * FEAT_BWD_WAVES_PER_SIMD)
        if name == "wide":  # (stronger than the feature backward's own CUs x 3)
            assert items[0] > cus * 4, (name, what, items, cus)
    # where the computed grid is smaller than the list, items are popped: "wide" at 1 .. 4 waves per SIMD, "narrow" at 1
    if (name == "wide" and waves <= 4) or (name == "narrow" and waves == 1):
        assert items[0] > workgroups, (name, what, "no item is popped", items, workgroups)


def _check_forward(name, out):
    f = S.forward(name)
    assert out["num_rendered"] == int(f["num_rendered"]) and np.array_equal(out["radii"], f["radii"]), name
    assert np.array_equal(_bits(out["color"]), _bits(f["color"])) and np.array_equal(_bits(out["depth"]), _bits(f["depth"])), name


def _check_distortion_image(got, want, tag):
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64).reshape(want.shape) - want).max()) / scale
    print(f"  {tag}: image error {err:.2e} of {scale:.3e} (bar {DH.TOL:.0e})")
    assert err <= DH.TOL, (tag, err)


@pytest.mark.parametrize("name", SCENES)
def test_feature_image_and_backward(name):
    e = S.feature_expectation(name)
    FH.assert_share_visible(e["want"], e["share"], tag=name)
    got, out = S.run_step(name, features=True)
    _check_forward(name, out)
    # the image: equal as floats to the oracle's slice renders (test_feature_image_equals_the_slice_renders_as_floats)
    assert out["features"].shape == e["image"].shape and np.abs(out["features"]).max() > 0.1
    assert np.array_equal(_bits(out["features"]), _bits(e["image"])), np.abs(out["features"] - e["image"]).max()
    _check_items(name, "feature backward", out["items"], _grids()[1])
    worst = FH.assert_feature_grads_close(got, e["want"], e["smax"], tag=f"features [{name}]", keys=list(got))
    print(f"  features [{name}]: worst {worst:.2e}")


@pytest.mark.parametrize("mapped", [False, True], ids=["linear", "mapped"])
@pytest.mark.parametrize("name", SCENES)
def test_distortion_image_and_backward(name, mapped):
    e = S.distortion_expectation(name, mapped=mapped)
    tag = f"distortion [{name}{', mapped' if mapped else ''}]"
    DH.assert_share_visible(e, tag)
    got, out = S.run_step(name, distortion=True, mapped=mapped, lam=e["lam"])
    _check_forward(name, out)
    _check_distortion_image(out["distortion"], e["image"], tag)
    _check_items(name, "distortion backward", out["items"], _grids()[0])
    assert all(np.isfinite(v).all() for v in got.values())
    worst = assert_grads_close(got, e["want"], tol=DH.TOL, tag=tag, masked=e["masked"], keys=DH.KEYS)
    print(f"  {tag}: worst {worst:.2e} (bar {DH.TOL:.0e}), masked rows {int(e['masked'].sum())}, lam {e['lam']:.0e}")
    assert_grads_close(got, e["colour_only"], tol=DH.TOL, tag=tag + " dL_dsh", masked=e["masked"], keys=["dL_dsh"])


@pytest.mark.parametrize("name", SCENES)
def test_one_step_with_every_loss_twice(name):
    """K7, then the feature backward, then the distortion backward on one view, and the same step once more: a cursor one of
    them left standing shows as missing items in the next launch of that queue kind."""
    e = S.step_expectation(name)
    f, d = S.feature_expectation(name), S.distortion_expectation(name)
    rest = ["dL_dsh", "dL_dfeatures"]  # (no float64 share in them)
    steps = []
    for i in range(2):
        got, out = S.run_step(name, features=True, distortion=True, alpha=True, lam=e["lam"])
        tag = f"step {i} [{name}]"
        _check_forward(name, out)
        assert np.array_equal(_bits(out["features"]), _bits(f["image"])), tag
        _check_distortion_image(out["distortion"], d["image"], tag)
        _check_items(name, f"step {i}, distortion backward", out["items"], _grids()[0])
        worst = FH.assert_feature_grads_close(got, e["want"], e["smax"], tol=DH.TOL, tag=tag, masked=e["masked"], keys=DH.KEYS)
        FH.assert_feature_grads_close(got, e["want"], e["smax"], tag=tag, keys=rest)
        print(f"  {tag}: worst {worst:.2e} (bar {DH.TOL:.0e})")
        assert K.acc_tables_are_zero(), tag
        steps.append(out)
    a, b = steps
    assert a["num_rendered"] == b["num_rendered"] and a["items"] == b["items"]
    for k in ("color", "depth", "features", "distortion", "alpha"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (name, k, "differs between the two steps")


def test_contribution_trace_where_its_pops_succeed():
    """"wide": 4 800 quadrant items for 4 096 waves at the default grid.  Bit for bit, as
    test_gpu_contrib.py::test_exhaustive_cases_bit_for_bit."""
    from test_gpu_contrib import _trace

    e = S.trace_expectation("wide")
    assert int(e["tied"]) == 0, "a pixel with a tied top weight: the scene is the wrong choice, not the kernel"
    table, top_id, top_w = _trace(S.scene("wide"))
    want = e["table"]
    bad = np.argwhere(table != want)
    print(f"  wide: rows hit {int((want[:, 0] > 0).sum())} of {want.shape[0]}, cells that differ {len(bad)}, top ids that differ "
          f"{int((top_id != e['top_id']).sum())}, top weights that differ {int((top_w != e['top_weight']).sum())}")
    assert len(bad) == 0, (bad[:5], table[bad[:5, 0]], want[bad[:5, 0]])
    assert np.array_equal(top_id, e["top_id"]) and np.array_equal(top_w.view(np.uint32), e["top_weight"].view(np.uint32))
    assert int((want[:, 0] > 0).sum()) > 1000


@pytest.mark.parametrize("waves", ["1", "2", "3", "5", "8"])
def test_on_other_grid_shapes(waves, tmp_path):
    """This file (without this test) in a fresh process per value of GSR_BLEND_WAVES_PER_SIMD, on the parent's expectations."""
    path = str(tmp_path / "expect.npz")
    for name in SCENES:
        S.forward(name), S.feature_expectation(name), S.distortion_expectation(name), S.distortion_expectation(name, mapped=True)
        S.step_expectation(name)
    S.trace_expectation("wide")
    S.save(path)
    env = {k: v for k, v in os.environ.items() if k != KNOB}
    env.update({KNOB: waves, S.EXPECT_ENV: path})
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-s", "-k",
                        "not test_on_other_grid_shapes"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print("\n".join(ln for ln in r.stdout.splitlines() if "items" in ln or " passed" in ln or " failed" in ln))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:]
