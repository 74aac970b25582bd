"""Without a GPU: the yardstick of tests/test_gpu_k7_matrix.py and the two debug entry points it proves its dispatch with.

  * the combined builder of <G, C> + <GA, A> + <GD, D> (k7_matrix_helpers.expectation, rows without FAST: the float32 oracle's
    linearity construction) against float64 autograd (oracle/torch_ref.render_f64) at f64_regimes.TOL, on the "depth" regime
    case of tests/f64_regimes.py and on seed 8 of the shape sweep;
  * the sweep's discrimination condition, on the oracle alone;
  * gsr_debug_blend_backward_launches / gsr_debug_blend_backward_items: NULL / non-positive arguments are refused, and a
    fresh process that never launched a backward reads 32 zeros."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import alpha_helpers as AH
import f64_regimes as R
import k7_matrix_helpers as K
from helpers import assert_grads_close, seed_gradient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f64_alpha_term(f, r, GA):
    """float64 autograd of <GA, A>, A the first channel of the ones render on background 0 -> gradient dict in the
    reference's conventions (f64_regimes: dL_dscales w.r.t. the modified scale)."""
    from oracle.torch_ref import render_f64

    case, d = r["case"], torch.float64
    sc, cam = case["sc"], case["cam"]
    P, W, H = sc["xyz"].shape[0], case["W"], case["H"]
    leaf = lambda t: t.to(d).clone().requires_grad_(True)  # noqa: E731
    xyz, op, scl, rot = leaf(sc["xyz"]), leaf(sc["opacity"]), leaf(sc["scaling"]), leaf(sc["rotation"])
    m2 = torch.zeros(P, 3, dtype=d, requires_grad=True)
    render_f64(f, xyz, m2, op, scl, rot, None, torch.ones(P, 3, dtype=d), None, cam.world_view_transform,
               cam.full_proj_transform, cam.camera_center, torch.zeros(3), W, H, case["tfx"], case["tfy"], r["sm"], r["D"],
               dL_dimage=AH.ones_gradient(GA, H, W).to(d))
    out = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy()
           for k, t in dict(dL_dmeans3D=xyz, dL_dmeans2D=m2, dL_dopacity=op, dL_dscales=scl, dL_drotations=rot).items()}
    out["dL_dscales"] = out["dL_dscales"] / r["sm"]
    return out


def _regimes(name):
    if name == "depth":
        r = R.regime("depth")
        H, W = r["case"]["H"], r["case"]["W"]
        return r, seed_gradient(H, W, 83)[:1] * H * W
    from test_gpu_parity import sweep_case

    seed = int(name[5:])
    case, sm, D = sweep_case(seed)
    H, W = case["H"], case["W"]
    r = dict(name=name, case=case, D=D, sm=sm, colors_precomp=None, cov3D_precomp=None, G=seed_gradient(H, W, seed) * (H * W),
             GD=seed_gradient(H, W, seed + 90)[:1] * (H * W))
    return r, seed_gradient(H, W, seed + 50)[:1] * (H * W)


@pytest.mark.parametrize("name", ["depth", "sweep8"])
def test_combined_expectation_equals_float64_autograd(oracle, name):
    """The float32 oracle-built sum of the three constructions == float64 autograd of the one loss, rows under flipped
    pixels masked and bounded as everywhere (f64_regimes.masked_rows).  Measured: worst 1.6e-6 of a tensor's maximum on the
    regime case (2 flipped pixels of 27 200, 127 Gaussians under them), 1.3e-6 on sweep seed 8 (none flipped); bar 2e-5."""
    from helpers import oracle_forward

    r, GA = _regimes(name)
    kw = dict(D=r["D"], scale_modifier=r["sm"])
    f = oracle_forward(oracle, r["case"], **kw)
    want, shares = K.expectation(oracle, r["case"], r["G"], GA, r["GD"], shares=True, **kw)
    got64, stats, _ = R.f64_run(f, r)  # <G, C> + <GD, D>
    a64 = _f64_alpha_term(f, r, GA)
    for k, v in a64.items():
        got64[k] = got64[k] + v.reshape(got64[k].shape)
    masked, report = R.masked_rows(r, f, stats)
    keys = R.grad_keys(r)
    worst = assert_grads_close(want, got64, tol=R.TOL, tag=f"combined expectation vs float64 [{name}]", masked=masked, keys=keys)
    rows = {n: K.share_rows(want, s) for n, s in shares.items()}
    print(f"  [{name}] worst {worst:.2e} (bar {R.TOL}), {report}; rows whose share > {AH.SHARE_REL} of the total's maximum: {rows}")
    # every term is in the sum: on the sweep seed each share is visible in the total (on the regime case, a scene of nearly
    # opaque disks, the alpha share is not: 2 rows), and on both the alpha share is the float64 term's by its own maximum
    if name != "depth":
        assert all(n >= K.SWEEP_SHARE_ROWS for rr in rows.values() for n in rr.values()), rows
    assert_grads_close(shares["alpha"], a64, tol=R.TOL, tag=f"alpha share vs float64 [{name}]", masked=masked, keys=list(AH.SHARE_KEYS))


@pytest.mark.parametrize("name", ["p2000", "p20000", "ragged"])
def test_matrix_scenes_discriminate(oracle, name):
    """The scenes of the 24 rows, on the oracle alone: with all three terms in the loss the alpha share and the depth share
    each pass alpha_helpers.assert_share_visible (> 1e-2 of the total's maximum on >= 100 rows of each tensor).  Measured
    minima over the tensors, alpha / depth: 225 / 317, 283 / 293, 184 / 236."""
    case, G, GA, GD = K.scene(name)
    want, shares = K.expectation(oracle, case, G, GA, GD, shares=True)
    for n in ("alpha", "depth"):
        AH.assert_share_visible(want, shares[n], tag=f"{name} {n} share")
    # ... and with the alpha term alone next to the colour (the rows without DEPTH)
    want, shares = K.expectation(oracle, case, G, GA, None, shares=True)
    AH.assert_share_visible(want, shares["alpha"], tag=f"{name} alpha share, no depth term")
    want, shares = K.expectation(oracle, case, G, None, GD, shares=True)
    AH.assert_share_visible(want, shares["depth"], tag=f"{name} depth share, no alpha term")


@pytest.mark.parametrize("seed", range(12))
def test_sweep_discrimination_condition(oracle, seed):
    """On seeds 2, 3, 6, 7, 8, 9, 10, 11 the alpha share and the depth share each exceed 1e-2 of the total's maximum on >= 8 rows
    of each of alpha_helpers.SHARE_KEYS (measured minima over the tensors, alpha / depth: 46 / 53, 10 / 13, 17 / 33, 48 / 138,
    113 / 257, 19 / 37, 89 / 232, 96 / 304); seeds 0, 1, 4, 5 (P <= 256 on one-pixel-wide or empty views: 0 - 5 such rows on
    some tensor) are compared without it.  Also: the two-term expectation is the three-term one without its depth share."""
    s = K.sweep_expectation(oracle, seed)
    K.assert_sweep_discriminates(s, seed)
    if seed not in K.SWEEP_DISCRIMINATING:
        assert min(n for r in s["rows"].values() for n in r.values()) <= 5
    for k in AH.SHARE_KEYS:
        d = np.abs(s["want3"][k] - s["shares"]["depth"][k] - s["want2"][k].reshape(s["want3"][k].shape)).max()
        assert d <= 1e-12 * max(np.abs(s["want3"][k]).max(), 1e-30), (k, d)


def test_debug_entry_points_refuse_bad_arguments_and_start_from_zero():
    from gaussianeditor_amd import _native

    L = _native.lib()
    one, c2 = ctypes.c_void_p(256), (ctypes.c_int64 * 2)(7, 7)
    assert L.gsr_debug_blend_backward_launches(None) == -1
    assert L.gsr_debug_blend_backward_items(None, 64, 64, None, c2) == -1
    assert L.gsr_debug_blend_backward_items(None, 64, 64, one, None) == -1
    assert L.gsr_debug_blend_backward_items(None, 0, 64, one, c2) == -1 and L.gsr_debug_blend_backward_items(None, 64, -1, one, c2) == -1
    assert L.gsr_debug_blend_backward_items(None, 16400, 16400, one, c2) == -1  # (more than GSR_MAX_TILES tiles)
    assert c2[0] == 7 and c2[1] == 7
    # a fresh process that launched nothing reads zeros (this one may have run GPU tests before)
    code = ("import ctypes; from gaussianeditor_amd import _native; c = (ctypes.c_uint64 * 32)(*([9] * 32)); "
            "assert _native.lib().gsr_debug_blend_backward_launches(c) == 0; print('counts', sum(c), len(c))")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0 and "counts 0 32" in p.stdout, p.stdout + p.stderr
    assert len(K.ROWS) == 24 and sorted(K.index(r) for r in K.ROWS) == [i for i in range(32) if not (i & 2 and i & 4)]
    assert all(K.row_of(K.index(r)) == r for r in K.ROWS)
