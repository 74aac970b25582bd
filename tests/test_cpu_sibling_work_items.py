"""CPU companion of tests/test_gpu_sibling_work_items.py: the scenes of tests/sibling_helpers.py have the shape the GPU
file needs, and its comparisons would notice a lost work item.

The expectations are linear in the pixel gradient, so "the kernel lost an item" is modelled exactly by the expectation of a
pixel gradient that is zero on that item's pixels: the lightest tile of "narrow" (one whole item, the smallest gradient a
lost item can take away) and quadrants 0 and 1 of one of its heavy tiles (one half item).  The unchanged comparison
functions, at their unchanged bars, must fail on all four.

Measured here: the lightest tile of "narrow" holds 9 entries; losing it moves the feature expectation by 1.9e-2 of the
scale (dL_dfeatures: 5.7e-2; bar 1e-5) and the distortion expectation by 1.9e-3 (bar 2e-5); losing the half item moves them
by 2.9e-1 and 3.8e-1.  The float32 oracle's colour backward lies within 3.0e-6 ("wide", P = 3 223) and 9.3e-6 ("narrow",
P = 3 700; no row masked on either) of float64 autograd."""
import numpy as np
import pytest

import contrib_helpers as CH
import distortion_helpers as DH
import features_helpers as FH
import sibling_helpers as S
from helpers import assert_grads_close, oracle_backward, oracle_forward


@pytest.mark.parametrize("name", ["wide", "narrow"])
def test_scene_shape_masked_rows_and_the_oracles_margin(oracle, name):
    case = S.scene(name)
    f = S.forward(name)
    shape = S.tile_shape(name, f)
    assert shape["tiles"] == {"wide": 1200, "narrow": 300}[name]
    P = case["sc"]["xyz"].shape[0]
    for mapped in (False, True):
        e = S.distortion_expectation(name, mapped=mapped)  # (asserts the cap on the masked rows)
        DH.assert_share_visible(e, f"{name} mapped {mapped}")
    assert int(e["masked"].sum()) <= S.SCENES[name]["masked_cap"] * P
    fe = S.feature_expectation(name)
    FH.assert_share_visible(fe["want"], fe["share"], tag=name)
    # the float32 oracle against float64 autograd on the colour loss: the margin the oracle-built expectations leave
    full = oracle_forward(oracle, case)
    got = oracle_backward(oracle, case, full, S.inputs(name)["G"])
    worst = assert_grads_close(got, e["colour_only"], tol=DH.TOL, tag=name, masked=e["masked"], keys=DH.KEYS + ["dL_dsh"])
    print(f"  {name}: P {P}, masked rows {int(e['masked'].sum())}, oracle against float64 {worst:.2e} (bar {DH.TOL:.0e})")


def _lost_items(name):
    shape = S.tile_shape(name, S.forward(name))
    heavy = int(np.nonzero(shape["heavy"])[0][0])
    return {"the lightest tile": S.tile_mask(name, shape["lightest"]), "a half item": S.tile_mask(name, heavy, (0, 1))}


@pytest.mark.parametrize("lost", ["the lightest tile", "a half item"])
def test_a_lost_item_fails_the_feature_comparison(lost):
    e = S.feature_expectation("narrow")
    FH.assert_feature_grads_close(e["want"], e["want"], e["smax"], tag="narrow, nothing lost", keys=list(e["want"]))
    less = S.feature_expectation("narrow", GF=S.inputs("narrow")["GF"] * _lost_items("narrow")[lost])
    with pytest.raises(AssertionError):
        FH.assert_feature_grads_close(less["want"], e["want"], e["smax"], tag=f"narrow without {lost}", keys=list(e["want"]))
    with pytest.raises(AssertionError):  # ... and on dL_dfeatures alone
        FH.assert_feature_grads_close(less["want"], e["want"], e["smax"], tag=f"narrow without {lost}", keys=["dL_dfeatures"])


@pytest.mark.parametrize("lost", ["the lightest tile", "a half item"])
def test_a_lost_item_fails_the_distortion_comparison(lost):
    e = S.distortion_expectation("narrow")
    assert_grads_close(e["want"], e["want"], tol=DH.TOL, tag="narrow", masked=e["masked"], keys=DH.KEYS)
    less = S.distortion_expectation("narrow", GDist=S.inputs("narrow")["GDist"] * _lost_items("narrow")[lost], lam=e["lam"])
    err = max(np.abs(less["want"][k] - e["want"][k]).max() / np.abs(e["want"][k]).max() for k in DH.KEYS)
    print(f"  narrow without {lost}: the expectation moves by {err:.2e} of its maximum (bar {DH.TOL:.0e})")
    with pytest.raises(AssertionError):
        assert_grads_close(less["want"], e["want"], tol=DH.TOL, tag=f"narrow without {lost}", masked=e["masked"], keys=DH.KEYS)


@pytest.mark.parametrize("name", ["fifteen_tiles", "ragged"])
def test_the_packed_trace_reference_is_contrib_helpers_exhaustive_one(oracle, name):
    exp = CH.exhaustive_expectation(oracle, name)
    got = S.exhaustive_trace(oracle, exp["case"])
    assert got["tied"] == exp["tied"] == 0
    assert np.array_equal(got["table"], CH.expected_table(exp))
    assert np.array_equal(got["top_id"], exp["top_id"])
    assert np.array_equal(got["top_weight"].view(np.uint32), exp["top_weight"].view(np.uint32))


def test_the_store_survives_a_file(tmp_path):
    e = S.feature_expectation("narrow")
    S.forward("narrow")
    path = str(tmp_path / "expect.npz")
    S.save(path)
    kept = dict(S._store)
    try:
        S._store.clear()
        S.load(path)
        assert sorted(S._store) == sorted(kept) and all(np.array_equal(S._store[k], kept[k]) for k in kept)
        again = S.feature_expectation("narrow")
        assert all(np.array_equal(again["want"][k], e["want"][k]) for k in e["want"]) and again["smax"] == e["smax"]
    finally:
        S._store.clear()
        S._store.update(kept)
