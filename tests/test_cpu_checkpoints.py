"""GPU-less: every scene of tests/checkpoint_helpers.py is in the regime it was built for, by the oracle alone -- R, on(), deep,
ns and the family rules -- and, for the one-tile scenes, the oracle's gradients (the GPU tests' 1e-5 reference) are within
f64_regimes.TOL of float64 autograd with that module's bounded mask.  A scene that drifts out of its regime fails here, not
silently on the GPU.

`cap` (2 600 tiles, 4.0 M list entries) and `wide` (8 385 tiles) assert R / deep / ns only: float64 autograd of them is out of
reach (render_f64 holds a tile's whole list per pixel; minutes and gigabytes at these sizes).

Measured (oracle against float64, worst tensor): 5.7e-7 (saturating) .. 5.8e-6 (edge257, dL_dscales), reach 2.4e-6; no pixel
flipped and no row masked on any scene; the oracle takes 0.1-0.4 s per one-tile scene, float64 under 1 s, `cap` 5 s (forward
only); the file 14 s."""
import numpy as np
import pytest

import checkpoint_helpers as C
import f64_regimes as F
from helpers import assert_grads_close, rel_err


def test_the_model_on_the_table_by_hand():
    """ns() on the table's boundaries, worked out by hand from FINE_POS; a tile is cut only if deeper than FINE_POS[1]."""
    assert C.FINE_POS == (0, 256, 512, 768, 1024, 1280, 1536, 2048, 2560, 3072, 4096, 5120, 6144, 8192, 12288, 16384)
    assert all(b > a for a, b in zip(C.FINE_POS, C.FINE_POS[1:])) and C.FINE_POS[6:8] == (1536, 2048)
    want = {1: 1, 256: 1, 257: 2, 1536: 6, 1537: 7, 2048: 7, 2049: 8, 3297: 10, 16384: 15, 16385: 16, 17489: 16, 10 ** 6: 16}
    assert {d: C.ns(d) for d in want} == want
    assert C.uniform_pos(4)[:3] == (0, 256, 512) and C.ns(513, C.uniform_pos(4)) == 3
    assert C.on(1200, 16, 16) and not C.on(1199, 16, 16) and C.on(1200 * 4096, 1024, 1024) and not C.on(2047 * 4225, 1040, 1040)


@pytest.mark.parametrize("name", C.ONE_TILE)
def test_one_tile_scene_is_in_its_regime(oracle, name):
    r, fa, f = C.scene(oracle, name), C.facts(oracle, name), C.forward(oracle, name)
    W, H = r["case"]["W"], r["case"]["H"]
    R, deep, ns = fa["R"], int(fa["deep"][0]), int(fa["ns"][0])
    print(f"  {name}: R {R}, on {fa['on']}, deep {deep}, ns {ns}")
    assert fa["T"] == 1 and ns == C.ns(deep)
    if name == "reach":  # every slot, and the tail behind the table's reach
        assert R == 17500 and fa["on"] and deep > C.FINE_POS[-1] and ns == C.CK_MAX
    elif name == "ragged":  # an image smaller than a tile; slots on both sides of the 256 -> 512 stride change
        assert W < 16 and H < 16 and fa["on"] and deep > C.FINE_POS[8] and ns == 10
    elif name == "just_on":
        assert R == 1300 and fa["on"] and deep > C.FINE_POS[1] and ns == 6
    elif name == "just_off":
        assert R == 1199 and not fa["on"] and deep > C.FINE_POS[1]
    elif name.startswith("edge"):
        # K6 walks (and checkpoints) all 17 500 positions -- the pixels beside the cube never stop --, K7's walk ends at n
        assert r["n"] == int(name[4:]) and deep == r["n"] and R == 17500 and fa["on"]
        assert float(f["final_T"].max()) == 1.0
    elif name == "saturating":
        # (the issue asks for final_T < 1e-4 on every pixel; final_T is the transmittance in front of the entry that would
        #  take it below 1e-4, so it never is.  What is meant is asserted on the walk itself: every pixel STOPS, in the first
        #  half of the list, and checkpoints lie behind the chunk in which the last one does)
        stop = C.stop_positions(f, W, H)
        assert R >= 3000 and fa["on"] and C.FINE_POS[1] < deep < R // 2
        assert (stop > 0).all() and deep <= int(stop.max()) < R // 2, (int(stop.min()), int(stop.max()))
        assert float(f["final_T"].max()) < 1e-2  # (a stopped pixel's: T (1 - alpha) < 1e-4 with alpha <= 0.99)
        unwritten = [p for p in C.FINE_POS if int(stop.max()) + 64 <= p < R]
        assert len(unwritten) >= 3 and ns == 9, (unwritten, ns)
    # the reference of the GPU comparison against float64
    want, mask, report = C.f64(oracle, name)
    g = C.backward(oracle, name)
    worst = assert_grads_close({k: g[k] for k in want}, want, tol=F.TOL, tag=f"{name}: oracle vs float64", masked=mask)
    errs = {k[3:]: rel_err(np.asarray(g[k]).reshape(want[k].shape)[~mask], want[k][~mask]) for k in want}
    print(f"  {name}: {report}; oracle vs float64 worst {worst:.2e} " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert worst <= F.TOL / 2, "the reference itself is too far from float64 for the GPU comparison: choose another seed"


def test_cap_has_more_checkpointing_tiles_than_slots_to_own(oracle):
    """R / deep / ns only (module docstring: no float64 run at this size)."""
    fa = C.facts(oracle, "cap")
    T, L, deep = fa["T"], fa["lengths"], fa["deep"]
    print(f"  cap: R {fa['R']} = {fa['R'] / T:.0f} per tile, lists {L.min()}..{L.max()}, deep {deep.min()}..{deep.max()}, "
          f"sum of the 2 048 largest ns {int(np.sort(fa['ns'])[-C.CK_TILES_CAP:].sum())}")
    assert T == 2600 > C.CK_TILES_CAP and fa["on"] and fa["R"] >= 1.1 * 1200 * T
    assert (L > 0).all()  # every tile is ranked: T - 2 048 = 552 get no slot ...
    assert deep.min() > C.FINE_POS[1]  # ... and each of them is walked deeper than the first checkpoint
    assert (fa["ns"] >= 2).all()


def test_wide_has_deep_tiles_at_both_ends_of_a_list_the_kernel_re_reads(oracle):
    """R / deep / ns only.  Under GSR_CK_CHUNKS=4 every view checkpoints, at 256 k: deep > 512 reaches three segments."""
    r, fa = C.scene(oracle, "wide"), C.facts(oracle, "wide")
    deep = fa["deep"]
    first, last = np.nonzero(deep[:200] > 512)[0], C.REGS_TILES + 1 + np.nonzero(deep[C.REGS_TILES + 1:] > 512)[0]
    print(f"  wide: R {fa['R']}, T {fa['T']}, deep > 512 in tiles {first.tolist()} and {last.tolist()}")
    assert r["case"]["sc"]["xyz"].shape[0] <= 30000 and (r["case"]["W"], r["case"]["H"]) == (2064, 1040)
    assert fa["T"] == 129 * 65 > C.REGS_TILES
    assert first.size >= 4 and last.size >= 4
    assert all(n >= 3 for n in fa["ns"][first]) and all(n >= 3 for n in fa["ns"][last])
