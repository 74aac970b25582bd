"""-m gpu: the forward's checkpoints (K6) and the backward's list segments (K7) as production runs them -- no knob in the
environment: the non-uniform table checkpoint_helpers.FINE_POS, GSR_BWD_SEG's default of 5 eighths with the 4/5 rule -- on the
scenes of tests/checkpoint_helpers.py, whose regimes tests/test_cpu_checkpoints.py proves from the oracle alone.

  A. every one-tile scene and every edge(n): forward bit-identical to the oracle at every stage, gradients through the L1 module
     within f64_regimes.TOL of float64 autograd and within 1e-5 of the oracle, the launch counter that moved carries the SEG
     bit iff on(R, W, H), and the work list holds exactly ns(deep) list-segment items where the tile must be cut, none where
     it must not be;
  B. `saturating` (K6 leaves the walk early: checkpoints behind the stop are never written) with the image scratch poisoned;
  C. `cap`: more checkpointing tiles than CK_TILES_CAP -- the tiles without slots are never cut;
  D. `wide`: the work-list kernel's re-read path (T > 8 192 tiles) with segments, in ONE fresh process under GSR_CK_CHUNKS=4
     GSR_BWD_SEG=1, against a second one with GSR_BWD_SEG=0;
  E. neighbours of a checkpointed view: depth / abs / alpha / fast-exp backwards, apply_weights, a colour-override render served
     by view reuse between a render and its backward, deep -> shallow -> deep views.

The six gaps and the tests that reach them (each test asserts the precondition that proves it did, from the oracle):
  1. slots 10-15 and the tail beyond 16 384      test_one_tile_scene[reach], [edge16384], [edge16385]  (ns = 16 / 15 / 16)
  2. the table's boundaries                       test_one_tile_scene[edge256 .. edge16385]             (deep == n exactly)
  3. more than CK_TILES_CAP checkpointing tiles   test_cap_tiles_without_slots_are_never_cut            (T = 2 600, deep > 256 in all)
  4. the re-read path with segments               test_wide_in_fresh_processes                          (T = 8 385, segment items > 0)
  5. K6 stops early / writes more than K7 uses    test_saturating_under_poison; test_one_tile_scene[edge*] (K6 walks 17 500, K7 n)
  6. calls sharing a checkpointed view's state    test_neighbour_rows, test_neighbour_depth_row,
                                                  test_apply_weights_beside_a_checkpointed_view,
                                                  test_colour_override_between_render_and_backward, test_deep_shallow_deep

Bars: bit identity for the forward; f64_regimes.TOL against float64 (its bounded mask); helpers.assert_grads_close at 1e-5
against the oracle; SPREAD = 2e-6 (test_gpu_parity.test_backward_run_to_run_spread) between two runs of the same backward.

Measured on the MI355X (one run of the file; work list as (items, list-segment items); worst |got - want| / max |want| over a
scene's tensors against the oracle / against float64; no row masked anywhere: 0 flipped pixels on every scene):
  scene       R      deep   ns  launched   work list   vs oracle  vs float64
  reach       17 500 17 489 16  -S---[2]   (16, 16)    1.25e-6    2.31e-6
  ragged       3 300  3 297 10  -S---[2]   (10, 10)    8.03e-7    2.88e-6
  just_on      1 300  1 300  6  -S---[2]   (6, 6)      7.43e-7    3.08e-6
  just_off     1 199  1 199  -  -----[0]   (2, 0)      1.11e-6    1.36e-6
  edge256     17 500    256  1  -S---[2]   (2, 0)      7.18e-7    4.09e-6
  edge257     17 500    257  2  -S---[2]   (2, 0)      7.63e-7    5.81e-6   the 4/5 rule keeps the tile whole
  edge1536    17 500  1 536  6  -S---[2]   (6, 6)      4.94e-7    2.53e-6
  edge1537    17 500  1 537  7  -S---[2]   (7, 7)      4.94e-7    2.33e-6
  edge2048    17 500  2 048  7  -S---[2]   (7, 7)      5.60e-7    2.28e-6   the 4/5 rule cuts the tile
  edge2049    17 500  2 049  8  -S---[2]   (8, 8)      5.14e-7    1.27e-6
  edge16384   17 500 16 384 15  -S---[2]   (15, 15)    1.25e-6    2.36e-6
  edge16385   17 500 16 385 16  -S---[2]   (16, 16)    1.25e-6    2.31e-6
  saturating   6 000  2 632  9  -S---[2]   (9, 9)      1.35e-6    1.49e-6   under poison 0xFF / 0x5A: 12 guarded allocations
                                                                            each, forward bit-identical, spread 1.9e-8 / 1.5e-7
  cap          4 006 496, 2 600 tiles, lists 589..2 294: -S---[2], (2 614, 16) -- at most 13 585 segment items, 552 tiles without
               slots -- 1.11e-6 against the oracle
  wide         162 808, 8 385 tiles, GSR_CK_CHUNKS=4: GSR_BWD_SEG=1 -S---[2] (8 325, 384), 5.65e-7; GSR_BWD_SEG=0 -----[0]
               (8 111, 0), 6.06e-7; forward bit-identical, spread between the two 4.0e-7
  ragged's neighbours: -S-B-[10] (10, 10) 8.03e-7, absgrad 8.35e-7; -S--L[18] (10, 10) 1.10e-6; FS---[3] (10, 10) 1.6e-8 (against
               the product's own FAST backward); --D--[4] (2, 0) 9.69e-7 beside the colour-only run's (10, 10); a colour-override
               render between render and backward: spread 2.5e-8
  Every stage of every forward was bit-exact (test_gpu_parity._compare_forward's report: all True).
  The saturating scene had to be walked ~2 000 deep before its tile was cut: with the opaque wall 320, 1 000 and 1 500 positions
  deep the work list held (2, 0), with it 2 000 or more deep (ns, ns) (checkpoint_helpers._saturating says why).
  time: the file 25 s; the two fresh processes of `wide` 4.5 s + 5.0 s, `cap` 5.1 s (3.8 s of them the oracle), reach 2.0 s
  (oracle + float64 of 17 500 entries in one tile), every edge(n) 0.7 s, saturating 0.3 s, everything else below 0.4 s.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import checkpoint_helpers as C
import f64_regimes as F
import k7_matrix_helpers as K
from helpers import assert_grads_close, hip_state, oracle_forward, rel_err, seed_gradient, settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
SPREAD = 2e-6
#: set in the fresh processes of part D ("seg:<npz>" / "control:<npz>"): their tests are defined there and only there
CHILD = os.environ.get("GSR_CHECKPOINT_TESTS_CHILD")
PLAIN = (0, None, 0, 0, 0)


@pytest.fixture(scope="module", autouse=True)
def _knobs():
    """Production runs with none of the knobs: a knob in the environment would turn this file into a test of something else, so
    it FAILS (the children of part D run under exactly the knobs their parent gave them)."""
    have = {k: os.environ[k] for k in C.KNOBS if k in os.environ}
    if CHILD is None:
        assert not have, f"unset {sorted(have)}: this file tests the default checkpoint table and work-list rules"
    else:
        assert have == dict(C.WIDE_KNOBS, GSR_BWD_SEG="1" if CHILD.startswith("seg:") else "0"), have
    yield


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def _forward(oracle, name):
    """test_gpu_parity._compare_forward on the scene (every integer stage bit-exact), and the images and the blend's per-pixel
    state bit for bit -> the oracle's forward."""
    import test_gpu_parity as tp

    r = C.scene(oracle, name)
    case = r["case"]
    f, (R, color, depth, radii, geom, binning, img) = tp._compare_forward(oracle, case)
    st = hip_state(case["sc"]["xyz"].shape[0], R, case["W"], case["H"], geom, binning, img)
    assert np.array_equal(_bits(color.cpu().numpy()), _bits(f["color"])), (name, "colour image")
    assert np.array_equal(_bits(depth.cpu().numpy()), _bits(f["depth"])), (name, "depth image")
    assert np.array_equal(_bits(st["final_T"]), _bits(f["final_T"])), (name, "final_T")
    assert np.array_equal(st["n_contrib"], f["n_contrib"].reshape(-1)), (name, "n_contrib")
    return f, color


def _l1_backward(oracle, name):
    """The gradients through the L1 module (test_gpu_parity._grads_hip) held to float64 and to the oracle -> (gradients, index
    of the K7 launch counter that moved)."""
    import test_gpu_parity as tp

    r = C.scene(oracle, name)
    torch.cuda.synchronize()
    before = K.launches()
    h = tp._grads_hip(r["case"], r["G"])
    hit = np.nonzero(K.launches() - before)[0].tolist()
    assert len(hit) == 1, (name, "one K7 launch expected", hit)
    g = C.backward(oracle, name)
    worst = assert_grads_close(h, g, tol=1e-5, tag=f"{name}: L1 module vs oracle", keys=list(h))
    want, mask, report = C.f64(oracle, name)
    w64 = assert_grads_close(h, want, tol=F.TOL, tag=f"{name}: L1 module vs float64", masked=mask, keys=list(want))
    print(f"  {name}: launched {K.row_id(K.row_of(hit[0]))}, vs oracle {worst:.2e}, vs float64 {w64:.2e} ({report})")
    return h, hit[0]


def _direct_backward(oracle, name, **kw):
    """One forward + backward through _C (k7_matrix_helpers.run): the gradients held to the oracle -> (gradients, out)."""
    r = C.scene(oracle, name)
    got, out = K.run(r["case"], PLAIN, r["G"], **kw)
    worst = assert_grads_close(got, C.backward(oracle, name), tol=1e-5, tag=f"{name}: _C vs oracle", keys=list(got))
    print(f"  {name}: _C launched {K.row_id(K.row_of(out['index']))}, work list {out['items']}, vs oracle {worst:.2e}")
    return got, out


if CHILD is None:
    # -----------------------------------------------------------------------------------------------------------------
    # A. one tile
    @pytest.mark.parametrize("name", [n for n in C.ONE_TILE if n != "saturating"])
    def test_one_tile_scene(oracle, name):
        fa = C.facts(oracle, name)
        deep, ns = int(fa["deep"][0]), int(fa["ns"][0])
        if name.startswith("edge"):
            assert deep == int(name[4:])  # (the precondition the boundary rests on; tests/test_cpu_checkpoints.py has the rest)
        _forward(oracle, name)
        _, l1 = _l1_backward(oracle, name)
        _, out = _direct_backward(oracle, name)
        items, seg = out["items"]
        print(f"  {name}: deep {deep}, ns {ns}, on {fa['on']}: work list ({items}, {seg})")
        for index in (l1, out["index"]):
            assert bool(index & 2) == bool(fa["on"]), (name, K.row_id(K.row_of(index)), "SEG bit != on()")
        if name in C.CUT:
            assert seg == ns, (name, "the tile must be cut into ns segments", seg, ns)
        elif name in C.NEVER_CUT:
            assert seg == 0, (name, seg)
        else:
            assert name in C.EITHER and seg in (0, ns), (name, seg, ns)
        assert items - seg in ((1, 2) if seg == 0 else (0,)), (name, "one tile: whole, halved or cut", out["items"])

    # -----------------------------------------------------------------------------------------------------------------
    # B. K6 leaves the walk early
    def test_saturating_under_poison(oracle):
        """No gradient may depend on a checkpoint slot K6 never wrote: with every allocation of the product poisoned (0xFF: NaN
        as a float, 0x5A: a large finite one) the forward is what it is without, bit for bit, and the backward within the
        run-to-run spread."""
        from guarded_alloc import GuardedAllocator

        name = "saturating"
        fa = C.facts(oracle, name)
        ns = int(fa["ns"][0])
        assert fa["on"] and C.FINE_POS[1] < int(fa["deep"][0]) < fa["R"] // 2
        _forward(oracle, name)
        _l1_backward(oracle, name)
        plain, out = _direct_backward(oracle, name)
        assert out["index"] & 2 and out["items"] == (ns, ns), out["items"]
        for pattern in (0xFF, 0x5A):
            with GuardedAllocator(pattern) as ga:
                got, o = _direct_backward(oracle, name)
                ga.assert_clean()
                made = len(ga)
            assert made > 0 and o["items"] == out["items"] and o["index"] == out["index"]
            for k in ("color", "depth"):
                assert np.array_equal(_bits(o[k]), _bits(out[k])), (k, f"depends on the poison {pattern:#04x}")
            spread = {k: rel_err(got[k], plain[k]) for k in got}
            print(f"  saturating, poison {pattern:#04x}: {made} guarded allocations, spread {max(spread.values()):.1e}")
            assert max(spread.values()) <= SPREAD, spread

    # -----------------------------------------------------------------------------------------------------------------
    # C. more checkpointing tiles than slots
    def test_cap_tiles_without_slots_are_never_cut(oracle):
        fa = C.facts(oracle, "cap")
        T, nonempty = fa["T"], int((fa["lengths"] > 0).sum())
        assert T > C.CK_TILES_CAP and fa["on"] and nonempty == T and fa["deep"].min() > C.FINE_POS[1]
        t0 = time.time()
        _forward(oracle, "cap")
        got, out = _direct_backward(oracle, "cap")
        items, seg = out["items"]
        most = int(np.sort(fa["ns"])[-C.CK_TILES_CAP:].sum())
        print(f"  cap: work list ({items}, {seg}), at most {most} segment items, {nonempty - C.CK_TILES_CAP} tiles without slots; "
              f"{time.time() - t0:.1f} s with the oracle")
        assert out["index"] & 2
        assert 0 < seg <= most, (seg, most)
        assert items - seg >= nonempty - C.CK_TILES_CAP, (items, seg)  # whole or halved, never segments

    # -----------------------------------------------------------------------------------------------------------------
    # D. the work list's re-read path with segments: fresh processes
    def _fresh(cmd, env, timeout=300):
        return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)

    def test_wide_in_fresh_processes(tmp_path):
        path = str(tmp_path / "wide_seg.npz")
        env = {k: v for k, v in os.environ.items() if k not in C.KNOBS}
        for mode, seg_share, passed in (("seg", "1", 1), ("control", "0", 1)):
            t0 = time.time()
            p = _fresh([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", os.path.abspath(__file__), "-k", f"wide_child_{mode}"],
                       dict(env, GSR_CHECKPOINT_TESTS_CHILD=f"{mode}:{path}", **dict(C.WIDE_KNOBS, GSR_BWD_SEG=seg_share)))
            assert p.returncode == 0, (p.stdout + p.stderr)[-6000:]
            assert f"{passed} passed" in p.stdout, p.stdout[-3000:]
            print("\n".join(ln.lstrip(".") for ln in p.stdout.splitlines() if ln.lstrip(".").startswith("  ") or "passed" in ln))
            print(f"  fresh process ({mode}): {time.time() - t0:.1f} s")
        assert os.path.exists(path)

    # -----------------------------------------------------------------------------------------------------------------
    # E. neighbours of a checkpointed view
    def _ragged_gradients(oracle):
        r = C.scene(oracle, "ragged")
        H, W = r["case"]["H"], r["case"]["W"]
        GA = seed_gradient(H, W, 5)[:1] * H * W
        GD = seed_gradient(H, W, 7)[:1] * H * W / float(r["case"]["cam"].camera_center.norm())
        return r, GA, GD

    ROWS = [(0, 1, 0, 1, 0), (0, 1, 0, 0, 1), (1, 1, 0, 0, 0)]

    @pytest.mark.parametrize("row", ROWS, ids=K.row_id)
    def test_neighbour_rows(oracle, row):
        """The abs-grad, alpha and fast-exp backwards of a view that checkpoints by default: k7_matrix_helpers.check_row, and
        the tile is cut into the ns segments the colour-only backward cuts it into."""
        fa = C.facts(oracle, "ragged")
        assert fa["on"] and int(fa["ns"][0]) == 10
        r, GA, GD = _ragged_gradients(oracle)
        rep = K.check_row(oracle, r["case"], row, r["G"], GA, GD, f"{K.row_id(row)} ragged")
        assert rep["items"] == (10, 10), rep["items"]

    def test_neighbour_depth_row(oracle):
        """The depth backward excludes SEG by design: on a view whose colour-only backward launches -S---[2] and is cut into
        ns segments it must launch --D--[4] and cut nothing.  check_row's comparison, written out: check_row would take the
        colour-only run the depth run must differ from through the row's own SEG switch (0), and on this view that run
        launches the SEG kernel."""
        import alpha_helpers as AH

        row = (0, 0, 1, 0, 0)
        tag = f"{K.row_id(row)} ragged"
        fa = C.facts(oracle, "ragged")
        assert fa["on"] and int(fa["ns"][0]) == 10
        r, _, GD = _ragged_gradients(oracle)
        want, shares = K.expectation(oracle, r["case"], r["G"], None, GD, shares=True)
        AH.assert_share_visible(want, shares["depth"], tag=tag + " depth share")
        got, out = K.run(r["case"], row, r["G"], None, GD)  # (asserts that counter 4 and no other rose by one)
        assert out["index"] == K.index(row) and out["items"][1] == 0 and out["items"][0] in (1, 2), out["items"]
        colour_only, oc = K.run(r["case"], (0, 1, 0, 0, 0), r["G"])
        assert oc["items"] == (10, 10), oc["items"]
        AH.assert_differs_from_colour_only(got, colour_only, want, tag=tag + " depth")
        worst = assert_grads_close(got, want, tol=1e-5, tag=tag, keys=list(got))
        print(f"  {tag}: items {out['items']}, worst {worst:.2e}; the colour-only run's {oc['items']}")
        assert K.acc_tables_are_zero()

    def test_apply_weights_beside_a_checkpointed_view(oracle):
        """apply_weights (C = 1) of the view between a checkpointed render and a second one: exact against the oracle (0/1
        masks), and the render after it is the render before it."""
        from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

        r = C.scene(oracle, "ragged")
        case = r["case"]
        sc, cam, W, H, P = case["sc"], case["cam"], case["W"], case["H"], case["sc"]["xyz"].shape[0]
        assert C.facts(oracle, "ragged")["on"]
        mask = (torch.rand(1, H, W, generator=torch.Generator().manual_seed(12)) > 0.5).float()
        w_ref, c_ref = np.zeros((P, 1), np.float32), np.zeros((P,), np.int32)
        oracle.apply_weights(sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], None, cam.world_view_transform,
                             cam.full_proj_transform, cam.camera_center, W, H, case["tfx"], case["tfy"], mask, w_ref, c_ref)
        first, _ = _direct_backward(oracle, "ragged")
        w = torch.zeros((P, 1), device=DEV)
        cnt = torch.zeros((P, 1), dtype=torch.int32, device=DEV)
        GaussianRasterizer(settings(case, DEV, D=0)).apply_weights(
            sc["xyz"].to(DEV), None, sc["opacity"].to(DEV), None, w, sc["scaling"].to(DEV), sc["rotation"].to(DEV), None, cnt,
            mask.to(DEV))
        torch.cuda.synchronize()
        assert c_ref.sum() > 0 and np.array_equal(cnt.cpu().numpy().reshape(-1), c_ref) and np.array_equal(w.cpu().numpy(), w_ref)
        again, out = _direct_backward(oracle, "ragged")
        assert out["items"][1] == 10 and max(rel_err(again[k], first[k]) for k in first) <= SPREAD

    def test_colour_override_between_render_and_backward(oracle):
        """Full render -> colour-override render of the same camera, served by view reuse (rasterize_gaussians_aux on the first
        render's state: the AUX kernel must not touch the checkpoint pool, tile_maxc or ck_work) -> backward of the FIRST."""
        import test_gpu_parity as tp
        from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer, _reuse

        r = C.scene(oracle, "ragged")
        case, G = r["case"], r["G"]
        sc, W, H, P = case["sc"], case["W"], case["H"], case["sc"]["xyz"].shape[0]
        assert C.facts(oracle, "ragged")["on"]
        plain = tp._grads_hip(case, G)
        leaf = lambda t: t.to(DEV).clone().requires_grad_(True)  # noqa: E731
        xyz, op, sh, scl, rot = (leaf(sc[k]) for k in ("xyz", "opacity", "features", "scaling", "rotation"))
        m2d = torch.zeros_like(xyz, requires_grad=True)
        rast = GaussianRasterizer(settings(case, DEV))
        color, radii, depth = rast(xyz, m2d, op, shs=sh, scales=scl, rotations=rot)
        e = _reuse._local.entries[xyz.device]
        state = lambda: hip_state(P, e.R, W, H, e.geom, e.binning, e.img)  # noqa: E731
        st0, hits = state(), _reuse.stats["hits"]
        cols = torch.rand(P, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
        with torch.no_grad():
            sem, _, _ = rast(xyz, torch.zeros_like(xyz), op, colors_precomp=cols, scales=scl, rotations=rot)
        assert _reuse.stats["hits"] == hits + 1, "the colour-override render was not served from the first render's state"
        assert rel_err(sem.cpu().numpy(), oracle_forward(oracle, case, colors_precomp=cols.cpu())["color"]) <= 1e-6
        st1 = state()
        for k in ("n_contrib", "final_T", "ranges", "point_list"):
            assert np.array_equal(st0[k].view(np.uint32), st1[k].view(np.uint32)), (k, "changed by the colour-override render")
        torch.cuda.synchronize()
        before = K.launches()
        (color * G.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        hit = np.nonzero(K.launches() - before)[0].tolist()
        assert hit == [K.index((0, 1, 0, 0, 0))], hit
        assert K.work_items(e.img, H, W) == (10, 10)
        got = dict(dL_dmeans3D=xyz.grad, dL_dopacity=op.grad, dL_dmeans2D=m2d.grad, dL_dsh=sh.grad, dL_dscales=scl.grad,
                   dL_drotations=rot.grad)
        got = {k: v.cpu().numpy() for k, v in got.items()}
        spread = {k: rel_err(got[k], plain[k]) for k in got}
        print(f"  ragged, colour-override render in between: spread {max(spread.values()):.1e}")
        assert max(spread.values()) <= SPREAD, spread
        assert_grads_close(got, C.backward(oracle, "ragged"), tol=1e-5, tag="ragged after the override render", keys=list(got))

    def test_deep_shallow_deep(oracle):
        """reach -> just_off -> reach through the L1 module in one process: a view without checkpoints between two with."""
        fa = [C.facts(oracle, n) for n in ("reach", "just_off")]
        assert fa[0]["on"] and not fa[1]["on"]
        images, indices = [], []
        for name in ("reach", "just_off", "reach"):
            _, color = _forward(oracle, name)
            _, index = _l1_backward(oracle, name)
            images.append(color.cpu().numpy())
            indices.append(index)
        assert np.array_equal(_bits(images[0]), _bits(images[2]))
        assert [bool(i & 2) for i in indices] == [True, False, True], indices

else:
    # -----------------------------------------------------------------------------------------------------------------
    # D, in the fresh processes
    _MODE, _PATH = CHILD.split(":", 1)

    def _wide_run(oracle):
        fa = C.facts(oracle, "wide")
        assert fa["T"] > C.REGS_TILES and (fa["deep"][:200] > 512).sum() >= 4 and (fa["deep"][C.REGS_TILES + 1:] > 512).sum() >= 4
        _forward(oracle, "wide")
        return _direct_backward(oracle, "wide")

    if _MODE == "seg":
        def test_wide_child_seg(oracle):
            got, out = _wide_run(oracle)
            assert out["index"] == K.index((0, 1, 0, 0, 0)) and out["items"][1] > 0, out["items"]
            np.savez(_PATH, color=out["color"], items=np.array(out["items"]), **got)
    else:
        def test_wide_child_control(oracle):
            """GSR_BWD_SEG=0: the same forward, no tile cut -- the gradients of the segmented backward are these."""
            want = np.load(_PATH)
            got, out = _wide_run(oracle)
            assert out["items"][1] == 0 and int(want["items"][1]) > 0, (out["items"], want["items"])
            assert np.array_equal(_bits(out["color"]), _bits(want["color"]))
            spread = {k: rel_err(want[k], got[k]) for k in got}
            print(f"  wide: segmented {tuple(int(v) for v in want['items'])} vs whole {out['items']}: spread {max(spread.values()):.1e}")
            assert max(spread.values()) <= SPREAD, spread
