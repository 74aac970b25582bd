"""-m gpu: the blend backward's flush (the `flush` of backward_tile, gsr_blend.hip: one lane per (chunk slot, accumulator
column), unconditional LDS reads, the column's term chosen by selects, one exec region around the atomic) at the shapes where
one wrong slot, column or stale LDS row shows.  Every comparison is with the CPU oracle at helpers.assert_grads_close's
defaults, through k7_matrix_helpers.run (which also proves the kernel that ran); the scenes' premises are asserted on the
oracle's forward alone.

  one tile, list lengths 1, 63, 64, 65, 128, 129   a 16 x 16 image whose tile lists every Gaussian and whose deepest
            contributor is the list's last entry: full chunks, the partial last chunk (the walk is back to front: the partial
            chunk is the list's FRONT), a used slot at the highest index of a partial chunk;
  one tile, n = 1, 4, 5, 16, 17 small Gaussians, each reaching ONE quadrant (asserted: the alpha >= 1/255 ellipse against the
            quadrants' pixel rectangles), dealt round robin over the quadrants, and 64 large ones that reach all four: the
            numbers of chunk slots some quadrant kept at the edges of a 4-slot flush instruction and of a wave's 16 slots;
  one tile, whole chunks no quadrant keeps (160 entries of opacity 0.002 < 1/255, by depth between two groups of 40): two
            adjacent chunks without a survivor, one of each parity of the double buffer, between chunks with survivors;
  more items than persistent workgroups (scene 2 of test_gpu_k7_work_items.py, the count asserted as there): an LDS row left
            non-zero by one item would reach the next item of the same workgroup; and the same in a fresh process with list
            segments and half tiles forced, together with the 8 SEG rows of the instantiation matrix (the 16 others run here);
  K7 alone  gsr_blend_backward into a caller's table with the row mask: marked rows == non-zero rows; and on the one-tile
            scenes, where every (Gaussian, column) receives exactly one atomic, two backwards leave bit-identical tables
            wherever the LDS cell behind the atomic has one value -- with the pixel gradient confined to one quadrant at a
            time on every scene, with the whole gradient on the scene whose Gaussians reach one quadrant each (three or four
            quadrant waves add to a cell in the order they arrive: such cells differ from run to run in the kernel before
            this file as well, profiles/k7_flush_used_slots_ab.md section 3);
  self-clean   every comparison above ends with the persistent accumulator table all zero behind gsr_preprocess_backward.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import k7_matrix_helpers as K
from helpers import assert_grads_close, make_case, oracle_backward, oracle_forward, seed_gradient, settings

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: set in the fresh process of test_forced_segments_and_seg_rows_in_a_fresh_process: the tests of that process exist there only
CHILD = os.environ.get("GSR_TEST_K7_FLUSH_CHILD")
SEG_KNOBS = {"GSR_CK_CHUNKS": "4", "GSR_BWD_SEG": "1", "GSR_CK_DEBUG": "1"}
LENGTHS = (1, 63, 64, 65, 128, 129)
PLACED = (1, 4, 5, 16, 17)
_cache = {}


def _finish(case, oracle):
    H, W = case["H"], case["W"]
    G = seed_gradient(H, W, 5) * (H * W)
    f = oracle_forward(oracle, case)
    return case, G, f, oracle_backward(oracle, case, f, G)


def _pixels(case, xyz):
    """Pixel coordinates of world points (ndc2Pix of the reference's projection)."""
    h = torch.cat([xyz, torch.ones(len(xyz), 1)], 1) @ case["cam"].full_proj_transform
    ndc = h[:, :2] / h[:, 3:4]
    return torch.stack([((ndc[:, 0] + 1) * case["W"] - 1) * 0.5, ((ndc[:, 1] + 1) * case["H"] - 1) * 0.5], 1)


def _quadrants_reached(f, ids):
    """Per Gaussian of `ids`: how many 8 x 8 quadrants of tile 0 its alpha >= 1/255 ellipse reaches (the minimum of the
    quadratic form over the quadrant's pixel-centre rectangle against 2 ln(255 o), in float64)."""
    co, xy = f["conic_opacity"].astype(np.float64)[ids], f["means2D"].astype(np.float64)[ids]
    A, B, C, o = co[:, 0], co[:, 1], co[:, 2], co[:, 3]
    tau2 = 2.0 * np.log(np.maximum(255.0 * o, 1e-30))
    n = np.zeros(len(ids), dtype=np.int64)
    for q in range(4):
        xl, yl = 8 * (q & 1) - xy[:, 0], 8 * (q >> 1) - xy[:, 1]
        xh, yh = xl + 7, yl + 7
        cx, cy = np.clip(0, xl, xh), np.clip(0, yl, yh)
        x1, y2 = np.clip(-B * cy / A, xl, xh), np.clip(-B * cx / C, yl, yh)
        q1 = A * x1 * x1 + 2 * B * x1 * cy + C * cy * cy
        q2 = A * cx * cx + 2 * B * cx * y2 + C * y2 * y2
        n += (o >= 1.0 / 255.0) & (np.minimum(q1, q2) <= tau2)
    return n


def _scene(key, oracle):
    """(case, G, the oracle's forward, the oracle's gradients), built once per process and never modified."""
    if key in _cache:
        return _cache[key]
    kind, n = key
    if kind == "len":  # n Gaussians about a pixel wide around the camera's target: one tile lists them all
        case = make_case(n, 16, 16, seed=30 + n, s0=0.3, scale_xyz=0.5)
    elif kind == "placed":  # n of 4 096 candidates, each within a pixel of the centre of quadrant i % 4
        case = make_case(4096, 16, 16, seed=41, s0=0.3, scale_xyz=1.6)
        sc = case["sc"]
        px = _pixels(case, sc["xyz"])
        per_q = [torch.nonzero(((px - torch.tensor([3.5 + 8 * (q & 1), 3.5 + 8 * (q >> 1)])).abs().max(dim=1).values < 1.0))[:, 0]
                 for q in range(4)]
        pick = torch.stack([per_q[i % 4][i // 4] for i in range(n)])
        for k in ("xyz", "scaling", "rotation", "opacity", "features"):
            sc[k] = sc[k][pick].contiguous()
        sc["scaling"] = torch.full_like(sc["scaling"], 0.03)  # 0.1 pixel: the 0.3 low-pass makes it 0.56, the ellipse < 2 wide
        sc["opacity"] = torch.full_like(sc["opacity"], 0.8)
    elif kind == "large":  # n Gaussians six pixels wide: every quadrant keeps every one
        case = make_case(n, 16, 16, seed=47, s0=0.3, scale_xyz=0.5)
        case["sc"]["scaling"] = torch.full_like(case["sc"]["scaling"], 1.7)
        case["sc"]["opacity"] = torch.full_like(case["sc"]["opacity"], 0.05)
    else:  # "gap": 40 in front, 160 of opacity 0.002 in the middle, 40 behind, along the viewing direction
        case = make_case(240, 16, 16, seed=43, s0=0.3)
        sc, c = case["sc"], case["cam"].camera_center
        fwd = -c / c.norm()
        u = sc["xyz"]  # uniform in [-1, 1]^3
        lateral = 0.5 * (u - (u @ fwd)[:, None] * fwd[None, :])
        t = 0.3 * u[:, 2] + torch.cat([torch.full((40,), -1.0), torch.zeros(160), torch.full((40,), 1.0)])
        sc["xyz"] = (lateral + t[:, None] * fwd[None, :]).contiguous()
        sc["opacity"] = sc["opacity"].clone()
        sc["opacity"][40:200] = 0.002
    _cache[key] = _finish(case, oracle)
    return _cache[key]


def _compare(key, oracle, row=(0, None, 0, 0, 0)):
    case, G, f, want = _scene(key, oracle)
    got, out = K.run(case, row, G)
    assert out["R"] == f["num_rendered"]
    worst = assert_grads_close(got, want, tag=str(key), keys=list(got))
    assert K.acc_tables_are_zero(), (key, "the persistent accumulator table is not all zero behind gsr_preprocess_backward")
    print(f"  {key}: R {out['R']}, deepest contributor {int(f['n_contrib'].max())}, items {out['items']}, "
          f"kernel {K.row_id(K.row_of(out['index']))}, worst {worst:.2e}")
    return f, out


def _k7_alone(case, G):
    """gsr_blend_backward alone into a caller's table (cleared by the call), with the row mask -> (acc (P,16), touched (P,))."""
    from gaussianeditor_amd import _native
    from test_gpu_alpha import _forward_state

    P, H, W = case["sc"]["xyz"].shape[0], case["H"], case["W"]
    rs = settings(case, K.DEV)
    R, _, _, _, geom, binning, img = _forward_state(case)
    Gd = G.to(K.DEV).contiguous()
    acc = torch.full((P, 16), float("nan"), device=K.DEV)
    touched = torch.full((((P + 15) // 16) * 16,), 7, dtype=torch.uint8, device=K.DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    _native.check("k7", _native.lib().gsr_blend_backward(torch.cuda.current_stream().cuda_stream, P, R, W, H, p(rs.bg), p(geom),
                                                         p(binning), p(img), p(Gd), p(acc), p(touched), 4))
    torch.cuda.synchronize()
    return acc.cpu().numpy(), touched[:P].cpu().numpy()


if CHILD is None:
    @pytest.mark.parametrize("L", LENGTHS)
    def test_one_tile_list_lengths(oracle, L):
        f = _scene(("len", L), oracle)[2]
        assert f["num_rendered"] == L and int(f["n_contrib"].max()) == L, "one tile lists every Gaussian, and the last one contributes"
        _compare(("len", L), oracle)

    @pytest.mark.parametrize("n", PLACED)
    def test_one_tile_small_gaussians_that_reach_one_quadrant_each(oracle, n):
        f = _scene(("placed", n), oracle)[2]
        assert f["num_rendered"] == n and (_quadrants_reached(f, np.arange(n)) == 1).all()
        _compare(("placed", n), oracle)

    def test_one_tile_large_gaussians_that_reach_every_quadrant(oracle):
        f = _scene(("large", 64), oracle)[2]
        assert f["num_rendered"] == 64 and int(f["n_contrib"].max()) == 64 and (_quadrants_reached(f, np.arange(64)) == 4).all()
        _compare(("large", 64), oracle)

    def test_one_tile_with_whole_chunks_that_no_quadrant_keeps(oracle):
        f = _scene(("gap", 240), oracle)[2]
        order = f["point_list"][f["ranges"][0, 0]:f["ranges"][0, 1]]
        assert f["num_rendered"] == 240 and int(f["n_contrib"].max()) == 240
        # by depth: positions 40 .. 199 hold the 160 entries below 1/255; back to front the chunks are [176, 240), [112, 176),
        # [48, 112), [0, 48): the second and the third hold nothing any quadrant keeps
        assert sorted(order[40:200].tolist()) == list(range(40, 200)) and (_quadrants_reached(f, np.arange(40, 200)) == 0).all()
        assert (_quadrants_reached(f, order[:40]) > 0).any() and (_quadrants_reached(f, order[200:]) > 0).any()
        _compare(("gap", 240), oracle)

    @pytest.mark.parametrize("key", [("len", 129), ("placed", 17), ("large", 64), ("gap", 240)], ids=lambda k: f"{k[0]}{k[1]}")
    def test_k7_alone_row_mask_and_bit_identical_tables_on_one_tile(oracle, key):
        """One tile, whole (16 x 16 is below every cut): the row mask marks exactly the rows that are not all zero, and every
        (Gaussian, column) receives exactly one atomic.  The table then has ONE value wherever the LDS cell behind the atomic
        has one: the four quadrant waves' ds_add_f32 reach a cell in any order, so a cell that three or four quadrants add
        non-zeros to rounds differently from run to run (measured on the kernel before this file as on the one with it:
        profiles/k7_flush_used_slots_ab.md), and one that at most two do cannot (x + y commutes, and a wave without a gradient
        adds zeros, exactly).  So bit identity is asked with the pixel gradient confined to one quadrant at a time -- every
        slot that quadrant keeps goes through the flush, the other waves add zeros -- and, on the scene whose Gaussians
        reach one quadrant each, with the whole gradient."""
        case, G, f, _ = _scene(key, oracle)
        acc, touched = _k7_alone(case, G)
        _, touched2 = _k7_alone(case, G)
        rows = (acc != 0).any(axis=1)
        assert np.isfinite(acc).all() and rows.any()
        assert np.array_equal(touched != 0, rows) and touched.max() == 1 and np.array_equal(touched, touched2)
        masks = [torch.ones(1, 16, 16)] if key[0] == "placed" else []
        for q in range(4):
            m = torch.zeros(1, 16, 16)
            m[:, 8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8] = 1.0
            masks.append(m)
        marked = 0
        for i, m in enumerate(masks):
            a1, t1 = _k7_alone(case, G * m)
            a2, t2 = _k7_alone(case, G * m)
            assert np.array_equal(a1.view(np.uint32), a2.view(np.uint32)), (key, i, "two backwards of one tile differ")
            assert np.array_equal(t1 != 0, (a1 != 0).any(axis=1)) and np.array_equal(t1, t2)
            marked += int(t1.sum())
        assert marked >= int(rows.sum())  # (every Gaussian with a gradient has one from some quadrant)

    def test_more_items_than_workgroups(oracle):
        from test_gpu_k7_work_items import _scene as work_scene, _workgroups

        case, G, f, want = work_scene("scene2")
        got, out = K.run(case, (0, None, 0, 0, 0), G)
        assert out["R"] == f["num_rendered"] and out["items"][0] > _workgroups(), (out["items"], _workgroups())
        worst = assert_grads_close(got, want, tag="scene2", keys=list(got))
        assert K.acc_tables_are_zero()
        acc, touched = _k7_alone(case, G)
        assert np.isfinite(acc).all() and np.array_equal(touched != 0, (acc != 0).any(axis=1))
        print(f"  scene2: items {out['items']}, workgroups {_workgroups()}, worst {worst:.2e}, rows marked {int(touched.sum())}")

    @pytest.mark.parametrize("row", [r for r in K.ROWS if not r[1]], ids=K.row_id)
    def test_row_without_seg(oracle, row):
        case, G, GA, GD = K.scene("p2000")
        K.check_row(oracle, case, row, G, GA, GD, f"{K.row_id(row)} p2000")

    def test_forced_segments_and_seg_rows_in_a_fresh_process():
        env = dict(os.environ, GSR_TEST_K7_FLUSH_CHILD="1", **SEG_KNOBS)
        p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", os.path.abspath(__file__)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert p.returncode == 0 and "9 passed" in p.stdout, (p.stdout + p.stderr)[-4000:]  # (scene 2 and the 8 SEG rows)
        print("\n".join(ln.lstrip(".") for ln in p.stdout.splitlines() if ln.lstrip(".").startswith("  ") or "passed" in ln))
else:
    def test_child_scene2_with_list_segments_and_half_tiles(oracle):
        from test_gpu_k7_work_items import _scene as work_scene

        case, G, f, want = work_scene("scene2")
        got, out = K.run(case, (0, 1, 0, 0, 0), G)
        assert out["R"] == f["num_rendered"] and out["items"][1] >= 1, ("no list-segment item in the work list", out["items"])
        worst = assert_grads_close(got, want, tag="scene2, segments forced", keys=list(got))
        assert K.acc_tables_are_zero()
        print(f"  scene2, segments forced: items {out['items']}, worst {worst:.2e}")

    @pytest.mark.parametrize("row", [r for r in K.ROWS if r[1]], ids=K.row_id)
    def test_child_seg_row(oracle, row):
        case, G, GA, GD = K.scene("p20000")
        K.check_row(oracle, case, row, G, GA, GD, f"{K.row_id(row)} p20000")
