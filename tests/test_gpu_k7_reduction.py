"""-m gpu: the packed wave reduction of the blend backward's group loop (wave_sum4_pack and the single ds_add_f32 behind it,
gsr_blend.hip) on scenes small enough that ONE wrong lane shows: every lane of a wave ends up with the total of one (moment,
entry) of a group of four, and the lowest lane of every total adds it to the LDS accumulator of the entry's chunk slot.

  a. lane coverage   one 16 x 16 tile under 5 Gaussians that cover it (5: two groups, the second padded with three null
                     entries), dL_dpixel non-zero at ONE pixel: a backward for each of the 64 pixels of quadrant 0 and for four
                     pixels of each other quadrant.  With one live lane per wave a total taken from the wrong lane, or a lane
                     left out of a sum, is a wrong value, not a rounding error;
  b. group padding   the same tile under P = 1 .. 9 Gaussians, dense dL_dpixel: 1 .. 3 null entries, one to three groups;
  c. quadrant sums   32 x 32 (four tiles), small Gaussians whose alpha >= 1/255 footprint reaches exactly 1, 2 and 4 quadrants
                     of their tile (asserted on the oracle's own geometry): the LDS accumulation over the four waves;
  d. row widths      the padding scenes under depth gradients (10 moments), absgrad (11), both (12), the alpha image's
                     gradient and the hardware 2^x.

Every comparison: all rasterizer-input gradients against the CPU oracle (the builders of tests/k7_matrix_helpers.py), bars
helpers.assert_grads_close with its defaults, 1e-5 of the tensor's maximum + the per-row bar.  The hardware-2^x rows are held
to the oracle too (it has no such exponential: 2^x differs from expf by about an ulp, and on scenes of at most nine Gaussians
no pixel's alpha lies within that of the 1/255 threshold).  absgrad: against the per-pixel expectation over the centred
4 x 4 block (k7_matrix_helpers.abs_expectation), and dominance over the signed gradient on the whole image.
"""
import numpy as np
import pytest
import torch

import abs_helpers as AB
import k7_matrix_helpers as K
from helpers import assert_grads_close, make_case, oracle_forward, seed_gradient

pytestmark = pytest.mark.gpu
_cache = {}

#: nine Gaussians of the 16 x 16 scenes: (pixel x, pixel y, sigma in pixels, opacity), all wide enough to cover the tile
COVER = [(7.3, 8.1, 6.0, 0.45), (5.2, 6.4, 7.0, 0.35), (10.6, 9.3, 6.5, 0.40), (8.8, 4.9, 8.0, 0.30), (6.1, 11.2, 7.5, 0.50),
         (9.4, 7.7, 6.8, 0.25), (4.3, 9.9, 9.0, 0.35), (11.5, 5.6, 7.2, 0.30), (7.9, 7.2, 8.5, 0.40)]


def _placed(W, H, spec, seed=11, depth0=3.6):
    """A case whose Gaussians are isotropic and sit where `spec` = [(px, py, sigma_px, opacity)] says, each a little deeper
    than the one before (a strict depth order)."""
    P = len(spec)
    case = make_case(P, W, H, seed=seed)
    cam, sc = case["cam"], case["sc"]
    inv = torch.linalg.inv(cam.world_view_transform.double())  # row vectors: view = [world, 1] @ wv
    xyz, scl, op = torch.zeros(P, 3), torch.zeros(P, 3), torch.zeros(P, 1)
    for i, (px, py, sigma, o) in enumerate(spec):
        z = depth0 + 0.11 * i
        xc = ((px + 0.5) * 2.0 / W - 1.0) * z * case["tfx"]
        yc = ((py + 0.5) * 2.0 / H - 1.0) * z * case["tfy"]
        xyz[i] = (torch.tensor([xc, yc, z, 1.0], dtype=torch.float64) @ inv)[:3].float()
        scl[i] = sigma * z * 2.0 * case["tfy"] / H  # sigma_px = s * focal / z, focal = H / (2 tan(fovy / 2))
        op[i] = o
    sc["xyz"], sc["scaling"], sc["opacity"] = xyz.contiguous(), scl.contiguous(), op.contiguous()
    sc["rotation"] = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1).contiguous()
    return case


def _cover_case(oracle, P):
    """The 16 x 16 tile under the first P Gaussians of COVER -> (case, oracle forward); checked once: they sit where they were
    put, and each one reaches alpha >= 1/255 at every pixel of the tile."""
    if ("cover", P) not in _cache:
        case = _placed(16, 16, COVER[:P])
        f = oracle_forward(oracle, case)
        assert f["num_rendered"] == P and (f["radii"] > 0).all()
        m, co = f["means2D"].astype(np.float64), f["conic_opacity"].astype(np.float64)
        assert np.abs(m - np.array([s[:2] for s in COVER[:P]])).max() < 1e-3, m
        ys, xs = np.mgrid[0:16, 0:16]
        for i in range(P):
            dx, dy = m[i, 0] - xs, m[i, 1] - ys
            power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
            assert (co[i, 3] * np.exp(power)).min() > 1.5 / 255.0, (i, "does not cover the tile")
        assert f["final_T"].min() > 1e-3  # (no pixel saturates: all P entries are blended at every pixel)
        _cache["cover", P] = (case, f)
    return _cache["cover", P]


def _dense(H, W, case):
    """The three pixel gradients of a scene, balanced as in k7_matrix_helpers.scene."""
    return (seed_gradient(H, W, 3) * H * W, seed_gradient(H, W, 5)[:1] * H * W,
            seed_gradient(H, W, 7)[:1] * H * W / float(case["cam"].camera_center.norm()))


def _check(oracle, case, row, G, GA=None, GD=None, tag=""):
    """One backward of the product under `row` against the oracle's expectation -> (gradients, outputs of K.run)."""
    want, _ = K.expectation(oracle, case, G, GA, GD)
    got, out = K.run(case, row, G, GA, GD)
    worst = assert_grads_close(got, want, tag=tag, keys=list(got))
    assert any(np.abs(want[k]).max() > 0 for k in got), (tag, "the expectation is all zero")
    return got, out, worst


# ---------------------------------------------------------------------------------------------------------------------
# a. lane coverage
QUADRANT_PIXELS = {0: [(y, x) for y in range(8) for x in range(8)], 1: [(0, 8), (3, 13), (6, 10), (7, 15)],
                   2: [(8, 0), (11, 5), (13, 2), (15, 7)], 3: [(8, 8), (10, 15), (14, 11), (15, 12)]}


@pytest.mark.parametrize("quadrant", sorted(QUADRANT_PIXELS))
def test_one_live_lane(oracle, quadrant):
    case, f = _cover_case(oracle, 5)
    worst = 0.0
    for y, x in QUADRANT_PIXELS[quadrant]:
        G = torch.zeros(3, 16, 16)
        G[:, y, x] = torch.tensor([1.0, -0.7, 0.4])
        got, out, w = _check(oracle, case, (0, None, 0, 0, 0), G, tag=f"one-hot pixel ({y}, {x})")
        assert out["items"] == (1, 0), out["items"]  # (one tile, one item)
        # every one of the five Gaussians gets a gradient from the pixel (two groups, the second with three null entries)
        assert (np.abs(got["dL_dopacity"]).reshape(5) > 0).all(), (y, x, got["dL_dopacity"])
        worst = max(worst, w)
    print(f"  quadrant {quadrant}: {len(QUADRANT_PIXELS[quadrant])} one-hot backwards, worst {worst:.2e} = {worst / 1e-5:.3f} bar")


# ---------------------------------------------------------------------------------------------------------------------
# b. group padding
@pytest.mark.parametrize("P", range(1, 10))
def test_group_padding(oracle, P):
    case, _ = _cover_case(oracle, P)
    G, _, _ = _dense(16, 16, case)
    _, out, worst = _check(oracle, case, (0, None, 0, 0, 0), G, tag=f"P = {P}")
    print(f"  P = {P}: items {out['items']}, worst {worst:.2e} = {worst / 1e-5:.3f} bar")


# ---------------------------------------------------------------------------------------------------------------------
# c. quadrant sums
#: (px, py, sigma_px, opacity, quadrants of its tile it must reach): 32 x 32, tiles of 16, quadrants of 8
REACH = [(3.5, 4.0, 0.7, 0.9, 1), (7.5, 3.0, 0.7, 0.9, 2), (7.5, 7.5, 0.7, 0.9, 4), (4.2, 7.5, 0.75, 0.85, 2),
         (27.0, 27.5, 0.7, 0.9, 1), (23.5, 23.5, 0.8, 0.8, 4), (20.0, 23.5, 0.7, 0.9, 2), (23.5, 11.0, 0.7, 0.9, 2),
         (7.4, 7.6, 1.1, 0.5, 4), (12.0, 20.0, 0.7, 0.9, 1)]


def _quadrants_reached(f, i, W, H):
    m, co = f["means2D"][i].astype(np.float64), f["conic_opacity"][i].astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    dx, dy = m[0] - xs, m[1] - ys
    power = -0.5 * (co[0] * dx * dx + co[2] * dy * dy) - co[1] * dx * dy
    alpha = np.minimum(0.99, co[3] * np.exp(power))
    hit = (power <= 0) & (alpha >= 1.0 / 255.0)
    # (nothing may sit at the threshold: the count must not depend on the last bits of an exponential -- 2e-5 is half a
    # percent of 1/255, thousands of binary32 roundings)
    assert not ((np.abs(alpha - 1.0 / 255.0) < 2e-5) & (power <= 0)).any(), (i, "a pixel at the alpha threshold")
    return {(y // 8, x // 8) for y, x in zip(*np.nonzero(hit))}


def test_quadrant_sums(oracle):
    W = H = 32
    case = _placed(W, H, [s[:4] for s in REACH])
    f = oracle_forward(oracle, case)
    for i, spec in enumerate(REACH):
        q = _quadrants_reached(f, i, W, H)
        assert len({(y // 2, x // 2) for y, x in q}) == 1, (i, "reaches more than one tile", q)
        assert len(q) == spec[4], (i, spec, sorted(q))
    assert sorted({s[4] for s in REACH}) == [1, 2, 4]
    G, GA, GD = _dense(H, W, case)
    for row, ga, gd in (((0, None, 0, 0, 0), None, None), ((0, 0, 1, 1, 1), GA, GD)):
        _, out, worst = _check(oracle, case, row, G, ga, gd, tag=f"quadrant sums {K.row_id(tuple(int(bool(v)) for v in row))}")
        print(f"  quadrant sums, launched [{out['index']}]: items {out['items']}, worst {worst:.2e} = {worst / 1e-5:.3f} bar")


# ---------------------------------------------------------------------------------------------------------------------
# d. row widths
#: name -> (FAST, SEG, DEPTH, ABS, ALPHA); moments per entry 10, 11, 12, 9, 9
WIDTHS = {"depth": (0, 0, 1, 0, 0), "abs": (0, None, 0, 1, 0), "depth+abs": (0, 0, 1, 1, 0), "alpha": (0, None, 0, 0, 1),
          "fast": (1, None, 0, 0, 0)}


@pytest.mark.parametrize("P", range(1, 10))
@pytest.mark.parametrize("width", sorted(WIDTHS))
def test_row_widths(oracle, width, P):
    row = WIDTHS[width]
    case, _ = _cover_case(oracle, P)
    G, GA, GD = _dense(16, 16, case)
    GA, GD = (GA if row[4] else None), (GD if row[2] else None)
    tag = f"{width} P = {P}"
    got, out, worst = _check(oracle, case, row, G, GA, GD, tag=tag)
    line = f"  {tag}: launched [{out['index']}], worst {worst:.2e} = {worst / 1e-5:.3f} bar"
    if row[3]:
        a, sg = out["absgrad"].astype(np.float64), np.abs(got["dL_dmeans2D"][:, :2].astype(np.float64))
        assert a.shape == (P, 3) and (a[:, 2] == 0).all() and np.isfinite(a).all()
        assert (sg - a[:, :2]).max() <= 1e-5 * a.max(), (tag, "dominance")
        pixels = AB.block_pixels(16, 16, K.BLOCK)
        m = AB.pixel_mask(16, 16, pixels)
        want_a, signed = K.abs_expectation(oracle, case, G, GA, GD, pixels)
        gb, ob = K.run(case, row, G * m, None if GA is None else GA * m, None if GD is None else GD * m)
        wa = assert_grads_close(dict(absgrad=ob["absgrad"]), dict(absgrad=want_a), tag=tag + ": absgrad vs per-pixel expectation")
        assert_grads_close(dict(signed=gb["dL_dmeans2D"][:, :2]), dict(signed=signed), tag=tag + ": block means2D.grad")
        line += f", absgrad {wa:.2e}"
    assert K.acc_tables_are_zero(), tag
    print(line)


def test_the_widths_ran_their_kernels():
    """(last in the file) the instantiations the row-width cases were meant to launch did run in this process."""
    c = K.launches()
    for width, row in WIDTHS.items():
        assert any(c[K.index((row[0], s, row[2], row[3], row[4]))] >= 9 for s in (0, 1)), (width, K.counter_table(c))
