"""-m gpu: gsr_trace_contributions -- the per-Gaussian contribution statistics and the per-pixel pick buffer -- against the
CPU oracle's own blending weights (tests/contrib_helpers.py), bit for bit: the table is integer, so nothing here has a
tolerance except the two comparisons with float quantities of other kernels (the backward trick, the alpha image).

The quadrant cut of the launch (1, 2 or 4 items per quadrant) follows the grid, compute units x 4 x
GSR_BLEND_WAVES_PER_SIMD (4 by default): `_grid` reads the knob as the library does, the cut tests take the image sizes next
to the thresholds of the grid in use, and test_on_one_wave_per_simd reruns the file in a fresh process with the knob at 1,
where cuts 1 and 2 are reached at images of 365 x 361 and 253 x 249 instead of 733 x 729 and 509 x 505."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import contrib_helpers as CH
from helpers import hip_state, settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "GSR_BLEND_WAVES_PER_SIMD"
P_BIG = 5000


def _c():
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    return _C


def _oracle():
    from oracle import cpu as O

    O.build()
    return O


def forward_split(grid, quads):
    """gsr_blend.hip, forward_split() for a launch no backward follows (the trace kernels): items a quadrant is cut into."""
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
    return torch.cuda.get_device_properties(DEV).multi_processor_count * 4 * _waves_per_simd()


def _size(cut):
    """(W, H) of an image of n x n tiles that the rule cuts `cut` ways: the smallest such n, for 4 the largest.  Ragged."""
    ns = [n for n in range(1, 129) if forward_split(_grid(), 4 * n * n) == cut]
    assert ns, (cut, _grid())
    n = max(ns) if cut == 4 else min(ns)
    return 16 * n - 3, 16 * n - 7


def _dev(t):
    return t.to(DEV).contiguous()


def _trace(case, masks=None, table=None, flags=0, return_pixels=True):
    """GaussianRasterizer.trace_contributions of the case's view -> (table, top_id, top_weight) as numpy (the table is the
    device tensor `table` accumulated into, or a fresh one)."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    sc = case["sc"]
    P = sc["xyz"].shape[0]
    C = 0 if masks is None else masks.shape[0]
    if table is None:
        table = torch.zeros((P, 3 + C), dtype=torch.int64, device=DEV)
    with options.override(flags):
        out = GaussianRasterizer(settings(case, DEV, D=0)).trace_contributions(
            _dev(sc["xyz"]), _dev(sc["opacity"]), scales=_dev(sc["scaling"]), rotations=_dev(sc["rotation"]), stats=table,
            image_weights=None if masks is None else _dev(masks), return_pixels=return_pixels)
    torch.cuda.synchronize()
    if not return_pixels:
        assert out is None
        return table.cpu().numpy(), None, None
    return table.cpu().numpy(), out[0].cpu().numpy().reshape(-1), out[1].cpu().numpy().reshape(-1)


def _render(case, flags=0, colors=None):
    sc, cam = case["sc"], case["cam"]
    e = torch.empty(0, device=DEV)
    return _c().rasterize_gaussians(
        _dev(case["bg"]), _dev(sc["xyz"]), e if colors is None else _dev(colors), _dev(sc["opacity"]), _dev(sc["scaling"]),
        _dev(sc["rotation"]), 1.0, e, _dev(cam.world_view_transform), _dev(cam.full_proj_transform), case["tfx"], case["tfy"],
        case["H"], case["W"], _dev(sc["features"]) if colors is None else e, case["D"], _dev(cam.camera_center), False, False,
        flags=flags)


def _np_masks(masks):
    return None if masks is None else masks.numpy().reshape(masks.shape[0], -1)


# ---- the exhaustive cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [0, 1, 3])
@pytest.mark.parametrize("name", list(CH.EXHAUSTIVE))
def test_exhaustive_cases_bit_for_bit(name, C):
    """Every column of every row and both pixel images, against the oracle's weights of every Gaussian: C = 0, a binary mask,
    three float masks with values below 0, above 1 and exactly 0 and 1."""
    exp = CH.exhaustive_expectation(_oracle(), name)
    assert exp["tied"] == 0, "a pixel with a tied top weight: the case is the wrong choice, not the kernel"
    case = exp["case"]
    H, W = case["H"], case["W"]
    masks = CH.make_masks(H, W, C) if C else None
    if C == 3:
        m = masks.numpy()
        assert (m < 0).any() and (m > 1).any() and (m[1:] == 0).any() and (m[1:] == 1).any() and set(np.unique(m[0])) == {0.0, 1.0}
    table, top_id, top_w = _trace(case, masks)
    want = CH.expected_table(exp, _np_masks(masks))
    bad = np.argwhere(table != want)
    print(f"  {name} C={C}: rows hit {int((want[:, 0] > 0).sum())} of {want.shape[0]}, cells that differ {len(bad)}, top ids that "
          f"differ {int((top_id != exp['top_id']).sum())}, top weights that differ {int((top_w != exp['top_weight']).sum())}")
    assert len(bad) == 0, (bad[:5], table[bad[:5, 0]], want[bad[:5, 0]])
    assert np.array_equal(top_id, exp["top_id"]) and np.array_equal(top_w.view(np.uint32), exp["top_weight"].view(np.uint32))
    assert int((want[:, 0] > 0).sum()) > 20 and (top_id == -1).any()


@pytest.mark.parametrize("name", list(CH.EXHAUSTIVE))
def test_constant_masks(name):
    """mask == 1 => weighted_q == total_q; mask == 0 => 0 (and values beyond [0, 1] clamp to them)."""
    case = CH.exhaustive_expectation(_oracle(), name)["case"]
    H, W = case["H"], case["W"]
    masks = torch.stack([torch.ones(H, W), torch.zeros(H, W), torch.full((H, W), 7.5)])
    table, _, _ = _trace(case, masks, return_pixels=False)
    assert table[:, 0].any()
    assert np.array_equal(table[:, 3], table[:, 0]) and not table[:, 4].any() and np.array_equal(table[:, 5], table[:, 0])
    nan = torch.stack([torch.full((H, W), float("nan")), torch.full((H, W), -2.0)])
    table2, _, _ = _trace(case, nan, return_pixels=False)
    assert np.array_equal(table2[:, :3], table[:, :3]) and not table2[:, 3:].any()


# ---- accumulation --------------------------------------------------------------------------------------------------------
class _PC:
    def __init__(self, sc):
        self._sc = {k: _dev(v) for k, v in sc.items() if torch.is_tensor(v)}

    get_xyz = property(lambda s: s._sc["xyz"])
    get_opacity = property(lambda s: s._sc["opacity"])
    get_scaling = property(lambda s: s._sc["scaling"])
    get_rotation = property(lambda s: s._sc["rotation"])


def test_views_accumulate_in_any_order():
    from gaussianeditor_amd.contrib import ContributionStats, trace_view

    O = _oracle()
    P, W, H, seed, s0 = CH.EXHAUSTIVE["six_tiles"]
    A, B = CH.contrib_case(P, W, H, seed, s0, view=0), CH.contrib_case(P, W, H, seed, s0, view=1)
    masks = CH.make_masks(H, W, 2, seed=5)
    pc = _PC(A["sc"])
    single = {}
    for tag, case in (("A", A), ("B", B)):
        single[tag] = _trace(case, masks, return_pixels=False)[0]
    assert single["A"][:, 0].any() and single["B"][:, 0].any() and not np.array_equal(single["A"], single["B"])
    # (view A is the exhaustive case: its single table is the oracle's)
    assert np.array_equal(single["A"], CH.expected_table(CH.exhaustive_expectation(O, "six_tiles"), _np_masks(masks)))
    tables = []
    for order in ((A, B), (B, A)):
        st = ContributionStats(P, channels=2, device=DEV)
        for case in order:
            assert trace_view(case["cam"].to(DEV), pc, st, mask=masks) is None
        assert st.views == 2
        tables.append(st.table.cpu().numpy())
    assert np.array_equal(tables[0], tables[1])
    assert np.array_equal(tables[0], CH.merge_tables(single["A"], single["B"]))


# ---- the quadrant cuts ---------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _big_scene(W, H):
    return CH.contrib_case(P_BIG, W, H, 7, 0.03)


@functools.lru_cache(None)
def _big_case(W, H):
    """The P = 5000 scene at one size, the oracle's weights of 255 probe Gaussians (every 20th) and its final transmittance:
    computed once per size, never written to."""
    O = _oracle()
    case = _big_scene(W, H)
    # (every 20th Gaussian and five more: 255 probes fill 85 oracle calls of three columns)
    probes = np.sort(np.concatenate([np.arange(0, P_BIG, 20), np.arange(7, P_BIG, 1000)]))
    assert len(probes) == 255 and len(np.unique(probes)) == 255
    weights, final_T = CH.oracle_weights(O, case, probes)
    return case, probes, weights, final_T


def _backward_trick(case):
    """sum_p w per Gaussian the former way: render with colours 1, backward with dL/dpixel = 1 -> dL_dcolors[:, 0]; and the
    render's alpha image."""
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    sc = case["sc"]
    P = sc["xyz"].shape[0]
    cols = torch.ones(P, 3, device=DEV, requires_grad=True)
    xyz = _dev(sc["xyz"])
    outs = GaussianRasterizer(settings(case, DEV, D=0))(xyz, torch.zeros_like(xyz), _dev(sc["opacity"]), colors_precomp=cols,
                                                        scales=_dev(sc["scaling"]), rotations=_dev(sc["rotation"]),
                                                        return_alpha=True)
    outs[0].sum().backward()
    torch.cuda.synchronize()
    return cols.grad[:, 0].double().cpu().numpy(), outs[-1].detach().double().cpu().numpy()


@pytest.mark.parametrize("cut", [1, 2, 4])
def test_quadrant_cuts(cut):
    """P = 5000 at the image size next to the cut's threshold: the probes' rows exact, the pixel images consistent with the
    probes and the table, and the totals against the product's own backward trick and alpha image."""
    W, H = _size(cut)
    assert forward_split(_grid(), 4 * ((W + 15) // 16) * ((H + 15) // 16)) == cut
    case, probes, weights, final_T = _big_case(W, H)
    masks = CH.make_masks(H, W, 3, seed=21)
    table, top_id, top_w = _trace(case, masks)
    want = CH.expected_rows(weights, _np_masks(masks))
    hit = int((want[:, 0] > 0).sum())
    cols = [0, 2, 3, 4, 5]
    differ = int((table[probes][:, cols] != want[:, cols]).sum())
    print(f"  cut {cut} {W}x{H} grid {_grid()}: probes hit {hit} of {len(probes)}, probe cells that differ {differ}")
    assert hit >= 200 and differ == 0
    # all rows: the histogram of the pick buffer
    assert np.array_equal(table[:, 1], np.bincount(top_id[top_id >= 0], minlength=P_BIG))
    assert (top_id >= -1).all() and (top_id < P_BIG).all() and np.array_equal(top_id == -1, top_w == 0)
    # the pick buffer against the probes: no probe weighs more than the top, and where the top is a probe it is that weight
    assert (top_w[None, :] >= weights).all()
    row_of = np.full(P_BIG, -1)
    row_of[probes] = np.arange(len(probes))
    is_probe = (top_id >= 0) & (row_of[np.maximum(top_id, 0)] >= 0)
    px = np.nonzero(is_probe)[0]
    assert len(px) > 100 and np.array_equal(top_w[px], weights[row_of[top_id[px]], px])
    # ... and a probe is the top wherever its weight reaches the top weight (no ties among 255 probes is not assumed: >=)
    probe_top = np.array([(top_id == g).sum() for g in probes])
    assert (probe_top <= ((weights == top_w[None, :]) & (weights > 0)).sum(axis=1)).all()
    assert np.array_equal(table[probes, 1], probe_top)
    # all rows: max_bits is a weight some pixel saw, the weighted sums never exceed the total
    mx = table[:, 2].astype(np.uint32).view(np.float32)
    assert np.array_equal(table[:, 0] > 0, mx > 0) and float(mx.max()) <= 0.99 and (table[:, 3:] <= table[:, :1]).all()
    # all rows: the totals against the backward trick (the project's bar: 1e-5 of the tensor's largest entry) and the alpha image
    total = table[:, 0].astype(np.float64) / CH.Q_ONE
    trick, alpha = _backward_trick(case)
    err = float(np.abs(total - trick).max() / np.abs(trick).max())
    rel = abs(total.sum() - alpha.sum()) / alpha.sum()
    rel_oracle = abs(total.sum() - (1.0 - final_T.astype(np.float64)).sum()) / alpha.sum()
    print(f"  cut {cut}: total vs the backward trick {err:.2e} of its largest entry (bar 1e-5); sum of totals vs sum of alpha "
          f"{rel:.2e} (the oracle's alpha: {rel_oracle:.2e}; bar 1e-6)")
    assert err <= 1e-5 and rel <= 1e-6 and rel_oracle <= 1e-6


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast_exp"])
@pytest.mark.parametrize("cut", [1, 2, 4])
def test_every_channel_count_at_every_cut(cut, fast):
    """The 24 instantiations: C = 0 .. 3 at each cut in both exp modes give the same first three columns, the same pixel
    images and the same column per mask channel."""
    from gaussianeditor_amd import options

    W, H = _size(cut)
    case = _big_case(W, H)[0]
    flags = options.FLAG_FAST_EXP if fast else 0
    masks = CH.make_masks(H, W, 3, seed=21)
    full, top_id, top_w = _trace(case, masks, flags=flags)
    assert full[:, 0].any() and np.array_equal(full[:, 1], np.bincount(top_id[top_id >= 0], minlength=P_BIG))
    for C in (0, 1, 2):
        t, ti, tw = _trace(case, masks[:C] if C else None, flags=flags)
        assert np.array_equal(t, full[:, :3 + C]) and np.array_equal(ti, top_id) and np.array_equal(tw, top_w), C
    t, _, _ = _trace(case, masks[1:2], flags=flags, return_pixels=False)
    assert np.array_equal(t[:, 3], full[:, 4]) and np.array_equal(t[:, :3], full[:, :3])


# ---- flags ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["FAST_EXP", "ANTIALIAS", "TILE_BOUNDS_ALPHA"])
def test_flags_against_one_hot_features(flag):
    """Under the flags the oracle has no rule for, the feature image of one-hot features (P = 256 channels: one call) is the
    weight of every (Gaussian, pixel) from the same walker and the same flags; the table and the pixel images exactly."""
    from gaussianeditor_amd import options

    flags = getattr(options, "FLAG_" + flag)
    P, W, H, seed, s0 = CH.EXHAUSTIVE["fifteen_tiles"]
    case = CH.contrib_case(P, W, H, seed, s0)
    R, _, _, _, geom, binning, img = _render(case, flags)
    st = hip_state(P, R, W, H, geom, binning, img)
    weights = _c().rasterize_features(torch.eye(P, device=DEV), R, geom, binning, img, H, W, flags=flags).cpu().numpy().reshape(P, -1)
    plain = CH.exhaustive_expectation(_oracle(), "fifteen_tiles")["weights"]
    masks = CH.make_masks(H, W, 3)
    top_id, top_w, tied = CH.expected_top(weights, np.arange(P), st["ranges"], st["point_list"], W, H)
    want = CH.expected_rows(weights, _np_masks(masks))
    want[:, 1] = np.bincount(top_id[top_id >= 0], minlength=P)
    table = torch.zeros((P, 6), dtype=torch.int64, device=DEV)
    out = _c().trace_contributions_state(table, R, geom, binning, img, H, W, image_weights=_dev(masks), return_pixels=True,
                                         flags=flags)
    torch.cuda.synchronize()
    print(f"  {flag}: R {R}, weights that differ from the unflagged oracle's {int((weights != plain).sum())}, tied pixels {tied}")
    assert tied == 0
    if flag != "TILE_BOUNDS_ALPHA":  # (that flag changes the lists, not a weight: DESIGN, "images ... are unchanged")
        assert (weights != plain).any()
    assert np.array_equal(table.cpu().numpy(), want)
    assert np.array_equal(out[0].cpu().numpy().reshape(-1), top_id) and np.array_equal(out[1].cpu().numpy().reshape(-1), top_w)
    # the full path (preprocess without colours + bin + trace) under the flag: the same table
    assert np.array_equal(_trace(case, masks, flags=flags)[0], want)


# ---- determinism ---------------------------------------------------------------------------------------------------------
def test_three_runs_are_identical():
    W, H = _size(4)
    case = _big_case(W, H)[0]
    masks = CH.make_masks(H, W, 3, seed=21)
    runs = [_trace(case, masks) for _ in range(3)]
    assert runs[0][0][:, 0].any()
    for r in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(r, runs[0]))


# ---- buffers and state ---------------------------------------------------------------------------------------------------
def test_guard_bands_and_full_writes():
    """Under GuardedAllocator every buffer the binding allocates is poisoned and banded: the guards stay intact, and both
    pixel images are fully written (equal to the unguarded run's, poison nowhere)."""
    from guarded_alloc import GuardedAllocator

    exp = CH.exhaustive_expectation(_oracle(), "fifteen_tiles")
    case = exp["case"]
    masks = CH.make_masks(case["H"], case["W"], 3)
    want = CH.expected_table(exp, _np_masks(masks))
    for pattern in (0xA5, 0x7F):
        with GuardedAllocator(pattern, device=DEV) as ga:
            table = ga.place(torch.zeros((want.shape[0], 6), dtype=torch.int64))
            got, top_id, top_w = _trace(case, masks, table=table)
            assert len(ga) > 4
            ga.assert_clean()
        assert np.array_equal(got, want)
        assert np.array_equal(top_id, exp["top_id"]) and np.array_equal(top_w.view(np.uint32), exp["top_weight"].view(np.uint32))


def test_on_a_side_stream():
    exp = CH.exhaustive_expectation(_oracle(), "ragged")
    case = exp["case"]
    masks = CH.make_masks(case["H"], case["W"], 1)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        got, top_id, top_w = _trace(case, masks)
    s.synchronize()
    assert np.array_equal(got, CH.expected_table(exp, _np_masks(masks))) and np.array_equal(top_id, exp["top_id"])
    assert np.array_equal(top_w.view(np.uint32), exp["top_weight"].view(np.uint32))


def test_saved_state_is_left_intact():
    """On the state of a render: the table is the full path's, n_contrib / final_T / ranges / lists are unchanged, and the
    render's own auxiliary kernel still computes the same image afterwards."""
    exp = CH.exhaustive_expectation(_oracle(), "six_tiles")
    case = exp["case"]
    P, H, W = case["sc"]["xyz"].shape[0], case["H"], case["W"]
    R, color, _, _, geom, binning, img = _render(case)
    before = hip_state(P, R, W, H, geom, binning, img)
    bufs = [b.clone() for b in (geom, binning)]
    table = torch.zeros((P, 3), dtype=torch.int64, device=DEV)
    for _ in range(2):  # (back to back on one state: the second launch finds the queue's cursors cleared)
        out = _c().trace_contributions_state(table, R, geom, binning, img, H, W, return_pixels=True)
    torch.cuda.synchronize()
    after = hip_state(P, R, W, H, geom, binning, img)
    for k in ("final_T", "n_contrib", "ranges", "point_list"):
        assert np.array_equal(before[k], after[k]), k
    assert torch.equal(bufs[0], geom) and torch.equal(bufs[1], binning)
    want = CH.expected_table(exp)
    assert np.array_equal(table.cpu().numpy(), CH.merge_tables(want, want))
    assert np.array_equal(out[0].cpu().numpy().reshape(-1), exp["top_id"])
    sc = case["sc"]
    again = _c().rasterize_gaussians_aux(_dev(case["bg"]), torch.ones(P, 3, device=DEV), R, geom, binning, img, H, W)
    first = _render(case, colors=torch.ones(P, 3))[1]
    assert torch.equal(again, first) and sc["xyz"].shape[0] == P


def test_empty_view_and_empty_scene():
    """R == 0: -1 / 0 images and an untouched table (its version counter still moves: the call is a writer).  P == 0."""
    P, W, H, seed, s0 = CH.EXHAUSTIVE["ragged"]
    case = CH.contrib_case(P, W, H, seed, s0)
    behind = dict(case, sc=dict(case["sc"], xyz=(case["sc"]["xyz"] * 0.1 + case["cam"].camera_center * 2.0).contiguous()))
    table = torch.full((P, 4), 7, dtype=torch.int64, device=DEV)
    v0 = table._version
    got, top_id, top_w = _trace(behind, CH.make_masks(H, W, 1), table=table)
    assert (got == 7).all() and (top_id == -1).all() and top_id.shape == (H * W,) and not top_w.any()
    assert table._version > v0
    empty = dict(case, sc={k: (v[:0].contiguous() if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == P else v)
                           for k, v in case["sc"].items()})
    got, top_id, top_w = _trace(empty)
    assert got.shape == (0, 3) and (top_id == -1).all() and top_id.shape == (H * W,) and not top_w.any()
    assert _trace(empty, return_pixels=False)[1] is None


def test_version_counter_of_the_table_moves():
    case = CH.exhaustive_expectation(_oracle(), "one_tile")["case"]
    table = torch.zeros((200, 3), dtype=torch.int64, device=DEV)
    v0 = table._version
    _trace(case, table=table, return_pixels=False)
    assert table._version > v0 and bool(table.any())


# ---- the public layer ----------------------------------------------------------------------------------------------------
def test_trace_view_equals_the_raw_call_and_patches_a_model():
    from gaussianeditor_amd import contrib

    exp = CH.exhaustive_expectation(_oracle(), "fifteen_tiles")
    case = exp["case"]
    P, H, W = case["sc"]["xyz"].shape[0], case["H"], case["W"]
    masks = CH.make_masks(H, W, 1)
    raw, top_id, top_w = _trace(case, masks)
    st = contrib.ContributionStats(P, channels=1, device=DEV)
    pc = _PC(case["sc"])
    out = contrib.trace_view(case["cam"].to(DEV), pc, st, mask=masks[0].bool(), return_pixels=True)  # (H,W), any dtype
    assert st.views == 1 and np.array_equal(st.table.cpu().numpy(), raw)
    assert np.array_equal(out[0].cpu().numpy().reshape(-1), top_id) and np.array_equal(out[1].cpu().numpy().reshape(-1), top_w)
    assert np.array_equal(raw, CH.expected_table(exp, _np_masks(masks)))

    class Model(_PC):
        pass

    contrib.patch_gaussian_model(Model)
    st2 = contrib.ContributionStats(P, channels=1, device=DEV)
    assert Model(case["sc"]).apply_contributions(case["cam"].to(DEV), st2, mask=masks) is None
    assert torch.equal(st2.table, st.table) and st2.views == 1
    assert torch.equal(st.top_count.cpu(), torch.from_numpy(exp["top_count"]))
    assert np.array_equal(st.max_weight.cpu().numpy(), exp["weights"].max(axis=1))
    assert float((st.total.cpu() - torch.from_numpy(exp["weights"].astype(np.float64).sum(axis=1))).abs().max()) <= 1e-6
    merged = contrib.ContributionStats(P, channels=1, device=DEV).merge(st).merge(st2)
    assert merged.views == 2 and np.array_equal(merged.table.cpu().numpy(), CH.merge_tables(raw, raw))


def test_label_differs_from_the_unweighted_vote():
    """The discrimination: on a binary mask the contribution-weighted label lies in [0, 1] and differs from apply_weights'
    `weights / cnt` on at least 100 Gaussians of the P = 5000 case."""
    from gaussianeditor_amd import contrib
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    W, H = _size(4)
    case = _big_case(W, H)[0]
    sc = case["sc"]
    mask = CH.make_masks(H, W, 1, seed=33)
    # (a mask with structure: the left part of the image, so that Gaussians straddle its edge)
    mask[0] = (torch.arange(W)[None, :] < 0.45 * W).float().expand(H, W)
    st = contrib.ContributionStats(P_BIG, channels=1, device=DEV)
    contrib.trace_view(case["cam"].to(DEV), _PC(sc), st, mask=mask)
    label = st.label()[:, 0].cpu().numpy()
    w = torch.zeros((P_BIG, 1), device=DEV)
    cnt = torch.zeros((P_BIG, 1), dtype=torch.int32, device=DEV)
    GaussianRasterizer(settings(case, DEV, D=0)).apply_weights(_dev(sc["xyz"]), None, _dev(sc["opacity"]), None, w,
                                                                _dev(sc["scaling"]), _dev(sc["rotation"]), None, cnt, _dev(mask))
    vote = (w / (cnt + 1e-7)).cpu().numpy()[:, 0].astype(np.float64)
    hit = st.table[:, 0].cpu().numpy() > 0
    assert np.array_equal(hit, cnt.cpu().numpy()[:, 0] > 0)  # the same walk: the same Gaussians are blended somewhere
    differ = int((np.abs(label - vote) > 1e-3).sum())
    print(f"  label vs vote: {int(hit.sum())} Gaussians hit, {differ} differ by more than 1e-3, largest {np.abs(label - vote).max():.3f}")
    assert float(label.min()) >= 0.0 and float(label.max()) <= 1.0 and differ >= 100
    sel = st.select(0.5).cpu().numpy()
    assert sel.any() and not sel.all() and not sel[~hit].any()
    assert np.array_equal(st.low_contribution(max_weight_below=0.0, total_below=1e-30).cpu().numpy(), ~hit)


# ---- the other grid ------------------------------------------------------------------------------------------------------
def test_on_one_wave_per_simd():
    """This file once more in a fresh process with GSR_BLEND_WAVES_PER_SIMD=1 (read once per process): cuts 1 and 2 at small
    images, every check above at that grid's thresholds."""
    env ={k: v for k, v in os.environ.items() if k != KNOB}
    env[KNOB] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-s", "-k",
                        "not test_on_one_wave_per_simd"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("  cut") or " passed" in ln or " failed" in ln))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:]
