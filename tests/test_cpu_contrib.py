"""CPU: the contribution statistics' header wording and ABI, the argument validation of gsr_trace_contributions and of its
binding without a device, the arithmetic of ContributionStats, and the expectation builder of tests/contrib_helpers.py
held to the oracle's own transmittance."""
import ctypes
import os

import numpy as np
import pytest
import torch

import contrib_helpers as CH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_abi_wording():
    from gaussianeditor_amd import _native

    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "#define GSR_ABI_VERSION 6" in hdr and "int gsr_trace_contributions(" in hdr
    doc = hdr[hdr.index("Contribution statistics and the pick buffer"):hdr.index("int gsr_trace_contributions(")]
    for word in ("total_q", "top_count", "max_bits", "weighted_q", "trunc(x * 2^32)", "front-most", "2^53", "NaN -> 0",
                 "no float atomics", "GSR_ERR_BAD_CHANNELS", "IN PLACE"):
        assert word in doc, word
    res, args = _native.SIGNATURES["gsr_trace_contributions"]
    assert res is ctypes.c_int and len(args) == 14 and args[2] is ctypes.c_int64 and args[-1] is ctypes.c_uint
    assert "gsr_*" in open(os.path.join(ROOT, "gaussianeditor_amd", "csrc", "gsr.map")).read()
    assert hasattr(_native.lib(), "gsr_trace_contributions")


def test_argument_validation_needs_no_gpu():
    from gaussianeditor_amd import _native

    L = _native.lib()
    one = ctypes.c_void_p(256)  # never dereferenced
    call = L.gsr_trace_contributions
    # channels first, in front of every other check
    assert call(None, 10, 5, 64, 64, 4, None, None, None, None, None, None, None, 0) == -2
    assert call(None, 10, 5, 64, 64, -1, one, one, one, None, one, None, None, 0) == -2
    # unknown flags (64: GSR_FLAG_DEPTH_GRAD is not a view flag; 2048: no such bit)
    for bad in (64, 2048):
        assert call(None, 10, 5, 64, 64, 1, one, one, one, one, one, None, None, bad) == -1
    assert call(None, 10, 5, 64, 64, 1, one, one, one, one, None, None, None, 0) == -1  # no table
    assert call(None, 10, 5, 64, 64, 1, one, one, None, one, one, None, None, 0) == -1  # no image state
    assert call(None, 10, 5, 64, 64, 1, one, one, one, None, one, None, None, 0) == -1  # C > 0 without image_weights
    assert call(None, 10, 5, 64, 64, 0, one, one, one, one, one, None, None, 0) == -1  # C == 0 with image_weights
    assert call(None, -1, 5, 64, 64, 0, one, one, one, None, one, None, None, 0) == -1
    assert call(None, 10, -5, 64, 64, 0, one, one, one, None, one, None, None, 0) == -1
    assert call(None, 10, 5, 0, 64, 0, one, one, one, None, one, None, None, 0) == -1
    assert call(None, 10, 5, 64, -64, 0, one, one, one, None, one, None, None, 0) == -1
    assert call(None, 10, 5, 64, 64, 0, None, one, one, None, one, None, None, 0) == -1  # R > 0 without the geometry state
    assert call(None, 10, 5, 64, 64, 0, one, one, one, None, ctypes.c_void_p(260), None, None, 0) == -1  # int64 table: 8 bytes
    # an empty view without pixel images is a valid call that touches nothing
    assert call(None, 10, 0, 64, 64, 0, None, None, one, None, one, None, None, 0) == 0
    assert call(None, 10, 0, 64, 64, 1, None, None, one, one, one, None, None, 1024) == 0  # (GSR_FLAG_ANTIALIAS is a view flag)


def test_binding_shape_and_dtype_errors():
    from gaussianeditor_amd import _native
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C

    e = torch.empty(0, dtype=torch.uint8)
    state = lambda stats, **kw: _C.trace_contributions_state(stats, 0, e, e, e, 8, 12, **kw)  # noqa: E731
    with pytest.raises(RuntimeError, match="`stats` must be an int64 tensor"):
        state(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="`stats` must be a tensor"):
        state(None)
    with pytest.raises(RuntimeError, match=r"`stats` must be a \(4, 4\) tensor"):
        state(torch.zeros(4, 3, dtype=torch.int64), image_weights=torch.zeros(1, 8, 12))
    with pytest.raises(RuntimeError, match=r"`stats` must be a \(4, 3\) tensor"):
        state(torch.zeros(4, 5, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="`stats` must be contiguous"):
        state(torch.zeros(4, 6, dtype=torch.int64)[:, ::2])
    with pytest.raises(RuntimeError, match=r"`image_weights` must be a \(C, 8, 12\) tensor"):
        state(torch.zeros(4, 4, dtype=torch.int64), image_weights=torch.zeros(1, 12, 8))
    with pytest.raises(RuntimeError, match="`image_weights` must be a float32 tensor"):
        state(torch.zeros(4, 4, dtype=torch.int64), image_weights=torch.zeros(1, 8, 12, dtype=torch.float64))
    with pytest.raises(_native.GsrError, match="Unsupported number of channels: 4"):
        state(torch.zeros(4, 7, dtype=torch.int64), image_weights=torch.zeros(4, 8, 12))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a table with rows on the host
        state(torch.zeros(4, 3, dtype=torch.int64))
    # P == 0 returns at once, on any device
    assert state(torch.zeros(0, 3, dtype=torch.int64)) is None
    top_id, top_w = state(torch.zeros(0, 4, dtype=torch.int64), image_weights=torch.zeros(1, 8, 12), return_pixels=True)
    assert top_id.dtype == torch.int32 and tuple(top_id.shape) == (8, 12) and bool((top_id == -1).all())
    assert top_w.dtype == torch.float32 and not top_w.any()
    # the rasterizer's method: same checks, and no CPU path
    rs = GaussianRasterizationSettings(8, 12, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                       False, False)
    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match=r"`stats` must be a \(4, 3\) tensor"):
        GaussianRasterizer(rs).trace_contributions(x, torch.ones(4, 1), scales=x, rotations=torch.ones(4, 4),
                                                   stats=torch.zeros(5, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GaussianRasterizer(rs).trace_contributions(x, torch.ones(4, 1), scales=x, rotations=torch.ones(4, 4),
                                                   stats=torch.zeros(4, 3, dtype=torch.int64))
    assert GaussianRasterizer(rs).trace_contributions(x[:0], torch.ones(0, 1), scales=x[:0], rotations=torch.ones(0, 4),
                                                      stats=torch.zeros(0, 3, dtype=torch.int64)) is None


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_contribution_stats_arithmetic_and_merge():
    import gaussianeditor_amd
    from gaussianeditor_amd.contrib import ContributionStats, Q_ONE

    assert gaussianeditor_amd.ContributionStats is ContributionStats
    s = ContributionStats(4, channels=2, device="cpu")
    assert tuple(s.table.shape) == (4, 5) and s.table.dtype == torch.int64 and len(s) == 4 and s.views == 0
    s.table[0] = torch.tensor([3 << 31, 7, _bits(0.75), 3 << 30, 0])                # total 1.5, weighted 0.75 | 0
    s.table[1] = torch.tensor([1 << 30, 0, _bits(0.002), 1 << 30, 1 << 29])         # total 0.25, weighted 0.25 | 0.125
    s.table[3] = torch.tensor([(1 << 53) + 1, 2, _bits(0.99), 1, (1 << 53) + 1])    # beyond float64's integers: still a sum
    s.views = 2
    assert s.total.dtype == torch.float64 and s.total.tolist()[:3] == [1.5, 0.25, 0.0]
    assert s.weighted.dtype == torch.float64 and s.weighted[:2].tolist() == [[0.75, 0.0], [0.25, 0.125]]
    assert s.max_weight.dtype == torch.float32 and s.max_weight.tolist() == [0.75, float(np.float32(0.002)), 0.0, float(np.float32(0.99))]
    assert s.top_count.dtype == torch.int64 and s.top_count.tolist() == [7, 0, 0, 2]
    lab = s.label()
    assert lab.dtype == torch.float64 and tuple(lab.shape) == (4, 2)
    assert lab[0, 0].item() == pytest.approx(0.5, abs=1e-7) and lab[1].tolist() == pytest.approx([1.0, 0.5], abs=1e-6)
    assert lab[2].tolist() == [0.0, 0.0] and float(lab.min()) >= 0.0 and float(lab.max()) <= 1.0
    assert s.select(0.6).tolist() == [False, True, False, False]
    assert s.low_contribution(max_weight_below=0.01).tolist() == [False, True, True, False]
    assert s.low_contribution(max_weight_below=0.0).tolist() == [False, False, False, False]
    assert s.low_contribution(max_weight_below=0.0, total_below=1.0).tolist() == [False, True, True, False]
    assert s.low_contribution().tolist() == [False, True, True, False]  # (default: below 1 / 255)
    o = ContributionStats(4, channels=2, device="cpu")
    o.table[0] = torch.tensor([1 << 31, 1, _bits(0.8), 0, 1 << 31])
    o.table[2] = torch.tensor([5, 1, _bits(0.001), 5, 0])
    o.views = 3
    want = s.table + o.table
    want[:, 2] = torch.maximum(s.table[:, 2], o.table[:, 2])
    a = ContributionStats(4, 2, "cpu").merge(s).merge(o)
    b = ContributionStats(4, 2, "cpu").merge(o).merge(s)
    assert torch.equal(a.table, want) and torch.equal(b.table, want) and a.views == b.views == 5
    assert a.max_weight[0].item() == float(np.float32(0.8)) and a.table[3, 0].item() == (1 << 53) + 1
    assert np.array_equal(CH.merge_tables(s.table.numpy(), o.table.numpy()), want.numpy())
    with pytest.raises(ValueError, match="merge"):
        a.merge(ContributionStats(4, 1, "cpu"))
    a.reset()
    assert not a.table.any() and a.views == 0
    with pytest.raises(ValueError):
        ContributionStats(4, channels=4, device="cpu")
    with pytest.raises(RuntimeError, match="at least one mask channel"):
        ContributionStats(4, device="cpu").select(0.5)
    assert Q_ONE == 4294967296.0


def test_trace_view_checks_its_arguments_without_a_device():
    from gaussianeditor_amd import contrib

    class PC:
        get_xyz = torch.zeros(4, 3)

    with pytest.raises(ValueError, match="rows"):
        contrib.trace_view(None, PC(), contrib.ContributionStats(5, device="cpu"))
    with pytest.raises(ValueError, match="needs no mask"):
        contrib.trace_view(None, PC(), contrib.ContributionStats(4, device="cpu"), mask=torch.zeros(8, 8))
    with pytest.raises(ValueError, match="a mask of 2 channels"):
        contrib.trace_view(None, PC(), contrib.ContributionStats(4, 2, device="cpu"))

    class Model:
        pass

    contrib.patch_gaussian_model(Model)
    assert callable(Model.apply_contributions)


def test_helper_restates_the_definitions():
    w = np.array([[0.0, 0.5, 0.25], [0.99, 0.5, 0.0]], np.float32)
    assert CH.q(w).tolist() == [[0, 1 << 31, 1 << 30], [int(np.floor(float(np.float32(0.99)) * 2.0 ** 32)), 1 << 31, 0]]
    m = CH.clamp_mask(np.array([-1.0, np.nan, 0.0, 0.3, 1.0, 7.0], np.float32))
    assert m.tolist() == [0.0, 0.0, 0.0, float(np.float32(0.3)), 1.0, 1.0]
    rows = CH.expected_rows(w, np.array([[1.0, 0.5, 2.0], [0.0, -3.0, np.nan]], np.float32))
    assert rows[:, 0].tolist() == [3 << 30, int(CH.q(w)[1].sum())] and rows[:, 1].tolist() == [0, 0]
    assert rows[:, 2].tolist() == [_bits(0.5), _bits(0.99)]
    assert rows[0, 3] == (1 << 30) + (1 << 30) and rows[:, 4].tolist() == [0, 0]
    # ties: the front-most entry of the tile's list wins, whatever the Gaussians' numbers are
    ranges, plist = np.array([[0, 2]], np.uint32), np.array([1, 0], np.uint32)
    top_id, top_w, tied = CH.expected_top(w, [0, 1], ranges, plist, 3, 1)
    assert top_id.tolist() == [1, 1, 0] and top_w.tolist() == [float(np.float32(0.99)), 0.5, 0.25] and tied == 1
    top_id, _, _ = CH.expected_top(w, [0, 1], ranges, np.array([0, 1], np.uint32), 3, 1)
    assert top_id.tolist() == [1, 0, 0]
    top_id, top_w, _ = CH.expected_top(np.zeros((2, 3), np.float32), [0, 1], ranges, plist, 3, 1)
    assert top_id.tolist() == [-1, -1, -1] and not top_w.any()


@pytest.mark.parametrize("name", list(CH.EXHAUSTIVE))
def test_reference_weights_sum_to_the_oracles_alpha(oracle, name):
    """sum_g w per pixel equals 1 - final_T within 1e-6 on the exhaustive cases, which are what the issue says they are: no
    pixel with a tied top weight, pixels that saturate, many distinct top ids, lists longer than one chunk where stated."""
    exp = CH.exhaustive_expectation(oracle, name)
    P, W, H, _, _ = CH.EXHAUSTIVE[name]
    w, final_T = exp["weights"], exp["final_T"]
    assert w.shape == (P, H * W) and float(w.min()) >= 0.0 and float(w.max()) <= 0.99
    err = float(np.abs(w.astype(np.float64).sum(axis=0) - (1.0 - final_T.astype(np.float64))).max())
    ranges = exp["state"][1]["ranges"].astype(np.int64)
    lens = ranges[:, 1] - ranges[:, 0]
    distinct = len(np.unique(exp["top_id"][exp["top_id"] >= 0]))
    saturated = int((final_T < 2e-4).sum())
    print(f"  {name}: sum_g w vs 1 - final_T {err:.2e}; tiles {lens.size}, empty {int((lens == 0).sum())}, longest list "
          f"{int(lens.max())}; tied pixels {exp['tied']}, saturated {saturated}, distinct top ids {distinct}")
    assert err <= 1e-6
    # (distinct top ids, measured: 49, 20 on the one-tile case of 256 pixels, up to 82 -- the pick buffer is no constant image)
    assert exp["tied"] == 0 and saturated > 0 and distinct >= 16
    assert int(exp["top_count"].sum()) == int((exp["top_id"] >= 0).sum())
    if name == "six_tiles":
        assert lens.size == 6 and int((lens == 0).sum()) == 2 and int((lens > 64).sum()) == 3
    if name == "one_tile":
        assert lens.tolist() == [200]
    if name == "fifteen_tiles":
        assert lens.size == 15 and int((lens == 0).sum()) == 6
