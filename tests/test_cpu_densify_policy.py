"""CPU: the densification policy's two restatements agree with each other and with torch.quantile, and the new entry points
and wrappers validate their arguments before they touch a device."""
import ctypes

import numpy as np
import pytest
import torch

import densify_helpers as dh


def _t(accum, denom, mask, scaling):
    return (torch.from_numpy(accum.copy())[:, None], torch.from_numpy(denom.copy())[:, None], torch.from_numpy(mask.copy()),
            torch.from_numpy(scaling.copy()))


@pytest.mark.parametrize("P", dh.PS)
def test_numpy_select_equals_the_reference_lines(P):
    """select_np (the kernels' arithmetic) against gaussian_model.py:771-777 / :732-739 / :676-683 run by torch on the CPU:
    masks and counts exact, the threshold equal by value."""
    n_sel = 0
    for kind in dh.KINDS:
        case = dh.select_case(P, kind)
        for pct in dh.PERCENTS:
            a = dh.select_np(*case, dh.MAX_GRAD, pct, dh.PERCENT_DENSE, dh.EXTENT)
            b = dh.select_torch(*_t(*case), dh.MAX_GRAD, pct, dh.PERCENT_DENSE, dh.EXTENT)
            tag = (P, kind, pct)
            assert np.array_equal(a[0], b[0].numpy()) and np.array_equal(a[1], b[1].numpy()), tag
            assert a[2:5] == b[2:5], tag
            if pct < 1:
                assert dh.same_value(a[5], b[5]), (tag, a[5], float(b[5]))
            else:
                assert b[5] is None and a[5] == 0
            n_sel += a[3] + a[4]
    assert P < 255 or n_sel > 0  # the cases do select rows


@pytest.mark.parametrize("P", dh.PS)
def test_quantile_restatement_equals_torch_quantile(P):
    from oracle.cpu import _quantile_f32

    for kind in dh.KINDS:
        accum, denom, mask, _ = dh.select_case(P, kind)
        with np.errstate(all="ignore"):
            g = (accum / denom).astype(np.float32)
        g[np.isnan(g)] = 0
        g[~mask] = 0
        nnz = int(np.count_nonzero(g))
        for pct in (0.01, 0.5):
            q = 1 - nnz * pct / P
            with np.errstate(all="ignore"):
                got = _quantile_f32(g, q)
            want = torch.quantile(torch.from_numpy(g), q)
            assert dh.same_value(got, want), (P, kind, pct, got, float(want))


def test_boundary_constants_pin_the_scalar_rounding():
    """The shared cases hold rows exactly at both thresholds, and both thresholds differ between binary32 and double."""
    accum, denom, mask, scaling = dh.select_case(257, "sparse")
    with np.errstate(all="ignore"):
        g = accum / denom
    assert (g[mask] == np.float32(dh.MAX_GRAD)).any() and (scaling.max(axis=1) == dh.T_DENSE).any()
    assert float(dh.T_DENSE) > dh.PERCENT_DENSE * dh.EXTENT  # a double comparison would call the boundary rows "large"
    clone, split, *_ = dh.select_np(accum, denom, mask, scaling, dh.MAX_GRAD, 1.0, dh.PERCENT_DENSE, dh.EXTENT)
    at = (g == np.float32(dh.MAX_GRAD)) & mask
    assert (clone | split)[at].all()                      # g == (float)max_grad is selected (>=)
    edge = scaling.max(axis=1) == dh.T_DENSE
    assert not split[edge].any() and clone[edge & at].all()  # max(scaling) == t_dense is cloned (<=), never split (>)


def test_entry_points_validate_before_touching_the_device():
    from gaussianeditor_amd import _native

    L = _native.lib()
    one = ctypes.c_void_p(256)
    sz = ctypes.c_size_t(0)
    assert L.gsr_densify_workspace_size(1 << 24, ctypes.byref(sz)) == 0 and sz.value > 4 * (1 << 24)
    assert L.gsr_densify_workspace_size(0, ctypes.byref(sz)) == 0 and sz.value > 0
    assert L.gsr_densify_workspace_size((1 << 24) + 1, ctypes.byref(sz)) == -1
    assert L.gsr_densify_workspace_size(-1, ctypes.byref(sz)) == -1
    assert L.gsr_densify_workspace_size(10, None) == -1
    # statistics
    ptrs = (ctypes.c_void_p * 8)(*([256] * 8))
    none1 = (ctypes.c_void_p * 1)(None)
    assert L.gsr_densify_stats(None, 0, 1, None, None, None, None, None) == 0  # P == 0: an empty call
    assert L.gsr_densify_stats(None, -1, 1, ptrs, ptrs, one, one, one) == -1
    assert L.gsr_densify_stats(None, 10, 0, ptrs, ptrs, one, one, one) == -1
    assert L.gsr_densify_stats(None, 10, 9, ptrs, ptrs, one, one, one) == -1
    assert L.gsr_densify_stats(None, 10, 1, None, ptrs, one, one, one) == -1
    assert L.gsr_densify_stats(None, 10, 1, ptrs, None, one, one, one) == -1
    assert L.gsr_densify_stats(None, 10, 1, none1, ptrs, one, one, one) == -1
    assert L.gsr_densify_stats(None, 10, 1, ptrs, ptrs, None, one, one) == -1
    assert L.gsr_densify_stats(None, 10, 1, ptrs, ptrs, one, None, one) == -1
    assert L.gsr_densify_stats(None, 10, 1, ptrs, ptrs, one, one, None) == -1
    # selection
    res = _native.DensifyResult(7, 7, 7, 7.0)
    def select(P, accum=one, denom=one, mask=one, scaling=one, mg=2e-4, pct=0.01, work=one, c=one, s=one, r=res):
        return L.gsr_densify_select(None, P, accum, denom, mask, scaling, mg, pct, 0.01, 1.0, work, c, s,
                                    None if r is None else ctypes.byref(r))
    assert select(0) == 0 and (res.nonzero, res.n_clone, res.n_split, res.threshold) == (0, 0, 0, 0.0)
    assert select(10, r=None) == -1
    assert select(-1) == -1 and select((1 << 24) + 1) == -1
    assert select(10, mg=0.0) == -1 and select(10, mg=-1.0) == -1 and select(10, mg=float("nan")) == -1
    assert select(10, pct=-0.5) == -1
    for k in ("accum", "denom", "mask", "scaling", "work", "c", "s"):
        assert select(10, **{k: None}) == -1, k
    assert select(10, work=ctypes.c_void_p(260)) == -1  # 8-byte aligned scratch
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.gsr_densify_plans(None, 10, ctypes.byref(a), ctypes.byref(b)) == -1
    assert L.gsr_densify_plans(one, 10, None, ctypes.byref(b)) == -1
    assert L.gsr_densify_plans(one, (1 << 24) + 1, ctypes.byref(a), ctypes.byref(b)) == -1
    assert L.gsr_densify_plans(ctypes.c_void_p(1 << 20), 5000, ctypes.byref(a), ctypes.byref(b)) == 0
    assert (1 << 20) + 256 + 8192 + 4 * 5000 <= a.value < b.value and a.value % 256 == 0 and b.value % 256 == 0
    # split positions
    def split(P=10, n_split=3, N=2, **kw):
        args = dict(xyz=one, scaling=one, rotation=one, sel=one, plan=one, noise=one, out=one)
        args.update(kw)
        return L.gsr_densify_split_xyz(None, P, args["xyz"], args["scaling"], args["rotation"], args["sel"], args["plan"], n_split,
                                       N, args["noise"], args["out"])
    assert split(P=0, n_split=0) == 0 and split(n_split=0) == 0  # nothing to do
    assert split(P=-1) == -1 and split(n_split=-1) == -1 and split(n_split=11) == -1
    assert split(N=0) == -1 and split(N=9) == -1
    for k in ("xyz", "scaling", "rotation", "sel", "plan", "noise", "out"):
        assert split(**{k: None}) == -1, k
    # prune mask: max_radii2D and drop may be NULL, the others not
    def keep(P=10, **kw):
        args = dict(opacity=one, scaling=one, radii=None, mask=one, drop=None, keep=one)
        args.update(kw)
        return L.gsr_densify_keep(None, P, args["opacity"], args["scaling"], args["radii"], args["mask"], args["drop"], 0.005, 20.0,
                                  1.0, args["keep"])
    assert keep(P=0) == 0 and keep(P=-1) == -1
    for k in ("opacity", "scaling", "mask", "keep"):
        assert keep(**{k: None}) == -1, k


def test_wrappers_validate_devices_dtypes_and_ranges():
    """No CPU fallback; wrong dtypes, more than 8 views, N outside 1..8, max_grad <= 0 and P > 2**24 are refused in Python."""
    from gaussianeditor_amd import densify

    for name in ("add_densification_stats", "select_densification", "split_positions", "prune_keep_mask", "densify_and_prune"):
        assert name in densify.__all__ and callable(getattr(densify, name))
    P = 4
    f = torch.zeros(P)
    g, r = torch.zeros(P, 3), torch.zeros(P, dtype=torch.int32)
    with pytest.raises(ValueError):
        densify.add_densification_stats(f, f, f, [g] * 9, [r] * 9)
    with pytest.raises(ValueError):
        densify.add_densification_stats(f, f, f, [], [])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        densify.add_densification_stats(f, f, f, [g], [r])
    kw = dict(max_grad=2e-4, max_densify_percent=0.01, percent_dense=0.01, extent=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        densify.select_densification(f, f, torch.ones(P, dtype=torch.bool), g, **kw)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            densify.select_densification(f, f, torch.ones(P, dtype=torch.bool), g, **dict(kw, max_grad=bad))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        densify.split_positions(g, g, torch.zeros(P, 4), torch.ones(P, dtype=torch.bool), torch.zeros(2 * P, 3))
    for bad in (0, 9):
        with pytest.raises(ValueError):
            densify.split_positions(g, g, torch.zeros(P, 4), torch.ones(P, dtype=torch.bool), torch.zeros(2 * P, 3), N=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        densify.prune_keep_mask(f, g, torch.ones(P, dtype=torch.bool), min_opacity=0.005, max_screen_size=20, extent=1.0)
    # dtypes are looked at first, so a wrong one is named even here
    with pytest.raises(RuntimeError, match="dtype"):
        densify.select_densification(f.double(), f, torch.ones(P, dtype=torch.bool), g, **kw)
    with pytest.raises(RuntimeError, match="dtype"):
        densify.select_densification(f, f, torch.ones(P, dtype=torch.int32), g, **kw)
    with pytest.raises(RuntimeError, match="dtype"):
        densify.add_densification_stats(f, f, f, [g], [r.long()])
    with pytest.raises(RuntimeError, match="dtype"):
        densify.split_positions(g, g.half(), torch.zeros(P, 4), torch.ones(P, dtype=torch.bool), torch.zeros(2 * P, 3))
    with pytest.raises(RuntimeError, match="dtype"):
        densify.prune_keep_mask(f, g, torch.ones(P), min_opacity=0.005, max_screen_size=20, extent=1.0)
