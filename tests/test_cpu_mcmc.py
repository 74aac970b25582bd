"""CPU: the parts of the 3DGS-MCMC strategy that need no GPU -- argument validation of the gsr_mcmc_*
entry points, the header / binding / export agreement, and the restatements of tests/mcmc_helpers.py checked against
something simpler than themselves: a brute-force cumulative search, the expected frequencies, and mpmath."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import mcmc_helpers as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ENTRY_POINTS = ("gsr_mcmc_noise", "gsr_mcmc_workspace_size", "gsr_mcmc_sample", "gsr_mcmc_relocation_values", "gsr_mcmc_scatter")
MIN_OPACITY = 0.005


def test_entry_points_are_declared_typed_and_exported():
    from gaussianeditor_amd import _native, mcmc

    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    for name in ENTRY_POINTS:
        assert f"int {name}(" in hdr and name in _native.SIGNATURES and hasattr(_native.lib(), name)
    declared = sorted(set(re.findall(r"\b(gsr_mcmc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == sorted(ENTRY_POINTS) == sorted(k for k in _native.SIGNATURES if k.startswith("gsr_mcmc_"))
    assert _native.lib().gsr_abi_version() == 6 and "#define GSR_ABI_VERSION 6" in hdr
    assert ctypes.sizeof(_native.McmcRecord) == 32 and ctypes.sizeof(_native.McmcTensor) == 40
    assert (_native.MCMC_COPY, _native.MCMC_VALUE, _native.MCMC_ZERO) == tuple(
        int(re.search(rf"#define GSR_MCMC_{k} (\d+)", hdr).group(1)) for k in ("COPY", "VALUE", "ZERO"))
    for name in ("inject_noise", "classify_and_sample", "relocation_values", "relocate", "add_new", "mcmc_refine"):
        assert name in mcmc.__all__ and callable(getattr(mcmc, name))
    assert mcmc.RATIO_CAP == mh.RATIO_CAP == 51
    # nothing of the package imports the oracle
    src = open(os.path.join(ROOT, "gaussianeditor_amd", "mcmc.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M)


def test_argument_validation_needs_no_gpu():
    """NULL pointers, negative sizes and misaligned memory come back as GSR_ERR_BAD_ARGUMENT (-1) before the device is
    touched; P == 0 / n == 0 are valid empty calls."""
    from gaussianeditor_amd import _native

    L = _native.lib()
    a = ctypes.c_void_p(256)  # never dereferenced
    odd = ctypes.c_void_p(258)
    # noise
    assert L.gsr_mcmc_noise(None, 0, None, None, None, None, None, None, 100.0, 0.995, 1.0) == 0
    assert L.gsr_mcmc_noise(None, -1, a, a, a, a, a, None, 100.0, 0.995, 1.0) == -1
    assert L.gsr_mcmc_noise(None, 1 << 31, a, a, a, a, a, None, 100.0, 0.995, 1.0) == -1
    for hole in range(5):
        args = [a] * 5
        args[hole] = None
        assert L.gsr_mcmc_noise(None, 10, *args, None, 100.0, 0.995, 1.0) == -1, hole
    assert L.gsr_mcmc_noise(None, 10, odd, a, a, a, a, None, 100.0, 0.995, 1.0) == -1      # xyz not 4-byte aligned
    assert L.gsr_mcmc_noise(None, 10, a, a, ctypes.c_void_p(260), a, a, None, 100.0, 0.995, 1.0) == -1  # rotation not 16-byte aligned
    # workspace size
    sz = ctypes.c_size_t(0)
    assert L.gsr_mcmc_workspace_size(0, ctypes.byref(sz)) == 0 and sz.value >= 256
    assert L.gsr_mcmc_workspace_size(1_000_000, ctypes.byref(sz)) == 0 and 4_000_000 <= sz.value < 4_200_000
    assert L.gsr_mcmc_workspace_size(-1, ctypes.byref(sz)) == -1 and L.gsr_mcmc_workspace_size(10, None) == -1
    # sample
    rec = _native.McmcRecord(7, 7, 7, 7)
    assert L.gsr_mcmc_sample(None, 0, 0, None, None, 0.005, None, 1, None, None, None, None, None, None, ctypes.byref(rec)) == 0
    assert (rec.n_dead, rec.n_alive, rec.n_draws, rec.total) == (0, 0, 0, 0)
    assert L.gsr_mcmc_sample(None, 0, 5, None, None, 0.005, None, 0, None, None, None, None, None, None, ctypes.byref(rec)) == 0
    assert L.gsr_mcmc_sample(None, 10, 5, a, None, 0.005, a, 0, a, a, a, a, a, a, None) == -1          # no record
    assert L.gsr_mcmc_sample(None, -1, 5, a, None, 0.005, a, 0, a, a, a, a, a, a, ctypes.byref(rec)) == -1
    assert L.gsr_mcmc_sample(None, 10, -1, a, None, 0.005, a, 0, a, a, a, a, a, a, ctypes.byref(rec)) == -1
    assert L.gsr_mcmc_sample(None, 10, 5, a, None, 0.005, a, 0, ctypes.c_void_p(260), a, a, a, a, a, ctypes.byref(rec)) == -1  # workspace
    for hole in (3, 8, 9, 10, 12):  # opacity, workspace, dead_sel, dead_idx, count
        args = [None, 10, 0, a, None, 0.005, None, 0, a, a, a, None, a, None]
        args[hole] = None
        assert L.gsr_mcmc_sample(*args, ctypes.byref(rec)) == -1, hole
    for hole in (6, 11, 13):  # u, src, ratio: needed once draws are requested
        args = [None, 10, 5, a, None, 0.005, a, 0, a, a, a, a, a, a]
        args[hole] = None
        assert L.gsr_mcmc_sample(*args, ctypes.byref(rec)) == -1, hole
    # relocation values
    assert L.gsr_mcmc_relocation_values(None, 0, 5, None, None, None, None, 0.005, None, None) == 0
    assert L.gsr_mcmc_relocation_values(None, 10, 0, None, None, None, None, 0.005, None, None) == 0
    assert L.gsr_mcmc_relocation_values(None, -1, 5, a, a, a, a, 0.005, a, a) == -1
    assert L.gsr_mcmc_relocation_values(None, 10, -5, a, a, a, a, 0.005, a, a) == -1
    for hole in (3, 4, 5, 6, 8, 9):
        args = [None, 10, 5, a, a, a, a, 0.005, a, a]
        args[hole] = None
        assert L.gsr_mcmc_relocation_values(*args) == -1, hole
    # scatter
    T = _native.McmcTensor
    one = (T * 1)(T(a, a, None, 12, _native.MCMC_COPY))
    assert L.gsr_mcmc_scatter(None, 10, 0, None, None, 10, 1, one) == 0 and L.gsr_mcmc_scatter(None, 0, 5, None, None, 0, 1, one) == 0
    assert L.gsr_mcmc_scatter(None, 10, 5, a, None, 10, 0, None) == 0
    assert L.gsr_mcmc_scatter(None, 10, 5, None, None, 10, 1, one) == -1 and L.gsr_mcmc_scatter(None, 10, 5, a, None, 10, 1, None) == -1
    assert L.gsr_mcmc_scatter(None, -1, 5, a, None, 10, 1, one) == -1 and L.gsr_mcmc_scatter(None, 10, -5, a, None, 10, 1, one) == -1
    assert L.gsr_mcmc_scatter(None, 10, 5, a, None, -1, 1, one) == -1 and L.gsr_mcmc_scatter(None, 10, 5, a, None, 10, 33, one) == -1
    for bad in (T(None, a, None, 12, 0), T(a, None, None, 12, 0), T(a, a, None, 12, 1), T(a, a, a, 12, 3), T(a, a, a, 12, -1),
                T(a, a, None, 6, 0), T(a, a, None, 0, 0), T(a, a, None, (1 << 20) + 4, 0), T(odd, a, None, 12, 0),
                T(a, odd, None, 12, 0), T(a, a, odd, 12, 1), T(None, None, None, 12, 2)):
        assert L.gsr_mcmc_scatter(None, 10, 5, a, None, 10, 1, (T * 1)(bad)) == -1, (bad.base, bad.dst, bad.values, bad.row_bytes, bad.role)


def test_wrappers_refuse_cpu_tensors_and_name_the_argument():
    import torch

    from gaussianeditor_amd import mcmc

    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="xyz .*no CPU fallback"):
        mcmc.inject_noise(x, x, torch.zeros(4, 4), torch.zeros(4, 1), x, scaler=1.0)
    with pytest.raises(RuntimeError, match="opacity .*no CPU fallback"):
        mcmc.classify_and_sample(torch.zeros(4), torch.zeros(2))
    with pytest.raises(RuntimeError, match="opacity .*no CPU fallback"):
        mcmc.relocation_values(torch.zeros(4), x, torch.zeros(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32))


# ----------------------------------------------------------------------------------------------------------------------
# the sampling restatement
# ----------------------------------------------------------------------------------------------------------------------
def _brute(opacity, u, min_opacity, mask):
    """Cumulative linear search, one draw at a time."""
    _, _, k = mh.weights_int(opacity, mask, min_opacity)
    total = sum(k)
    out = []
    for x in u:
        t = mh.draw_int(x, total)
        acc, hit = 0, -1
        for j, w in enumerate(k):
            acc += w
            if acc > t:
                hit = j
                break
        out.append(hit)
    return out, total


@pytest.mark.parametrize("P", [1, 2, 257])
def test_sampling_restatement_equals_a_brute_force_search(P):
    rng = np.random.default_rng(P)
    opacity = rng.random(P).astype(F)
    opacity[::3] = F(0.001)              # dead
    opacity[0] = F(0.7)
    if P > 2:
        opacity[5] = F(MIN_OPACITY)      # exactly at the threshold: dead
        opacity[7] = np.nan              # neither
    mask = rng.random(P) < 0.8
    mask[0] = True
    u = np.concatenate((rng.random(500).astype(F), [F(0), F(1 - 2.0 ** -24)])).astype(F)
    got = mh.sample_int(opacity, u, MIN_OPACITY, mask, n_draws=len(u))
    want, total = _brute(opacity, u, MIN_OPACITY, mask)
    assert got["src"].tolist() == want and got["record"][3] == total > 0
    assert all(mask[j] and opacity[j] > F(MIN_OPACITY) for j in want)
    assert np.array_equal(got["count"], np.bincount(want, minlength=P))
    assert np.array_equal(got["ratio"], np.minimum(got["count"][want] + 1, 51))
    dead = mask & (opacity <= F(MIN_OPACITY))
    assert np.array_equal(got["dead_sel"], dead) and got["dead_idx"].tolist() == np.flatnonzero(dead).tolist()
    assert got["record"][:2] == (int(dead.sum()), int((mask & (opacity > F(MIN_OPACITY))).sum()))
    if P > 2:
        assert got["dead_sel"][5] and not got["dead_sel"][7] and got["count"][7] == 0
    # u = 0 draws the first alive row, the largest u the last one
    alive = np.flatnonzero(mask & (opacity > F(MIN_OPACITY)))
    assert want[-2] == alive[0] and want[-1] == alive[-1]


def test_sampling_frequencies_follow_the_weights():
    rng = np.random.default_rng(8)
    opacity = np.array([0.9, 0.003, 0.25, 0.5, 0.011, 0.75, 0.05, 0.33], F)
    n = 200_000
    u = rng.random(n).astype(F)  # (float32 of a double: a multiple of 2^-24 below 1, or 1.0 rounded up, which draws as the largest u)
    got = mh.sample_int(opacity, u, MIN_OPACITY, None, n_draws=n)
    _, _, k = mh.weights_int(opacity, None, MIN_OPACITY)
    total = sum(k)
    assert got["record"] == (1, 7, n, total) and got["count"][1] == 0 and int(got["count"].sum()) == n
    for j, w in enumerate(k):
        p = w / total
        sd = math.sqrt(n * p * (1 - p))
        assert abs(int(got["count"][j]) - n * p) <= 5 * sd, (j, int(got["count"][j]), n * p, sd)


# ----------------------------------------------------------------------------------------------------------------------
# the relocation restatement
# ----------------------------------------------------------------------------------------------------------------------
def _mp_values(o32, n, min_opacity):
    """(o' clamped, o / denom) by mpmath at 80 digits from the float32 opacity."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 80
    o = min(mp.mpf(float(o32)), mp.mpf(1) - mp.mpf(2) ** -24)
    n = min(n, 51)
    op = 1 - (1 - o) ** (mp.mpf(1) / n)
    denom = mp.mpf(0)
    for i in range(1, n + 1):
        for k in range(i):
            denom += mp.binomial(i - 1, k) * (-1) ** k * op ** (k + 1) / mp.sqrt(k + 1)
    f = o / denom
    op = min(max(op, mp.mpf(float(F(min_opacity)))), mp.mpf(1) - mp.mpf(2) ** -23)
    return op, f


@pytest.mark.parametrize("n", [1, 2, 5, 20, 51, 60])
def test_relocation_restatement_against_mpmath(n):
    """binary64 in the stated order stays within 1e-11 (relative) of the 80-digit evaluation over the whole range: the
    clamp of o at 1 - 2^-24 is what bounds the cancellation of the alternating sum."""
    pytest.importorskip("mpmath")
    grid = [np.nextafter(F(MIN_OPACITY), F(1)), F(0.5), F(0.99), F(1 - 2.0 ** -24), F(1.0)]
    op, f = mh.relocation_f64(np.array(grid, F), np.full(len(grid), n), MIN_OPACITY)
    worst = 0.0
    for i, o in enumerate(grid):
        want_op, want_f = _mp_values(o, n, MIN_OPACITY)
        e_op = abs(float((op[i] - want_op) / want_op))
        e_f = abs(float((f[i] - want_f) / want_f))
        worst = max(worst, e_op, e_f)
        assert e_op <= 1e-11 and e_f <= 1e-11, (float(o), n, e_op, e_f)
    print(f"n = {n}: worst relative error of the float64 restatement against mpmath {worst:.2e}")
    # o = 1.0 is clamped to 1 - 2^-24 and n = 60 capped at 51: the same numbers as those inputs give
    assert op[4] == op[3] and f[4] == f[3]
    if n == 60:
        op51, f51 = mh.relocation_f64(np.array(grid, F), np.full(len(grid), 51), MIN_OPACITY)
        assert np.array_equal(op, op51) and np.array_equal(f, f51)


def test_one_draw_leaves_opacity_and_scale_as_they_are():
    """n = 1: o' = 1 - (1 - o) and denom = o', so the source keeps its opacity and its scale up to the rounding of that one
    subtraction: 2^-53 absolute, at most 2^-53 / min_opacity < 1e-13 relative."""
    o = np.array([np.nextafter(F(MIN_OPACITY), F(1)), 0.02, 0.5, 0.99, 1 - 2.0 ** -24], F)
    op, f = mh.relocation_f64(o, np.ones(len(o), np.int64), MIN_OPACITY)
    o64 = np.minimum(o.astype(np.float64), 1 - 2.0 ** -23)  # (the new opacity's own clamp applies to the last one)
    assert np.abs(op - o64).max() <= 2.0 ** -52 and np.abs(f - 1.0).max() <= 1e-13
    sr = np.log(np.array([[0.01, 0.02, 0.3]] * len(o), F))
    new_o, new_s = mh.relocation_values_f64(o, sr, np.arange(len(o)), np.ones(len(o), np.int32), MIN_OPACITY)
    assert np.allclose(new_o, np.log(o64 / (1 - o64)), rtol=1e-12, atol=1e-12) and np.allclose(new_s, sr.astype(np.float64), rtol=0, atol=1e-12)
