"""CPU: the sizes tests/test_gpu_size_regimes.py uses lie in the second size regime they claim, and the cases are not
degenerate there.

Every threshold is parsed out of the sources' text (densify_helpers.kernel_constants): CMP_ROWS / VIEW_MSG_ROWS, the step of
compact_scan_kernel's carry loop, CMP_MAX_TENSORS, CMP_TENSORS_PER_BLOCK, DNS_BLOCK, DNS_MAX_BLOCKS, MC_BLOCK, LT_W, LT_H,
LTHREADS, the two grid caps of 4096 blocks and append_rows_kernel's 64 bytes per thread.  A later change of one of them
fails here instead of moving the GPU tests back into the first regime without a word.

The large references then run once without a GPU: selection counts, survivors on both sides of row 1 048 576, dead rows
beyond block 1024, draws on both sides; and the float32 evaluation that stands in for the reference's own float32 result
at the loss shape the fixture does not hold is pinned to the fixture's arrays on every fixture case.  The file runs in
about 10 s: 3 s for the float64 and float32 losses at 3 x 145 x 577, 1 s each for mcmc_helpers.sample_int over 1 049 601
rows in Python integers, the selection's reference lines at that size and the generation of the large inputs.
"""
import numpy as np
import pytest
import torch

import densify_helpers as dh
import loss_helpers as LH
import mcmc_helpers as mh

K = dh.kernel_constants()


def _blocks(n, per):
    return (n + per - 1) // per


def test_constants_are_the_ones_the_issue_was_derived_from():
    assert K["CMP_ROWS"] == K["VIEW_MSG_ROWS"] == K["SPLIT_ROWS"] == 1024 and K["SCAN_CHUNK"] == 1024
    assert K["CMP_ROWS"] * K["SCAN_CHUNK"] == dh.SCAN_EDGE
    assert K["CMP_MAX_TENSORS"] == K["PY_CHUNK"] == K["MC_MAX_TENSORS"] == 32 and K["CMP_TENSORS_PER_BLOCK"] == 8
    assert (K["DNS_BLOCK"], K["DNS_MAX_BLOCKS"], K["MC_BLOCK"]) == (256, 1024, 256)
    assert (K["LT_W"], K["LT_H"], K["LTHREADS"]) == (64, 16, 256)
    assert K["APPEND_MAX_BLOCKS"] == K["MC_SCATTER_MAX_BLOCKS"] == 4096 and K["APPEND_BLOCK_BYTES"] == 256 * 64


def test_compaction_sizes_enter_the_carry_loop():
    """compact_scan_kernel takes a second trip when there are more row blocks than SCAN_CHUNK."""
    nb = _blocks(dh.PC, K["CMP_ROWS"])
    assert nb == K["SCAN_CHUNK"] + 2 and dh.PC - (nb - 1) * K["CMP_ROWS"] == 1  # two blocks in the second trip, the last with one row
    assert _blocks(dh.SCAN_EDGE, K["CMP_ROWS"]) == K["SCAN_CHUNK"]               # exactly one full trip
    assert _blocks(dh.SCAN_EDGE + 1, K["CMP_ROWS"]) == K["SCAN_CHUNK"] + 1
    assert len(dh.compact_tensors(4)) > K["CMP_TENSORS_PER_BLOCK"]                 # two blockIdx.y groups
    widths = sorted({t.element_size() * (t.numel() // 4) for t in dh.compact_tensors(4)})
    assert widths == [1, 2, 3, 4, 8, 12, 16, 20, 180]                             # all three branches of compact_apply_kernel


def test_compaction_masks_keep_rows_on_the_sides_they_claim():
    masks = dh.compact_masks(dh.PC)
    lo = {k: int(m[:dh.SCAN_EDGE].sum()) for k, m in masks.items()}
    hi = {k: int(m[dh.SCAN_EDGE:].sum()) for k, m in masks.items()}
    tail = dh.PC - dh.SCAN_EDGE
    assert 0.49 * dh.SCAN_EDGE < lo["random"] < 0.51 * dh.SCAN_EDGE and 0.4 * tail < hi["random"] < 0.6 * tail
    assert (lo["tail_only"], hi["tail_only"]) == (0, tail)
    assert lo["head_kept"] == dh.SCAN_EDGE and 0.4 * tail < hi["head_kept"] < 0.6 * tail and bool(masks["head_kept"][-1])
    assert (lo["last_row"], hi["last_row"]) == (0, 1) and bool(masks["last_row"][-1])
    for P in (dh.SCAN_EDGE, dh.SCAN_EDGE + 1):  # the random mask cut to the two sizes around the edge
        assert 0 < int(masks["random"][:P].sum()) < P and bool(masks["random"][P - 1])  # the last block has its survivor


def test_plan_consumers_have_rows_in_the_second_trip():
    xyz, scaling, rot, sel, noise = dh.split_case_large(dh.PC)
    idx = np.flatnonzero(sel)
    assert {0, dh.SCAN_EDGE - 1, dh.SCAN_EDGE, dh.PC - 1} <= set(idx.tolist()) and 300 <= idx.size <= 304
    assert noise.shape == (2 * idx.size, 3)
    want, l1, pxyz = dh.split_np(xyz, scaling, rot, sel, noise, 2)
    ref64, _, _ = dh.split_np(xyz, scaling, rot, sel, noise, 2, dtype=np.float64)
    assert (np.abs(want.astype(np.float64) - ref64) <= dh.split_bound(l1, pxyz)).all()
    grads5, rgb, touched = dh.message_case_large(dh.PC)
    any_nz = torch.cat([g.reshape(dh.PC, -1) for g in grads5] + [rgb], dim=1).ne(0).any(dim=1)
    assert torch.equal(any_nz, touched) and 0.008 * dh.PC < int(touched.sum()) < 0.012 * dh.PC
    assert int(touched[dh.SCAN_EDGE:dh.SCAN_EDGE + 1024].sum()) >= 2 and bool(touched[dh.PC - 1])
    for t in grads5 + [rgb]:  # no tensor alone gives the mask away, and no -0 hides in an untouched row
        nz = t.ne(0).any(dim=1)
        assert 0 < int(nz.sum()) < int(touched.sum())
        assert not bool(torch.signbit(t[~nz]).any())


@pytest.mark.parametrize("P", (dh.PD, dh.PC))
def test_densify_sizes_stride_and_select_something(P):
    """densify_grad_kernel / densify_hist_kernel: the grid is capped at DNS_MAX_BLOCKS blocks of DNS_BLOCK rows."""
    assert _blocks(P, K["DNS_BLOCK"]) > K["DNS_MAX_BLOCKS"]
    assert P % K["DNS_BLOCK"] != 0 and P % (K["DNS_BLOCK"] * K["DNS_MAX_BLOCKS"]) != 0  # ragged block, ragged second trip
    assert P <= 1 << 24                                                               # select_densification's own limit
    for kind in ("sparse", "lowbyte", "extremes"):
        accum, denom, mask, scaling = dh.select_case(P, kind)
        for pct in dh.PERCENTS:
            clone, split, nnz, n_clone, n_split, thr = dh.select_torch(
                torch.from_numpy(accum.copy())[:, None], torch.from_numpy(denom.copy())[:, None], torch.from_numpy(mask.copy()),
                torch.from_numpy(scaling.copy()), dh.MAX_GRAD, pct, dh.PERCENT_DENSE, dh.EXTENT)
            print(f"  P={P} {kind} {pct}: nonzero {nnz}, clones {n_clone}, splits {n_split}")
            assert n_clone > 0 and n_split > 0 and nnz >= n_clone + n_split, (P, kind, pct)
            stride = K["DNS_BLOCK"] * K["DNS_MAX_BLOCKS"]
            assert bool((clone | split)[stride:].any()) and bool((clone | split)[:stride].any())  # both trips matter


def test_append_and_scatter_sizes_pass_the_grid_caps():
    cap_bytes = K["APPEND_MAX_BLOCKS"] * K["APPEND_BLOCK_BYTES"]
    assert cap_bytes == 64 * 1024 * 1024
    assert (dh.P_APPEND + dh.N_APPEND) * mh.F_REST_WORDS * 4 > cap_bytes           # the (P, 15, 3) float32 tensor strides
    assert (dh.P_APPEND + dh.N_APPEND) * 12 < cap_bytes                             # ... its narrow neighbours do not
    cap_words = K["MC_SCATTER_MAX_BLOCKS"] * K["MC_BLOCK"]
    assert cap_words == 1024 * 1024
    mask = mh.refine_mask_large()
    n_dead = int(mask[::mh.DEAD_EVERY].sum())                                       # the dead rows inside the mask: the draws
    print(f"  refine at P = {mh.P_REFINE}: {n_dead} dead rows inside the mask")
    assert n_dead >= 23303 and n_dead * mh.F_REST_WORDS > cap_words                 # relocation: COPY and ZERO of f_rest stride
    n_new = int(mh.GROW_REFINE * mh.P_REFINE) - mh.P_REFINE
    assert n_new * mh.F_REST_WORDS > cap_words                                      # growth: COPY into the appended rows strides
    assert n_dead * 3 < cap_words and n_new * 3 < cap_words                         # VALUE rows (1 and 3 words) cannot at this P
    # ... so the VALUE role has a relocation of its own, on narrow tensors: 3-word rows, more than cap_words / 3 draws
    assert mh.N_VALUE * 3 > cap_words > (mh.N_VALUE - 500) * 3 and mh.N_VALUE < mh.P_VALUE
    par, dead, src, new_o, new_s = mh.relocate_case_large()
    assert dead.numel() == src.numel() == mh.N_VALUE and bool((dead[1:] > dead[:-1]).all())
    is_dead = torch.zeros(mh.P_VALUE, dtype=torch.bool)
    is_dead[dead] = True
    assert not bool(is_dead[src].any())                                             # no source is a dead row
    order = src.argsort()
    same = src[order][1:] == src[order][:-1]
    assert int(same.sum()) > mh.N_VALUE // 2                                        # most sources are drawn several times ...
    assert torch.equal(new_s[order][1:][same], new_s[order][:-1][same]) and torch.equal(new_o[order][1:][same], new_o[order][:-1][same])


def test_mcmc_sample_case_reaches_long_and_empty_runs():
    """mcmc_scan_kernel: thread t owns blocks [t * run, (t + 1) * run) with run = ceil(nb / MC_BLOCK)."""
    P = dh.PC
    nb = _blocks(P, K["MC_BLOCK"])
    run = _blocks(nb, K["MC_BLOCK"])
    assert run == 17 and (K["MC_BLOCK"] - 1) * run > nb > (K["MC_BLOCK"] - 16) * run  # the last threads' runs are empty
    assert nb % run != 0                                                              # one thread's run is cut short
    opacity, mask, u = mh.large_sample_case(P)
    want = mh.sample_int(opacity, u, 0.005, mask, mh.N_LARGE_DRAWS)
    n_dead, n_alive, n_draws, total = want["record"]
    dead = want["dead_idx"]
    assert 0.04 * P < n_dead < 0.05 * P and n_draws == mh.N_LARGE_DRAWS and total > 2 ** 32
    per_block = np.bincount(dead // K["CMP_ROWS"], minlength=_blocks(P, K["CMP_ROWS"]))
    assert (per_block > 0).all()                                                      # dead rows in every compaction block
    assert int((dead >= dh.SCAN_EDGE).sum()) > 20 and dead[-1] == P - 1               # ... beyond block 1024, the last row too
    src = want["src"]
    assert int((src >= dh.SCAN_EDGE).sum()) > 10 and int((src < dh.SCAN_EDGE).sum()) > 10
    assert src[1] == P - 2 and src[0] == int(np.flatnonzero(mask & (opacity > np.float32(0.005)))[0])
    assert int(want["ratio"].max()) >= 2


def test_loss_shape_has_more_slots_than_threads():
    planes, H, W = LH.LARGE_SHAPE
    slots = planes * _blocks(H, K["LT_H"]) * _blocks(W, K["LT_W"])
    assert slots == 300 > K["LTHREADS"] and slots % K["LTHREADS"] != 0 and H % K["LT_H"] == 1 and W % K["LT_W"] == 1
    assert max(int(np.prod(s[:-2])) * _blocks(s[-2], K["LT_H"]) * _blocks(s[-1], K["LT_W"]) for s in LH.SHAPES.values()) <= 18
    for variant in ("tex", "flat"):
        c = LH.large_case(variant)
        gmax = float(np.abs(c["grad"]).max())
        print(f"  {variant}: float32 vs float64: " + "  ".join(f"{k} {c['ref_error'][k] / (gmax if k == 'grad' else 1):.1e}"
                                                                for k in ("loss", "l1", "ssim", "grad")) + "  [grad: of its maximum]")
        # the float32 evaluation errs as the reference does on the fixture (tests/test_cpu_loss.py: at most 2e-4 / 1e-5)
        assert c["ref_error"]["grad"] <= 2e-4 * gmax and c["ref_error"]["loss"] <= 1e-5
        closed = LH.closed_form_grad64(c["x"], c["y"], *LH.weights()[:2])
        assert np.abs(closed - c["grad"]).max() <= 1e-10 * gmax


@pytest.mark.parametrize("case", LH.CASES)
def test_float32_evaluation_reproduces_the_reference_fixture(case):
    """loss_helpers.loss_and_grad32 stands in for the reference's own float32 result where the fixture holds none.  It is the
    same formula in the same precision, not the same program, so its bits differ from the fixture's; what the bar takes from
    it is its distance from float64.  On every fixture case each of the two float32 results lies within the bar the OTHER one
    gives (2 x the other's error, or the floor): the stand-in would pass the GPU test as the kernels must, and the fixture
    would pass under the stand-in's bar.  No number beyond fixture_bar's own formula enters.  Measured: the stand-in's
    gradient error is 0.67 .. 1.47 of the reference's over the twelve cases."""
    fx, e = LH.fixture(), LH.expectation(case)
    ref, mine = LH.reference_error(case), LH.float32_error(fx[f"{case}/x"], fx[f"{case}/y"], e)
    bar_ref, bar_mine = LH.fixture_bar(case), LH.bar_of_error(mine, e)
    assert bar_ref == LH.bar_of_error(ref, e)  # bar_of_error is fixture_bar's formula
    for k in ("loss", "l1", "ssim", "grad"):
        assert mine[k] <= bar_ref[k] and ref[k] <= bar_mine[k], (case, k, mine[k], ref[k])


def test_tensor_count_cases_take_two_and_three_chunks():
    assert dh.TENSOR_COUNTS == (K["PY_CHUNK"] + 1, 2 * K["PY_CHUNK"] + 1)
    assert _blocks(dh.P_COUNTS, K["CMP_ROWS"]) == 2
    for count in dh.TENSOR_COUNTS:
        ts, ex, n = dh.count_case(count)
        assert len(ts) == len(ex) == count and {1, 3, 4, 12, 16, 20, 180} <= {t.shape[1] for t in ts}
        assert any(e is None for e in ex) and any(e is not None for e in ex)
