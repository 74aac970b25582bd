"""-m gpu: the row-surgery and policy kernels ABOVE their one-chunk sizes -- the carry loop, per-thread run or grid stride
each of them enters only beyond a block-table threshold that the rest of the suite stays under.  Every comparison is with a
plain reference that knows nothing of blocks (torch boolean indexing and torch.cat on the CPU, the restatements of
tests/densify_helpers.py, tests/mcmc_helpers.py and tests/loss_helpers.py), bit for bit everywhere but the loss.
tests/test_cpu_size_regimes.py parses the thresholds out of the sources and checks that every size used here lies beyond
them, and that the cases are not degenerate.

    kernel, second regime                                          threshold            size used here
 1  compact_scan_kernel: carry across trips of 1024 blocks         P > 1 048 576        PC = 1 049 601 (1026 blocks), 1 048 576, 1 048 577
    its consumers compact_apply_kernel, densify_split_kernel,
    the MCMC iota source (dead_idx), gsr_view_message_plan / _pack                      PC
 2  append_rows_kernel: grid stride beyond 4096 x 256 x 64 B       > 67 108 864 B       (400 001 + 12 345) rows of 180 B = 74 222 280 B
 3  densify_grad_kernel / densify_hist_kernel: stride, LDS
    histograms filled over several trips                           P > 262 144          PD = 262 401 and PC; statistics with 8 views at PD
 4  mcmc_scan_kernel: run = ceil(nb / 256) blocks per thread       run > 2, empty runs  PC: nb = 4101, run = 17, threads 242 .. 255 empty
 5  mcmc_scatter_kernel: grid stride beyond 4096 x 256 words       n * words > 1 048 576  45-word f_rest rows, about 25 700 and 30 000 draws
 6  loss_finish_kernel: for (i = tid; i < n; i += 256)             > 256 slots          3 x 145 x 577: 300 slots
 7  densify.py compact_rows / append_rows: chunks of 32 tensors,
    blockIdx.y groups of 8                                         > 32 tensors         33 and 65 tensors at P = 1025
 8  compact_apply_kernel byte path, append_rows_kernel unaligned
    paths with 4-byte rows                                         pointer & 3, & 15    offsets 1, 2, 4, 8, 12 (Python glue and C ABI)

Measured on the MI355X, seconds per test (setup of the module's tensor set at PC: 0.44):
    compaction at PC: random 0.10, tail_only 0.01, head_kept 0.11, last_row < 0.005; at 1 048 576 / 1 048 577: 0.05 each
    split_positions 0.20    MCMC sampling 0.41    view-message plan 0.16    select at PD 0.32, at PC 0.56    statistics V = 8 0.63
    append 0.14    refine at 300 000 rows 2.26    relocate with 350 001 draws 0.04    loss tex 0.52, flat 0.52
    33 / 65 tensors 0.01 each    misaligned sources (Python) < 0.005    C ABI, per destination offset 0.01 or less
The file runs in 8.6 s.  Every test passed on the shipped kernels: no second regime computes anything but what its
reference does.  In the loss the product lands at 0.14 (tex) and 0.05 (flat) of the gradient's bar.

The tests do fail on wrong values: against a build in which compact_scan_kernel drops its carry, mcmc_scan_kernel caps its
run at 2 and append_rows_kernel, densify_grad_kernel / densify_hist_kernel, mcmc_scatter_kernel and loss_finish_kernel take one
trip only, the tests of regimes 1 to 6 failed -- all but `tail_only`, `last_row` and P = 1 048 576, which need no carry and
are there to say so -- with the first wrong row or block in the message (view messages: block 1024, offset 0 instead of
10 567), and the append of the 33 / 65-tensor cases with them (its 180-byte rows take four trips); the eight-view
statistics and the alignment tests, whose code that build left alone, passed.
"""
import ctypes

import numpy as np
import pytest
import torch

import densify_helpers as dh
import loss_helpers as LH
import mcmc_helpers as mh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGE = dh.SCAN_EDGE
PC, PD = dh.PC, dh.PD


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def _same(got, want, tag):
    """bit equality of a device tensor with a CPU tensor (bytes compared: a NaN or a -0 must not pass for its neighbour)"""
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, got.shape, want.dtype, want.shape)
    if got.numel() == 0:
        return
    a, b = got.contiguous().view(torch.uint8).reshape(-1), want.contiguous().view(torch.uint8).reshape(-1)
    if not torch.equal(a, b):
        row_bytes = max(1, a.numel() // got.shape[0])
        first = int((a != b).nonzero()[0]) // row_bytes
        raise AssertionError(f"{tag}: first wrong row {first} of {got.shape[0]} (1024-row block {first // 1024}), "
                             f"{int((a != b).sum())} bytes differ")


# ----------------------------------------------------------------------------------------------------------------------
# 1. compaction beyond one trip of the scan
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_rows():
    """The tensor set at PC, on the CPU and on the device, built once and freed after the module."""
    cpu = dh.compact_tensors(PC)
    out = dict(cpu=cpu, dev=[t.to(DEV) for t in cpu], masks=dh.compact_masks(PC))
    yield out
    out.clear()
    torch.cuda.empty_cache()


def _compact_and_compare(big_rows, P, keep, tag):
    from gaussianeditor_amd.densify import compact_rows

    outs = compact_rows([t[:P] for t in big_rows["dev"]], keep.to(DEV))
    torch.cuda.synchronize()
    assert len(outs) == len(big_rows["cpu"]) > 8
    for i, (o, t) in enumerate(zip(outs, big_rows["cpu"])):
        _same(o, t[:P][keep], f"{tag}, tensor {i} {tuple(t.shape[1:])} {t.dtype}")


@pytest.mark.parametrize("mask", ("random", "tail_only", "head_kept", "last_row"))
def test_compaction_beyond_one_scan_trip(big_rows, mask):
    """compact_scan_kernel (gsr_compact.hip), `for (base = 0; base < nb; base += 1024)` with `carry`: a second trip starts
    above 1024 blocks of CMP_ROWS = 1024 rows, P > 1 048 576.  Here P = PC = 1 049 601: 1026 row blocks, the second trip
    holds two, the last with one row.  compact_apply_kernel runs two blockIdx.y groups (11 tensors; rows of 1, 2, 3, 4, 8,
    12, 16, 20 and 180 bytes: its three branches).  compact_rows against t[keep] on the CPU, bit for bit.  The structured
    masks tell a lost or doubled carry apart: `tail_only` needs carry 0 (the output comes from the second trip alone),
    `head_kept` carry 1 048 576, `last_row` one survivor in the one-row block."""
    _compact_and_compare(big_rows, PC, big_rows["masks"][mask], f"PC, mask {mask}")


@pytest.mark.parametrize("P", (EDGE, EDGE + 1))
def test_compaction_at_the_edge_of_one_scan_trip(big_rows, P):
    """compact_scan_kernel at P = 1 048 576 (exactly 1024 blocks: the last size of one trip) and 1 048 577 (a second trip for
    one block of one row), random mask, the tensor set of the test above cut to P rows."""
    _compact_and_compare(big_rows, P, big_rows["masks"]["random"][:P], f"P = {P}, random mask")


# ----------------------------------------------------------------------------------------------------------------------
# 2. the consumers of the plan
# ----------------------------------------------------------------------------------------------------------------------
def test_split_positions_beyond_one_scan_trip():
    """densify_split_kernel reads block_off[blockIdx.x] of the plan compact_scan_kernel wrote; blocks 1024 and 1025 get theirs
    from the second trip (P > 1 048 576).  P = PC, N = 2, selected rows 0, 1 048 575, 1 048 576, PC - 1 and 300 random ones:
    bit equality with split_np and test_split_positions' split_bound check against float64."""
    from gaussianeditor_amd.densify import split_positions

    N = 2
    xyz, scaling, rot, sel, noise = dh.split_case_large(PC, N=N)
    want, l1, pxyz = dh.split_np(xyz, scaling, rot, sel, noise, N)
    got = split_positions(_dev(xyz), _dev(scaling), _dev(rot), _dev(sel), _dev(noise), N).cpu().numpy()
    n_split = int(sel.sum())
    assert got.shape == (N * n_split, 3)
    bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
    assert bad.size == 0, f"first wrong child {bad[0]}: parent row {np.flatnonzero(sel)[bad[0] % n_split]}"
    ref64, _, _ = dh.split_np(xyz, scaling, rot, sel, noise, N, dtype=np.float64)
    ratio = np.abs(got.astype(np.float64) - ref64) / dh.split_bound(l1, pxyz)
    print(f"split_xyz at PC, n_split={n_split}: max |error| / bound = {ratio.max():.4f}")
    assert (ratio <= 1.0).all(), float(ratio.max())


def test_mcmc_sampling_beyond_one_scan_trip_and_with_long_runs():
    """mcmc_scan_kernel (gsr_mcmc.hip): run = ceil(nb / 256) blocks of MC_BLOCK = 256 rows per thread; the suite reaches
    run = 2.  P = PC: nb = 4101, run = 17, threads 242 .. 255 have empty runs (lo == hi == nb).  The dead rows (about 4.5 %,
    in every 1024-row block, rows 1 048 575, 1 048 576 and PC - 1 among them) come out of compact_scan_kernel's second
    trip through the iota source of compact_apply_kernel.  n = 30 000 draws: dead_sel, dead_idx, src, count, ratio and the
    record against mcmc_helpers.sample_int, bit for bit; a second call gives the same bits."""
    import test_gpu_mcmc as tm

    opacity, mask, u = mh.large_sample_case(PC)
    want = mh.sample_int(opacity, u, tm.MIN_OPACITY, mask, mh.N_LARGE_DRAWS)
    got = tm._run_sample(opacity, u, mask, mh.N_LARGE_DRAWS)
    tm._assert_sample_equal(got, want)
    assert int((got["dead_idx"] >= EDGE).sum()) > 20 and got["dead_idx"][-1] == PC - 1 and got["src"][1] == PC - 2
    tm._assert_sample_equal(tm._run_sample(opacity, u, mask, mh.N_LARGE_DRAWS), got)


def test_view_message_plan_beyond_one_scan_trip():
    """gsr_view_message_plan / gsr_view_message_pack (compact_scan_kernel's block_off travels in the message; the suite
    reaches P = 20 000).  P = PC, synthetic dense gradients with about 1 % touched rows, the last rows of the last three
    blocks among them: the mask, the count, the block offsets against torch.searchsorted, the row numbers and every packed
    segment; then gsr_view_messages_accumulate of that one message into NaN-filled dense targets returns the inputs."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    P = PC
    grads_cpu, rgb_cpu, touched = dh.message_case_large(P)
    grads5, rgb = [g.to(DEV) for g in grads_cpu], rgb_cpu.to(DEV)
    plan, count = _C.view_message_plan(grads5, rgb)
    _same(plan[0].bool(), touched, "touched-row mask")
    want = touched.nonzero().view(-1)
    assert count == int(want.numel())
    cap = count + 5
    words, nb = _C.view_message_words(P, cap), (P + 1023) // 1024
    assert words == 4 + nb + 18 * cap and nb == 1026
    campos = torch.tensor([0.25, -1.5, 3.0], device=DEV)
    messages = torch.full((1, words + 7), float("nan"), device=DEV)[:, :words]
    _C.view_message_pack(plan, grads5, rgb, campos, cap, messages[0])
    msg = messages[0].cpu()
    assert torch.equal(msg[:3], campos.cpu()) and int(msg.view(torch.int32)[3]) == count
    boff = msg.view(torch.int32)[4:4 + nb].long()
    want_off = torch.searchsorted(want, torch.arange(nb) * 1024)
    wrong = (boff != want_off).nonzero()
    assert wrong.numel() == 0, f"first wrong block offset: block {int(wrong[0])}: {int(boff[wrong[0]])} != {int(want_off[wrong[0]])}"
    off = 4 + nb
    assert torch.equal(msg.view(torch.int32)[off:off + count].long(), want)
    off += cap
    for name, k, src in zip(("means3D", "scales", "rotations", "means2D", "opacities", "rgb"), (3, 3, 4, 3, 1, 3), grads_cpu + [rgb_cpu]):
        _same(msg[off:off + k * cap].view(cap, k)[:count], src[want], name)
        off += k * cap
    dense = [torch.full((P, k), float("nan"), device=DEV) for k in (3, 3, 4, 3, 1)] + [None]
    _C.view_messages_accumulate(messages, P, cap, 3, 16, grads5[0], dense)
    for name, got, src in zip(("means3D", "scales", "rotations", "means2D", "opacities"), dense[:5], grads_cpu):
        _same(got, src, f"accumulated {name}")


# ----------------------------------------------------------------------------------------------------------------------
# 3. densify selection and statistics beyond one trip of the grid
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (PD, PC))
def test_select_beyond_one_grid_trip(P):
    """densify_grad_kernel / densify_hist_kernel (gsr_densify.hip): the grid is capped at DNS_MAX_BLOCKS = 1024 blocks of 256
    rows and strides beyond, so above P = 262 144 a block's LDS histogram is filled over more than one trip (the suite
    reaches 70 001).  PD = 262 401 and PC = 1 049 601 (there the plans of both selections also take compact_scan_kernel's
    second trip): every densify_helpers.KINDS x PERCENTS cell through the body of test_select_equals_the_reference_lines,
    its assertions unchanged."""
    import test_gpu_densify_policy as tdp

    tdp.test_select_equals_the_reference_lines(P)


def test_stats_with_eight_views_at_PD():
    """densify_stats_kernel with V = 8 views (the suite stops at 3) at PD = 262 401 rows: the body of
    test_stats_bit_equal_and_invisible_rows_untouched."""
    import test_gpu_densify_policy as tdp

    tdp.test_stats_bit_equal_and_invisible_rows_untouched(PD, 8)


# ----------------------------------------------------------------------------------------------------------------------
# 4. append beyond the grid cap
# ----------------------------------------------------------------------------------------------------------------------
def test_append_rows_beyond_the_grid_cap():
    """append_rows_kernel (gsr_compact.hip): the grid is capped at 4096 blocks of 256 threads x 64 bytes and strides beyond,
    i.e. for a tensor above 67 108 864 bytes (the suite reaches about 20 MB).  P = 400 001, n = 12 345: the (P, 15, 3)
    float32 tensor is 74 222 280 bytes with its extension, once with `ext` given and once with None (zero rows); two narrow
    tensors ride in the same launch.  Against torch.cat on the CPU, bit for bit."""
    from gaussianeditor_amd.densify import append_rows

    P, n = dh.P_APPEND, dh.N_APPEND
    g = torch.Generator().manual_seed(41)
    big, big_ext = torch.randn(P, 15, 3, generator=g), torch.randn(n, 15, 3, generator=g)
    xyz, xyz_ext = torch.randn(P, 3, generator=g), torch.randn(n, 3, generator=g)
    flags = torch.randint(0, 255, (P,), generator=g, dtype=torch.uint8)
    ts, ex = [big, big, xyz, flags], [big_ext, None, xyz_ext, None]
    outs = append_rows([t.to(DEV) for t in ts], [None if e is None else e.to(DEV) for e in ex], n=n)
    torch.cuda.synchronize()
    for i, (o, t, e) in enumerate(zip(outs, ts, ex)):
        e = torch.zeros((n,) + tuple(t.shape[1:]), dtype=t.dtype) if e is None else e
        _same(o, torch.cat((t, e)), f"append tensor {i}")


# ----------------------------------------------------------------------------------------------------------------------
# 5. MCMC relocation and growth beyond the scatter's grid cap
# ----------------------------------------------------------------------------------------------------------------------
def test_refine_beyond_the_scatter_grid_cap():
    """mcmc_scatter_kernel (gsr_mcmc.hip): the grid is capped at 4096 blocks of 256 words and strides beyond, i.e. for
    n * words > 1 048 576 (the suite reaches about 3 500 draws).  One mcmc_refine round at P = 300 000 against
    mcmc_refine_torch under the comparison rules of test_two_refines_equal_the_torch_restatement: every 7th row dead, 60 % of
    the rows inside the mask -> about 25 700 relocations, and grow = 1.1 -> 30 000 appended rows.  f_rest keeps its full
    width of 45 words (the torch restatement runs on the device and takes well under a second), so it strides as a COPY of the
    relocation, as a ZERO of the sources' moments and as a COPY of the growth.  The VALUE role carries rows of 1 and 3 words
    and strides only above 349 525 draws: the next test."""
    import test_gpu_mcmc as tm
    from gaussianeditor_amd.mcmc import mcmc_refine

    P, cap = mh.P_REFINE, int(mh.GROW_REFINE * mh.P_REFINE) + 1000
    opt = tm._optimizer(tm._scene_par(P, 13, dead_every=mh.DEAD_EVERY))
    g = torch.Generator(device=DEV).manual_seed(9)
    extra = dict(xyz_gradient_accum=torch.rand((P, 1), device=DEV, generator=g), denom=torch.ones((P, 1), device=DEV),
                 max_radii2D=torch.rand(P, device=DEV, generator=g), mask=mh.refine_mask_large(P).to(DEV),
                 generation=torch.zeros(P, dtype=torch.int64, device=DEV))
    par, mom = tm._state(opt)
    before_par = {k: v.clone() for k, v in par.items()}
    before_mom = {k: (a.clone(), b.clone()) for k, (a, b) in mom.items()}
    kw = dict(cap_max=cap, min_opacity=tm.MIN_OPACITY, grow=mh.GROW_REFINE, generation_num=1)
    want_par, want_mom, want_extra, want_counts, touched = mh.mcmc_refine_torch(
        par, mom, extra, generator=torch.Generator(device=DEV).manual_seed(77), **kw)
    new_par, extra, counts = mcmc_refine(opt, extra, generator=torch.Generator(device=DEV).manual_seed(77), **kw)
    print(f"mcmc_refine at P = {P}: (P, n_dead, n_relocated, n_added) = {counts}")
    n_new = int(mh.GROW_REFINE * P) - P
    assert counts == want_counts and counts[0] == P and counts[2] == counts[1] and counts[3] == n_new
    assert counts[1] * mh.F_REST_WORDS > 4096 * 256 and n_new * mh.F_REST_WORDS > 4096 * 256  # both scatters stride
    final = P + n_new
    dead, src_r, src_g = touched["dead"], touched["src_relocate"], touched["src_grow"]
    assert bool(extra["mask"][:P][dead].all()) and bool(extra["mask"][:P][src_r].all())
    rows = torch.zeros(final, dtype=torch.bool, device=DEV)  # rows whose opacity / scaling were computed
    rows[dead] = rows[src_r] = rows[src_g] = True
    rows[P:] = True
    for k in mh.NAMES:
        p = opt.param_groups[mh.NAMES.index(k)]["params"][0]
        assert p is new_par[k] and p.requires_grad and p.shape == want_par[k].shape and p.shape[0] == final
        got = p.detach()
        if k in ("opacity", "scaling"):
            assert torch.equal(got[~rows], want_par[k][~rows]) and torch.equal(got[:P][~rows[:P]], before_par[k][~rows[:P]]), k
            assert tm._within_one_ulp(tm._np(got[rows]), tm._np(want_par[k][rows]).astype(np.float64)) <= 1.0, k
            assert torch.equal(got[P:], got[src_g]), k
        else:
            if not torch.equal(got, want_par[k]):
                wrong = (got != want_par[k]).reshape(final, -1).any(dim=1).nonzero()
                raise AssertionError(f"{k}: {wrong.numel()} wrong rows, the first {int(wrong[0])}")
            assert torch.equal(got[dead], before_par[k][src_r]) and torch.equal(got[P:], got[src_g]), k
        st = opt.state[p]
        for got_m, want_m, was in zip((st["exp_avg"], st["exp_avg_sq"]), want_mom[k], before_mom[k]):
            if not torch.equal(got_m, want_m):
                wrong = (got_m != want_m).reshape(final, -1).any(dim=1).nonzero()
                raise AssertionError(f"moments of {k}: {wrong.numel()} wrong rows, the first {int(wrong[0])}")
            assert not bool(got_m[src_r].any()) and not bool(got_m[P:].any()), k
            assert torch.equal(got_m[dead], was[dead]) and bool(was[dead].any()), k
    assert extra["mask"].dtype == torch.bool and torch.equal(extra["mask"], want_extra["mask"])
    assert torch.equal(extra["mask"][P:], extra["mask"][src_g])
    assert torch.equal(extra["generation"], want_extra["generation"]) and int((extra["generation"] == 1).sum()) == n_new
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(extra[k], want_extra[k]) and extra[k].shape[0] == final and not bool(extra[k][P:].any()), k


def test_relocate_values_beyond_the_scatter_grid_cap():
    """mcmc_scatter_kernel<GSR_MCMC_VALUE>: dst[d] = base[s] = values[r] strides for n * words > 1 048 576, with the 3-word
    scaling rows above 349 525 draws.  `relocate` of n = 350 001 dead rows out of P = 400 000 on three narrow groups (xyz:
    COPY, opacity and scaling: VALUE, their moments: ZERO; 1 050 003 words for the 3-word rows) against masked assignment in
    torch on the CPU, bit for bit.  The sources are drawn among 49 999 rows, so most are drawn several times."""
    from gaussianeditor_amd.mcmc import relocate

    par_cpu, dead, src, new_o, new_s = mh.relocate_case_large()
    P, n = mh.P_VALUE, mh.N_VALUE
    assert n * 3 > 4096 * 256 and int(dead.numel()) == n
    names = ("xyz", "opacity", "scaling")
    par = {k: torch.nn.Parameter(par_cpu[k].to(DEV)) for k in names}
    opt = torch.optim.Adam([dict(params=[par[k]], lr=1e-4, name=k) for k in names], lr=0.0, eps=1e-15)
    g = torch.Generator(device=DEV).manual_seed(3)
    for _ in range(2):  # non-zero moments
        for p in par.values():
            p.grad = torch.randn(p.shape, device=DEV, generator=g) * 1e-3
        opt.step()
    opt.zero_grad(set_to_none=True)
    before = {k: par[k].detach().cpu().clone() for k in names}
    mom = {k: (opt.state[par[k]]["exp_avg"].cpu().clone(), opt.state[par[k]]["exp_avg_sq"].cpu().clone()) for k in names}
    relocate(opt, dead.int().to(DEV), src.int().to(DEV), new_o.to(DEV), new_s.to(DEV))
    torch.cuda.synchronize()
    for k in names:
        want = before[k].clone()
        want[dead] = before[k][src]
        if k != "xyz":
            v = new_o if k == "opacity" else new_s
            want[dead] = v
            want[src] = v
        _same(par[k].detach(), want, k)
        for got_m, was, tag in zip((opt.state[par[k]]["exp_avg"], opt.state[par[k]]["exp_avg_sq"]), mom[k], ("exp_avg", "exp_avg_sq")):
            want_m = was.clone()
            want_m[src] = 0
            assert bool(was[src].ne(0).any())
            _same(got_m, want_m, f"{k}.{tag}")


# ----------------------------------------------------------------------------------------------------------------------
# 6. the loss's final sum over more slots than threads
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ("tex", "flat"))
def test_loss_with_more_slots_than_threads(variant):
    """loss_finish_kernel (loss/gsr_loss.hip): `for (i = tid; i < n; i += 256)` over the workgroups' slots takes a second
    trip above 256 slots = planes x ceil(H / 16) x ceil(W / 64) (the suite reaches 18).  Shape (3, 145, 577): 3 x 10 x 10 =
    300 slots, one ragged row and one ragged column of tiles.  Forward terms and gradient against float64
    (loss_helpers.loss_and_grad64) under the bars of test_loss_terms_and_gradient_against_float64 -- max(2 x the float32
    evaluation's own error against float64, 1e-6 absolute / 1e-6 of the gradient's largest entry); the fixture holds no
    arrays of this shape, so the float32 evaluation is loss_helpers.loss_and_grad32, which tests/test_cpu_size_regimes.py
    pins to the fixture.  Two runs give the same bits."""
    from gaussianeditor_amd.losses import photometric_loss

    c = LH.large_case(variant)
    runs = []
    for _ in range(2):
        x = torch.from_numpy(c["x"]).to(DEV).requires_grad_(True)
        loss, l1, ssim = photometric_loss(x, torch.from_numpy(c["y"]).to(DEV), lambda_dssim=LH.LAMBDA, return_terms=True)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().cpu().numpy(), l1.cpu().numpy(), ssim.cpu().numpy(), x.grad.cpu().numpy()))
    loss, l1, ssim, grad = runs[0]
    assert grad.shape == LH.LARGE_SHAPE and grad.dtype == np.float32
    gmax = float(np.abs(c["grad"]).max())
    err = dict(loss=abs(float(loss) - c["loss"]), l1=abs(float(l1) - c["l1"]), ssim=abs(float(ssim) - c["ssim"]),
               grad=float(np.abs(grad.astype(np.float64) - c["grad"]).max()))
    bar = c["bar"]
    print(f"  {variant}_145x577: " + "  ".join(f"{k} {err[k] / (gmax if k == 'grad' else 1.0):.1e} (bar {bar[k] / (gmax if k == 'grad' else 1.0):.1e})"
                                             for k in ("loss", "l1", "ssim", "grad")) + "  [grad: of its maximum]")
    for k in ("loss", "l1", "ssim", "grad"):
        assert err[k] <= bar[k], (variant, k, err[k], bar[k])
    for a, b in zip(*runs):
        assert np.array_equal(_bits(np.asarray(a, np.float32)), _bits(np.asarray(b, np.float32)))


# ----------------------------------------------------------------------------------------------------------------------
# 7. more tensors than one launch takes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", dh.TENSOR_COUNTS)
def test_more_tensors_than_one_launch_takes(count):
    """densify.py compact_rows / append_rows: Python chunks of 32 tensors (CMP_MAX_TENSORS), each launch with blockIdx.y
    groups of 8 (compaction) or one blockIdx.y per tensor (append); the suite reaches 18 tensors.  33 and 65 tensors at
    P = 1025 (two row blocks, the second with one row), rows of 1, 2, 3, 4, 8, 12, 16, 20 and 180 bytes in turn, every third
    extension None.  Against boolean indexing and torch.cat on the CPU, bit for bit."""
    from gaussianeditor_amd.densify import append_rows, compact_rows

    ts, ex, n = dh.count_case(count)
    P = dh.P_COUNTS
    keep = torch.rand(P, generator=torch.Generator().manual_seed(count)) < 0.5
    keep[P - 1] = True
    outs = compact_rows([t.to(DEV) for t in ts], keep.to(DEV))
    assert len(outs) == count
    for i, (o, t) in enumerate(zip(outs, ts)):
        _same(o, t[keep], f"compact_rows, tensor {i} of {count} ({t.shape[1]}-byte rows)")
    outs = append_rows([t.to(DEV) for t in ts], [None if e is None else e.to(DEV) for e in ex], n=n)
    assert len(outs) == count
    for i, (o, t, e) in enumerate(zip(outs, ts, ex)):
        e = torch.zeros((n, t.shape[1]), dtype=t.dtype) if e is None else e
        _same(o, torch.cat((t, e)), f"append_rows, tensor {i} of {count} ({t.shape[1]}-byte rows)")


# ----------------------------------------------------------------------------------------------------------------------
# 8. misaligned pointers with rows of a multiple of 4 bytes
# ----------------------------------------------------------------------------------------------------------------------
P_ALIGN, N_ALIGN = 2051, 37  # three row blocks, the last with three rows; odd, so that 4-byte rows end off 16-byte marks


def _offset_view(values, offset, dtype):
    """`values` (a CPU tensor) copied into a device byte buffer `offset` bytes behind its 256-byte aligned start, viewed as
    `dtype`: a contiguous tensor whose data_ptr() is off by `offset`."""
    raw = values.contiguous().view(torch.uint8).reshape(-1)
    buf = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    buf[offset:offset + raw.numel()] = raw.to(DEV)
    out = buf[offset:offset + raw.numel()].view(dtype).view(values.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == offset % 16
    return out


def _align_cases():
    """[(tag, CPU tensor, its extension, byte offset)]: 4-byte rows as (P, 4) uint8 at +1 and (P, 2) int16 at +2 (torch
    cannot view int16 on an odd address: that case goes through the C ABI below), float rows at +4, +8 and +12."""
    g = torch.Generator().manual_seed(5)
    P, n = P_ALIGN, N_ALIGN
    u8 = lambda r, k: torch.randint(0, 256, (r, k), generator=g, dtype=torch.uint8)  # noqa: E731
    i16 = lambda r, k: torch.randint(-30000, 30000, (r, k), generator=g, dtype=torch.int16)  # noqa: E731
    f32 = lambda r, k: torch.randn(r, k, generator=g)  # noqa: E731
    return [("(P,4) uint8 at +1", u8(P, 4), u8(n, 4), 1), ("(P,2) int16 at +2", i16(P, 2), i16(n, 2), 2),
            ("(P,3) float32 at +4", f32(P, 3), f32(n, 3), 4), ("(P,4) float32 at +8", f32(P, 4), f32(n, 4), 8),
            ("(P,45) float32 at +12", f32(P, 45), f32(n, 45), 12), ("(P,1) float32 at +4", f32(P, 1), f32(n, 1), 4)]


def test_misaligned_sources_through_the_python_entry_points():
    """compact_apply_kernel's byte path and append_rows_kernel's unaligned paths with rows of a multiple of 4 bytes on a
    pointer that is not (the suite reaches them only with rows of 1 and 3 bytes).  Reached through the PYTHON entry points:
    compact_rows and append_rows take a contiguous offset view as it is (`.contiguous()` makes no aligned copy), so the
    SOURCES and extensions are misaligned here -- by 1, 2, 4, 8 and 12 bytes; the destinations come from torch.empty and
    are aligned (the append's second part starts at dst + P * row_bytes, which is off the 16-byte marks for odd P).
    Misaligned destinations: the C ABI test below."""
    from gaussianeditor_amd.densify import append_rows, compact_rows

    cases = _align_cases()
    P, n = P_ALIGN, N_ALIGN
    keep = torch.rand(P, generator=torch.Generator().manual_seed(6)) < 0.5
    keep[[0, P - 1]] = True
    srcs = [_offset_view(t, off, t.dtype) for _, t, _, off in cases]
    exts = [_offset_view(e, off, e.dtype) for _, _, e, off in cases]
    for s, (tag, t, _, off) in zip(srcs, cases):
        assert s.data_ptr() % 16 == off and torch.equal(s.cpu(), t), tag
    for o, (tag, t, _, _) in zip(compact_rows(srcs, keep.to(DEV)), cases):
        _same(o, t[keep], "compact_rows " + tag)
    for o, (tag, t, e, _) in zip(append_rows(srcs, exts), cases):
        _same(o, torch.cat((t, e)), "append_rows " + tag)
    for o, (tag, t, _, _) in zip(append_rows(srcs, [None] * len(srcs), n=n), cases):
        _same(o, torch.cat((t, torch.zeros((n,) + tuple(t.shape[1:]), dtype=t.dtype))), "append_rows with zero rows " + tag)


@pytest.mark.parametrize("dst_off", (0, 1, 2, 4, 8, 12))
def test_misaligned_pointers_through_the_c_abi(dst_off):
    """The same paths reached through the C ABI (gsr_compact_plan / gsr_compact_apply / gsr_append_rows on raw pointers, as
    tests/helpers.py drives the debug exports), which the Python glue cannot reach: DESTINATIONS off by 1, 2, 4, 8 and 12
    bytes, and 4-byte rows ((P, 2) int16 in meaning) on an ODD source address.  Every destination is a
    guarded_alloc.GuardedAllocator buffer of exactly dst_off + the output's bytes: the back guard starts at the first byte
    behind the output, the dst_off bytes in front of it keep the poison.  Sources: 4-byte rows at +1, 12-byte rows at +4,
    16-byte rows at +8, 180-byte rows at +12, and an aligned 8-byte row (with dst_off != 0 the destination alone is off)."""
    from gaussianeditor_amd import _native
    from guarded_alloc import GuardedAllocator

    L = _native.lib()
    P, n, PAT = P_ALIGN, N_ALIGN, 0xA5
    g = torch.Generator().manual_seed(70 + dst_off)
    rows = [(4, 1), (12, 4), (16, 8), (180, 12), (8, 0)]  # (row bytes, source offset)
    src_cpu = [torch.randint(0, 256, (P, rb), generator=g, dtype=torch.uint8) for rb, _ in rows]
    ext_cpu = [torch.randint(0, 256, (n, rb), generator=g, dtype=torch.uint8) for rb, _ in rows]
    srcs = [_offset_view(t, off, torch.uint8) for t, (_, off) in zip(src_cpu, rows)]
    exts = [_offset_view(t, off, torch.uint8) for t, (_, off) in zip(ext_cpu, rows)]
    keep = torch.rand(P, generator=g) < 0.5
    keep[[0, P - 1]] = True
    k8 = keep.to(DEV).view(torch.uint8)
    s = torch.cuda.current_stream().cuda_stream
    nbytes = ctypes.c_size_t(0)
    _native.check("gsr_compact_workspace_size", L.gsr_compact_workspace_size(P, ctypes.byref(nbytes)))
    work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=DEV)
    kept = ctypes.c_int64(0)
    _native.check("gsr_compact_plan", L.gsr_compact_plan(s, P, k8.data_ptr(), work.data_ptr(), ctypes.byref(kept)))
    m = int(kept.value)
    assert m == int(keep.sum())
    with GuardedAllocator(PAT, device=DEV) as ga:
        cdst = [torch.empty(dst_off + m * rb, dtype=torch.uint8, device=DEV) for rb, _ in rows]
        adst = [torch.empty(dst_off + (P + n) * rb, dtype=torch.uint8, device=DEV) for rb, _ in rows]
        zdst = [torch.empty(dst_off + (P + n) * rb, dtype=torch.uint8, device=DEV) for rb, _ in rows]
    assert len(ga) == 3 * len(rows) and all(d.data_ptr() % 256 == 0 for d in cdst + adst + zdst)
    carr = (_native.CompactTensor * len(rows))()
    aarr = (_native.AppendTensor * len(rows))()
    zarr = (_native.AppendTensor * len(rows))()
    for i, (rb, _) in enumerate(rows):
        carr[i] = _native.CompactTensor(srcs[i].data_ptr(), cdst[i].data_ptr() + dst_off, rb)
        aarr[i] = _native.AppendTensor(srcs[i].data_ptr(), exts[i].data_ptr(), adst[i].data_ptr() + dst_off, rb)
        zarr[i] = _native.AppendTensor(srcs[i].data_ptr(), None, zdst[i].data_ptr() + dst_off, rb)
    _native.check("gsr_compact_apply", L.gsr_compact_apply(s, P, k8.data_ptr(), work.data_ptr(), len(rows), carr))
    _native.check("gsr_append_rows", L.gsr_append_rows(s, P, n, len(rows), aarr))
    _native.check("gsr_append_rows", L.gsr_append_rows(s, P, n, len(rows), zarr))
    ga.assert_clean()
    for i, (rb, off) in enumerate(rows):
        tag = f"{rb}-byte rows, source at +{off}, destination at +{dst_off}"
        for d in (cdst[i], adst[i], zdst[i]):
            assert bool((d[:dst_off] == PAT).all()), "bytes in front of the destination were written: " + tag
        _same(cdst[i][dst_off:].view(m, rb), src_cpu[i][keep], "gsr_compact_apply " + tag)
        _same(adst[i][dst_off:].view(P + n, rb), torch.cat((src_cpu[i], ext_cpu[i])), "gsr_append_rows " + tag)
        _same(zdst[i][dst_off:].view(P + n, rb), torch.cat((src_cpu[i], torch.zeros(n, rb, dtype=torch.uint8))),
              "gsr_append_rows with zero rows " + tag)
