"""-m gpu: Mip-Splatting's 3D filter (gaussianeditor_amd/filter3d.py, csrc/gsr_filter3d.hip) against
the restatements of tests/filter3d_helpers.py.

The sweep is held BIT FOR BIT -- filter_3D and the valid mask -- to the numpy binary64 restatement: add, multiply, divide,
compare and min in binary64 without contraction are exact IEEE operations on both sides, and the one rounding to binary32
is the same rounding.  Cases: P in {1, 63, 64, 65, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK, ROWS_PER_BLOCK + 1, 1000, 100003} x
V in {1, 2, C - 1, C, C + 1, 2 C + 1}, C = CAMERAS_PER_CHUNK (the largest P with V in {1, C + 1}), general cameras; the
float32 neighbours of every threshold; a row seen by exactly one camera, at the first and at the last position of a chunk;
all rows unseen; one row seen out of 100003, in the last block.

The apply is held to float64 torch operators with autograd under the project's rule for fused stages: per case and per
quantity max(2 x the error of the SAME torch operators run in float32 against float64, 1e-6 of the tensor's largest entry).
The kernels compute in binary64 from the binary32 inputs and round once, so what is measured is the output rounding.
Measured on the MI355X (error / bar; every case prints its own figures):

    apply: error / bar (the last column: rows whose cross term exceeds ten bars)
    | case | s_eff | o_eff | d_scales | d_opacity | d_scales from o_eff alone | rows |
    |---|---|---|---|---|---|---|
    | P=1 activated | 3.0e-09 / 6.5e-08 | 2.1e-09 / 2.2e-07 | 3.9e-07 / 9.5e-06 | 8.4e-09 / 4.1e-07 | 4.7e-07 / 9.5e-06 | 1 |
    | P=1 raw | 3.8e-11 / 1.3e-09 | 1.4e-09 / 5.7e-08 | 7.2e-10 / 1.8e-08 | 9.6e-10 / 4.2e-08 | 5.4e-10 / 1.8e-08 | 1 |
    | P=63 activated | 3.5e-08 / 1.0e-06 | 2.8e-08 / 9.4e-07 | 4.8e-05 / 1.5e-03 | 4.5e-08 / 2.0e-06 | 2.0e-05 / 1.5e-03 | 49 |
    | P=63 raw | 3.5e-08 / 1.0e-06 | 3.0e-08 / 1.0e-06 | 4.8e-08 / 2.5e-06 | 6.5e-09 / 2.8e-07 | 9.4e-09 / 2.5e-06 | 51 |
    | P=64 activated | 3.5e-08 / 1.0e-06 | 2.9e-08 / 9.4e-07 | 1.0e-04 / 2.4e-03 | 5.7e-08 / 2.5e-06 | 1.1e-04 / 2.4e-03 | 49 |
    | P=64 raw | 3.5e-08 / 1.0e-06 | 2.9e-08 / 1.0e-06 | 3.5e-08 / 3.2e-06 | 5.2e-09 / 2.1e-07 | 2.9e-08 / 3.2e-06 | 48 |
    | P=65 activated | 3.5e-08 / 1.0e-06 | 2.8e-08 / 9.4e-07 | 5.6e-05 / 1.4e-03 | 1.1e-07 / 2.8e-06 | 5.7e-05 / 1.4e-03 | 50 |
    | P=65 raw | 3.5e-08 / 1.0e-06 | 2.8e-08 / 1.0e-06 | 4.0e-08 / 1.7e-06 | 4.4e-09 / 1.7e-07 | 1.1e-08 / 1.7e-06 | 51 |
    | P=255 activated | 3.5e-08 / 1.0e-06 | 2.9e-08 / 9.7e-07 | 3.0e-05 / 9.5e-04 | 7.2e-08 / 2.4e-06 | 2.0e-05 / 9.5e-04 | 203 |
    | P=255 raw | 3.5e-08 / 1.0e-06 | 3.0e-08 / 1.0e-06 | 5.5e-08 / 1.9e-06 | 1.3e-08 / 5.0e-07 | 2.1e-08 / 1.9e-06 | 208 |
    | P=256 activated | 3.5e-08 / 1.0e-06 | 3.0e-08 / 9.8e-07 | 1.0e-04 / 2.1e-03 | 1.1e-07 / 3.0e-06 | 1.2e-04 / 2.1e-03 | 196 |
    | P=256 raw | 4.7e-08 / 1.0e-06 | 2.9e-08 / 1.0e-06 | 5.8e-08 / 3.4e-06 | 1.4e-08 / 4.3e-07 | 1.3e-08 / 3.4e-06 | 200 |
    | P=257 activated | 5.7e-08 / 1.0e-06 | 2.9e-08 / 9.9e-07 | 7.6e-05 / 2.6e-03 | 1.1e-07 / 2.5e-06 | 6.7e-05 / 2.6e-03 | 205 |
    | P=257 raw | 3.5e-08 / 1.0e-06 | 2.9e-08 / 1.0e-06 | 1.2e-07 / 2.6e-06 | 1.3e-08 / 3.5e-07 | 1.4e-08 / 2.6e-06 | 200 |
    | P=1000 activated | 3.5e-08 / 1.0e-06 | 3.0e-08 / 9.9e-07 | 1.2e-04 / 3.6e-03 | 1.1e-07 / 2.6e-06 | 9.0e-05 / 3.6e-03 | 773 |
    | P=1000 raw | 3.5e-08 / 1.0e-06 | 3.0e-08 / 1.0e-06 | 1.1e-07 / 2.6e-06 | 1.5e-08 / 4.8e-07 | 2.3e-08 / 2.6e-06 | 784 |
    | P=100003 activated | 6.0e-08 / 1.0e-06 | 3.0e-08 / 1.0e-06 | 2.4e-04 / 7.2e-03 | 1.8e-07 / 4.3e-06 | 2.4e-04 / 7.2e-03 | 73647 |
    | P=100003 raw | 5.9e-08 / 1.0e-06 | 3.0e-08 / 1.0e-06 | 1.2e-07 / 3.8e-06 | 3.0e-08 / 9.9e-07 | 4.8e-08 / 3.8e-06 | 77849 |
    | P=1000 raw, wide | 1.2e-04 / 3.0e-03 | 3.0e-08 / 1.0e-06 | 2.1e-04 / 7.2e-03 | 2.8e-08 / 6.8e-07 | - | - |

    sweep: all 50 cases of the ladder, the camera list, the camera-model cameras, the 2 x 11 boundary rows, the five
    one-camera cases, nothing seen and one row seen of 100003: 0 valid flags and 0 filter values differ in their bits.
    end to end (64 x 64, 2 000 Gaussians, every row seen): dL/draw_scales 2.6e-08 / 9.0e-07, dL/draw_opacity 5.5e-09 / 1.6e-07.

Also here: discrimination (the cross term d o_eff / d s exceeds ten bars on at least min(100, P / 4) rows of every case, and
the product's gradient with dL/ds_eff = None IS that term), the same bits on two runs and on a side stream
(tests/stream_order.py), guard bands around every buffer the module allocates or is handed (tests/guarded_alloc.py), the
NULL-gradient routes, and compute_3d_filter -> apply_3d_filter(from_raw=True) -> render under set_antialiasing(True) ->
backward end to end (64 x 64, 2 000 Gaussians, 3 ring cameras).
"""
import numpy as np
import pytest
import torch

import filter3d_helpers as FH
import stream_order as SO
from guarded_alloc import GuardedAllocator
from normals_helpers import bar_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = FH.CHUNK


def _bits(t):
    t = t.detach().contiguous()
    return (t.view(torch.uint8) if t.dtype == torch.bool else t.view(torch.int32)).cpu().numpy()


def _f64(t):
    return t.detach().cpu().double().numpy()


def _dev(a, grad=False):
    return torch.tensor(np.array(a)).to(DEV).requires_grad_(grad)


def _sweep(xyz, cameras):
    from gaussianeditor_amd import filter3d as F3

    f, valid = F3.compute_3d_filter(_dev(xyz), cameras, return_valid=True)
    torch.cuda.synchronize()
    assert f.dtype == torch.float32 and tuple(f.shape) == (len(xyz), 1) and valid.dtype == torch.bool and tuple(valid.shape) == (len(xyz),)
    return f.cpu().numpy(), valid.cpu().numpy()


def _assert_same(tag, got, want):
    (f, valid), (wf, wvalid) = got, want
    bad_v = int((valid != wvalid).sum())
    bad_f = int((f.view(np.int32) != wf.view(np.int32)).sum())
    print(f"  {tag}: {int(wvalid.sum())} of {len(wvalid)} rows seen; {bad_v} valid flags and {bad_f} filter values differ in their bits")
    assert bad_v == 0 and bad_f == 0, (tag, bad_v, bad_f)


# ---- the sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,V", FH.SWEEP_CASES)
def test_the_sweep_is_the_restatement_bit_for_bit(P, V):
    from gaussianeditor_amd import filter3d as F3

    case = FH.sweep_case(P, V)
    packed = F3.pack_cameras(case["cameras"], DEV)
    assert len(packed) == V
    _assert_same(f"sweep P={P} V={V}", _sweep(case["xyz"], packed), FH.sweep_expectation(P, V))


def test_a_camera_list_and_the_camera_model_cameras_give_the_same_bits():
    import camera_cases as CC
    from gaussianeditor_amd.synth import ring_cameras

    case = FH.sweep_case(1000, 2)
    _assert_same("camera list", _sweep(case["xyz"], list(case["cameras"])), FH.sweep_expectation(1000, 2))
    base = ring_cameras(3, 97, 61)[1]
    cams = [CC.general_camera(base, 97, 61, *CC.CAMERAS[n]) for n in CC.NAMES] + [base.to(DEV)]
    xyz = case["xyz"] / 3.0
    _assert_same("camera_cases", _sweep(xyz, cams), FH.sweep_ref(xyz, cams))


@pytest.mark.parametrize("cam", [dict(), dict(W=701, H=333, fovx=0.6, fovy=1.1)], ids=["640x480", "701x333"])
def test_the_float32_neighbours_of_every_threshold(cam):
    cam = FH.identity_camera(**cam)
    xyz, want, names = FH.boundary_rows(cam)
    got = _sweep(xyz, [cam])
    assert got[1].tolist() == want.tolist(), list(zip(names, got[1]))
    _assert_same("boundary rows", got, FH.sweep_ref(xyz, [cam]))


@pytest.mark.parametrize("at", [0, C - 1, C, 2 * C - 1, 2 * C], ids=lambda a: f"camera{a}")
def test_a_row_seen_by_exactly_one_camera_at_the_edges_of_a_chunk(at):
    """2 C + 1 cameras that look away from the rows, one -- the first or the last of a chunk -- that looks at them"""
    away = np.eye(4)
    away[0, 0], away[2, 2], away[3, 2] = -1.0, -1.0, -1.0
    cams = [FH.Cam(away, 320 + i, 200 + i, 0.9, 0.7) for i in range(2 * C + 1)]
    cams[at] = FH.identity_camera(W=333, H=222)
    xyz = FH.sweep_case(257, 1)["xyz"] * np.float32(0.1) + np.array([0, 0, 3.0], dtype=np.float32)
    want = FH.sweep_ref(xyz, cams)
    assert want[1].all() and FH.sweep_offenders(xyz, cams) == 0
    for i, c in enumerate(FH.camera_table(cams)):
        assert FH.sees(xyz, c)[0].any() == (i == at)
    _assert_same(f"only camera {at} sees", _sweep(xyz, cams), want)


def test_all_rows_unseen_take_100000_and_one_seen_row_in_the_last_block_sets_the_rest():
    cam = FH.identity_camera()
    fx = FH.camera_table([cam])[0]["fx"]
    P = 100_003
    xyz = FH.sweep_case(P, 1)["xyz"].copy()
    xyz[:, 2] = -np.abs(xyz[:, 2]) - 1.0      # behind the camera
    f, valid = _sweep(xyz, [cam])
    assert not valid.any() and (f == np.float32(100000.0 / fx * FH.SQRT_0_2)).all()
    _assert_same("nothing seen", (f, valid), FH.sweep_ref(xyz, [cam]))
    xyz[P - 2] = (0.25, -0.125, 7.5)          # the last block holds rows 99 840 ..
    assert (P - 2) // FH.ROWS == (P - 1) // FH.ROWS
    f, valid = _sweep(xyz, [cam])
    assert valid.sum() == 1 and valid[P - 2] and (f == np.float32(7.5 / fx * FH.SQRT_0_2)).all()
    _assert_same("one row seen", (f, valid), FH.sweep_ref(xyz, [cam]))


# ---- the apply ----------------------------------------------------------------------------------------------------------
def _apply(case, need=(True, True), up=(True, True)):
    """(s_eff, o_eff, d_scales | None, d_opacity | None) tensors of the product"""
    from gaussianeditor_amd import filter3d as F3

    s, o = _dev(case["scales"], need[0]), _dev(case["opacity"], need[1])
    s_eff, o_eff = F3.apply_3d_filter(s, o, _dev(case["filter"]), from_raw=case["from_raw"])
    outs = [t for t, u in zip((s_eff, o_eff), up) if u]
    if outs and any(need):
        torch.autograd.backward(outs, [_dev(case[k]) for k, u in zip(("g_s", "g_o"), up) if u])
    torch.cuda.synchronize()
    return s_eff.detach(), o_eff.detach(), s.grad, o.grad


def _compare(tag, key, got, want, bar):
    err = float(np.abs(_f64(got).reshape(want.shape) - want).max(initial=0.0))
    print(f"  {tag}: {key} error {err:.3e} bar {bar:.3e} (largest entry {float(np.abs(want).max(initial=0.0)):.3e})")
    assert err <= bar, (tag, key, err, bar)


@pytest.mark.parametrize("from_raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("P", FH.LADDER)
def test_apply_forward_and_backward(P, from_raw):
    case = FH.apply_case(P, from_raw)
    e, bars = FH.apply_expectation(P, from_raw)
    got = dict(zip(("s_eff", "o_eff", "d_scales", "d_opacity"), _apply(case)))
    tag = f"apply P={P} {'raw' if from_raw else 'activated'}"
    for k in ("s_eff", "o_eff", "d_scales", "d_opacity"):
        assert tuple(got[k].shape) == e[k].shape
        _compare(tag, k, got[k], e[k], bars[k])
    # at f = 0 the values are the (activated) inputs to the last bit and the cross term is exactly zero
    zero = case["filter"][:, 0] == 0
    if not from_raw:
        assert np.array_equal(_bits(got["s_eff"])[zero], case["scales"].view(np.int32)[zero])
        assert np.array_equal(_bits(got["o_eff"])[zero], case["opacity"].view(np.int32)[zero])
    # discrimination: the cross term alone (dL/ds_eff = None) is what the product returns for it, and it exceeds ten bars
    cross = FH.cross_term(case)
    big = int((np.abs(cross).max(axis=1) > 10.0 * bars["d_scales"]).sum())
    print(f"  {tag}: the cross term exceeds ten bars on {big} of {P} rows (needed {min(100, P / 4):.1f})")
    assert big >= min(100, P / 4)
    only = _apply(case, up=(False, True))
    _compare(tag, "d_scales through o_eff alone", only[2], cross, bars["d_scales"])
    assert not bool(only[2].cpu()[torch.tensor(zero)].any()), "the cross term at f = 0 is not exactly zero"
    assert float(np.abs(_f64(got["d_scales"]) - (e["d_scales"] - cross)).max()) > 10.0 * bars["d_scales"]


def test_apply_on_raw_scales_across_plus_minus_eight():
    """Every row independent, raw scales uniform over +-8 (scales up to 2981): the bar, without the share condition"""
    case = FH.apply_case(1000, True, wide=True)
    e, bars = FH.apply_expectation(1000, True, True)
    for k, g in zip(("s_eff", "o_eff", "d_scales", "d_opacity"), _apply(case)):
        _compare("apply P=1000 raw, wide", k, g, e[k], bars[k])


def test_bake_is_the_logarithm_and_the_logit_of_the_apply():
    from gaussianeditor_amd import filter3d as F3

    case = FH.apply_case(1000, True)
    s, o, f = (_dev(case[k]) for k in ("scales", "opacity", "filter"))
    ls, lo = F3.bake_3d_filter(s, o, f)
    s_eff, o_eff = F3.apply_3d_filter(s, o, f, from_raw=True)
    assert np.array_equal(_bits(ls), _bits(torch.log(s_eff))) and np.array_equal(_bits(lo), _bits(torch.logit(o_eff)))
    assert tuple(ls.shape) == (1000, 3) and tuple(lo.shape) == (1000, 1) and bool(torch.isfinite(ls).all())


# ---- robustness ---------------------------------------------------------------------------------------------------------
def _cell_inputs():
    from gaussianeditor_amd import filter3d as F3

    sw, ap = FH.sweep_case(100_003, C + 1), FH.apply_case(100_003, True)
    rec, f_max = F3.camera_records(sw["cameras"])
    t = lambda a, g=False: torch.tensor(np.array(a)).requires_grad_(g)  # noqa: E731
    return dict(xyz=t(sw["xyz"]), rec=torch.from_numpy(rec), f_max=f_max, scales=t(ap["scales"], True), opacity=t(ap["opacity"], True),
                g_s=t(ap["g_s"]), g_o=t(ap["g_o"]))


def _cell(put):
    """sweep -> apply(from_raw) -> backward on whatever stream is current; no host wait"""
    from gaussianeditor_amd import filter3d as F3

    i = _cell_inputs()
    xyz, rec, s, o, g_s, g_o = (put(i[k]) for k in ("xyz", "rec", "scales", "opacity", "g_s", "g_o"))
    f, valid = F3.compute_3d_filter(xyz, F3.PackedCameras(rec, i["f_max"]), return_valid=True)
    s_eff, o_eff = F3.apply_3d_filter(s, o, f, from_raw=True)
    torch.autograd.backward([s_eff, o_eff], [g_s, g_o])
    return dict(filter=f, valid=valid, s_eff=s_eff.detach(), o_eff=o_eff.detach()), dict(d_scales=s.grad, d_opacity=o.grad)


def _plain_put(t):
    return t.detach().to(DEV).requires_grad_(t.requires_grad)


def test_the_same_bits_on_two_runs_and_on_a_side_stream():
    det, grads = _cell(_plain_put)
    torch.cuda.synchronize()
    want, want_g = SO.host(det), SO.host(grads)
    det, grads = _cell(_plain_put)
    torch.cuda.synchronize()
    for a, b in ((SO.host(det), want), (SO.host(grads), want_g)):
        assert a.keys() == b.keys() and all(SO.same_bits(a[k], b[k]) for k in a)
    out, side = SO.run_cell(_cell, SO.SLEEP_FLOOR_MS, allocator=lambda: GuardedAllocator(0x5A))
    v = SO.verdict(out[0], want, side)
    print(f"  filter3d cell: {v}; {SO.report(side)}")
    assert v == "clean" and all(SO.same_bits(out[1][k], want_g[k]) for k in want_g)
    assert np.array_equal(want["filter"], FH.sweep_expectation(100_003, C + 1)[0])


@pytest.mark.parametrize("P,V", [(1000, C + 1), (FH.ROWS + 1, 1), (65, 2), (1, 1)])
def test_every_buffer_keeps_its_guard_bands(P, V):
    """Inputs, outputs, gradients and the sweep's workspace between bands of 0xFF (NaN as float32): the bands stay, and no
    output element keeps its poison."""
    from gaussianeditor_amd import filter3d as F3

    sw = FH.sweep_case(P, V)
    rec, f_max = F3.camera_records(sw["cameras"])
    with GuardedAllocator(0xFF, device=torch.device(DEV, torch.cuda.current_device())) as ga:
        res = []
        xyz, recs = ga.place(torch.tensor(sw["xyz"])), ga.place(torch.from_numpy(rec))
        f, valid = F3.compute_3d_filter(xyz, F3.PackedCameras(recs, f_max), return_valid=True)
        res += [f, valid.view(torch.uint8).float()]
        assert int(valid.view(torch.uint8).max()) <= 1
        for from_raw in (False, True):
            ap = FH.apply_case(P, from_raw)
            s, o = (ga.place(torch.tensor(ap[k]).requires_grad_(True)) for k in ("scales", "opacity"))
            s_eff, o_eff = F3.apply_3d_filter(s, o, ga.place(torch.tensor(ap["filter"])), from_raw=from_raw)
            torch.autograd.backward([s_eff, o_eff], [ga.place(torch.tensor(ap[k])) for k in ("g_s", "g_o")])
            res += [s_eff.detach(), o_eff.detach(), s.grad, o.grad]
        ga.assert_clean()
        # 2 + 2 x 5 placed inputs; workspace, filter, valid; 2 x (s_eff, o_eff, d_scales, d_opacity)
        assert len(ga) >= 12 + 3 + 8
    _assert_same("guarded sweep", (f.cpu().numpy(), valid.cpu().numpy()), FH.sweep_expectation(P, V))
    for t in res:
        assert not bool(torch.isnan(t).any()), "an output element was not written"


class _Counting:
    """the native library with the calls of the apply's backward counted"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "gsr_filter3d_apply_backward":
            return fn

        def counted(*a):
            self.calls.append(tuple(x is not None for x in a[-4:]))  # (dL_ds_eff, dL_do_eff, dL_dscales, dL_dopacity) given
            return fn(*a)

        return counted


def test_only_what_autograd_needs_is_computed(monkeypatch):
    """Through autograd: an input that requires no gradient gets none, an upstream gradient that is None is a NULL pointer,
    and a route that cannot produce anything launches nothing.  Through the C ABI: a NULL output pointer skips that output
    -- a poisoned buffer that was not passed stays poisoned -- and the outputs asked for are the bits of the full call."""
    from gaussianeditor_amd import _native
    from gaussianeditor_amd import filter3d as F3

    case = FH.apply_case(1000, True)
    full = _apply(case)
    lib = _Counting(_native.lib())
    monkeypatch.setattr(F3._native, "lib", lambda: lib)
    # (need scales, need opacity), (s_eff used, o_eff used) -> the call's four pointers, or None for no launch
    routes = [((True, True), (True, True), (True, True, True, True)), ((True, False), (True, True), (True, True, True, False)),
              ((False, True), (True, True), (True, True, False, True)), ((True, True), (False, True), (False, True, True, True)),
              ((True, True), (True, False), (True, False, True, False)), ((False, True), (True, False), None),
              ((False, False), (True, True), None)]
    for need, up, want in routes:
        lib.calls.clear()
        got = _apply(case, need=need, up=up)
        assert lib.calls == ([] if want is None else [want]), (need, up, lib.calls)
        for g, i in zip(got[2:], (2, 3)):
            assert (g is not None) == (want is not None and want[i]), (need, up, i)
        if up == (True, True):
            for g, f in zip(got[2:], full[2:]):
                assert g is None or np.array_equal(_bits(g), _bits(f))
    # opacity needed but only s_eff used: no gradient at all reaches it
    assert _apply(case, need=(False, True), up=(True, False))[3] is None
    monkeypatch.undo()

    L = _native.lib()
    st = torch.cuda.current_stream(DEV).cuda_stream
    s, o, f, g_s, g_o = (_dev(case[k]) for k in ("scales", "opacity", "filter", "g_s", "g_o"))
    for mask in ((1, 0), (0, 1), (1, 1)):
        bufs = [torch.full((1000, 3), float("nan"), device=DEV), torch.full((1000, 1), float("nan"), device=DEV)]
        ptrs = [b.data_ptr() if m else None for b, m in zip(bufs, mask)]
        assert L.gsr_filter3d_apply_backward(st, 1000, 1, s.data_ptr(), o.data_ptr(), f.data_ptr(), g_s.data_ptr(), g_o.data_ptr(), *ptrs) == 0
        torch.cuda.synchronize()
        for b, m, w in zip(bufs, mask, full[2:]):
            assert np.array_equal(_bits(b), _bits(w)) if m else bool(torch.isnan(b).all())


# ---- end to end ---------------------------------------------------------------------------------------------------------
class _Model:
    def __init__(self, sc, scaling, opacity):
        d = lambda t: t.to(DEV).clone().contiguous().requires_grad_(True)  # noqa: E731
        self._xyz, self._features, self._rotation = d(sc["xyz"]), d(sc["features"]), d(sc["rotation"])
        self._scaling_eff, self._opacity_eff = scaling, opacity
        self.active_sh_degree = self.max_sh_degree = 3

    get_xyz = property(lambda s: s._xyz)
    get_features = property(lambda s: s._features)
    get_opacity = property(lambda s: s._opacity_eff)
    get_scaling = property(lambda s: s._scaling_eff)
    get_rotation = property(lambda s: s._rotation)


def test_filter_then_apply_then_render_then_backward_end_to_end():
    """64 x 64, 2 000 Gaussians, 3 ring cameras: compute_3d_filter -> apply_3d_filter(from_raw=True) -> render under
    set_antialiasing(True) -> backward.  With the gradients retained at scales_eff / opacity_eff, the gradients at the raw
    parameters are the float64 chain of those retained gradients, within the rule's bar (the same chain in float32 torch
    operators sets it).  The renderer's own backward is held by its own tests."""
    import types

    import gaussianeditor_amd
    from gaussianeditor_amd import filter3d as F3
    from gaussianeditor_amd.gaussian_renderer import render
    from gaussianeditor_amd.synth import ring_cameras, seed_gradient, synth_scene

    H = W = 64
    sc = synth_scene(2000, seed=3, s0=0.03)
    cams = ring_cameras(3, W, H)
    xyz = sc["xyz"].to(DEV).contiguous()
    f, valid = F3.compute_3d_filter(xyz, F3.pack_cameras(cams, DEV), return_valid=True)
    want_f, want_valid = FH.sweep_ref(sc["xyz"].numpy(), cams)
    assert np.array_equal(_bits(f), want_f.view(np.int32)) and np.array_equal(valid.cpu().numpy(), want_valid) and want_valid.mean() > 0.5
    raw_s = torch.log(sc["scaling"]).to(DEV).contiguous().requires_grad_(True)
    raw_o = torch.logit(sc["opacity"]).to(DEV).contiguous().requires_grad_(True)
    s_eff, o_eff = F3.apply_3d_filter(raw_s, raw_o, f, from_raw=True)
    s_eff.retain_grad(), o_eff.retain_grad()
    pipe = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    gaussianeditor_amd.set_antialiasing(True)
    try:
        pkg = render(cams[1].to(DEV), _Model(sc, s_eff, o_eff), pipe, torch.tensor([0.1, 0.2, 0.3], device=DEV))
        (pkg["render"] * (seed_gradient(H, W, 3) * H * W).to(DEV)).sum().backward()
    finally:
        gaussianeditor_amd.set_antialiasing(False)
    torch.cuda.synchronize()
    g_s, g_o = s_eff.grad, o_eff.grad
    assert int((g_s.abs().sum(1) > 0).sum()) > 200 and int((g_o.abs() > 0).sum()) > 200

    def chain(dtype):
        t = lambda x, g=False: x.detach().cpu().to(dtype).requires_grad_(g)  # noqa: E731
        a, b = t(raw_s, True), t(raw_o, True)
        out = FH.apply_ref(a, b, t(f), True)
        ga, gb = torch.autograd.grad(list(out), [a, b], [t(g_s), t(g_o)])
        return ga.double().numpy(), gb.double().numpy()

    for name, got, w64, w32 in zip(("dL/draw_scales", "dL/draw_opacity"), (raw_s.grad, raw_o.grad), chain(torch.float64), chain(torch.float32)):
        _compare("end to end", name, got, w64, bar_of(w32, w64))
        assert float(np.abs(w64).max()) > 0
