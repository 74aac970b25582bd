"""-m gpu: the bilateral-grid slice and its TV regulariser (gaussianeditor_amd.bilagrid; the gsr_bilagrid_* entry points,
csrc/loss/gsr_bilagrid.hip) against the float64 restatement of tests/bilagrid_helpers.py (pinned by tests/test_cpu_bilagrid.py)
on every case there: five image shapes x four grid sizes, N = 3 grids, idx a Python int, [0, 2] and [1, 1].

The bar, per case and quantity (bilagrid_helpers.bar, the rule of tests/test_gpu_loss.py): the product's error against float64
must not exceed max(2 x the error of the float32 run of the same grid_sample restatement on the CPU against float64, 1e-6 of
the quantity's largest entry).

Discrimination, asserted on the expectation: in every case the guidance share of dL/dimage (what flows through the luminance
coordinate) and its direct share each exceed TEN bars on at least min(100, n / 4) values, so a backward without either
misses the bar of every case.

The scaling test.  "dL/dout scaled by 3.5 scales both gradients within one ulp" is asked of results that are each ONE
rounding away from the exact value: g1 = fl(S), g2 = fl(3.5 S).  3.5 g1 then differs from 3.5 S by up to 3.5 x half an ulp of
g1, g2 by up to half an ulp of g2, so the assertion is |g2 - 3.5 g1| <= ulp(g2) / 2 + 3.5 ulp(g1) / 2, evaluated in float64
(plus 2^-16 of that for the binary64 sums inside the kernels) -- half an ulp for each side, which is what a correctly rounded
implementation meets and nothing looser.  The three lowest mantissa bits of dL/dout are cleared so that 3.5 dL/dout is exact.

Measured on the MI355X, the product's error against float64 / the bar, both as a fraction of the quantity's largest entry:
    case            out                dL/dimage          dL/dgrids
    5x7_g2          3.4e-08 / 1.0e-06  3.2e-08 / 1.0e-06  2.6e-08 / 1.0e-06
    5x7_g354        3.6e-08 / 1.0e-06  2.7e-08 / 1.0e-06  2.9e-08 / 1.0e-06
    5x7_g16         2.7e-08 / 1.0e-06  2.4e-08 / 1.2e-06  3.1e-08 / 1.1e-06
    5x7_g32         3.0e-08 / 1.3e-06  1.6e-08 / 1.3e-06  2.9e-08 / 1.5e-06
    45x70_g2        5.4e-08 / 1.0e-06  4.1e-08 / 1.0e-06  3.3e-08 / 2.5e-06
    45x70_g354      3.8e-08 / 1.0e-06  4.0e-08 / 1.0e-06  3.7e-08 / 1.5e-06
    45x70_g16       4.4e-08 / 1.1e-06  2.8e-08 / 1.8e-06  3.3e-08 / 1.6e-06
    45x70_g32       3.7e-08 / 2.5e-06  2.2e-08 / 6.1e-06  2.7e-08 / 4.1e-06
    33x130_g2       4.0e-08 / 1.0e-06  4.2e-08 / 1.0e-06  3.2e-08 / 4.0e-06
    33x130_g354     4.2e-08 / 1.0e-06  4.1e-08 / 1.0e-06  3.3e-08 / 1.0e-06
    33x130_g16      4.3e-08 / 1.5e-06  4.9e-08 / 1.8e-06  3.5e-08 / 2.1e-06
    33x130_g32      4.2e-08 / 2.5e-06  3.6e-08 / 4.0e-06  3.2e-08 / 4.1e-06
    64x64_g2        5.0e-08 / 1.0e-06  3.8e-08 / 1.0e-06  4.2e-08 / 2.4e-06
    64x64_g354      4.4e-08 / 1.0e-06  3.2e-08 / 1.0e-06  2.1e-08 / 1.0e-06
    64x64_g16       3.9e-08 / 1.0e-06  3.5e-08 / 1.0e-06  4.5e-08 / 1.0e-06
    64x64_g32       4.0e-08 / 1.4e-06  5.5e-08 / 1.0e-06  3.0e-08 / 1.1e-06
    batch_g2_i02    4.2e-08 / 1.0e-06  3.3e-08 / 1.0e-06  2.7e-08 / 4.4e-06
    batch_g2_i11    4.0e-08 / 1.0e-06  2.4e-08 / 1.0e-06  4.0e-08 / 5.0e-06
    batch_g354_i02  4.3e-08 / 1.0e-06  3.8e-08 / 1.0e-06  4.3e-08 / 1.9e-06
    batch_g354_i11  5.1e-08 / 1.0e-06  3.8e-08 / 1.0e-06  3.8e-08 / 1.0e-06
    batch_g16_i02   3.7e-08 / 1.2e-06  3.8e-08 / 2.0e-06  4.1e-08 / 1.4e-06
    batch_g16_i11   3.7e-08 / 1.0e-06  2.7e-08 / 1.8e-06  5.5e-08 / 1.8e-06
    batch_g32_i02   3.9e-08 / 2.4e-06  3.4e-08 / 7.5e-06  3.8e-08 / 3.9e-06
    batch_g32_i11   4.4e-08 / 3.1e-06  3.4e-08 / 3.8e-06  4.4e-08 / 4.9e-06
i.e. every quantity is one float32 rounding (at most 6e-8) away from float64, 0.01 .. 0.06 of its bar.  TV and its gradient,
N = 1 and 3, the four grid sizes: 4.0e-09 .. 5.2e-08 against a bar of 1.0e-06 everywhere.  End to end: 4.9e-08 .. 9.0e-08 of the
largest entry.  The file runs in 4 s.
"""
import ctypes

import numpy as np
import pytest
import torch

import bilagrid_helpers as BH
from helpers import assert_grads_close, make_case, settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).reshape(-1).view(np.uint32)


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _idx(idx):
    if isinstance(idx, (int, torch.Tensor)):
        return idx
    return torch.tensor(idx, dtype=torch.int64, device=DEV)


def _run(case, dout=None, grids_grad=True, image_grad=True, idx=None):
    """(out, dL/dimage, dL/dgrids) of a named case (or a dict like bilagrid_helpers.make_case's)"""
    from gaussianeditor_amd.bilagrid import slice_image

    c = BH.make_case(case) if isinstance(case, str) else case
    grids = torch.tensor(c["grids"]).to(DEV).requires_grad_(grids_grad)
    image = torch.tensor(c["image"]).to(DEV).requires_grad_(image_grad)
    out = slice_image(grids, image, _idx(c["idx"] if idx is None else idx))
    out.backward(torch.tensor(c["dout"]).to(DEV) if dout is None else dout)
    torch.cuda.synchronize()
    return out.detach(), image.grad, grids.grad


@pytest.mark.parametrize("case", BH.CASES)
def test_slice_and_both_gradients_against_float64(case):
    c, e, bar = BH.make_case(case), BH.expectation(case), BH.bar(case)
    n = e["d_image"].size
    for share in ("d_image_guidance", "d_image_direct"):
        assert int((np.abs(e[share]) > 10 * bar["d_image"]).sum()) >= min(100, n // 4), (case, share)
    out, d_image, d_grids = _run(case)
    assert out.shape == c["image"].shape and d_image.shape == c["image"].shape and d_grids.shape == c["grids"].shape
    assert out.dtype == d_image.dtype == d_grids.dtype == torch.float32
    got = dict(out=_f64(out), d_image=_f64(d_image), d_grids=_f64(d_grids))
    err = {k: float(np.abs(got[k] - e[k]).max()) for k in got}
    top = {k: float(np.abs(e[k]).max()) for k in got}
    print(f"  {case}: " + "  ".join(f"{k} {err[k] / top[k]:.1e} / {bar[k] / top[k]:.1e}" for k in got))
    for k in got:
        assert err[k] <= bar[k], (case, k, err[k], bar[k])
    # grids no image selected: exact zeros (and every element was written: the buffer came from torch.empty)
    B = 1 if c["image"].ndim == 3 else c["image"].shape[0]
    for g in set(range(BH.N_GRIDS)) - set(BH.index_list(c["idx"], B)):
        assert not _bits(d_grids[g]).any(), (case, g)


def test_a_grid_selected_twice_gets_the_sum_of_both_images():
    case = "batch_g16_i11"
    c, bar = BH.make_case(case), BH.bar(case)
    both = _f64(_run(case)[2])
    parts = []
    for b in range(2):
        one = dict(grids=c["grids"], image=c["image"][b], dout=c["dout"][b], idx=1)
        parts.append(_f64(_run(one)[2]))
    assert np.abs(parts[0][1]).max() > 0 and np.abs(parts[1][1]).max() > 0
    assert np.abs(both - (parts[0] + parts[1])).max() <= bar["d_grids"]


def test_a_device_index_out_of_range_is_clamped():
    """The host never reads a tensor idx, so it cannot refuse it: the kernels clamp it to [0, N - 1] (include/gsr.h)."""
    case = "45x70_g354"
    want = _run(case)  # idx 2
    for idx, same_as in (([7], 2), ([-3], 0), ([2 ** 40], 2)):
        ref = want if same_as == 2 else _run(case, idx=0)
        got = _run(case, idx=idx)
        for a, b in zip(got, ref):
            assert np.array_equal(_bits(a), _bits(b)), idx
    # a () tensor and a (1,) tensor and the int are the same call
    for idx in (torch.tensor(2, device=DEV), torch.tensor([2], device=DEV)):
        for a, b in zip(_run(case, idx=idx), want):
            assert np.array_equal(_bits(a), _bits(b))


def _big_flat_case():
    """256 x 256 on a 2 x 2 x 2 grid: every pixel lands on the same eight vertices and 64 workgroups add to each"""
    rng = np.random.default_rng(99)
    shape = (3, 256, 256)
    image = rng.uniform(-0.2, 1.3, size=shape).astype(np.float32)
    while True:  # the input condition of bilagrid_helpers: no pixel within MARGIN of a discontinuity of the guidance term
        bad = BH.margin_violations(image, 2)
        if not bad.any():
            break
        image = np.where(bad[None], rng.uniform(-0.2, 1.3, size=shape).astype(np.float32), image)
    return dict(grids=(np.eye(3, 4).reshape(1, 12, 1, 1, 1) + 0.3 * rng.standard_normal((2, 12, 2, 2, 2))).astype(np.float32),
                image=image, idx=1, dout=(rng.standard_normal(shape) / (256 * 256)).astype(np.float32))


def test_two_runs_give_the_same_bits():
    for case in ("45x70_g16", _big_flat_case()):
        a, b = _run(case), _run(case)
        for u, v in zip(a, b):
            assert torch.equal(u, v) and np.array_equal(_bits(u), _bits(v))
        assert float(a[2].abs().max()) > 0 and float(a[1].abs().max()) > 0
    # the 256 x 256 sums against the eight-corner restatement (a sum over 65 536 pixels per vertex, 64 partials each)
    c = _big_flat_case()
    _, d_image, d_grids = BH.slice_numpy(c["grids"], c["image"][None], [1], c["dout"][None])
    got = _run(c)
    assert np.abs(_f64(got[2]) - d_grids).max() <= 1e-6 * np.abs(d_grids).max()
    assert np.abs(_f64(got[1]) - d_image[0]).max() <= 1e-6 * np.abs(d_image).max()


def _tv(N, grid, scale=None):
    from gaussianeditor_amd.bilagrid import total_variation_loss

    g = torch.tensor(BH.tv_case(N, grid)).to(DEV).requires_grad_(True)
    tv = total_variation_loss(g)
    (tv if scale is None else scale * tv).backward()
    torch.cuda.synchronize()
    return tv.detach(), g.grad


@pytest.mark.parametrize("N", (1, 3))
@pytest.mark.parametrize("grid", list(BH.GRIDS.values()), ids=list(BH.GRIDS))
def test_tv_and_its_gradient_against_float64(N, grid):
    e, bar = BH.tv_expectation(N, grid)
    tv, grad = _tv(N, grid)
    assert tv.shape == () and grad.shape == e["grad"].shape
    err = dict(tv=abs(float(tv) - e["tv"]), grad=float(np.abs(_f64(grad) - e["grad"]).max()))
    top = dict(tv=abs(e["tv"]), grad=float(np.abs(e["grad"]).max()))
    print(f"  tv N={N} {grid}: " + "  ".join(f"{k} {err[k] / top[k]:.1e} / {bar[k] / top[k]:.1e}" for k in err))
    for k in err:
        assert err[k] <= bar[k], (N, grid, k, err[k], bar[k])
    # twice the same bits; an upstream gradient of 3.5 is one rounding of 3.5 x the gradient
    tv2, grad2 = _tv(N, grid)
    assert np.array_equal(_bits(tv), _bits(tv2)) and np.array_equal(_bits(grad), _bits(grad2))
    g35 = _f64(_tv(N, grid, scale=3.5)[1])
    assert (np.abs(g35 - 3.5 * _f64(grad)) <= (1.0 + 2.0 ** -16) * _half_ulps(g35, _f64(grad))).all()


def _half_ulps(g2, g1):
    """ulp(g2) / 2 + 3.5 ulp(g1) / 2 of float32, elementwise, as float64"""
    u = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)  # noqa: E731
    return 0.5 * u(g2) + 1.75 * u(g1)


def test_upstream_gradient_scales_within_one_ulp():
    case = "45x70_g16"
    d = BH.make_case(case)["dout"].copy()
    d = (d.view(np.uint32) & np.uint32(0xFFFFFFF8)).view(np.float32)  # 3.5 x is exact now
    d35 = (3.5 * d.astype(np.float64)).astype(np.float32)
    assert np.array_equal(d35.astype(np.float64), 3.5 * d.astype(np.float64))
    one = _run(case, dout=torch.tensor(d).to(DEV))
    two = _run(case, dout=torch.tensor(d35).to(DEV))
    assert np.array_equal(_bits(one[0]), _bits(two[0]))
    for k in (1, 2):
        g1, g2 = _f64(one[k]), _f64(two[k])
        assert (g1 != g2).any()
        bad = np.abs(g2 - 3.5 * g1) > (1.0 + 2.0 ** -16) * _half_ulps(g2, g1)
        assert not bad.any(), (k, int(bad.sum()), float((np.abs(g2 - 3.5 * g1) / _half_ulps(g2, g1)).max()))


def test_only_what_autograd_needs_is_computed_and_no_grad_saves_nothing():
    from gaussianeditor_amd import bilagrid

    case = "45x70_g354"
    full = _run(case)
    _, d_image, d_grids = _run(case, image_grad=False)
    assert d_image is None and np.array_equal(_bits(d_grids), _bits(full[2]))
    _, d_image, d_grids = _run(case, grids_grad=False)
    assert d_grids is None and np.array_equal(_bits(d_image), _bits(full[1]))
    c = BH.make_case(case)
    grids = torch.tensor(c["grids"]).to(DEV).requires_grad_(True)
    image = torch.tensor(c["image"]).to(DEV).requires_grad_(True)
    with torch.no_grad():
        out = bilagrid.slice_image(grids, image, 2)
        tv = bilagrid.total_variation_loss(grids)
    assert not out.requires_grad and out.grad_fn is None and not tv.requires_grad and tv.grad_fn is None
    assert np.array_equal(_bits(out), _bits(full[0]))
    out = bilagrid.slice_image(grids.detach(), image.detach(), 2)  # grad mode, nothing to differentiate
    assert not out.requires_grad

    class Ctx:  # what the forward hands to autograd: nothing, unless a backward will follow
        saved = None

        def save_for_backward(self, *tensors):
            self.saved = tensors

        def set_materialize_grads(self, flag):
            pass

    idx = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    for need in (False, True):
        ctx = Ctx()
        bilagrid._SliceImage.forward(ctx, grids.detach(), image.detach(), idx, need)
        assert (ctx.saved is not None) == need
        ctx = Ctx()
        bilagrid._TotalVariation.forward(ctx, grids.detach(), need)
        assert (ctx.saved is not None) == need
    with pytest.raises(RuntimeError):  # once-differentiable: no silent second-order graph
        g, = torch.autograd.grad(bilagrid.slice_image(grids, image, 2).sum(), image, create_graph=True)
        g.sum().backward()


def test_module_is_the_identity_at_first_and_trains():
    from gaussianeditor_amd.bilagrid import BilateralGrid

    c = BH.make_case("batch_g16_i02")
    image = torch.tensor(c["image"]).to(DEV)
    m = BilateralGrid(3).to(DEV)
    out = m(image, torch.tensor([0, 2], device=DEV))
    assert float((out.detach() - image).abs().max()) <= 2e-7 * 1.3  # (one rounding of a sum of weights that is 1 to binary64)
    assert float(m.tv_loss().detach()) == 0.0
    (out * torch.tensor(c["dout"]).to(DEV)).sum().backward()
    assert m.grids.grad is not None and float(m.grids.grad[1].abs().max()) == 0.0 and float(m.grids.grad[0].abs().max()) > 0


def test_a_side_stream_gives_the_bits_of_the_default_stream():
    case = "33x130_g16"
    want = _run(case)
    tv_want = _tv(3, BH.GRIDS["g354"])
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        got = _run(case)
        tv_got = _tv(3, BH.GRIDS["g354"])
    s.synchronize()
    for a, b in zip(got + tv_got, want + tv_want):
        assert np.array_equal(_bits(a), _bits(b))


BAND = 4096


def _banded(nbytes):
    """(raw, interior): `nbytes` of 0xFF between two bands of BAND bytes of 0xFF, the interior 256-byte aligned"""
    raw = torch.full((2 * BAND + nbytes + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    lo = BAND + (-(raw.data_ptr() + BAND)) % 256
    return raw, lo, raw[lo:lo + nbytes]


@pytest.mark.parametrize("case", ("5x7_g32", "45x70_g16", "batch_g354_i11", "33x130_g2"))
def test_caller_owned_buffers_keep_their_guard_bands(case):
    """The C ABI with every output and the workspace between poisoned bands (0xFF: NaN as float32): the bands stay, and no
    element of an output keeps its poison."""
    from gaussianeditor_amd import _native

    L = _native.lib()
    c = BH.make_case(case)
    GX, GY, GZ = c["grid"]
    image = torch.tensor(c["image"]).to(DEV).reshape(-1, 3, *c["image"].shape[-2:])
    B, _, H, W = image.shape
    grids, dout = torch.tensor(c["grids"]).to(DEV), torch.tensor(c["dout"]).to(DEV)
    idx = torch.tensor(BH.index_list(c["idx"], B), dtype=torch.int64, device=DEV)
    nb, tvb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.gsr_bilagrid_workspace_size(B, H, W, GX, GY, GZ, ctypes.byref(nb)) == 0
    assert L.gsr_bilagrid_tv_workspace_size(BH.N_GRIDS, GX, GY, GZ, ctypes.byref(tvb)) == 0
    bufs = {k: _banded(n) for k, n in dict(out=image.numel() * 4, d_image=image.numel() * 4, d_grids=grids.numel() * 4,
                                            work=nb.value, tv_work=tvb.value, tv=4, tv_grad=grids.numel() * 4).items()}
    p = {k: v[2].data_ptr() for k, v in bufs.items()}
    one = torch.ones(1, device=DEV)
    s = torch.cuda.current_stream(DEV).cuda_stream
    dims = (B, H, W, BH.N_GRIDS, GX, GY, GZ)
    assert L.gsr_bilagrid_slice_forward(s, *dims, grids.data_ptr(), idx.data_ptr(), image.data_ptr(), p["out"]) == 0
    assert L.gsr_bilagrid_slice_backward(s, *dims, grids.data_ptr(), idx.data_ptr(), image.data_ptr(), dout.data_ptr(), p["work"],
                                         p["d_image"], p["d_grids"]) == 0
    assert L.gsr_bilagrid_tv_forward(s, BH.N_GRIDS, GX, GY, GZ, grids.data_ptr(), p["tv_work"], p["tv"]) == 0
    assert L.gsr_bilagrid_tv_backward(s, BH.N_GRIDS, GX, GY, GZ, grids.data_ptr(), one.data_ptr(), p["tv_grad"]) == 0
    torch.cuda.synchronize()
    for k, (raw, lo, inner) in bufs.items():
        assert bool((raw[:lo] == 0xFF).all()) and bool((raw[lo + inner.numel():] == 0xFF).all()), (case, k)
        if "work" not in k:
            assert not bool(torch.isnan(inner.view(torch.float32)).any()), (case, k, "an element was not written")
    e = BH.expectation(case)
    for k in ("out", "d_image", "d_grids"):
        got = bufs[k][2].view(torch.float32).cpu().numpy().astype(np.float64).reshape(e[k].shape)
        assert np.abs(got - e[k]).max() <= BH.bar(case)[k], (case, k)


def test_render_then_grid_then_loss_end_to_end():
    """Route one: render -> BilateralGrid -> photometric_loss -> backward.  Route two: the same render, image.backward(gradient
    = the float64 restatement's dL/dimage for the fused loss's dL/dout, cast to float32).  What reaches means3D, opacity, SH
    (and the rest) agrees to 1e-5 of each tensor's largest entry, the project's parity bar."""
    from gaussianeditor_amd.bilagrid import BilateralGrid
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer
    from gaussianeditor_amd.losses import photometric_loss

    case = make_case(2000, 64, 64, s0=0.05)
    sc, H, W = case["sc"], case["H"], case["W"]
    rng = np.random.default_rng(31)
    gt = torch.tensor(rng.uniform(0.0, 1.0, size=(3, H, W)).astype(np.float32)).to(DEV)
    m = BilateralGrid(3).to(DEV)
    with torch.no_grad():
        m.grids.add_(torch.tensor((0.3 * rng.standard_normal(tuple(m.grids.shape))).astype(np.float32)).to(DEV))
    names = ("xyz", "scaling", "rotation", "opacity", "features")

    def render():
        leaves = {k: sc[k].to(DEV).requires_grad_(True) for k in names}
        m2d = torch.zeros_like(leaves["xyz"], requires_grad=True)
        image = GaussianRasterizer(settings(case, DEV))(leaves["xyz"], m2d, leaves["opacity"], shs=leaves["features"],
                                                        scales=leaves["scaling"], rotations=leaves["rotation"])[0]
        return image, leaves, m2d

    def grads(leaves, m2d):
        torch.cuda.synchronize()
        return dict(dL_dmeans3D=leaves["xyz"].grad.cpu().numpy(), dL_dscales=leaves["scaling"].grad.cpu().numpy(),
                    dL_drotations=leaves["rotation"].grad.cpu().numpy(), dL_dopacity=leaves["opacity"].grad.cpu().numpy(),
                    dL_dsh=leaves["features"].grad.cpu().numpy(), dL_dmeans2D=m2d.grad.cpu().numpy())

    image, leaves, m2d = render()
    photometric_loss(m(image, 1), gt).backward()
    one = grads(leaves, m2d)
    assert m.grids.grad is not None and float(m.grids.grad[1].abs().max()) > 0
    image2, leaves2, m2d2 = render()
    assert np.array_equal(_bits(image), _bits(image2))
    with torch.no_grad():
        sliced = m(image2, 1)
    leaf = sliced.clone().requires_grad_(True)
    photometric_loss(leaf, gt).backward()
    _, d_image, _ = BH.slice_numpy(_f64(m.grids), _f64(image2)[None], [1], _f64(leaf.grad)[None])
    image2.backward(gradient=torch.tensor(d_image[0].astype(np.float32)).to(DEV))
    two = grads(leaves2, m2d2)
    assert int((np.abs(one["dL_dmeans3D"]).max(axis=1) > 0).sum()) >= 100
    worst = assert_grads_close(one, two, tol=1e-5, tag="render + grid + loss")
    print(f"  end to end: worst {worst:.1e}")
