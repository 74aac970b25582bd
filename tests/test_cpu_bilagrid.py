"""CPU: the yardstick of tests/test_gpu_bilagrid.py (tests/bilagrid_helpers.py) is pinned -- its two restatements of the slice
agree, the closed forms hold, the input condition holds for every case --, the C ABI declares and types the gsr_bilagrid_*
entry points, and gaussianeditor_amd.bilagrid refuses what it does not support by name, before any launch, without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bilagrid_helpers as BH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gsr_bilagrid_workspace_size", "gsr_bilagrid_slice_forward", "gsr_bilagrid_slice_backward",
           "gsr_bilagrid_tv_workspace_size", "gsr_bilagrid_tv_forward", "gsr_bilagrid_tv_backward")


def _as_batch(c):
    image, dout = c["image"], c["dout"]
    if image.ndim == 3:
        image, dout = image[None], dout[None]
    return image, dout, BH.index_list(c["idx"], image.shape[0])


@pytest.mark.parametrize("case", BH.CASES)
def test_the_two_restatements_agree(case):
    c, e = BH.make_case(case), BH.expectation(case)
    image, dout, idx = _as_batch(c)
    out, d_image, d_grids = BH.slice_numpy(c["grids"], image, idx, dout)
    for got, k in ((out, "out"), (d_image, "d_image"), (d_grids, "d_grids")):
        want = e[k].reshape(got.shape)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (case, k)
    # rows of grids that no image selected have no gradient at all
    for n in set(range(BH.N_GRIDS)) - set(idx):
        assert not e["d_grids"][n].any()


def test_identity_grid_returns_the_image_and_a_constant_grid_its_affine_map():
    rng = np.random.default_rng(5)
    image = rng.uniform(-0.2, 1.3, size=(2, 3, 9, 11))
    M = rng.standard_normal((3, 4))
    for restate in ("numpy", "torch"):
        for A, want in ((np.eye(3, 4), image),
                        (M, np.einsum("cm,bmhw->bchw", M[:, :3], image) + M[:, 3][None, :, None, None])):
            grids = np.broadcast_to(A.reshape(1, 12, 1, 1, 1), (2, 12, 4, 5, 3)).copy()
            if restate == "numpy":
                out = BH.slice_numpy(grids, image, [1, 0])[0]
            else:
                out = BH.slice_torch(torch.from_numpy(grids), torch.from_numpy(image), [1, 0]).numpy()
            assert np.abs(out - want).max() <= 1e-14


def test_tv_on_a_hand_computed_example():
    """One 2 x 2 x 2 grid whose entry (k, z, y, x) is k + 4 z + 2 y + x: every z difference is 4, every y difference 2, every x
    difference 1, over 12 * 4 differenced elements each: tv = 16 + 4 + 1; two grids, the second constant: tv = 21 / 2."""
    k, z, y, x = np.meshgrid(np.arange(12), np.arange(2), np.arange(2), np.arange(2), indexing="ij")
    g = (k + 4 * z + 2 * y + x).astype(np.float64)[None]
    assert float(BH.tv_torch(torch.from_numpy(g))) == 21.0
    both = np.concatenate([g, np.full_like(g, 3.0)])
    assert float(BH.tv_torch(torch.from_numpy(both))) == 10.5
    # gradient: 2 / count_d * (difference terms) / N; the corner (z, y, x) = (0, 0, 0) has -4, -2, -1 as its forward differences
    t = torch.from_numpy(g).requires_grad_(True)
    BH.tv_torch(t).backward()
    assert abs(float(t.grad[0, 0, 0, 0, 0]) - 2.0 * (-4 - 2 - 1) / 48.0) <= 1e-15


@pytest.mark.parametrize("case", BH.CASES)
def test_no_pixel_is_near_a_discontinuity_and_both_clamps_are_hit(case):
    c = BH.make_case(case)
    GZ = c["grid"][2]
    assert int(BH.margin_violations(c["image"], GZ).sum()) == 0
    gray = BH.gray64(c["image"])
    assert c["image"].min() >= -0.2 and c["image"].max() <= 1.3 and c["image"].dtype == np.float32
    assert (gray < 0).mean() >= 0.05 and (gray > 1).mean() >= 0.05, (case, (gray < 0).mean(), (gray > 1).mean())
    assert c["grids"].shape == (3, 12) + c["grid"][::-1]


def test_header_declares_the_entry_points_and_the_binding_types_them():
    from gaussianeditor_amd import _native

    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", code), s
        assert s in _native.SIGNATURES and hasattr(lib, s), s
    assert "GSR_ABI_VERSION 6" in hdr and "clamp" in hdr.lower() and "grid_sample" in hdr
    # argument checks need no GPU: sizes out of range, NULL pointers
    L = _native.lib()
    n = ctypes.c_size_t(0)
    assert L.gsr_bilagrid_workspace_size(1, 1080, 1920, 16, 16, 8, ctypes.byref(n)) == 0 and n.value % (8 * 48 * 8) == 0 and n.value > 0
    for bad in ((1, 64, 64, 1, 16, 8), (1, 64, 64, 16, 33, 8), (1, 64, 64, 16, 16, 17), (0, 64, 64, 16, 16, 8), (1, 0, 64, 16, 16, 8)):
        assert L.gsr_bilagrid_workspace_size(*bad, ctypes.byref(n)) == -1, bad
    assert L.gsr_bilagrid_workspace_size(1, 64, 64, 16, 16, 8, None) == -1
    assert L.gsr_bilagrid_tv_workspace_size(3, 16, 16, 8, ctypes.byref(n)) == 0 and n.value == 8 * ((3 * 12 * 8 * 16 * 16 + 255) // 256)
    assert L.gsr_bilagrid_tv_workspace_size(0, 16, 16, 8, ctypes.byref(n)) == -1
    one = ctypes.c_void_p(256)
    assert L.gsr_bilagrid_slice_forward(None, 1, 64, 64, 3, 16, 16, 8, None, one, one, one) == -1
    assert L.gsr_bilagrid_slice_forward(None, 1, 64, 64, 3, 16, 16, 1, one, one, one, one) == -1
    assert L.gsr_bilagrid_slice_backward(None, 1, 64, 64, 3, 16, 16, 8, one, one, one, one, None, None, one) == -1  # no workspace
    assert L.gsr_bilagrid_slice_backward(None, 1, 64, 64, 0, 16, 16, 8, one, one, one, one, one, one, one) == -1
    assert L.gsr_bilagrid_tv_forward(None, 1, 16, 16, 8, one, None, one) == -1
    assert L.gsr_bilagrid_tv_backward(None, 1, 16, 16, 8, one, None, one) == -1


def test_refusals_are_named_and_need_no_gpu():
    from gaussianeditor_amd import bilagrid

    grids = torch.zeros(3, 12, 8, 16, 16)
    image = torch.zeros(3, 6, 7)
    for shape in ((3, 12, 8, 16, 33), (3, 12, 8, 1, 16), (3, 12, 17, 16, 16), (3, 12, 1, 16, 16)):
        with pytest.raises(ValueError, match="grid size"):
            bilagrid.slice_image(torch.zeros(shape), image, 0)
        with pytest.raises(ValueError, match="grid size"):
            bilagrid.total_variation_loss(torch.zeros(shape))
    for kw in (dict(grid_x=33), dict(grid_y=1), dict(grid_w=17)):
        with pytest.raises(ValueError, match="grid size"):
            bilagrid.BilateralGrid(2, **kw)
    with pytest.raises(ValueError, match="num_images"):
        bilagrid.BilateralGrid(0)
    with pytest.raises(RuntimeError, match="expected grids of shape"):
        bilagrid.slice_image(torch.zeros(3, 11, 8, 16, 16), image, 0)
    with pytest.raises(RuntimeError, match="image must be float32"):
        bilagrid.slice_image(grids, image.double(), 0)
    with pytest.raises(RuntimeError, match="grids must be float32"):
        bilagrid.slice_image(grids.double(), image, 0)
    with pytest.raises(RuntimeError, match=r"\(3,H,W\) or \(B,3,H,W\)"):
        bilagrid.slice_image(grids, torch.zeros(4, 6, 7), 0)
    for idx in (3, -1):
        with pytest.raises(IndexError, match="out of range for 3 grids"):
            bilagrid.slice_image(grids, image, idx)
    with pytest.raises(RuntimeError, match="one grid index per image"):
        bilagrid.slice_image(grids, torch.zeros(2, 3, 6, 7), torch.tensor([0, 1, 2]))
    with pytest.raises(RuntimeError, match="one grid index per image"):
        bilagrid.slice_image(grids, image, torch.tensor([0, 1]))
    with pytest.raises(RuntimeError, match="must be int64"):
        bilagrid.slice_image(grids, image, torch.tensor([0], dtype=torch.int32))
    with pytest.raises(TypeError, match="idx must be an int"):
        bilagrid.slice_image(grids, image, 0.0)
    # everything well-formed but on the CPU: refused, not emulated
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bilagrid.slice_image(grids, image, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bilagrid.total_variation_loss(grids)
    m = bilagrid.BilateralGrid(4, 5, 6, 3)
    assert tuple(m.grids.shape) == (4, 12, 3, 6, 5) and m.grids.requires_grad
    assert torch.equal(m.grids[2, :, 1, 4, 3].reshape(3, 4), torch.eye(3, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(image, 0)
