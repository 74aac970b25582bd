"""GPU: size-independent properties of the path at BASELINE.json's FULL size (1 M Gaussians, 1920x1080), where the scalar
oracle would take minutes -- they need no second implementation:

  * the sorted instance list: keys (tile << 32 | depth bits, rasterizer_impl.cu:67-100) non-decreasing, equal keys in
    ascending Gaussian index (the stable sort of instances emitted in index order, :253-261), every tile's range the run of
    its key, the ranges a partition of [0, R), R = sum of tiles_touched, every listed Gaussian visible;
  * determinism: a second forward leaves bit-identical images, depths, radii, final_T, n_contrib, lists;
  * the background enters linearly: render(bg) - render(0) = final_T * bg (forward.cu:371-378);
  * the backward is linear in dL/dpixel (backward.cu:399-557 has no term of second order in it);
  * transmittance: final_T in (0, 1], n_contrib <= the tile's list length, pixels nothing reaches hold T = 1 and the background.

The three-way parity tests against the reference's own kernels run at this size too (test_gpu_reference.py); these are the
checks that would still hold a future kernel to the domain's invariants if the reference binaries were not at hand."""
import numpy as np
import pytest
import torch

from helpers import hip_state, make_case, seed_gradient, settings
from sort_matrix_helpers import assert_sorted_list_invariants

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, W, H = 1_000_000, 1920, 1080


@pytest.fixture(scope="module")
def full_case():
    return make_case(P, W, H, seed=0, s0=0.01, nviews=8, bg=(0.1, 0.2, 0.3))


def _forward(case, bg=None):
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    sc, cam = case["sc"], case["cam"]
    e = torch.empty(0, device=DEV)
    d = lambda t: t.to(DEV)  # noqa: E731
    bg_t = d(case["bg"] if bg is None else torch.tensor(bg, dtype=torch.float32))
    return _C.rasterize_gaussians(bg_t, d(sc["xyz"]), e, d(sc["opacity"]), d(sc["scaling"]), d(sc["rotation"]), 1.0, e,
                                  d(cam.world_view_transform), d(cam.full_proj_transform), case["tfx"], case["tfy"], H, W,
                                  d(sc["features"]), 3, d(cam.camera_center), False, False)


def test_full_size_sorted_list_invariants(full_case):
    R, color, depth, radii, geom, binning, img = _forward(full_case)
    st = hip_state(P, R, W, H, geom, binning, img)
    tt = st["tiles_touched"]
    assert R == int(tt.astype(np.int64).sum()) and R > 4_000_000
    # (sorted by (tile, depth bits), ties in ascending Gaussian index, the ranges the runs of the tile ids and a partition of
    #  [0, R), the depth bits the Gaussian's depth: shared with tests/test_gpu_sort_matrix.py)
    counts = assert_sorted_list_invariants(st, R, radii.cpu().numpy())
    # per pixel: the walk never goes past its tile's list; transmittance is a product of factors in (0.01, 1]
    ncon = st["n_contrib"].reshape(H, W).astype(np.int64)
    fT = st["final_T"].reshape(H, W)
    gx = (W + 15) // 16
    ty, tx = np.meshgrid(np.arange(H) // 16, np.arange(W) // 16, indexing="ij")
    assert (ncon <= counts[ty * gx + tx]).all()
    assert (fT > 0).all() and (fT <= 1).all() and (fT[ncon == 0] == 1).all()
    img_np = color.cpu().numpy()
    untouched = counts[ty * gx + tx] == 0
    assert untouched.any()
    for c in range(3):
        assert (img_np[c][untouched] == np.float32(full_case["bg"][c])).all()
    assert (depth.cpu().numpy()[0][untouched] == 0).all()


def test_full_size_forward_is_deterministic(full_case):
    a = _forward(full_case)
    sa = hip_state(P, a[0], W, H, a[4], a[5], a[6])
    ca, da, ra = a[1].clone(), a[2].clone(), a[3].clone()
    b = _forward(full_case)
    sb = hip_state(P, b[0], W, H, b[4], b[5], b[6])
    assert a[0] == b[0] and torch.equal(ca, b[1]) and torch.equal(da, b[2]) and torch.equal(ra, b[3])
    for k in ("keys", "point_list", "ranges", "n_contrib", "final_T", "tiles_touched", "means2D", "conic_opacity", "rgb"):
        assert np.array_equal(sa[k].view(np.uint8), sb[k].view(np.uint8)), k


def test_full_size_background_enters_linearly(full_case):
    R0, c0, d0, _, g0, b0, i0 = _forward(full_case, bg=(0.0, 0.0, 0.0))
    s0 = hip_state(P, R0, W, H, g0, b0, i0)
    c0 = c0.clone()
    bg = (0.7, 0.25, 0.9)
    R1, c1, d1, _, g1, b1, i1 = _forward(full_case, bg=bg)
    assert R0 == R1 and torch.equal(d0, d1)  # (depth has no background term, forward.cu:377)
    fT = torch.from_numpy(s0["final_T"].reshape(H, W)).to(DEV)
    for c in range(3):
        # out = C + T * bg, one fused multiply-add on the accumulated colour: against C + T * bg in two roundings <= 1 ulp of the sum
        want = c0[c] + fT * bg[c]
        assert (c1[c] - want).abs().max().item() <= 1.2e-7 * max(1.0, want.abs().max().item())


def test_full_size_backward_is_linear_in_the_pixel_gradient(full_case):
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

    sc = full_case["sc"]
    rs = settings(full_case, DEV)
    G1 = seed_gradient(H, W, 1).to(DEV)
    G2 = seed_gradient(H, W, 2).to(DEV)

    def grads(G):
        leaves = [sc[k].to(DEV).requires_grad_(True) for k in ("xyz", "features", "opacity", "scaling", "rotation")]
        m3, sh, op, s_, rot = leaves
        m2 = torch.zeros_like(m3, requires_grad=True)
        color, radii, depth = GaussianRasterizer(rs)(m3, m2, op, shs=sh, scales=s_, rotations=rot)
        return [g.clone() for g in torch.autograd.grad([color], leaves + [m2], grad_outputs=[G])]

    a, b = 0.75, -1.5
    g1, g2, g12 = grads(G1), grads(G2), grads(a * G1 + b * G2)
    for name, x1, x2, x12 in zip(("means3D", "sh", "opacity", "scales", "rotations", "means2D"), g1, g2, g12):
        want = a * x1.double() + b * x2.double()
        scale = max(want.abs().max().item(), 1e-30)
        err = (x12.double() - want).abs().max().item() / scale
        # float atomics in a different order per run + one rounding of the combined pixel gradient: far inside the 1e-5 bar
        assert err <= 5e-6, (name, err)
        assert want.abs().max().item() > 0, name
