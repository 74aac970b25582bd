"""-m gpu: absolute screen-space gradients (opt-in, gaussianeditor_amd.set_abs_grad / options.FLAG_ABS_GRAD).

`means2D.absgrad` of the product against the per-pixel construction of abs_helpers (one oracle backward per pixel of a
block S, summed in absolute value; held to float64 autograd by tests/test_cpu_abs_grad.py) on small cases, on every route
of the backward (SHs, precomputed colours, precomputed covariance, with the depth loss) and with list segments forced; at
full size, where per-pixel oracle runs are too dear, by the properties that pin the definition -- the one-pixel identity and
additivity over a partition of the pixels -- and dominance over the signed gradient; the ordinary gradients and the
persistent accumulator table are what they are without the flag."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import abs_helpers as AB
from helpers import assert_grads_close, make_case, oracle_forward, seed_gradient

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = {"p2000": (dict(P=2000, W=64, H=64, s0=0.05), 8), "p20000": (dict(P=20000, W=248, H=232, s0=0.03), 12)}


def _small(name):
    kw, n = SMALL[name]
    case = make_case(kw["P"], kw["W"], kw["H"], s0=kw["s0"])
    H, W = case["H"], case["W"]
    pixels = AB.block_pixels(H, W, n)
    G = seed_gradient(H, W, 3) * H * W * AB.pixel_mask(H, W, pixels)
    return case, G, pixels


def _check_small(oracle, case, G, pixels, tag, GD=None, **kw):
    want, signed = AB.abs_expectation(oracle, case, G, pixels, GD=GD, **kw)
    AB.assert_discriminates(want, signed, tag=tag)
    grads, got = AB.run_hip(case, G, GD=GD, **kw)
    assert got is not None and got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    a, s = got[:, :2].astype(np.float64), np.abs(grads["dL_dmeans2D"][:, :2].astype(np.float64))
    print(f"  {tag}: max |absgrad - expectation| / max = {np.abs(got - want).max() / want.max():.2e}, "
          f"max |grad - signed sum| / max = {np.abs(grads['dL_dmeans2D'][:, :2] - signed).max() / np.abs(signed).max():.2e}")
    worst = assert_grads_close(dict(absgrad=got), dict(absgrad=want), tag=tag + ": absgrad vs per-pixel oracle")
    assert_grads_close(dict(signed=grads["dL_dmeans2D"][:, :2]), dict(signed=signed), tag=tag + ": means2D.grad vs oracle")
    assert (got[:, 2] == 0).all() and (a >= s - 1e-5 * a.max()).all()
    return worst


@pytest.mark.parametrize("name", list(SMALL))
def test_absgrad_vs_per_pixel_oracle(oracle, name):
    case, G, pixels = _small(name)
    _check_small(oracle, case, G, pixels, name)


def test_absgrad_vs_per_pixel_oracle_precomputed_colours(oracle):
    case, G, pixels = _small("p20000")
    cols = torch.rand(20000, 3, generator=torch.Generator().manual_seed(3))
    _check_small(oracle, case, G, pixels, "colors_precomp", colors_precomp=cols)


def test_absgrad_vs_per_pixel_oracle_precomputed_covariance(oracle):
    case, G, pixels = _small("p20000")
    cov = torch.from_numpy(oracle_forward(oracle, case)["cov3D"].copy())
    _check_small(oracle, case, G, pixels, "cov3D_precomp", cov3D_precomp=cov)


def test_absgrad_vs_per_pixel_oracle_with_the_depth_loss(oracle):
    """The per-pixel term then carries the depth image's share of dL/dalpha (expectation per pixel through
    depth_helpers.depth_expectation); the backward runs the DEPTH + ABS kernel and K8+K9 with the depth flag."""
    case, G, pixels = _small("p20000")
    H, W = case["H"], case["W"]
    GD = seed_gradient(H, W, 7)[:1] * H * W * AB.pixel_mask(H, W, pixels)
    want_c, _ = AB.abs_expectation(oracle, case, G, pixels)
    _check_small(oracle, case, G, pixels, "depth", GD=GD)
    want_d, _ = AB.abs_expectation(oracle, case, G, pixels, GD=GD)
    assert np.abs(want_d - want_c).max() > 1e-2 * want_c.max()  # (the depth share is really in the expectation)


def _long_list_case():
    """tools/fuzz_v2.py configuration 365 (tests/test_gpu_round5.py): 2 x 16 pixels, ONE tile with a list of 3 231 entries."""
    from helpers import v2_fuzz_case

    case, sm, D = v2_fuzz_case(365)
    H, W = case["H"], case["W"]
    return case, sm, D, seed_gradient(H, W, 365) * (H * W), [(y, x) for y in range(H) for x in range(W)]


def test_absgrad_on_a_long_list(oracle):
    case, sm, D, G, pixels = _long_list_case()
    f = oracle_forward(oracle, case, scale_modifier=sm)
    assert f["num_rendered"] > 2048 and f["ranges"].reshape(-1, 2).shape[0] == 1  # (one tile, long list)
    _check_small(oracle, case, G, pixels, "long list", D=D, scale_modifier=sm)


def test_absgrad_with_forced_list_segments():
    """The long-list comparison again in a fresh process with the backward cutting the tile's list into segments that start
    from the forward's checkpoints (GSR_BWD_SEG=1, a checkpoint every 256 list positions; tests/test_gpu_f64_regimes.py forces
    them the same way): the SEG + ABS kernel."""
    env = dict(os.environ, GSR_CK_CHUNKS="4", GSR_BWD_SEG="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "test_absgrad_on_a_long_list"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "1 passed" in p.stdout, p.stdout[-2000:]
    print(p.stdout[-600:])


# ---------------------------------------------------------------------------------------------------------------------
# full size: the headline view and the 512 x 512 edit-loop view (SPLIT items, half tiles and segments together)
FULL = {"headline": (1_000_000, 1920, 1080, 0.01), "edit512": (1_000_000, 512, 512, 0.01)}


def _full(name):
    P, W, H, s0 = FULL[name]
    case = make_case(P, W, H, seed=0, s0=s0, view=0, nviews=8)
    return case, seed_gradient(H, W, 0) * H * W


def _one_pixel(case, G):
    H, W = case["H"], case["W"]
    return G * AB.pixel_mask(H, W, [(H // 2, W // 2)])


def _checker(case, parity):
    H, W = case["H"], case["W"]
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return (((yy + xx) & 1) == parity).float()[None]


def _acc_tables_are_zero():
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    torch.cuda.synchronize()
    assert _C._ACC_TABLES, "the persistent accumulator table is not in use"
    return all(not bool(t.any()) for t in _C._ACC_TABLES.values())


def _properties(case, G, flags, tag):
    """(a) one-pixel identity, (b) additivity, (c) dominance -> the flagged full-G run (gradients, absgrad)."""
    # (a) with G non-zero at a single pixel every Gaussian has one term: absgrad == |grad|
    g1, a1 = AB.run_hip(case, _one_pixel(case, G), flags=flags)
    assert (np.abs(g1["dL_dmeans2D"]).max(axis=1) > 0).sum() > 0
    assert_grads_close(dict(absgrad=a1[:, :2]), dict(absgrad=np.abs(g1["dL_dmeans2D"][:, :2])), tag=tag + " (a) one pixel")
    # (b) absolute sums add over any partition of the pixels
    g, a = AB.run_hip(case, G, flags=flags)
    _, ae = AB.run_hip(case, G * _checker(case, 0), flags=flags)
    _, ao = AB.run_hip(case, G * _checker(case, 1), flags=flags)
    assert_grads_close(dict(absgrad=a), dict(absgrad=ae.astype(np.float64) + ao.astype(np.float64)), tag=tag + " (b) additivity")
    # (c) it dominates the signed gradient, and is not the signed gradient
    ab, sg = a[:, :2].astype(np.float64), np.abs(g["dL_dmeans2D"][:, :2].astype(np.float64))
    short = (sg - ab).max()
    print(f"  {tag}: max (|grad| - absgrad) / max absgrad = {short / ab.max():.2e}")
    assert short <= 1e-5 * ab.max(), (tag, short / ab.max())
    AB.assert_discriminates(a, g["dL_dmeans2D"], tag=tag + " (c) dominance")
    assert (a[:, 2] == 0).all() and np.isfinite(a).all()
    return g, a


@pytest.mark.parametrize("name", list(FULL))
def test_absgrad_properties_at_full_size(name, tmp_path):
    """(a) one-pixel identity and (b) additivity pin the definition, (c) dominance that it is not the signed sum; (d) the
    eight ordinary gradients of the flagged backward are those of the unflagged one; (e) the persistent accumulator table is
    all zero after the flagged backward, and a following unflagged backward is bit-identical to one in a fresh process.
    (e) uses the one-pixel gradient: every accumulator cell then receives at most one non-zero add, so the float atomics
    cannot re-associate and the backward is deterministic -- with a dense gradient two unflagged backwards of ONE process
    already differ in the last bits (test_gpu_parity.py::test_backward_run_to_run_spread), and no comparison could be
    bit-exact.  The dense gradient is compared as well, by the bars every gradient comparison here uses."""
    case, G = _full(name)
    g, a = _properties(case, G, 0, name)
    assert _acc_tables_are_zero()  # (e) -- columns GSR_ACC_ABS2D included: gsr_abs_grad_take took them out
    # (d)
    g0, none = AB.run_hip(case, G, abs_grad=False)
    assert none is None
    assert_grads_close(g, g0, tag=name + " (d) flagged vs unflagged gradients")
    # (e) a flagged backward, then unflagged ones: the same bits as in a process that never saw the flag
    G1 = _one_pixel(case, G)
    AB.run_hip(case, G, flags=0)
    assert _acc_tables_are_zero()
    after, _ = AB.run_hip(case, G1, abs_grad=False)
    after_dense, _ = AB.run_hip(case, G, abs_grad=False)
    out = str(tmp_path / "fresh.npz")
    code = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']; import numpy as np; import abs_helpers as AB; "
            "import test_gpu_abs_grad as T; case, G = T._full(sys.argv[2]); "
            "g1, _ = AB.run_hip(case, T._one_pixel(case, G), abs_grad=False); g, _ = AB.run_hip(case, G, abs_grad=False); "
            "np.savez(sys.argv[3], **{'one_' + k: v for k, v in g1.items()}, **{'dense_' + k: v for k, v in g.items()})")
    p = subprocess.run([sys.executable, "-c", code, ROOT, name, out], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    fresh = np.load(out)
    for k, v in after.items():
        assert np.array_equal(v.view(np.uint32), fresh["one_" + k].view(np.uint32)), (name, k, "not bit-identical")
    assert_grads_close(after_dense, {k: fresh["dense_" + k] for k in after_dense}, tag=name + " (e) dense, after vs fresh process")


@pytest.mark.parametrize("name", list(FULL))
def test_absgrad_properties_with_antialiasing_alpha_bounds_and_fast_exp(name):
    from gaussianeditor_amd import options

    case, G = _full(name)
    _properties(case, G, options.FLAG_ANTIALIAS | options.FLAG_TILE_BOUNDS_ALPHA | options.FLAG_FAST_EXP, name + " aa+alpha+fast")
    assert _acc_tables_are_zero()


def test_absgrad_through_render_twice_with_view_reuse(oracle):
    """The editor's double render of a view (render(), then render(override_color=...) served by the blend kernel alone) with
    a backward through each image: both screen-space tensors get their own `.absgrad`, the first the expected one."""
    import gaussianeditor_amd
    from gaussianeditor_amd.diff_gaussian_rasterization import _reuse
    from gaussianeditor_amd.gaussian_renderer import render
    from test_gpu_round6 import _PC, _Pipe

    case, G, pixels = _small("p20000")
    P = case["sc"]["xyz"].shape[0]
    # (_PC keeps opacity / scaling / rotation behind activations: the expectation is built on what render() really passes on)
    pc = _PC(case["sc"], DEV)
    with torch.no_grad():
        case["sc"] = dict(case["sc"], opacity=pc.get_opacity.cpu().contiguous(), scaling=pc.get_scaling.cpu().contiguous(),
                          rotation=pc.get_rotation.cpu().contiguous())
    want, signed = AB.abs_expectation(oracle, case, G, pixels)
    cam, bg = case["cam"], case["bg"].to(DEV)
    for k in ("world_view_transform", "full_proj_transform", "camera_center"):
        setattr(cam, k, getattr(cam, k).to(DEV))
    mask = (torch.rand(P, 1, generator=torch.Generator().manual_seed(1)) > 0.6).float().repeat(1, 3).to(DEV)
    was = gaussianeditor_amd.get_view_reuse()
    gaussianeditor_amd.set_view_reuse(True)
    _reuse.forget()
    hits = _reuse.stats["hits"]
    gaussianeditor_amd.set_abs_grad(True)
    try:
        a = render(cam, pc, _Pipe, bg)
        b = render(cam, pc, _Pipe, bg, override_color=mask)
        assert _reuse.stats["hits"] == hits + 1
        ((a["render"] * G.to(DEV)).sum() + (b["render"] * G.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
    finally:
        gaussianeditor_amd.set_abs_grad(False)
        gaussianeditor_amd.set_view_reuse(was)
        _reuse.forget()
    va, vb = a["viewspace_points"], b["viewspace_points"]
    assert va is not vb and va.absgrad.shape == (P, 3) and vb.absgrad.shape == (P, 3) and va.absgrad is not vb.absgrad
    # the first render is the case's own; the second adds nothing to the first's screen-space tensor
    assert_grads_close(dict(absgrad=va.absgrad.cpu().numpy()), dict(absgrad=want), tag="render(): absgrad vs per-pixel oracle")
    assert_grads_close(dict(signed=va.grad.cpu().numpy()[:, :2]), dict(signed=signed), tag="render(): means2D.grad vs oracle")
    for v in (va, vb):
        ab, sg = v.absgrad[:, :2].double(), v.grad[:, :2].double().abs()
        assert bool((ab >= sg - 1e-5 * ab.max()).all()) and float(ab.max()) > 0 and bool((v.absgrad[:, 2] == 0).all())
    AB.assert_discriminates(vb.absgrad.cpu().numpy(), vb.grad.cpu().numpy(), tag="override-colour render")
    # the editor's statistic, unchanged code: the norm of the first two columns, per view
    stat = torch.norm(va.absgrad[:, :2], dim=-1, keepdim=True)
    assert stat.shape == (P, 1) and bool((stat >= torch.norm(va.grad[:, :2], dim=-1, keepdim=True) * (1 - 1e-5)).all())
