"""GPU: the densification policy kernels (gsr_densify_*, gaussianeditor_amd/densify.py) against their
numpy float32 restatement (bit for bit) and against the reference's lines run by torch (tests/densify_helpers.py)."""
import numpy as np
import pytest
import torch

import densify_helpers as dh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------------------------------------------------
# statistics
# ----------------------------------------------------------------------------------------------------------------------
def _stats_inputs(P, V, seed):
    rng = np.random.default_rng(seed)
    radii = [np.where(rng.random(P) < 0.5, rng.integers(1, 40, P), rng.integers(-2, 1, P)).astype(np.int32) for _ in range(V)]
    if P > 4 and V > 1:  # rows visible in exactly one view
        for v in range(V):
            radii[v][v::7] = 0
        radii[V - 1][3::7] = 9
    vis = np.max(radii, axis=0) > 0
    grads = [(rng.standard_normal((P, 3)) * 1e-3).astype(np.float32) for _ in range(V)]
    for v, g in enumerate(grads):  # whatever an invisible row's gradient holds never enters
        g[~vis, 0] = np.nan
        g[~vis, 1] = np.inf if v % 2 else -np.inf
    return grads, radii, vis


def _stats_run(P, V):
    """Two consecutive calls from a state with sentinels on the invisible rows.  Yields per call (what the kernel left, the
    numpy restatement, what torch's own ops on the GPU give from the same state, the visible rows, the sentinels)."""
    from gaussianeditor_amd.densify import add_densification_stats

    rng = np.random.default_rng(P + V)
    accum = (rng.random(P) * 1e-2).astype(np.float32)
    denom = rng.integers(0, 5, P).astype(np.float32)
    maxr = rng.integers(0, 30, P).astype(np.float32)
    state_np = (accum, denom, maxr)
    state = [_dev(x) for x in state_np]
    for call in range(2):
        grads, radii, vis = _stats_inputs(P, V, 100 * P + 10 * V + call)
        sent = (np.float32(-123.25), np.float32(77.5), np.float32(-5.0))  # sentinels on the invisible rows
        for x, t, sv in zip(state_np, state, sent):
            x[~vis] = sv
            t[_dev(~vis)] = float(sv)
        before = [t.clone() for t in state]
        want = dh.stats_np(*state_np, grads, radii)
        g_dev, r_dev = [_dev(g) for g in grads], [_dev(r) for r in radii]
        add_densification_stats(*state, g_dev, r_dev)
        torch.cuda.synchronize()
        ta, td, tr = before[0][:, None].clone(), before[1][:, None].clone(), before[2].clone()
        dh.stats_torch(ta, td, tr, g_dev, r_dev)  # torch's own ops on the GPU, from the same state
        yield call, [t.cpu().numpy() for t in state], want, (ta[:, 0].cpu().numpy(), td[:, 0].cpu().numpy(), tr.cpu().numpy()), vis, sent
        state_np = tuple(x.copy() for x in want[:3])


@pytest.mark.parametrize("V", (1, 3))
@pytest.mark.parametrize("P", dh.PS)
def test_stats_bit_equal_and_invisible_rows_untouched(P, V):
    for call, got, want, _, vis, sent in _stats_run(P, V):
        for name, g, w, sv in zip(("accum", "denom", "max_radii2D"), got, want[:3], sent):
            assert np.array_equal(_bits(g), _bits(w)), (name, P, V, call)
            assert np.array_equal(_bits(g[~vis]), _bits(np.full(int((~vis).sum()), sv))), (name, P, V, call)


@pytest.mark.parametrize("V", (1, 3))
@pytest.mark.parametrize("P", dh.PS)
def test_stats_within_the_bound_of_torch_ops(P, V):
    """Against torch's own ops on the GPU (they may fuse the sum of squares) every new accum lies within
    3 * 2^-24 * norm + 2^-24 * |accum|; denom and max_radii2D are equal.

    Measured on the MI355X: torch's GPU ops give the kernel's bits on every row of every case (ratio 0).  The bound has no
    room for a norm that differs in its last bit -- two correctly rounded sums accum + norm can then lie a whole ulp of accum
    apart, up to 2 * 2^-24 * |accum|; torch's CPU ops, which fuse differently, reach 1.76 of it against the exact
    restatement at P = 70 001 -- so a torch build that fuses the sum of squares on the GPU could miss it with no fault here."""
    for call, got, want, tor, vis, _ in _stats_run(P, V):
        err = np.abs(got[0].astype(np.float64) - tor[0].astype(np.float64))
        bound = 3 * U * want[3].astype(np.float64) + U * np.abs(want[0].astype(np.float64))
        ratio = float((err[vis] / np.maximum(bound[vis], 1e-300)).max()) if vis.any() else 0.0
        print(f"stats P={P} V={V} call {call}: max |accum - torch| / bound = {ratio:.4f}, rows that differ {int((err[vis] > 0).sum())}")
        assert (err[vis] <= bound[vis]).all(), (P, V, call, ratio)
        assert np.array_equal(got[1], tor[1]) and np.array_equal(got[2], tor[2])


def test_stats_wrapper_never_synchronises():
    from gaussianeditor_amd.densify import add_densification_stats

    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available")
    P = 257
    grads, radii, _ = _stats_inputs(P, 3, 5)
    state = [torch.zeros(P, device=DEV) for _ in range(3)]
    g_dev, r_dev = [_dev(g) for g in grads], [_dev(r) for r in radii]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        add_densification_stats(*state, g_dev, r_dev)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert float(state[1].sum()) > 0
    with pytest.raises(ValueError):
        add_densification_stats(*state, g_dev * 3, r_dev * 3)


# ----------------------------------------------------------------------------------------------------------------------
# selection
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", dh.PS)
def test_select_equals_the_reference_lines(P):
    from gaussianeditor_amd.densify import select_densification

    n_sel = 0
    for kind in dh.KINDS:
        accum, denom, mask, scaling = dh.select_case(P, kind)
        dev = [_dev(accum), _dev(denom), _dev(mask), _dev(scaling)]
        for pct in dh.PERCENTS:
            kw = dict(max_grad=dh.MAX_GRAD, max_densify_percent=pct, percent_dense=dh.PERCENT_DENSE, extent=dh.EXTENT)
            got = select_densification(*dev, **kw)
            want = dh.select_torch(torch.from_numpy(accum.copy())[:, None], torch.from_numpy(denom.copy())[:, None],
                                   torch.from_numpy(mask.copy()), torch.from_numpy(scaling.copy()), dh.MAX_GRAD, pct,
                                   dh.PERCENT_DENSE, dh.EXTENT)
            tag = (P, kind, pct)
            assert got.clone_sel.dtype == torch.bool and got.split_sel.dtype == torch.bool
            assert torch.equal(got.clone_sel.cpu(), want[0]) and torch.equal(got.split_sel.cpu(), want[1]), tag
            assert (got.nonzero, got.n_clone, got.n_split) == want[2:5], tag
            if pct < 1:
                assert dh.same_value(got.threshold, want[5]), (tag, got.threshold, float(want[5]))
            else:
                assert got.threshold == 0.0
            again = select_densification(*dev, **kw)  # integer atomics only: the same bits on every run
            assert torch.equal(again.clone_sel, got.clone_sel) and torch.equal(again.split_sel, got.split_sel), tag
            assert np.float32(again.threshold).tobytes() == np.float32(got.threshold).tobytes() or got.threshold != got.threshold
            assert (again.nonzero, again.n_clone, again.n_split) == (got.nonzero, got.n_clone, got.n_split)
            n_sel += got.n_clone + got.n_split
    assert P < 255 or n_sel > 0


# ----------------------------------------------------------------------------------------------------------------------
# split positions
# ----------------------------------------------------------------------------------------------------------------------
_WORST_SPLIT = [0.0]


@pytest.mark.parametrize("N", (1, 2, 3))
@pytest.mark.parametrize("n_split", (0, 1, 300))
def test_split_positions(n_split, N):
    from gaussianeditor_amd.densify import split_positions

    P = 2500  # three 1024-row blocks, the last one ragged
    rng = np.random.default_rng(10 * n_split + N)
    xyz = (rng.standard_normal((P, 3)) * 3).astype(np.float32)
    scaling = np.exp(rng.uniform(-6, -1, (P, 3))).astype(np.float32)
    rot = rng.standard_normal((P, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(0.1), np.log(10), (P, 1)))).astype(np.float32)
    sel = np.zeros(P, bool)
    if n_split:
        sel[rng.choice(P - 1, n_split - 1, replace=False)] = True
        sel[P - 1] = True  # the last row of the ragged block
    noise = rng.standard_normal((N * n_split, 3)).astype(np.float32)
    want, l1, pxyz = dh.split_np(xyz, scaling, rot, sel, noise, N)
    got_t = split_positions(_dev(xyz), _dev(scaling), _dev(rot), _dev(sel), _dev(noise), N)
    got = got_t.cpu().numpy()
    assert got.shape == (N * n_split, 3) and np.array_equal(_bits(got), _bits(want))
    if n_split == 0:
        return
    ref64, _, _ = dh.split_np(xyz, scaling, rot, sel, noise, N, dtype=np.float64)
    bound = dh.split_bound(l1, pxyz)
    ratio = np.abs(got.astype(np.float64) - ref64) / bound
    _WORST_SPLIT[0] = max(_WORST_SPLIT[0], float(ratio.max()))
    print(f"split_xyz n_split={n_split} N={N}: max |error| / bound = {ratio.max():.4f} (worst so far {_WORST_SPLIT[0]:.4f})")
    assert (ratio <= 1.0).all(), float(ratio.max())
    bmm = dh.split_torch(_dev(xyz), _dev(scaling), _dev(rot), _dev(sel), _dev(noise), N).cpu().numpy()
    assert (np.abs(got.astype(np.float64) - bmm.astype(np.float64)) <= 2 * bound).all()


# ----------------------------------------------------------------------------------------------------------------------
# prune mask
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_drop", (False, True))
@pytest.mark.parametrize("with_radii", (False, True))
def test_keep_mask(with_radii, with_drop):
    from gaussianeditor_amd.densify import prune_keep_mask

    P, min_opacity, max_screen, extent = 70001, 0.005, 20, dh.EXTENT
    rng = np.random.default_rng(3)
    opacity = rng.random(P).astype(np.float32) * np.float32(0.02)
    opacity[::9] = np.float32(min_opacity)                       # == (float)min_opacity: kept
    opacity[1::9] = np.nextafter(np.float32(min_opacity), np.float32(0))
    big = np.float32(0.1 * extent)
    scaling = (float(big) * rng.uniform(0.2, 0.99, (P, 3))).astype(np.float32)
    scaling[::13, 1] = big                                       # == (float)(0.1 * extent): kept
    scaling[2::13, 2] = np.nextafter(big, np.float32(1))
    mask = rng.random(P) < 0.6
    radii = rng.integers(0, 40, P).astype(np.float32)
    radii[::17] = np.float32(max_screen)                         # == max_screen_size: kept
    drop = rng.random(P) < 0.1
    want = dh.keep_np(opacity, scaling, mask, min_opacity, max_screen, extent, radii if with_radii else None,
                      drop if with_drop else None)
    want_t = dh.keep_torch(torch.from_numpy(opacity)[:, None], torch.from_numpy(scaling), torch.from_numpy(mask), min_opacity,
                           max_screen, extent, torch.from_numpy(radii) if with_radii else None,
                           torch.from_numpy(drop) if with_drop else None)
    assert np.array_equal(want, want_t.numpy())
    got = prune_keep_mask(_dev(opacity), _dev(scaling), _dev(mask), min_opacity=min_opacity, max_screen_size=max_screen,
                          extent=extent, max_radii2D=_dev(radii) if with_radii else None, drop=_dev(drop) if with_drop else None)
    got = got.cpu().numpy()
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    alive = ~drop if with_drop else np.ones(P, bool)
    assert got[~mask & alive].all()                               # unmasked rows are never pruned
    at = (opacity == np.float32(min_opacity)) & (scaling.max(axis=1) <= big) & alive
    if with_radii:
        at &= radii <= max_screen
    assert at.any() and got[at].all()
    assert not got[mask & (opacity < np.float32(min_opacity))].any()


# ----------------------------------------------------------------------------------------------------------------------
# the whole of densify_and_prune
# ----------------------------------------------------------------------------------------------------------------------
def _composite_setup():
    from helpers import make_case

    sc = make_case(3000, 64, 64, seed=11, s0=0.03)["sc"]
    sc["opacity"][::50] = 0.006
    d = lambda t: t.to(DEV).clone().contiguous()  # noqa: E731
    f = d(sc["features"])
    par = dict(xyz=d(sc["xyz"]), f_dc=f[:, :1].contiguous(), f_rest=f[:, 1:].contiguous(), opacity=torch.logit(d(sc["opacity"])),
               scaling=torch.log(d(sc["scaling"])), rotation=d(sc["rotation"]) * 1.7)
    par = {k: torch.nn.Parameter(v.reshape(v.shape[0], -1) if k == "opacity" else v) for k, v in par.items()}
    opt = torch.optim.Adam([dict(params=[par[k]], lr=1e-4, name=k) for k in dh.NAMES], lr=0.0, eps=1e-15)
    g = torch.Generator(device=DEV).manual_seed(3)
    for _ in range(2):  # non-zero moments
        for p in par.values():
            p.grad = torch.randn(p.shape, device=DEV, generator=g) * 1e-3
        opt.step()
    opt.zero_grad(set_to_none=True)
    return opt, g


def _gather_stats(extra, P, g, calls=3):
    from gaussianeditor_amd.densify import add_densification_stats

    for _ in range(calls):
        grads = [torch.randn((P, 3), device=DEV, generator=g) * 4e-4 for _ in range(2)]
        radii = [torch.randint(-1, 30, (P,), device=DEV, generator=g, dtype=torch.int32) for _ in range(2)]
        add_densification_stats(extra["xyz_gradient_accum"], extra["denom"], extra["max_radii2D"], grads, radii)


def _fresh_extra(P, g):
    return dict(xyz_gradient_accum=torch.zeros((P, 1), device=DEV), denom=torch.zeros((P, 1), device=DEV),
                max_radii2D=torch.zeros((P,), device=DEV), mask=torch.rand(P, device=DEV, generator=g) < 0.5,
                generation=torch.zeros(P, dtype=torch.int64, device=DEV))


def _densify_round(opt, extra, g, rnd, max_screen_size=20, screen_prune="reference"):
    """Statistics from three calls, then densify_and_prune on the optimizer against the restated reference lines from the
    same state and the same torch.randn draw.  Returns (the new extra, the counts)."""
    from gaussianeditor_amd.densify import densify_and_prune

    P = int(opt.param_groups[0]["params"][0].shape[0])
    _gather_stats(extra, P, g)
    par = {gr["name"]: gr["params"][0].detach() for gr in opt.param_groups}
    moments = {gr["name"]: (opt.state[gr["params"][0]]["exp_avg"], opt.state[gr["params"][0]]["exp_avg_sq"]) for gr in opt.param_groups}
    smax = torch.exp(par["scaling"]).max(dim=1).values
    kw = dict(max_grad=dh.MAX_GRAD, max_densify_percent=0.3, min_opacity=0.02, extent=dh.EXTENT, max_screen_size=max_screen_size,
              percent_dense=float(smax.median()) / dh.EXTENT, N=2, generation_num=rnd + 1, screen_prune=screen_prune)
    ref_gen = torch.Generator(device=DEV).manual_seed(1234 + rnd)
    want_par, want_mom, want_extra, want_counts = dh.densify_and_prune_torch(
        par, moments, extra, lambda n: torch.randn((n, 3), dtype=torch.float32, device=DEV, generator=ref_gen), **kw)
    new_par, extra, counts = densify_and_prune(opt, extra, generator=torch.Generator(device=DEV).manual_seed(1234 + rnd), **kw)
    print(f"densify_and_prune round {rnd} ({screen_prune}, max_screen_size={max_screen_size}): (before, n_clone, n_split, "
          f"n_pruned) = {counts}")
    assert counts == want_counts and min(counts[:3]) > 0
    final = counts[0] + counts[1] + counts[2] * (kw["N"] - 1) - counts[3]
    bound = want_extra["xyz_bound"]
    child = bound[:, 0] > 0
    assert int(child.sum()) > 0
    for k in dh.NAMES:
        p = opt.param_groups[dh.NAMES.index(k)]["params"][0]
        assert p is new_par[k] and p.requires_grad and p.shape == want_par[k].shape and p.shape[0] == final
        if k == "xyz":
            assert torch.equal(p.detach()[~child], want_par[k][~child])
            # the children: within the split bound of the float64 evaluation from the same float32 inputs, and within
            # twice the bound of the reference's own bmm route (both sides err)
            err = (p.detach().double() - want_extra["xyz64"]).abs()
            ratio = float((err[child] / bound[child]).max())
            err_bmm = (p.detach().double() - want_par[k].double()).abs()
            ratio_bmm = float((err_bmm[child] / bound[child]).max())
            print(f"  children's xyz: max |error| / bound = {ratio:.4f} against float64, {ratio_bmm:.4f} against the bmm route")
            assert ratio <= 1.0, ratio
            assert ratio_bmm <= 2.0, ratio_bmm
        else:
            assert torch.equal(p.detach(), want_par[k]), k  # (the children's scaling included)
        st = opt.state[p]
        assert torch.equal(st["exp_avg"], want_mom[k][0]) and torch.equal(st["exp_avg_sq"], want_mom[k][1]), k
    assert extra["mask"].dtype == torch.bool and torch.equal(extra["mask"], want_extra["mask"])
    assert torch.equal(extra["generation"], want_extra["generation"]) and int((extra["generation"] == rnd + 1).sum()) > 0
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert extra[k].shape == want_extra[k].shape and not bool(extra[k].any()), k
    return extra, counts


def test_densify_and_prune_equals_the_reference_lines():
    opt, g = _composite_setup()
    extra = _fresh_extra(int(opt.param_groups[0]["params"][0].shape[0]), g)
    extra, counts = _densify_round(opt, extra, g, 0)
    assert counts[3] > 0
    _densify_round(opt, extra, g, 1)  # a second densification on the result, after more statistics


def test_densify_and_prune_screen_size_variants():
    """screen_prune="accumulated" tests the max_radii2D gathered since the last densification (padded with zeros for the new
    rows) and prunes more than the reference's zeroed radii; a false max_screen_size switches the screen AND the world size
    terms off, as the reference's `if max_screen_size:` does, and prunes less."""
    pruned = {}
    for key, (mss, mode) in dict(reference=(20, "reference"), accumulated=(20, "accumulated"), none=(None, "reference"),
                                 zero=(0, "accumulated")).items():
        opt, g = _composite_setup()
        extra = _fresh_extra(int(opt.param_groups[0]["params"][0].shape[0]), g)
        pruned[key] = _densify_round(opt, extra, g, 0, max_screen_size=mss, screen_prune=mode)[1][3]
    assert pruned["accumulated"] > pruned["reference"] >= pruned["none"] == pruned["zero"] > 0
