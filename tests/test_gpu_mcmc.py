"""GPU: the 3DGS-MCMC kernels (gsr_mcmc_*, gaussianeditor_amd/mcmc.py) against the restatements of
tests/mcmc_helpers.py: the draws bit for bit against Python integers, the relocation values within one float32 ulp of
numpy float64, the noise within one ulp of the float64 evaluation, the composite against torch ops, and the version
counters in the sequences of tests/test_gpu_native_writes.py."""
import functools

import numpy as np
import pytest
import torch

import mcmc_helpers as mh
from helpers import make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
MIN_OPACITY = 0.005
U_MAX = F(1 - 2.0 ** -24)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _within_one_ulp(got, want64):
    """|got - want| <= one float32 ulp of the float64 value rounded to float32; returns the worst error in ulps."""
    want32 = want64.astype(F)
    ulp = np.spacing(np.abs(want32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want32.astype(np.float64)) / ulp
    return float(err.max()) if err.size else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# sampling
# ----------------------------------------------------------------------------------------------------------------------
def _sample_case(P, seed):
    rng = np.random.default_rng(seed)
    opacity = rng.random(P).astype(F)
    opacity[rng.random(P) < 0.2] = F(0.001)
    mask = rng.random(P) < 0.8
    if P > 16:
        opacity[3] = F(MIN_OPACITY)   # exactly at the threshold: dead
        opacity[4] = np.nextafter(F(MIN_OPACITY), F(1))
        opacity[9] = np.nan           # neither dead nor alive
        opacity[11] = F(1.0)
        mask[[3, 4, 9, 11]] = True
    return opacity, mask


def _run_sample(opacity, u, mask, n_draws):
    from gaussianeditor_amd.mcmc import classify_and_sample

    s = classify_and_sample(_dev(opacity), _dev(u), min_opacity=MIN_OPACITY, mask=None if mask is None else _dev(mask), n_draws=n_draws)
    return dict(dead_sel=_np(s.dead_sel), dead_idx=_np(s.dead_idx)[:s.n_dead], src=_np(s.src), count=_np(s.count), ratio=_np(s.ratio),
                record=(s.n_dead, s.n_alive, s.n_draws, s.total))


def _assert_sample_equal(got, want):
    assert got["record"] == want["record"], (got["record"], want["record"])
    for k in ("dead_sel", "dead_idx", "src", "count", "ratio"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("P", mh.PS)
def test_sampling_is_bit_equal_to_the_integer_restatement(P):
    opacity, mask = _sample_case(P, 100 + P)
    rng = np.random.default_rng(P)
    for with_mask in (True, False):
        m = mask if with_mask else None
        # relocation: one draw per dead row out of P uniform numbers, the two ends of u first
        u = rng.random(P).astype(F)
        u[u >= 1] = U_MAX
        u[0] = 0
        u[-1] = U_MAX
        got = _run_sample(opacity, u, m, None)
        _assert_sample_equal(got, mh.sample_int(opacity, u, MIN_OPACITY, m, None))
        again = _run_sample(opacity, u, m, None)  # the same bits on a second call
        _assert_sample_equal(again, got)
        # growth: a given number of draws
        n = max(3, P // 20)
        u = np.concatenate(([F(0), U_MAX], np.minimum(rng.random(n - 2).astype(F), U_MAX))).astype(F)
        got = _run_sample(opacity, u, m, n)
        want = mh.sample_int(opacity, u, MIN_OPACITY, m, n)
        _assert_sample_equal(got, want)
        if want["record"][3] > 0:
            alive = np.flatnonzero((np.ones(P, bool) if m is None else m) & (opacity > F(MIN_OPACITY)))
            assert got["src"][0] == alive[0] and got["src"][1] == alive[-1]  # u = 0 and the largest u


def test_sampling_edge_cases():
    P = 301
    u = np.minimum(np.random.default_rng(1).random(P).astype(F), U_MAX)
    half = np.where(np.arange(P) % 2 == 0, F(0.6), F(0.3)).astype(F)
    # none dead; all dead (total == 0 with draws requested, in both modes); an all-False mask
    for opacity, mask, n_draws, record in ((half, None, None, (0, P, 0, None)),
                                           (np.full(P, 0.001, F), None, None, (P, 0, P, 0)),
                                           (np.full(P, 0.001, F), None, 40, (P, 0, 40, 0)),
                                           (half, np.zeros(P, bool), 40, (0, 0, 40, 0))):
        got = _run_sample(opacity, u, mask, n_draws)
        want = mh.sample_int(opacity, u, MIN_OPACITY, mask, n_draws)
        _assert_sample_equal(got, want)
        assert got["record"][:3] == record[:3] and (record[3] is None or got["record"][3] == record[3])
        if got["record"][3] == 0:
            assert (got["src"] == -1).all() and not got["ratio"].any() and not got["count"].any()
    # one alive row among 300 dead: every draw hits it and the ratio caps at 51
    opacity = np.full(P, 0.001, F)
    opacity[123] = F(0.8)
    got = _run_sample(opacity, u, None, None)
    _assert_sample_equal(got, mh.sample_int(opacity, u, MIN_OPACITY, None, None))
    assert got["record"][:3] == (300, 1, 300) and (got["src"][:300] == 123).all() and got["src"][300] == -1
    assert got["count"][123] == 300 and (got["ratio"][:300] == 51).all() and got["ratio"][300] == 0
    # an empty scene and no draws
    from gaussianeditor_amd.mcmc import classify_and_sample

    s = classify_and_sample(torch.zeros(0, device=DEV), torch.zeros(5, device=DEV))
    assert (s.n_dead, s.n_alive, s.n_draws, s.total) == (0, 0, 0, 0) and s.src.tolist() == [-1] * 5
    s = classify_and_sample(_dev(half), torch.zeros(0, device=DEV), n_draws=0)
    assert (s.n_dead, s.n_alive, s.n_draws) == (0, P, 0) and s.total > 0


# ----------------------------------------------------------------------------------------------------------------------
# relocation values
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [257, 70001])
def test_relocation_values_within_one_ulp_of_float64(P):
    from gaussianeditor_amd.mcmc import relocation_values

    rng = np.random.default_rng(P)
    opacity, mask = _sample_case(P, 7 + P)
    opacity[20:40] = np.linspace(0.9, 1.0, 20).astype(F)
    opacity[40] = U_MAX
    scaling_raw = (np.log(0.02) + 0.5 * rng.standard_normal((P, 3))).astype(F)
    n = min(P, 4000)
    src = rng.integers(0, P, n).astype(np.int32)
    src[:41] = np.arange(41)
    src[-3:] = -1                                    # no draw: zeros
    ratio = rng.integers(1, 52, n).astype(np.int32)
    ratio[:60] = np.arange(60) % 51 + 1
    ratio[60:64] = [60, 0, 51, 1]                     # beyond the cap and below 1: clamped to 1..51
    opacity[src[src >= 0]] = np.where(np.isnan(opacity[src[src >= 0]]), F(0.3), opacity[src[src >= 0]])
    new_o, new_s = relocation_values(_dev(opacity), _dev(scaling_raw), _dev(src), _dev(ratio), min_opacity=MIN_OPACITY)
    want_o, want_s = mh.relocation_values_f64(opacity, scaling_raw, src, ratio, MIN_OPACITY)
    assert new_o.shape == (n, 1) and new_s.shape == (n, 3) and new_o.dtype == new_s.dtype == torch.float32
    worst = max(_within_one_ulp(_np(new_o).reshape(-1), want_o), _within_one_ulp(_np(new_s), want_s))
    print(f"P = {P}: relocation values, worst error against float64 rounded to float32: {worst:.2f} ulp")
    assert np.isfinite(_np(new_o)).all() and np.isfinite(_np(new_s)).all() and worst <= 1.0
    assert not _np(new_o)[-3:].any() and not _np(new_s)[-3:].any()


def _optimizer(par, moments=True, seed=3):
    par = {k: torch.nn.Parameter(v.clone()) for k, v in par.items()}
    opt = torch.optim.Adam([dict(params=[par[k]], lr=1e-4, name=k) for k in mh.NAMES], lr=0.0, eps=1e-15)
    if moments:
        g = torch.Generator(device=DEV).manual_seed(seed)
        for _ in range(2):  # non-zero moments
            for p in par.values():
                p.grad = torch.randn(p.shape, device=DEV, generator=g) * 1e-3
            opt.step()
        opt.zero_grad(set_to_none=True)
    return opt


def _scene_par(P, seed, dead_every=None, s0=0.03):
    sc = make_case(P, 64, 64, seed=seed, s0=s0)["sc"]
    d = lambda t: t.to(DEV).clone().contiguous()  # noqa: E731
    f = d(sc["features"])
    opacity = d(sc["opacity"]).reshape(-1, 1).clamp(0.01, 0.99)
    if dead_every:
        opacity[::dead_every] = 0.003
    return dict(xyz=d(sc["xyz"]), f_dc=f[:, :1].contiguous(), f_rest=f[:, 1:].contiguous(), opacity=torch.logit(opacity),
                scaling=torch.log(d(sc["scaling"])), rotation=d(sc["rotation"]) * 1.7)


def _state(opt):
    par = {g["name"]: g["params"][0].detach() for g in opt.param_groups}
    mom = {g["name"]: (opt.state[g["params"][0]]["exp_avg"], opt.state[g["params"][0]]["exp_avg_sq"]) for g in opt.param_groups}
    return par, mom


def test_one_source_many_draws_reads_only_old_values():
    """One alive row among 300 dead ones: 300 draws of the same source.  Every dead row and the source itself must end with
    the value computed from the source's OLD opacity and scale at ratio 51; a kernel that read the source after one of the
    draws had written it would compound the correction."""
    from gaussianeditor_amd.mcmc import classify_and_sample, relocate, relocation_values

    P, alive = 301, 123
    par = _scene_par(P, 21)
    par["opacity"][:] = -6.0          # sigmoid = 0.0025: dead
    par["opacity"][alive] = 1.2
    opt = _optimizer(par)
    old_par, old_mom = ({k: v.clone() for k, v in _state(opt)[0].items()}, {k: (a.clone(), b.clone()) for k, (a, b) in _state(opt)[1].items()})
    opacity = torch.sigmoid(old_par["opacity"]).reshape(-1)
    u = torch.rand(P, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    s = classify_and_sample(opacity, u, min_opacity=MIN_OPACITY)
    assert (s.n_dead, s.n_alive, s.n_draws) == (300, 1, 300)
    src, ratio, dead = s.src[:300], s.ratio[:300], s.dead_idx[:300]
    new_o, new_s = relocation_values(opacity, old_par["scaling"], src, ratio, min_opacity=MIN_OPACITY)
    want_o, want_s = mh.relocation_values_f64(_np(opacity), _np(old_par["scaling"]), _np(src), _np(ratio), MIN_OPACITY)
    assert _within_one_ulp(_np(new_o).reshape(-1), want_o) <= 1.0 and _within_one_ulp(_np(new_s), want_s) <= 1.0
    assert len(torch.unique(new_o)) == 1 and len(torch.unique(new_s, dim=0)) == 1
    relocate(opt, dead, src, new_o, new_s)
    par, mom = _state(opt)
    for k in ("xyz", "f_dc", "f_rest", "rotation"):
        assert torch.equal(par[k], old_par[k][alive].expand_as(par[k])), k
    assert torch.equal(par["opacity"], new_o[:1].expand(P, 1)) and torch.equal(par["scaling"], new_s[:1].expand(P, 3))
    assert _within_one_ulp(_np(par["opacity"]).reshape(-1), np.full(P, want_o[0])) <= 1.0
    keep = torch.ones(P, dtype=torch.bool, device=DEV)
    keep[alive] = False
    for k in mh.NAMES:
        for got, was in zip(mom[k], old_mom[k]):
            assert not bool(got[alive].any()) and torch.equal(got[keep], was[keep]) and bool(was[alive].any()), k


# ----------------------------------------------------------------------------------------------------------------------
# scatter and composite
# ----------------------------------------------------------------------------------------------------------------------
def test_two_refines_equal_the_torch_restatement():
    from gaussianeditor_amd.mcmc import mcmc_refine

    P0, cap = 3000, 3200
    opt = _optimizer(_scene_par(P0, 11, dead_every=50))
    g = torch.Generator(device=DEV).manual_seed(9)
    extra = dict(xyz_gradient_accum=torch.rand((P0, 1), device=DEV, generator=g), denom=torch.ones((P0, 1), device=DEV),
                 max_radii2D=torch.rand(P0, device=DEV, generator=g), mask=torch.rand(P0, device=DEV, generator=g) < 0.6,
                 generation=torch.zeros(P0, dtype=torch.int64, device=DEV))
    expected_added = (150, 50)  # int(1.05 * 3000) - 3000; the budget: 3200 - 3150
    for rnd in range(2):
        P = int(opt.param_groups[0]["params"][0].shape[0])
        if rnd == 1:  # fresh dead rows for the second refine, inside and outside the mask
            with torch.no_grad():
                opt.param_groups[mh.NAMES.index("opacity")]["params"][0][7::97] = -8.0
        par, mom = _state(opt)
        before_par = {k: v.clone() for k, v in par.items()}
        before_mom = {k: (a.clone(), b.clone()) for k, (a, b) in mom.items()}
        kw = dict(cap_max=cap, min_opacity=MIN_OPACITY, grow=1.05, generation_num=rnd + 1)
        want_par, want_mom, want_extra, want_counts, touched = mh.mcmc_refine_torch(
            par, mom, extra, generator=torch.Generator(device=DEV).manual_seed(77 + rnd), **kw)
        versions = {k: v._version for k, v in par.items()}
        new_par, extra, counts = mcmc_refine(opt, extra, generator=torch.Generator(device=DEV).manual_seed(77 + rnd), **kw)
        print(f"mcmc_refine round {rnd}: (P, n_dead, n_relocated, n_added) = {counts}")
        assert counts == want_counts and counts[0] == P and counts[1] > 0 and counts[2] == counts[1] and counts[3] == expected_added[rnd]
        final = P + counts[3]
        assert final <= cap
        dead, src_r, src_g = touched["dead"], touched["src_relocate"], touched["src_grow"]
        assert bool(extra["mask"][:P][dead].all()) and bool(extra["mask"][:P][src_r].all())  # only masked rows take part
        rows = torch.zeros(final, dtype=torch.bool, device=DEV)  # rows whose opacity / scaling were computed
        rows[dead] = rows[src_r] = rows[src_g] = True
        rows[P:] = True
        for k in mh.NAMES:
            p = opt.param_groups[mh.NAMES.index(k)]["params"][0]
            assert p is new_par[k] and p.requires_grad and p.shape == want_par[k].shape and p.shape[0] == final
            got = p.detach()
            if k in ("opacity", "scaling"):
                assert torch.equal(got[~rows], want_par[k][~rows]) and torch.equal(got[:P][~rows[:P]], before_par[k][~rows[:P]]), k
                # the computed values: float32 of a float64 evaluation on both sides, the restatement's sum in another order
                assert _within_one_ulp(_np(got[rows]), _np(want_par[k][rows]).astype(np.float64)) <= 1.0, k
                assert torch.equal(got[P:], got[src_g]), k  # growth: the new row and its source carry the draw's value
            else:
                assert torch.equal(got, want_par[k]), k  # row order and copied columns: exact
                assert torch.equal(got[dead], before_par[k][src_r]) and torch.equal(got[P:], got[src_g]), k
            st = opt.state[p]
            for got_m, want_m, was in zip((st["exp_avg"], st["exp_avg_sq"]), want_mom[k], before_mom[k]):
                assert torch.equal(got_m, want_m), k
                assert not bool(got_m[src_r].any()) and not bool(got_m[P:].any()), k        # zero on sources and appended rows
                assert torch.equal(got_m[dead], was[dead]) and bool(was[dead].any()), k      # the dead rows' moments stay
            if rnd == 0:
                assert par[k]._version > versions[k], k  # written in place through raw pointers: the counter moved
        assert extra["mask"].dtype == torch.bool and torch.equal(extra["mask"], want_extra["mask"])
        assert torch.equal(extra["mask"][P:], extra["mask"][src_g])
        assert torch.equal(extra["generation"], want_extra["generation"]) and int((extra["generation"] == rnd + 1).sum()) == counts[3]
        for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
            assert torch.equal(extra[k], want_extra[k]) and extra[k].shape[0] == final and not bool(extra[k][P:].any()), k
    assert int(opt.param_groups[0]["params"][0].shape[0]) == cap
    # the budget is reached: a third refine relocates and adds nothing more
    _, extra, counts = mcmc_refine(opt, extra, cap_max=cap, min_opacity=MIN_OPACITY, generator=torch.Generator(device=DEV).manual_seed(1))
    assert counts[0] == cap and counts[3] == 0 and int(opt.param_groups[0]["params"][0].shape[0]) == cap


# ----------------------------------------------------------------------------------------------------------------------
# noise
# ----------------------------------------------------------------------------------------------------------------------
def _noise_case(P, seed):
    rng = np.random.default_rng(seed)
    xyz = (rng.uniform(0.25, 2.0, (P, 3)) * rng.choice([-1.0, 1.0], (P, 3))).astype(F)
    scaling_raw = (np.log(0.3) + 0.5 * rng.standard_normal((P, 3))).astype(F)
    rotation_raw = (rng.standard_normal((P, 4)) * rng.choice([0.01, 1.0, 1.7, 300.0], (P, 1))).astype(F)  # not normalised
    o = np.where(rng.random(P) < 0.5, rng.uniform(0.0005, 0.06, P), rng.uniform(0.06, 0.999, P))
    opacity_raw = np.log(o / (1 - o)).astype(F).reshape(P, 1)
    noise = rng.standard_normal((P, 3)).astype(F)
    mask = rng.random(P) < 0.7
    return xyz, scaling_raw, rotation_raw, opacity_raw, noise, mask


@pytest.mark.parametrize("P", mh.PS)
def test_noise_within_one_ulp_of_float64(P):
    """The kernel evaluates in binary64 and rounds at the store, so the bar is one float32 ulp of the new xyz (DESIGN.md
    section 21: 0.5 ulp of rounding plus the last-place differences of the device's double exp)."""
    from gaussianeditor_amd.mcmc import inject_noise

    xyz, sr, rot, orw, noise, mask = _noise_case(P, 40 + P)
    scaler = 0.7
    worst = 0.0
    for m in (None, mask):
        x = _dev(xyz)
        v = x._version
        inject_noise(x, _dev(sr), _dev(rot), _dev(orw), _dev(noise), scaler=scaler, mask=None if m is None else _dev(m))
        assert x._version > v
        got = _np(x)
        want = mh.noise_f64(xyz, sr, rot, orw, noise, scaler, m)
        worst = max(worst, _within_one_ulp(got, want))
        if m is not None:
            assert np.array_equal(got[~m].view(np.int32), xyz[~m].view(np.int32))  # frozen rows: bit-identical
        o = 1 / (1 + np.exp(-orw.astype(np.float64).reshape(-1)))
        sel = (np.ones(P, bool) if m is None else m)
        assert np.array_equal(got[o >= 0.5], xyz[o >= 0.5])                        # the gate underflows: no change
        low = sel & (o < 0.01)
        if low.any():
            assert (got[low] != xyz[low]).any()                                    # ... and below the threshold it moves
    print(f"P = {P}: noise, worst error against the float64 evaluation: {worst:.3f} ulp of the new xyz (bar 1)")
    assert worst <= 1.0
    x = _dev(xyz)
    inject_noise(x, _dev(sr), _dev(rot), _dev(orw).reshape(-1), _dev(noise), scaler=0.0)  # the identity; opacity as (P,)
    assert np.array_equal(_np(x).view(np.int32), xyz.view(np.int32))


def test_noise_never_synchronises_and_checks_its_arguments_by_name():
    from gaussianeditor_amd.mcmc import inject_noise

    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available")
    P = 257
    xyz, sr, rot, orw, noise, mask = (_dev(a) for a in _noise_case(P, 3))
    before = xyz.clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        inject_noise(xyz, sr, rot, orw, noise, scaler=0.5, mask=mask)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert not torch.equal(xyz, before)
    for name, bad, msg in (("scaling_raw", sr[:-1], "scaling_raw has shape"), ("rotation_raw", rot.double(), "rotation_raw has dtype"),
                           ("noise", noise.t().contiguous().t(), "noise must be contiguous"), ("opacity_raw", orw.cpu(), "opacity_raw .*no CPU"),
                           ("mask", mask.float(), "mask has dtype")):
        args = dict(scaling_raw=sr, rotation_raw=rot, opacity_raw=orw, noise=noise, mask=mask)
        args[name] = bad
        with pytest.raises(RuntimeError, match=msg):
            inject_noise(xyz, args["scaling_raw"], args["rotation_raw"], args["opacity_raw"], args["noise"], scaler=0.5, mask=args["mask"])


# ----------------------------------------------------------------------------------------------------------------------
# version counters: full render A, a native write, colour-override render B of the same camera (test_gpu_native_writes.py)
# ----------------------------------------------------------------------------------------------------------------------
RP, RW, RH = 3000, 250, 131
MIN_DIFF = 100


class _PC:
    """What render() reads of a GaussianModel: get_xyz is the Parameter itself, the others fresh activations."""

    def __init__(self, sc, dev):
        self._xyz = torch.nn.Parameter(sc["xyz"].to(dev))
        opacity = sc["opacity"].clamp(1e-4, 1 - 1e-4).clone()
        opacity[::10] = 0.002  # dead rows for the relocation
        self._opacity = torch.nn.Parameter(torch.logit(opacity).to(dev))
        self._scaling = torch.nn.Parameter(torch.log(sc["scaling"]).to(dev))
        self._rotation = torch.nn.Parameter(sc["rotation"].to(dev))
        self._features = torch.nn.Parameter(sc["features"].to(dev))
        self.active_sh_degree = self.max_sh_degree = 3

    get_xyz = property(lambda s: s._xyz)
    get_opacity = property(lambda s: torch.sigmoid(s._opacity))
    get_scaling = property(lambda s: torch.exp(s._scaling))
    get_rotation = property(lambda s: torch.nn.functional.normalize(s._rotation))
    get_features = property(lambda s: s._features)

    def optimizer(self):
        named = dict(xyz=self._xyz, features=self._features, opacity=self._opacity, scaling=self._scaling, rotation=self._rotation)
        return torch.optim.Adam([dict(params=[p], lr=1e-4, name=k) for k, p in named.items()], lr=0.0, eps=1e-15)


class _Pipe:
    compute_cov3D_python = False
    convert_SHs_python = False


@pytest.fixture
def reuse():
    import gaussianeditor_amd
    from gaussianeditor_amd.diff_gaussian_rasterization import _reuse

    was = gaussianeditor_amd.get_view_reuse()
    gaussianeditor_amd.set_view_reuse(True)
    _reuse.forget()
    for k in _reuse.stats:
        _reuse.stats[k] = 0
    yield _reuse
    _reuse.forget()
    gaussianeditor_amd.set_view_reuse(was)


@functools.lru_cache(maxsize=None)
def _render_scene():
    case = make_case(RP, RW, RH, seed=5, s0=0.08)
    cam = case["cam"]
    for a in ("world_view_transform", "full_proj_transform", "camera_center"):
        setattr(cam, a, getattr(cam, a).to(DEV))
    colours = torch.rand(RP, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    return case, case["bg"].to(DEV), colours


def _override(pc):
    from gaussianeditor_amd.gaussian_renderer import render

    case, bg, colours = _render_scene()
    out = render(case["cam"], pc, _Pipe, bg, override_color=colours)
    return {k: out[k].detach().clone() for k in ("render", "radii", "depth_3dgs")}


def _without_reuse(fn):
    import gaussianeditor_amd

    gaussianeditor_amd.set_view_reuse(False)
    try:
        return fn()
    finally:
        gaussianeditor_amd.set_view_reuse(True)


def _write_between_renders(reuse, write):
    """A; write(pc); B.  B must miss view reuse and equal a fresh render, and the write must have changed the image."""
    from gaussianeditor_amd.gaussian_renderer import render

    case, bg, _ = _render_scene()
    pc = _PC(case["sc"], DEV)
    before = _without_reuse(lambda: _override(pc))
    render(case["cam"], pc, _Pipe, bg)  # A
    hits = reuse.stats["hits"]
    write(pc)
    b = _override(pc)  # B
    gained = reuse.stats["hits"] - hits
    after = _without_reuse(lambda: _override(pc))
    n = int((before["render"] != after["render"]).sum())
    print(f"reuse-off override image before / after the write: {n} of {before['render'].numel()} values differ")
    assert n >= MIN_DIFF, n
    stale = [k for k in ("render", "radii", "depth_3dgs") if not torch.equal(b[k], after[k])]
    assert gained == 0 and not stale, f"hits gained: {gained}, outputs that differ from the full render: {stale}"


def test_inject_noise_between_two_renders_misses_view_reuse(reuse):
    from gaussianeditor_amd.mcmc import inject_noise

    def write(pc):
        noise = torch.randn(RP, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
        # k = 0: the gate is 1/2 for every row, so the visible Gaussians move
        inject_noise(pc._xyz, pc._scaling.detach(), pc._rotation.detach(), pc._opacity.detach(), noise, scaler=20.0, k=0.0)

    _write_between_renders(reuse, write)


def test_relocate_between_two_renders_misses_view_reuse(reuse):
    from gaussianeditor_amd.mcmc import classify_and_sample, relocate, relocation_values

    def write(pc):
        opt = pc.optimizer()
        opacity = torch.sigmoid(pc._opacity.detach()).reshape(-1)
        u = torch.rand(RP, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
        s = classify_and_sample(opacity, u, min_opacity=MIN_OPACITY)
        assert s.n_dead == RP // 10 == s.n_draws
        n = s.n_draws
        new_o, new_s = relocation_values(opacity, pc._scaling.detach(), s.src[:n], s.ratio[:n], min_opacity=MIN_OPACITY)
        relocate(opt, s.dead_idx[:n], s.src[:n], new_o, new_s)

    _write_between_renders(reuse, write)
