"""The blend backward's instantiation matrix: blend_backward_kernel<FAST, SEG, DEPTH, ABS, ALPHA> (gsr_blend.hip), 24 kernels
(DEPTH excludes SEG), each held to ONE builder of the expected gradients of <G, C> + <GA, A> + <GD, D>.

A row is (FAST, SEG, DEPTH, ABS, ALPHA); its index in gsr_debug_blend_backward_launches is FAST | SEG << 1 | DEPTH << 2 |
ABS << 3 | ALPHA << 4.

The builder (`expectation`):
  rows without FAST  the oracle's linearity construction as it exists -- alpha_helpers.alpha_expectation(..., GD=...), which
                     uses depth_helpers.depth_expectation (tests/test_cpu_k7_matrix.py holds the sum to float64 autograd);
  rows with FAST     (the oracle has no hardware 2^x) the same construction on the product's own FAST colour-only backward in
                     this process: the ordinary render with G, the "ones" render (colours (1,1,1), background 0) with
                     (GA, 0, 0), the depth-colour render (colours (d_i, 0, 0) from K1's exported depths, background 0) with
                     (GD, 0, 0) plus dL/dd_i * depth_helpers.view_z_row on means3D.  The three share geometry and opacities,
                     hence every skip and stop decision: no pixel is masked.
With ABS the expected absgrad is abs_helpers.abs_sum over a pixel block of that same expectation with all pixel gradients
masked to the one pixel (with FAST: one-pixel backwards of the product, deterministic -- each accumulator cell gets one add).

The route (`run`) calls _C.rasterize_gaussians and _C.rasterize_gaussians_backward directly, keeps the image state, proves
which kernel ran (the launch counter of exactly the intended index rose by one, no other moved) and reports what the
backward's work list held (gsr_debug_blend_backward_items)."""
import ctypes

import numpy as np
import torch

import abs_helpers as AB
import alpha_helpers as AH
import depth_helpers as DH
from helpers import assert_grads_close, settings

DEV = "cuda:0"
BLOCK = 4  # the centred pixel block of the absgrad comparison
#: the 24 rows (FAST, SEG, DEPTH, ABS, ALPHA)
ROWS = [(f, s, d, a, l) for l in (0, 1) for a in (0, 1) for d in (0, 1) for s in (0, 1) for f in (0, 1) if not (s and d)]
#: the sweep seeds on which a comparison must be able to see the alpha and the depth share (tests/test_cpu_k7_matrix.py)
SWEEP_DISCRIMINATING, SWEEP_SHARE_ROWS = (2, 3, 6, 7, 8, 9, 10, 11), 8


def index(row):
    f, s, d, a, l = row
    return int(bool(f)) | int(bool(s)) << 1 | int(bool(d)) << 2 | int(bool(a)) << 3 | int(bool(l)) << 4


def row_of(i):
    return (i & 1, i >> 1 & 1, i >> 2 & 1, i >> 3 & 1, i >> 4 & 1)


def row_id(row):
    return "".join(n if v else "-" for n, v in zip(("F", "S", "D", "B", "L"), row)) + f"[{index(row)}]"


def launches():
    """Launch counts of K7 in this process by instantiation index -> int64 (32,)."""
    from gaussianeditor_amd import _native

    c = (ctypes.c_uint64 * 32)()
    _native.check("gsr_debug_blend_backward_launches", _native.lib().gsr_debug_blend_backward_launches(c))
    return np.array(list(c), dtype=np.int64)


def work_items(img, H, W):
    """(items, list-segment items) of the work list the latest backward of the image state `img` built."""
    from gaussianeditor_amd import _native

    c = (ctypes.c_int64 * 2)()
    s = torch.cuda.current_stream(img.device).cuda_stream
    _native.check("gsr_debug_blend_backward_items", _native.lib().gsr_debug_blend_backward_items(s, W, H, img.data_ptr(), c))
    return int(c[0]), int(c[1])


def k1_depths(P, geom):
    """K1's view-space depths of the view whose geometry state is `geom` -> float32 (P,)."""
    from gaussianeditor_amd import _native

    d = torch.zeros(P, dtype=torch.float32, device=geom.device)
    s = torch.cuda.current_stream(geom.device).cuda_stream
    _native.check("export_geom", _native.lib().gsr_debug_export_geom(s, P, geom.data_ptr(), None, d.data_ptr(), None, None,
                                                                     None, None))
    torch.cuda.synchronize()
    return d.cpu().numpy()


def counter_table(counts=None):
    c = launches() if counts is None else counts
    return "  ".join(f"{row_id(r)}={int(c[index(r)])}" for r in ROWS)


def run(case, row, G, GA=None, GD=None, colors_precomp=None, bg=None, D=None, scale_modifier=1.0):
    """One forward + one backward of <G, C> (+ <GA, A>) (+ <GD, D>) through _C directly, expected to launch the instantiation
    `row` = (FAST, SEG, DEPTH, ABS, ALPHA); SEG None: either (whether the forward leaves checkpoints depends on the view).
    Asserts that exactly that launch counter rose by one -- or, where nothing is rendered (R == 0: the library launches
    nothing), that none moved.  -> (gradients by the oracle's names, numpy; dict(color, depth, alpha | None, absgrad | None, R,
    items = (items, segment items) | None, index | None, geom))."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    fast, seg, depth, ab, al = row
    assert (GD is not None) == bool(depth) and (GA is not None) == bool(al), "the loss terms are the row's switches"
    sc = case["sc"]
    H, W, P = case["H"], case["W"], sc["xyz"].shape[0]
    rs = settings(case if bg is None else dict(case, bg=bg), DEV, D=D, scale_modifier=scale_modifier)
    e = torch.empty(0, device=DEV)
    t = lambda k: sc[k].to(DEV).contiguous()  # noqa: E731
    xyz, op, scl, rot = t("xyz"), t("opacity"), t("scaling"), t("rotation")
    cols = e if colors_precomp is None else colors_precomp.to(DEV).contiguous()
    sh = t("features") if colors_precomp is None else e
    flags = options.FLAG_FAST_EXP if fast else 0
    R, color, dimg, radii, geom, binning, img = _C.rasterize_gaussians(
        rs.bg, xyz, cols, op, scl, rot, rs.scale_modifier, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, sh,
        rs.sh_degree, rs.campos, False, False, flags=flags)
    alpha = _C.alpha_image(img, H, W) if al else None
    absgrad = torch.empty((P, 3), dtype=torch.float32, device=DEV) if ab else None
    dev = lambda g: None if g is None else g.to(DEV).contiguous()  # noqa: E731
    torch.cuda.synchronize()
    before = launches()
    m2, dcol, dop, m3, _, dsh, dscl, drot = _C.rasterize_gaussians_backward(
        rs.bg, xyz, radii, cols, scl, rot, rs.scale_modifier, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
        dev(G), sh, rs.sh_degree, rs.campos, geom, R, binning, img, False, flags=flags, dL_dout_depth=dev(GD),
        abs_grad_out=absgrad, dL_dout_alpha=dev(GA))
    torch.cuda.synchronize()
    delta = launches() - before
    launched, items = None, None
    if R == 0:
        assert not delta.any(), (row_id(row), "a view that renders nothing launched K7", counter_table(delta))
    else:
        allowed = [index((fast, s, depth, ab, al)) for s in ((0, 1) if seg is None and not depth else (seg,))]
        hit = np.nonzero(delta)[0].tolist()
        assert len(hit) == 1 and delta[hit[0]] == 1 and hit[0] in allowed, (
            f"wanted one launch of {row_id(row)}, the counters moved by: " + (counter_table(delta) if delta.any() else "nothing"))
        launched, items = hit[0], work_items(img, H, W)
        assert items[1] == 0 or launched & 2, (row_id(row), items)  # (segment items only in a SEG launch)
    npy = lambda x: None if x is None else x.detach().cpu().numpy()  # noqa: E731
    grads = dict(dL_dmeans2D=npy(m2), dL_dopacity=npy(dop), dL_dmeans3D=npy(m3), dL_dscales=npy(dscl), dL_drotations=npy(drot))
    grads["dL_dsh" if colors_precomp is None else "dL_dcolors"] = npy(dsh if colors_precomp is None else dcol)
    return grads, dict(color=npy(color), depth=npy(dimg), alpha=npy(alpha), absgrad=npy(absgrad), R=int(R), items=items,
                       index=launched, geom=geom)


def _oracle_expectation(O, case, G, GA, GD, shares, **kw):
    H, W = case["H"], case["W"]
    total, a_share = AH.alpha_expectation(O, case, G, torch.zeros(1, H, W) if GA is None else GA, GD=GD, **kw)
    out = {}
    if shares and GA is not None:
        out["alpha"] = a_share
    if shares and GD is not None:  # by linearity: what the depth term adds to the same construction
        without, _ = AH.alpha_expectation(O, case, G, torch.zeros(1, H, W) if GA is None else GA, GD=None, **kw)
        out["depth"] = {k: total[k] - without[k] for k in a_share}
    return total, out


def _product_expectation(case, G, GA, GD, seg, **kw):
    H, W, P = case["H"], case["W"], case["sc"]["xyz"].shape[0]
    base = (1, seg, 0, 0, 0)
    g1, o1 = run(case, base, G, **kw)
    total, out = {k: v.astype(np.float64) for k, v in g1.items()}, {}

    def add(name, g):
        out[name] = {k: g[k].astype(np.float64) for k in g if k not in AH.COLOUR_KEYS}
        for k, v in out[name].items():
            total[k] = total[k] + v.reshape(total[k].shape)

    if GA is not None:
        add("alpha", run(case, base, AH.ones_gradient(GA, H, W), colors_precomp=torch.ones(P, 3), bg=torch.zeros(3), **kw)[0])
    if GD is not None:
        g3 = run(case, base, AH.ones_gradient(GD, H, W), colors_precomp=DH.depth_colors(k1_depths(P, o1["geom"])),
                 bg=torch.zeros(3), **kw)[0]
        gd = g3["dL_dcolors"].astype(np.float64).reshape(P, 3)[:, 0]
        g3["dL_dmeans3D"] = g3["dL_dmeans3D"].astype(np.float64) + gd[:, None] * DH.view_z_row(case)[None, :]
        add("depth", g3)
    return total, out


def expectation(O, case, G, GA=None, GD=None, fast=False, seg=None, shares=False, **kw):
    """Expected gradients of <G, C> (+ <GA, A>) (+ <GD, D>) -> (total, {"alpha": share, "depth": share}), float64 dicts by the
    oracle's names (module docstring).  kw: D, scale_modifier.  `seg`: with FAST, the SEG switch the product's colour-only
    backwards must run with (None: either)."""
    if fast:
        return _product_expectation(case, G, GA, GD, seg, **kw)
    return _oracle_expectation(O, case, G, GA, GD, shares, **kw)


def abs_expectation(O, case, G, GA, GD, pixels, fast=False, seg=None, **kw):
    """abs_helpers.abs_sum over `pixels` of the expectation with every pixel gradient masked to the one pixel
    -> (absgrad (P,3), signed sum (P,2))."""
    H, W, P = case["H"], case["W"], case["sc"]["xyz"].shape[0]

    def term(y, x):
        m = AB.pixel_mask(H, W, [(y, x)])
        return expectation(O, case, G * m, None if GA is None else GA * m, None if GD is None else GD * m, fast=fast, seg=seg,
                           **kw)[0]["dL_dmeans2D"]
    return AB.abs_sum(term, pixels, P)


def share_rows(total, share, keys=AH.SHARE_KEYS):
    """{key: rows on which `share` exceeds alpha_helpers.SHARE_REL of the total's maximum}."""
    rows = {}
    for k in keys:
        P = np.asarray(total[k]).shape[0]
        s = np.abs(np.asarray(share[k], dtype=np.float64).reshape(P, -1)).max(axis=1)
        rows[k] = int((s > AH.SHARE_REL * np.abs(total[k]).max()).sum())
    return rows


def errors(got, want, keys=None):
    """{key: max |got - want| / max |want|}."""
    out = {}
    for k in (keys if keys is not None else got):
        a = np.asarray(got[k], dtype=np.float64)
        b = np.asarray(want[k], dtype=np.float64).reshape(a.shape)
        out[k] = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if a.size else 0.0
    return out


def acc_tables_are_zero():
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    torch.cuda.synchronize()
    assert _C._ACC_TABLES, "the persistent accumulator table is not in use"
    return all(not bool(t.any()) for t in _C._ACC_TABLES.values())


def check_row(O, case, row, G, GA, GD, tag, bar=1e-5, **kw):
    """The whole comparison of one row on one scene (G, GA, GD: the scene's three pixel gradients; the row's switches say
    which enter the loss) -> report dict(worst, worst_abs, items)."""
    fast, seg, depth, ab, al = row
    H, W = case["H"], case["W"]
    GA, GD = (GA if al else None), (GD if depth else None)
    rep = {}
    want, shares = expectation(O, case, G, GA, GD, fast=fast, seg=seg, shares=True, **kw)
    if al:
        AH.assert_share_visible(want, shares["alpha"], tag=tag + " alpha share")
    if depth:
        AH.assert_share_visible(want, shares["depth"], tag=tag + " depth share")
    got, out = run(case, row, G, GA, GD, **kw)
    rep["items"] = out["items"]
    if seg:
        assert out["items"][1] >= 1, (tag, "no list-segment item in the backward's work list", out["items"])
    if al:  # ... and the product's gradients differ from its own without the alpha term by more than ten bars
        AH.assert_differs_from_colour_only(got, run(case, (fast, seg, depth, ab, 0), G, None, GD, **kw)[0], want, tag=tag + " alpha")
    if depth:  # ... and from its own without the depth term
        AH.assert_differs_from_colour_only(got, run(case, (fast, seg, 0, ab, al), G, GA, None, **kw)[0], want, tag=tag + " depth")
    err = errors(got, want)
    rep["worst"] = assert_grads_close(got, want, tol=bar, tag=tag, keys=list(got))
    print(f"  {tag}: items {out['items']}, worst {rep['worst']:.2e} = {rep['worst'] / bar:.3f} bar; "
          + ", ".join(f"{k[3:]} {v:.1e}" for k, v in err.items()))
    if ab:
        a, sg = out["absgrad"].astype(np.float64), np.abs(got["dL_dmeans2D"][:, :2].astype(np.float64))
        assert (a[:, 2] == 0).all() and np.isfinite(a).all() and (sg - a[:, :2]).max() <= bar * a.max(), (tag, "dominance")
        # the pixel block: absgrad against the per-pixel expectation, the signed screen-space gradient against its sum
        pixels = AB.block_pixels(H, W, BLOCK)
        m = AB.pixel_mask(H, W, pixels)
        mask = lambda g: None if g is None else g * m  # noqa: E731
        want_a, signed = abs_expectation(O, case, G, GA, GD, pixels, fast=fast, seg=seg, **kw)
        AB.assert_discriminates(want_a, signed, tag=tag + " block")
        gb, ob = run(case, row, G * m, mask(GA), mask(GD), **kw)
        if seg:
            assert ob["items"][1] >= 1, (tag, "block run: no list-segment item", ob["items"])
        rep["worst_abs"] = assert_grads_close(dict(absgrad=ob["absgrad"]), dict(absgrad=want_a), tol=bar, tag=tag + ": absgrad vs per-pixel expectation")
        assert_grads_close(dict(signed=gb["dL_dmeans2D"][:, :2]), dict(signed=signed), tol=bar, tag=tag + ": block means2D.grad")
        assert (ob["absgrad"][:, 2] == 0).all()
        print(f"  {tag}: absgrad worst {rep['worst_abs']:.2e} = {rep['worst_abs'] / bar:.3f} bar")
    assert acc_tables_are_zero(), (tag, "a persistent accumulator table is not all zero after the row")
    return rep


def scene(name):
    """(case, G, GA, GD) -- the scene of tests/test_gpu_alpha.py with a depth gradient.  The depth image holds view-space z,
    about the camera's distance from the scene's centre (4.0 here), where colour and alpha lie in [0, 1]: a unit pixel
    gradient on it outweighs the other two terms by that factor, and the alpha share of the 70 x 45 scene then exceeds 1e-2
    of the total's maximum on 98 rows of dL_dopacity only (oracle alone; the discrimination condition asks for 100).  Divided
    by that distance the three terms balance: the alpha share is visible on >= 184 rows of every tensor and the depth share
    on >= 236, on all three scenes (oracle alone, tests/test_cpu_k7_matrix.py)."""
    from helpers import seed_gradient
    from test_gpu_alpha import _case

    case, G, GA = _case(name)
    H, W = case["H"], case["W"]
    return case, G, GA, seed_gradient(H, W, 7)[:1] * H * W / float(case["cam"].camera_center.norm())


# ---- the shape sweep under the opt-in losses ------------------------------------------------------------------------
_sweep = {}


def sweep_expectation(O, seed):
    """Configuration `seed` of test_gpu_parity.sweep_case with its three pixel gradients and the oracle's expectations, built
    once per process -> dict(case, sm, D, G, GA, GD, f, want3, want2, shares, rows)."""
    if seed not in _sweep:
        from helpers import oracle_forward, seed_gradient
        from test_gpu_parity import sweep_case

        case, sm, D = sweep_case(seed)
        H, W = case["H"], case["W"]
        G = seed_gradient(H, W, seed) * (H * W)
        GA, GD = seed_gradient(H, W, seed + 50)[:1] * (H * W), seed_gradient(H, W, seed + 90)[:1] * (H * W)
        kw = dict(D=D, scale_modifier=sm)
        want3, shares = expectation(O, case, G, GA, GD, shares=True, **kw)
        want2, _ = AH.alpha_expectation(O, case, G, GA, **kw)
        rows = {n: share_rows(want3, s) for n, s in shares.items()}
        _sweep[seed] = dict(case=case, sm=sm, D=D, G=G, GA=GA, GD=GD, kw=kw, f=oracle_forward(O, case, scale_modifier=sm),
                            want3=want3, want2=want2, shares=shares, rows=rows)
    return _sweep[seed]


def assert_sweep_discriminates(s, seed):
    """On SWEEP_DISCRIMINATING seeds the alpha and the depth share each exceed alpha_helpers.SHARE_REL of the total's maximum
    on >= SWEEP_SHARE_ROWS rows of each of alpha_helpers.SHARE_KEYS: a condition on the expectation alone."""
    print(f"  sweep seed {seed}: rows whose share > {AH.SHARE_REL} of the total's maximum: {s['rows']}")
    if seed in SWEEP_DISCRIMINATING:
        assert all(n >= SWEEP_SHARE_ROWS for r in s["rows"].values() for n in r.values()), (seed, s["rows"])


def write_base(path):
    """The FAST base of the SEG rows: (1,0,0,0,0) on the 20 000-Gaussian scene -> npz (the forward image and the gradients).
    Meant for a fresh process whose backward never cuts a list (GSR_BWD_SEG=0): by default a view with lists this long
    runs the SEG kernels."""
    case, G, _, _ = scene("p20000")
    got, out = run(case, (1, 0, 0, 0, 0), G)
    np.savez(path, color=out["color"], items=np.array(out["items"]), **got)
    print(f"base {row_id((1, 0, 0, 0, 0))}: items {out['items']}; {counter_table()}")

