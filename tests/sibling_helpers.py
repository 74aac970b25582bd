"""Scenes and expectations for the work-item tests of K7's siblings -- feature_backward_kernel, distortion_backward_kernel,
their forwards and trace_contributions_kernel (gsr_blend.hip) -- at the sizes where their queues are really popped
(tests/test_gpu_sibling_work_items.py, tests/test_cpu_sibling_work_items.py).

Two scenes, built as scene 2 of tests/test_gpu_k7_work_items.py is (make_case plus a concatenated cluster), but lean:

  "wide"    640 x 480, 40 x 30 = 1 200 tiles: more work items than the 1 024 / 768 workgroups of the two backwards on a
            256-CU device, more quadrant items (4 800) than the forwards' 4 096 waves;
  "narrow"  320 x 240, 300 tiles: more items than the 256 workgroups of a launch with one wave per SIMD.

A sparse background of LARGE Gaussians (a hundred-odd, each over many tiles: a tile's list is about ten entries, and its
pixels really blend them -- small Gaussians leave tiles whose lists hold only the 3-sigma rectangles of neighbours, and
whose gradient is nothing) puts a short list (under 64 entries) on every tile; a cluster of small Gaussians in the middle puts lists
of several hundred entries on about twenty tiles.  Between the two the cluster's fringe would leave tiles of 64 .. 128
entries: `scene` removes the cluster Gaussians on such tiles' lists (and on tiles whose list is long but no pixel of which
blends more than 128 entries) and repeats until none is left, so that the oracle forward shows exactly two populations --
`tile_shape` asserts them: every tile non-empty, at least HEAVY_MIN tiles with a list of more than 128 entries AND a pixel
whose n_contrib exceeds 128 (three or more chunks of 64: each parity of the kernels' double buffers is reused), all others
under 64 entries.  The backward's work list cuts a tile in two when its evaluated entries reach max(64, ten eighths of a
workgroup's fair share): the heavy tiles become half items, the light ones stay whole.

The Gaussians on the list of the lightest tile get opacity LIGHTEST_OPACITY, so that the loss of that one tile's gradient
is above the bars of the comparisons (tests/test_cpu_sibling_work_items.py shows that it is).

Expectations (all from what the project has: features_helpers.feature_expectation, distortion_helpers.f64_distortion,
alpha_helpers, contrib_helpers, oracle.cpu) are computed once per process into a flat {name: array} store, which `save`
writes to an .npz and `load` reads back: the child processes of the GPU file's other-grid runs get the parent's."""
import os

import numpy as np
import torch

import distortion_helpers as DH
import features_helpers as FH
from helpers import make_case, oracle_forward, seed_gradient

#: environment variable: the .npz of expectations a child process loads instead of computing them
EXPECT_ENV = "GSR_TEST_SIBLING_EXPECT"
SCENES = {
    "wide": dict(W=640, H=480, C=5, background=dict(P=160, seed=31, s0=0.25, scale_xyz=3.0),
                 cluster=dict(P=4000, seed=12, s0=0.012, scale_xyz=0.3), masked_cap=0.02),
    "narrow": dict(W=320, H=240, C=17, background=dict(P=120, seed=41, s0=0.25, scale_xyz=3.0),
                   cluster=dict(P=4000, seed=12, s0=0.008, scale_xyz=0.5), masked_cap=0.0),
}
HEAVY_MIN = 8
LIGHTEST_OPACITY = 0.6
_KEYS = ("xyz", "scaling", "rotation", "opacity", "features")
_scenes, _store = {}, {}


def _oracle():
    from oracle import cpu

    cpu.build()
    return cpu


def tile_table(f, W, H):
    """(list length, largest n_contrib of a pixel) per tile of the oracle forward `f` (or of any dict with ranges, n_contrib)."""
    r = np.asarray(f["ranges"]).astype(np.int64)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    nc = np.zeros((gy * 16, gx * 16), np.int64)
    nc[:H, :W] = np.asarray(f["n_contrib"]).reshape(H, W)
    return r[:, 1] - r[:, 0], nc.reshape(gy, 16, gx, 16).max(axis=(1, 3)).reshape(-1)


def heavy_tiles(f, W, H):
    n, ncmax = tile_table(f, W, H)
    return (n > 128) & (ncmax > 128)


def tile_shape(name, f):
    """Assert the two populations of the scene (module docstring) on the oracle forward -> dict(tiles, heavy, lightest)."""
    kw = SCENES[name]
    n, _ = tile_table(f, kw["W"], kw["H"])
    heavy = heavy_tiles(f, kw["W"], kw["H"])
    print(f"  {name}: {n.size} tiles, {int((n == 0).sum())} empty, {int(heavy.sum())} heavy (lists up to {int(n.max())}), "
          f"the others {int(n[~heavy].min())} .. {int(n[~heavy].max())} entries")
    assert n.size == ((kw["W"] + 15) // 16) * ((kw["H"] + 15) // 16) and (n > 0).all(), (name, "an empty tile")
    assert int(heavy.sum()) >= HEAVY_MIN, (name, int(heavy.sum()))
    assert int(n[~heavy].max()) < 64, (name, int(n[~heavy].max()))
    return dict(tiles=int(n.size), heavy=heavy, lightest=int(np.argmin(n)))


def scene(name):
    """The case of SCENES[name] -- built once, never modified."""
    if name in _scenes:
        return _scenes[name]
    O, kw = _oracle(), SCENES[name]
    W, H, Pb = kw["W"], kw["H"], kw["background"]["P"]
    case = make_case(W=W, H=H, **kw["background"])
    cluster = make_case(W=W, H=H, **kw["cluster"])["sc"]
    for k in _KEYS:
        case["sc"][k] = torch.cat([case["sc"][k], cluster[k]], 0).contiguous()
    for _ in range(16):
        f = oracle_forward(O, case)
        n, _nc = tile_table(f, W, H)
        fringe = (n >= 64) & ~heavy_tiles(f, W, H)
        if not fringe.any():
            break
        drop = np.zeros(case["sc"]["xyz"].shape[0], bool)
        for t in np.nonzero(fringe)[0]:
            ids = f["point_list"][int(f["ranges"][t][0]):int(f["ranges"][t][1])].astype(np.int64)
            drop[ids[ids >= Pb]] = True  # (the cluster's rows follow the background's)
        assert drop.any(), (name, "a tile of 64 or more background entries: thin the background")
        keep = torch.from_numpy(~drop)
        for k in _KEYS:
            case["sc"][k] = case["sc"][k][keep].contiguous()
    t = int(np.argmin(n))
    ids = torch.from_numpy(f["point_list"][int(f["ranges"][t][0]):int(f["ranges"][t][1])].astype(np.int64))
    op = case["sc"]["opacity"].clone()
    op[ids] = LIGHTEST_OPACITY
    case["sc"]["opacity"] = op.contiguous()
    _scenes[name] = case
    return case


# ---- inputs ---------------------------------------------------------------------------------------------------------
def inputs(name):
    """dict(G (3,H,W), GF (C,H,W), GDist (1,H,W), GA (1,H,W), feats (P,C)) of a scene: the pixel gradients of the feature and
    the distortion tests, and the alpha gradient of tests/test_gpu_alpha.py's scale."""
    case = scene(name)
    H, W, C = case["H"], case["W"], SCENES[name]["C"]
    return dict(G=seed_gradient(H, W, 3) * H * W, GF=FH.feature_gradient(H, W, C), GDist=DH.weights(case),
                GA=seed_gradient(H, W, 5)[:1] * H * W, feats=FH.make_features(case["sc"]["xyz"].shape[0], C))


def tile_mask(name, tile, quadrants=(0, 1, 2, 3)):
    """(1,H,W) float mask: 0 on the pixels of the given quadrants (8 x 8; 0 1 / 2 3) of tile `tile`, 1 elsewhere."""
    kw = SCENES[name]
    W, H = kw["W"], kw["H"]
    gx = (W + 15) // 16
    x0, y0 = 16 * (tile % gx), 16 * (tile // gx)
    m = torch.ones(1, H, W)
    for q in quadrants:
        qx, qy = x0 + 8 * (q & 1), y0 + 8 * (q >> 1)
        m[0, qy:qy + 8, qx:qx + 8] = 0.0
    return m


# ---- expectations ---------------------------------------------------------------------------------------------------
def _put(prefix, d):
    for k, v in d.items():
        _store[f"{prefix}/{k}"] = np.asarray(v)


def sub(prefix):
    """{key: array} of everything stored under `prefix`/."""
    n = len(prefix) + 1
    return {k[n:]: v for k, v in _store.items() if k.startswith(prefix + "/")}


def forward(name):
    """The oracle forward of the scene: dict(color, depth, radii, ranges, n_contrib, final_T, num_rendered)."""
    p = f"{name}/fwd"
    if f"{p}/color" not in _store:
        f = oracle_forward(_oracle(), scene(name))
        _put(p, {k: f[k] for k in ("color", "depth", "radii", "ranges", "n_contrib", "final_T")})
        _store[f"{p}/num_rendered"] = np.asarray(int(f["num_rendered"]))
    return sub(p)


def feature_expectation(name, GF=None):
    """features_helpers.feature_expectation of <G, C> + <GF, F> -> dict(image (C,H,W), want {key}, share {key}, smax {key});
    want holds dL_dfeatures.  `GF`: another feature gradient than the scene's (not stored)."""
    p = f"{name}/feat"
    if GF is not None or f"{p}/image" not in _store:
        O, case, i = _oracle(), scene(name), inputs(name)
        total, share, dfeat, smax = FH.feature_expectation(O, case, i["G"], i["GF"] if GF is None else GF, i["feats"])
        out = dict(want=dict(total, dL_dfeatures=dfeat), share=share, smax=smax)
        if GF is not None:
            return out
        _store[f"{p}/image"] = FH.oracle_feature_image(O, case, i["feats"])
        for k, v in out.items():
            _put(f"{p}/{k}", v)
    return dict(image=_store[f"{p}/image"], want=sub(f"{p}/want"), share=sub(f"{p}/share"),
                smax={k: float(v) for k, v in sub(f"{p}/smax").items()})


def distortion_expectation(name, mapped=False, GDist=None, lam=None):
    """distortion_helpers.expectation(colour=True) of the scene: <G, C> + lam <GDist, D>, near_far = NEAR_FAR if `mapped`
    -> dict(image, want, share, colour_only, lam, masked).  The rows f64_regimes.masked_rows leaves out are capped at
    SCENES[name]["masked_cap"] of P (a condition on the scene).  `GDist`, `lam`: another gradient, with the weight of the
    scene's own expectation (not stored)."""
    p = f"{name}/dist{int(mapped)}"
    if GDist is not None or f"{p}/image" not in _store:
        case = scene(name)
        P = case["sc"]["xyz"].shape[0]
        f = oracle_forward(_oracle(), case)
        e, masked = DH.expectation_of(case, f, f"{name}{', mapped' if mapped else ''}", near_far=DH.NEAR_FAR if mapped else None,
                                      colour=True, GDist=GDist, lam=lam)
        cap = SCENES[name]["masked_cap"] * P
        print(f"  {name}{', mapped' if mapped else ''}: masked rows {int(masked.sum())} of {P} (cap {cap:.0f}), lam {e['lam']:.0e}")
        assert int(masked.sum()) <= cap, (name, int(masked.sum()), cap)
        out = dict(image=e["image"], want=e["want"], share=e["share"], colour_only=e["colour_only"], lam=e["lam"], masked=masked)
        if GDist is not None:
            return out
        for k, v in out.items():
            if isinstance(v, dict):
                _put(f"{p}/{k}", v)
            else:
                _store[f"{p}/{k}"] = np.asarray(v)
    return dict(image=_store[f"{p}/image"], want=sub(f"{p}/want"), share=sub(f"{p}/share"), colour_only=sub(f"{p}/colour_only"),
                lam=float(_store[f"{p}/lam"]), masked=_store[f"{p}/masked"].astype(bool))


def step_expectation(name):
    """The summed expectation of ONE step with the colour, alpha, feature and distortion losses,
    <G, C> + <GA, A> + <GF, F> + lam <GDist, D>: features_helpers.feature_expectation(GA=) -- the oracle's colour, alpha and
    slice backwards -- plus the float64 distortion share -> dict(want {key}, smax {key}, masked, lam)."""
    p = f"{name}/step"
    if f"{p}/lam" not in _store:
        O, case, i = _oracle(), scene(name), inputs(name)
        d = distortion_expectation(name)
        total, _, dfeat, smax = FH.feature_expectation(O, case, i["G"], i["GF"], i["feats"], GA=i["GA"])
        want = dict(total, dL_dfeatures=dfeat)
        for k, s in d["share"].items():
            if k in want and k != "dL_dsh":  # (the distortion image does not depend on the colours)
                want[k] = want[k] + s.reshape(want[k].shape)
        _put(f"{p}/want", want)
        _put(f"{p}/smax", smax)
        _store[f"{p}/lam"] = np.asarray(d["lam"])
    return dict(want=sub(f"{p}/want"), smax={k: float(v) for k, v in sub(f"{p}/smax").items()},
                masked=distortion_expectation(name)["masked"], lam=float(_store[f"{p}/lam"]))


def exhaustive_trace(O, case):
    """contrib_helpers' exhaustive reference of a case: every (Gaussian, pixel) weight from oracle.cpu.blend_forward, as
    contrib_helpers.oracle_weights takes it (background 0, a colour column that is 1 for the Gaussian asked for and 0 for
    every other entry of the pixel's list: the pixel's colour is w itself).  A column serves MANY Gaussians here, no two of
    them on one tile's list (a greedy colouring of the tile lists), and a call leaves the ranges of the tiles none of its
    Gaussians is listed on empty: some hundreds of short calls where one column per Gaussian takes minutes.
    -> dict(table (P,3) int64, top_id (H W), top_weight (H W), tied)."""
    import contrib_helpers as CH

    P, W, H = case["sc"]["xyz"].shape[0], case["W"], case["H"]
    geom, binning = CH.oracle_state(O, case)
    ranges, plist = binning["ranges"].astype(np.int64), binning["point_list"].astype(np.int64)
    T, gx = ranges.shape[0], (W + 15) // 16
    pix = np.arange(H * W)
    tile_of_pixel = (pix // W // 16) * gx + (pix % W) // 16
    order = np.argsort(tile_of_pixel, kind="stable")
    first = np.searchsorted(tile_of_pixel[order], np.arange(T + 1))
    pixels_of = [order[first[t]:first[t + 1]] for t in range(T)]
    tiles_of = {}
    for t in range(T):
        for g in plist[ranges[t, 0]:ranges[t, 1]]:
            tiles_of.setdefault(int(g), []).append(t)
    used, slots = [set() for _ in range(T)], []  # slots[s]: Gaussians no two of which share a tile
    for g in sorted(tiles_of, key=lambda g: -max(ranges[t, 1] - ranges[t, 0] for t in tiles_of[g])):
        taken = set().union(*(used[t] for t in tiles_of[g]))
        s = next(i for i in range(len(taken) + 1) if i not in taken)
        for t in tiles_of[g]:
            used[t].add(s)
        if s == len(slots):
            slots.append([])
        slots[s].append(g)
    table = np.zeros((P, 3), np.int64)
    top_w, top_id = np.zeros(H * W, np.float32), np.full(H * W, -1, np.int32)
    tied = 0
    for s0 in range(0, len(slots), 3):
        cols, owner = np.zeros((P, 3), np.float32), np.full((3, T), -1, np.int32)
        active = np.zeros(T, bool)
        for c, members in enumerate(slots[s0:s0 + 3]):
            for g in members:
                cols[g, c] = 1.0
                owner[c, tiles_of[g]] = g
                active[tiles_of[g]] = True
        cut = dict(binning, ranges=np.where(active[:, None], binning["ranges"], 0).astype(np.uint32))
        img = O.blend_forward(geom, cut, cols, np.zeros(3, np.float32), W, H)["color"].reshape(3, -1)
        for c, members in enumerate(slots[s0:s0 + 3]):
            w = img[c]
            for g in members:
                table[g] = CH.expected_rows(w[np.concatenate([pixels_of[t] for t in tiles_of[g]])][None, :])[0]
            who = owner[c][tile_of_pixel]
            tied += int(((w == top_w) & (w > 0)).sum())
            better = w > top_w
            top_w[better], top_id[better] = w[better], who[better]
    table[:, 1] = np.bincount(top_id[top_id >= 0], minlength=P)
    return dict(table=table, top_id=top_id, top_weight=top_w, tied=tied)


def trace_expectation(name):
    """exhaustive_trace of the scene, stored."""
    p = f"{name}/trace"
    if f"{p}/table" not in _store:
        _put(p, exhaustive_trace(_oracle(), scene(name)))
    return sub(p)


# ---- the store ------------------------------------------------------------------------------------------------------
def save(path):
    np.savez(path, **_store)


def load(path):
    with np.load(path) as z:
        for k in z.files:
            _store[k] = z[k]


if os.environ.get(EXPECT_ENV):
    load(os.environ[EXPECT_ENV])


# ---- the product ----------------------------------------------------------------------------------------------------
def run_step(name, features=False, distortion=False, mapped=False, alpha=False, lam=1.0, G=True):
    """One render and one autograd backward of <G, C> (+ <GF, F>) (+ lam <GDist, D>) (+ <GA, A>) through GaussianRasterizer
    -> (gradients by the oracle's names, numpy; dict(color, depth, radii, features, distortion, alpha as numpy | None,
    num_rendered, items = k7_matrix_helpers.work_items of the list the LAST blend backward of the step left))."""
    import k7_matrix_helpers as K
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer
    from helpers import settings

    case, i = scene(name), inputs(name)
    sc, H, W = case["sc"], case["H"], case["W"]
    dev = DH.DEV
    leaf = lambda t: t.to(dev).clone().requires_grad_(True)  # noqa: E731
    lv = dict(dL_dmeans3D=leaf(sc["xyz"]), dL_dopacity=leaf(sc["opacity"]), dL_dsh=leaf(sc["features"]),
              dL_dscales=leaf(sc["scaling"]), dL_drotations=leaf(sc["rotation"]))
    m2d = lv["dL_dmeans2D"] = torch.zeros_like(lv["dL_dmeans3D"], requires_grad=True)
    kw = {}
    if distortion:
        kw["return_distortion"] = DH.NEAR_FAR if mapped else True
    if alpha:
        kw["return_alpha"] = True
    if features:
        kw["features"] = lv["dL_dfeatures"] = leaf(i["feats"])
    outs = GaussianRasterizer(settings(case, dev))(lv["dL_dmeans3D"], m2d, lv["dL_dopacity"], shs=lv["dL_dsh"],
                                                   scales=lv["dL_dscales"], rotations=lv["dL_drotations"], **kw)
    assert len(outs) == 3 + bool(alpha) + bool(features) + bool(distortion)
    color, radii, depth = outs[:3]
    rest = list(outs[3:])
    dimg = rest.pop() if distortion else None
    fimg = rest.pop() if features else None
    aimg = rest.pop() if alpha else None
    node = color.grad_fn  # the render's autograd node: its image state and num_rendered, before the backward frees them
    img, num_rendered = node.saved_tensors[9], int(node.num_rendered)
    loss = (color * i["G"].to(dev)).sum() if G else 0.0
    if features:
        loss = loss + (fimg * i["GF"].to(dev)).sum()
    if distortion:
        loss = loss + lam * (dimg * i["GDist"].to(dev)).sum()
    if alpha:
        loss = loss + (aimg * i["GA"].to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).cpu().numpy() for k, v in lv.items()}
    npy = lambda t: None if t is None else t.detach().cpu().numpy()  # noqa: E731
    return grads, dict(color=npy(color), depth=npy(depth), radii=npy(radii), features=npy(fimg), distortion=npy(dimg),
                       alpha=npy(aimg), num_rendered=num_rendered, items=K.work_items(img, H, W))
