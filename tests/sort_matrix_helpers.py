"""The binning's radix sorts at both block widths: scenes with hand-set depths and positions, the launch counters
(gsr_debug_sort_launches) and the comparisons of tests/test_gpu_sort_matrix.py.

with_sort_width (gsr_binning.hip) compiles every sort twice: 1024 threads per block ("wide": NW = 16 waves, ITEMS = 4 keys per
thread) for sorts of up to 1024 blocks of 4096 keys, 256 threads ("narrow": NW = 4, ITEMS = 16; group_scatter_kernel<11, 256>
owns BPT = 8 bins per thread) beyond, i.e. above 4 194 304 keys.  GSR_SORT_THREADS=256|1024 (read once per process) gives every
sort of the process one width, so the narrow kernels can be held to the CPU oracle on scenes of a few thousand Gaussians.

Counter indices (include/gsr.h):
   0 ..  7  sort_scatter_kernel<IOTA, K, TH>      IOTA | (K is uint32) << 1 | (TH == 1024) << 2
   8 .. 15  depth_scatter_kernel<LAST, IOTA, TH>  LAST | IOTA << 1 | (TH == 1024) << 2
  16 .. 19  group_scatter_kernel<BITS, TH>        (BITS == 11) | (TH == 1024) << 1
  20        sort_scan_kernel launches with more than SORT_THREADS * SCAN_PER = 2048 blocks (the carry round)
Never launched, by the host code (gsr_binning.hip, gsr_capi.hip, gsr_knn.hip):
   1, 5     IOTA with 16-bit keys: the only sort with K = uint16_t is the tile-pair sort (launch_pair_sort), whose values are
            the Gaussian indices emit_keys_kernel wrote (iota_first = false); IOTA sorts (the depth order of the pair-sort
            path, the Morton codes of KNN / near) have 32-bit keys;
  11, 15    LAST & IOTA of the grouped depth sort: IOTA is pass 0, and preprocess_end_impl always adds a third or a fourth
            pass behind the two that gsr_preprocess_begin enqueues, so the last pass is pass 2 or 3;
  21 .. 23  reserved.

The scenes use a camera on the world's z axis (synth.look_at_camera from (0, 0, -4) towards the origin): its view matrix holds
0 and +-1, so K1's depth of a Gaussian at world z is fl(z + 4) and a depth that is a dyadic number is reproduced bit for bit --
ties are exact ties, and which byte of the key two depths differ in is chosen, not hoped for.  `place` puts a Gaussian's centre
on a given pixel position at a given depth.
"""
import ctypes

import numpy as np
import torch

from gaussianeditor_amd.synth import look_at_camera
from helpers import hip_state, make_case, oracle_forward

DEV = "cuda:0"
SORT_KPB, WIDE_MAX_BLOCKS, SCAN_ROUND = 4096, 1024, 256 * 8
GROUP_MAX, RECT32_EDGE = 2048, 256
SCAN_CARRY = 20
NEVER = (1, 5, 11, 15, 21, 22, 23)
DEPTH_SCENES = ("flat", "two_depths", "deep", "culled_interleaved", "low_byte", "high_byte", "tiny1", "tiny63", "tiny64", "tiny65")
GROUP_SCENES = ("one_group_of_many", "four_groups_each", "one_group")
TILE_KEYS_32 = "tile_keys_32"  # an image that takes the tile-pair sort by its size, with 32-bit tile ids
SCENES = DEPTH_SCENES + GROUP_SCENES + (TILE_KEYS_32,)
_cases, _oracle = {}, {}


def scatter_index(iota, u32, wide):
    return int(bool(iota)) | int(bool(u32)) << 1 | int(bool(wide)) << 2


def depth_index(last, iota, wide):
    return 8 + (int(bool(last)) | int(bool(iota)) << 1 | int(bool(wide)) << 2)


def group_index(bits11, wide):
    return 16 + (int(bool(bits11)) | int(bool(wide)) << 1)


def is_wide_index(i):
    """Whether counter i < 20 belongs to a 1024-thread instantiation."""
    return bool((i - 16) >> 1 & 1) if i >= 16 else bool(i >> 2 & 1)


def launches():
    """Launch counts of the radix scatter kernels in this process -> int64 (24,)."""
    from gaussianeditor_amd import _native

    c = (ctypes.c_uint64 * 24)()
    _native.check("gsr_debug_sort_launches", _native.lib().gsr_debug_sort_launches(c))
    return np.array(list(c), dtype=np.int64)


def counter_table(c):
    return " ".join(f"[{i}]={int(v)}" for i, v in enumerate(c) if v) or "all 0"


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def axis_case(P, W, H, seed, s0=0.05):
    case = make_case(P, W, H, seed=seed, s0=s0, nviews=1, sh_degree=0)
    case["cam"] = look_at_camera((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), W, H)  # (the ring camera's field of view: tfx, tfy stay)
    return case


def place(case, px, py, depth):
    """Centres on the pixel positions (px, py) (forward.cu's ndc2Pix inverted) at view depth `depth`; depth <= 0.2 is culled."""
    W, H = case["W"], case["H"]
    d = np.asarray(depth, dtype=np.float64)
    view = np.stack([((2.0 * np.asarray(px, dtype=np.float64) + 1.0) / W - 1.0) * case["tfx"] * d,
                     ((2.0 * np.asarray(py, dtype=np.float64) + 1.0) / H - 1.0) * case["tfy"] * d, d], axis=1)
    wv = case["cam"].world_view_transform.double().numpy()  # p_view = p_world @ wv[:3, :3] + wv[3, :3]
    world = (view - wv[3, :3]) @ np.linalg.inv(wv[:3, :3])
    case["sc"]["xyz"] = torch.tensor(world, dtype=torch.float32).contiguous()
    return case


def _build(name):
    g = np.random.default_rng(sum(name.encode()))
    if name in DEPTH_SCENES:
        P = dict(flat=8193, two_depths=4097, deep=4095, culled_interleaved=4160, low_byte=5000, high_byte=5000).get(name)
        if P is None:
            P = int(name[4:])
        W, H = 160, 120
        case = axis_case(P, W, H, seed=P)
        i = np.arange(P)
        if name == "flat":               # blocks of 4096, 4096 and 1 key: every depth key is 0x40800000
            d = np.full(P, 4.0)
        elif name == "two_depths":       # 0x40800000 / 0x40a00000 alternate in every ballot
            d = np.where(i % 2 == 0, 4.0, 5.0)
        elif name == "deep":             # 0.25 .. 60: the keys differ in the exponent
            d = np.exp(g.random(P) * 5.5 - 1.4)
        elif name == "culled_interleaved":
            d = 3.0 + 2.0 * g.random(P)
            d[::3] = -1.0                # behind the camera: key 0xffffffff, no tile
        elif name == "low_byte":         # 4 + k ulp, k < 256
            d = 4.0 + g.integers(0, 256, P) * 2.0 ** -21
        elif name == "high_byte":        # 0x3f000000, 0x40000000, 0x41000000, 0x42000000
            d = np.array([0.5, 2.0, 8.0, 32.0])[g.integers(0, 4, P)]
        else:
            d = 3.0 + 2.0 * g.random(P)
        return place(case, g.random(P) * W, g.random(P) * H, d)
    if name == TILE_KEYS_32:  # 257 x 256 = 65 792 tiles: ids of 17 bits; a fifth of the Gaussians in the last tile row (ids >= 65 535)
        P, W, H = 5000, 4112, 4096
        case = axis_case(P, W, H, seed=3)
        case["sc"]["scaling"] = torch.full((P, 3), 0.004)
        py = g.random(P) * H
        py[::5] = 4080.0 + 16.0 * g.random(P)[::5]
        return place(case, g.random(P) * W, py, 3.0 + 2.0 * g.random(P))
    if name == "one_group":
        P, W, H = 4100, 128, 128
        return place(axis_case(P, W, H, seed=7), g.random(P) * W, g.random(P) * H, 3.0 + 2.0 * g.random(P))
    W = H = 2064  # 129 x 129 tiles, 17 x 17 = 289 groups: 11-bit group ids
    P = dict(one_group_of_many=5000, four_groups_each=2100)[name]
    case = axis_case(P, W, H, seed=P)
    case["sc"]["scaling"] = torch.full((P, 3), 0.005)  # (a radius of 6 .. 10 pixels at depth 3 .. 5)
    d = 3.0 + 2.0 * g.random(P)
    if name == "one_group_of_many":      # group (8, 8) = pixels [1024, 1152)^2, a tile's margin kept
        return place(case, 1040.0 + 96.0 * g.random(P), 1040.0 + 96.0 * g.random(P), d)
    c = np.arange(P) % 256               # the 16 x 16 interior corners of the group grid
    return place(case, 128.0 * (1 + c % 16) - 0.5, 128.0 * (1 + c // 16) - 0.5, d)


def scene(name):
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


def expectation(oracle, name):
    """The oracle's forward of a scene, computed once per process and left unchanged."""
    if name not in _oracle:
        _oracle[name] = oracle_forward(oracle, scene(name))
    return _oracle[name]


def depth_keys(f):
    return (f["keys"] & np.uint64(0xffffffff)).astype(np.uint32)


def span_bits(f):
    """Bits in which the smallest and the largest depth key of the rendered Gaussians differ (preprocess_end_impl: nbits)."""
    k = depth_keys(f)
    return int(int(k.max()) ^ int(k.min())).bit_length() if k.size else 0


def tile_groups(f, W):
    """Group id of every instance's tile."""
    gx = (W + 15) // 16
    t = (f["keys"] >> np.uint64(32)).astype(np.int64)
    return (t // gx // 8) * ((gx + 7) // 8) + (t % gx) // 8


def assert_scene_is_what_it_claims(name, f):
    """The structure a scene is named after, read off the oracle's forward."""
    case = scene(name)
    P, W = case["sc"]["xyz"].shape[0], case["W"]
    k, tt = depth_keys(f), f["tiles_touched"]
    kinds = np.unique(k)
    if name == "flat":
        assert kinds.tolist() == [0x40800000] and (tt > 0).all()
    elif name == "two_depths":
        assert kinds.tolist() == [0x40800000, 0x40a00000]
        assert np.array_equal(f["depths"].view(np.uint32), np.where(np.arange(P) % 2 == 0, 0x40800000, 0x40a00000))
    elif name == "deep":
        assert span_bits(f) > 24
    elif name == "culled_interleaved":
        assert not tt[::3].any() and (tt[1::3] > 0).all() and (tt[2::3] > 0).all()
    elif name == "low_byte":
        assert span_bits(f) <= 8 and kinds.size == 256 and (kinds >> 8 == 0x408000).all()
    elif name == "high_byte":
        assert kinds.tolist() == [0x3f000000, 0x40000000, 0x41000000, 0x42000000] and (tt > 0).all()
    elif name == "one_group_of_many":
        assert (tile_groups(f, W) == 8 * 17 + 8).all() and (tt > 0).all()
    elif name == "four_groups_each":
        assert (tt == 4).all()
        order = np.argsort(f["point_list"], kind="stable")
        per = np.sort(tile_groups(f, W)[order].reshape(P, 4), axis=1)
        assert (np.diff(per, axis=1) > 0).all() and 4 * P > 2 * SORT_KPB  # four different groups each; G = 4 P: three blocks
    elif name == "one_group":
        assert (tile_groups(f, W) == 0).all()
    elif name == TILE_KEYS_32:
        assert legacy_by_size(W, case["H"]) and int((f["keys"] >> np.uint64(32) > np.uint64(0xffff)).sum()) > 1000


# ---- what a forward must launch --------------------------------------------------------------------------------------------
def legacy_by_size(W, H):
    gx, gy = (W + 15) // 16, (H + 15) // 16
    return ((gx + 7) // 8) * ((gy + 7) // 8) > GROUP_MAX or gx > RECT32_EDGE or gy > RECT32_EDGE


def _wide(n, forced):
    return forced == 1024 if forced else (n + SORT_KPB - 1) // SORT_KPB <= WIDE_MAX_BLOCKS


def expected_launches(P, W, H, R, nbits, legacy, forced):
    """Counter increments of one forward: P Gaussians, R instances, `nbits` = span_bits; `legacy`: GSR_BIN_LEGACY=1;
    `forced`: GSR_SORT_THREADS or 0.  (The group instances G <= R: their sort is wide whenever one of R keys is.)"""
    c = np.zeros(24, dtype=np.int64)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    if legacy or legacy_by_size(W, H):
        passes = 2 if nbits <= 16 else (nbits + 7) // 8
        c[scatter_index(1, 1, _wide(P, forced))] += 1
        c[scatter_index(0, 1, _wide(P, forced))] += passes - 1
        if R > 0:
            tile_bits = int(gx * gy).bit_length()
            c[scatter_index(0, tile_bits > 16, _wide(R, forced))] += (tile_bits + 7) // 8
            if (R + SORT_KPB - 1) // SORT_KPB > SCAN_ROUND:
                c[SCAN_CARRY] += (tile_bits + 7) // 8
    else:
        passes = 3 if nbits <= 24 else 4
        c[depth_index(0, 1, _wide(P, forced))] += 1
        c[depth_index(0, 0, _wide(P, forced))] += passes - 2
        c[depth_index(1, 0, _wide(P, forced))] += 1
        if R > 0:
            assert forced or _wide(R, 0)
            c[group_index(((gx + 7) // 8) * ((gy + 7) // 8) > 256, _wide(R, forced))] += 1
    assert (P + SORT_KPB - 1) // SORT_KPB <= SCAN_ROUND
    return c, passes


def forward(case):
    """One forward through _C.rasterize_gaussians -> (R, colour image, radii, exported state, counter increments)."""
    from gaussianeditor_amd.diff_gaussian_rasterization import _C

    sc, cam = case["sc"], case["cam"]
    e = torch.empty(0, device=DEV)
    d = lambda t: t.to(DEV)  # noqa: E731
    before = launches()
    R, color, depth, radii, geom, binning, img = _C.rasterize_gaussians(
        d(case["bg"]), d(sc["xyz"]), e, d(sc["opacity"]), d(sc["scaling"]), d(sc["rotation"]), 1.0, e,
        d(cam.world_view_transform), d(cam.full_proj_transform), case["tfx"], case["tfy"], case["H"], case["W"],
        d(sc["features"]), case["D"], d(cam.camera_center), False, False)
    torch.cuda.synchronize()
    rose = launches() - before
    st = hip_state(sc["xyz"].shape[0], R, case["W"], case["H"], geom, binning, img)
    return R, color.cpu().numpy(), radii.cpu().numpy(), st, rose


def check_scene(oracle, name, legacy, forced):
    """test_gpu_round3._lists_match on a scene, bit for bit, + exactly the expected counters rose -> what the run left."""
    case = scene(name)
    f = expectation(oracle, name)
    assert_scene_is_what_it_claims(name, f)
    R, color, radii, st, rose = forward(case)
    assert R == f["num_rendered"], name
    assert np.array_equal(st["point_list"], f["point_list"]) and np.array_equal(st["keys"], f["keys"]), name
    assert np.array_equal(st["ranges"], f["ranges"]), name
    assert np.array_equal(st["n_contrib"], f["n_contrib"]), name
    assert np.array_equal(color.view(np.uint32), f["color"].view(np.uint32)), name
    want, passes = expected_launches(case["sc"]["xyz"].shape[0], case["W"], case["H"], R, span_bits(f), legacy, forced)
    assert np.array_equal(rose, want), (name, counter_table(rose), counter_table(want))
    print(f"  {name}: P {case['sc']['xyz'].shape[0]} {case['W']}x{case['H']} R {R}, {passes} depth passes, rose {counter_table(rose)}")
    return dict(point_list=st["point_list"], color=color)


# ---- the sorted list's invariants, where the oracle is too slow ----------------------------------------------------------
def assert_sorted_list_invariants(st, R, rad):
    """keys = tile << 32 | depth bits non-decreasing, equal keys in ascending Gaussian index, every tile's range the run of
    its key, the ranges a partition of [0, R), a Gaussian listed once per tile it touches and every listed one visible, the
    depth bits of an instance its Gaussian's depth.  `st`: helpers.hip_state; -> instances per tile."""
    keys, pl, ranges, tt = st["keys"], st["point_list"].astype(np.int64), st["ranges"].astype(np.int64), st["tiles_touched"]
    assert R == int(tt.astype(np.int64).sum())
    assert np.array_equal(tt > 0, rad > 0)                       # tiles only for visible Gaussians, and for every one
    assert (keys[1:] >= keys[:-1]).all()                           # sorted by (tile, depth bits)
    ties = keys[1:] == keys[:-1]
    assert (pl[1:][ties] > pl[:-1][ties]).all()  # equal keys: ascending Gaussian index (stable)
    assert (rad[pl] > 0).all()
    assert np.array_equal(np.bincount(pl, minlength=tt.shape[0]), tt.astype(np.int64))
    # the depth bits of an instance are its Gaussian's depth
    assert np.array_equal((keys & np.uint64(0xffffffff)).astype(np.uint32), st["depths"][pl].view(np.uint32))
    # ranges: tile t owns exactly the run of keys with tile id t; empty tiles hold (0, 0); together a partition of [0, R)
    tile_of = (keys >> np.uint64(32)).astype(np.int64)
    T = ranges.shape[0]
    counts = np.bincount(tile_of, minlength=T)
    starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
    nonempty = counts > 0
    assert np.array_equal(ranges[nonempty, 0], starts[nonempty]) and np.array_equal(ranges[nonempty, 1], (starts + counts)[nonempty])
    assert (ranges[~nonempty] == 0).all() and int(counts.sum()) == R
    return counts
