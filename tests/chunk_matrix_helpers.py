"""The grouped binning's chunk stage (gsr_binning.hip: group_chunk_kernel<SCATTER, NB>, group_colscan_kernel) at every chunk
length: scenes, a CPU census of what the kernels will meet, the launch counters (gsr_debug_group_launches) and the comparison
of tests/test_gpu_chunk_matrix.py.  tests/test_cpu_chunk_matrix.py holds every scene to the regimes it claims, on the census.

The sorted group instances of a view are padded per group to a multiple of `chunk` = 64 NB; one wave takes a chunk in NB
batches of 64 items, lane t = tile t of the group.  group_chunk_items(G) picks the chunk by the view's G; GSR_GROUP_CHUNK=
64|128|256|512 (read once per process) gives every view of the process one length, so NB = 2, 4, 8 -- otherwise reached
above 1, 2 and 4 million group instances -- can be held to the CPU oracle on scenes of a few thousand Gaussians.

The append pass stages (Gaussian, destination) pairs in LDS: `cap` = 1024 entries if (R / G + 1) * chunk <= 820, else 2048.
A batch whose entries do not fit is taken in parts: 1 if tot_l + tot_h <= cap (tot_l: entries of items 0 .. 31, tot_h: of
32 .. 63), 2 if max(tot_l, tot_h) <= cap, else 4; the stage is written out ("flush") before a part that would overflow it.

Counter indices (include/gsr.h): log2(NB) | SCATTER << 2 | (cap == 2048) << 3.
Never launched, by the host code (gsr_binning.hip: launch_chunks, launch_grouped):
   7         <append, NB = 8, cap 1024>: R >= G, so (R / G + 1) * 512 >= 1024 > 820;
   8 .. 11   the count pass has no stage (lds = 0): it is counted with cap bit 0.

The scenes use sort_matrix_helpers.axis_case / place: an axis camera and dyadic depths, so depth order, ties and therefore
which items share a batch are chosen, not hoped for.  A "tiny" Gaussian has a radius of 2 pixels (one tile, or a few at a
tile edge); a "band" Gaussian covers the whole image.
"""
import ctypes
import os
import re

import numpy as np

import sort_matrix_helpers as S
from helpers import oracle_forward

CHUNKS = (64, 128, 256, 512)
NEVER = (7, 8, 9, 10, 11)
GROUP_EDGE, GROUP_TILES = 8, 64
SEGMENT_P = (1, 64, 65, 128, 129, 193, 256, 257, 449, 512, 513)  # chunk - 63, chunk, chunk + 1 of every chunk length; 65
MIXED = ("mixed", "mixed_unaligned", "mixed_few")
SCENES = MIXED + tuple(f"segment_{p}" for p in SEGMENT_P) + ("exact_fit", "long_column", "ragged", "hole", "four_groups_each")
BAND = 64
_cases, _oracle, _census = {}, {}, {}


def count_index(chunk):
    return (chunk // 64).bit_length() - 1


def append_index(chunk, cap):
    return count_index(chunk) | 4 | (8 if cap == 2048 else 0)


def reachable(chunk):
    """The counters a process whose every view has chunk length `chunk` can raise."""
    return (count_index(chunk),) + tuple(append_index(chunk, cap) for cap in (1024, 2048) if append_index(chunk, cap) not in NEVER)


def launches():
    """Launch counts of group_chunk_kernel in this process -> int64 (16,)."""
    from gaussianeditor_amd import _native

    c = (ctypes.c_uint64 * 16)()
    _native.check("gsr_debug_group_launches", _native.lib().gsr_debug_group_launches(c))
    return np.array(list(c), dtype=np.int64)


def kernel_constants():
    """GROUP_CHUNKS_TARGET, the stage rule's bound (820) and its two capacities, COLSCAN_WAVES, COLSCAN_REG, parsed out of the
    sources' text."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussianeditor_amd", "csrc")
    with open(os.path.join(csrc, "gsr_common.h")) as f:
        common = f.read()
    with open(os.path.join(csrc, "gsr_binning.hip")) as f:
        binning = f.read()
    out = dict(GROUP_CHUNKS_TARGET=int(re.search(r"constexpr int GROUP_CHUNKS_TARGET = (\d+);", common).group(1)))
    m = re.search(r"a\.stage_cap = \(R / b\.G \+ 1\) \* \(int64_t\)b\.chunk <= (\d+) \? (\d+)u : (\d+)u;", binning)
    out.update(STAGE_BOUND=int(m.group(1)), CAP_SMALL=int(m.group(2)), CAP_LARGE=int(m.group(3)))
    m = re.search(r"constexpr int COLSCAN_WAVES = (\d+), COLSCAN_REG = (\d+);", binning)
    out.update(COLSCAN_WAVES=int(m.group(1)), COLSCAN_REG=int(m.group(2)))
    # the part rule and the chunk rule, as text: a rewrite of either has to come by here
    assert "const int nparts = tot_l + tot_h <= cap ? 1 : (max(tot_l, tot_h) <= cap ? 2 : 4);" in binning
    assert "if (staged + total > cap) flush();" in binning
    assert "while (per < 8 && batches > (int64_t)GROUP_CHUNKS_TARGET * per) per *= 2;" in common
    return out


def natural_chunk(G, target):
    """group_chunk_items (gsr_common.h)."""
    batches, per = (G + 63) // 64, 1
    while per < 8 and batches > target * per:
        per *= 2
    return 64 * per


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def _tiny(case, P):
    case["sc"]["scaling"][:P] = 0.0005  # (a pixel radius of ceil(3 sqrt(0.3 + ~0)) = 2)


def _interior(g, n, W, H, corners=0.05):
    """Pixel positions inside their tile (one tile each); a fraction `corners` of them on a tile corner (four tiles)."""
    gx, gy = W // 16, H // 16
    px = 16.0 * g.integers(0, gx, n) + 3.0 + 9.0 * g.random(n)
    py = 16.0 * g.integers(0, gy, n) + 3.0 + 9.0 * g.random(n)
    c = g.random(n) < corners
    px[c] = 16.0 * g.integers(1, gx, int(c.sum())) - 0.5
    py[c] = 16.0 * g.integers(1, gy, int(c.sum())) - 0.5
    return px, py


def _mixed(name, g):
    """[near tiny | band of 64 | far tiny] in depth: the band starts at sorted position `near` of the one group."""
    W = H = 128
    ntiny, near = dict(mixed=(2400, 192), mixed_unaligned=(2400, 200), mixed_few=(100, 0))[name]
    P = ntiny + BAND
    case = S.axis_case(P, W, H, seed=P)
    _tiny(case, ntiny)
    case["sc"]["scaling"][ntiny:] = 6.0  # (hundreds of pixels)
    px, py = _interior(g, ntiny, W, H)
    d = np.concatenate([2.0 + np.arange(near) * 2.0 ** -10, 4.0 + g.integers(0, 4096, ntiny - near) * 2.0 ** -12,
                        3.0 + np.arange(BAND) * 2.0 ** -10])
    return S.place(case, np.concatenate([px, 40.0 + 48.0 * g.random(BAND)]), np.concatenate([py, 40.0 + 48.0 * g.random(BAND)]), d)


def _build(name):
    g = np.random.default_rng(sum(name.encode()))
    if name in MIXED:
        return _mixed(name, g)
    if name.startswith("segment_"):
        P, W, H = int(name[8:]), 128, 128
        case = S.axis_case(P, W, H, seed=P)
        _tiny(case, P)
        px, py = _interior(g, P, W, H, corners=0.0)
        return S.place(case, px, py, 3.0 + g.integers(0, 8192, P) * 2.0 ** -12)
    if name == "long_column":
        # 275 chunks of 64: 18 rows per wave of the column scan, i.e. TWO rows in its second round -- with one (17 000 Gaussians,
        # 266 chunks, 17 rows) the running sum of that round is never read
        P, W, H = 17600, 128, 128
        case = S.axis_case(P, W, H, seed=P)
        _tiny(case, P)
        px, py = _interior(g, P, W, H)
        return S.place(case, px, py, 3.0 + g.integers(0, 8192, P) * 2.0 ** -12)
    if name == "ragged":  # 13 x 9 tiles: groups (1, 0), (0, 1), (1, 1) hang over the image's edge
        ntiny, W, H = 1500, 200, 136
        P = ntiny + BAND
        case = S.axis_case(P, W, H, seed=P)
        _tiny(case, ntiny)
        case["sc"]["scaling"][ntiny:] = 6.0
        d = np.concatenate([2.0 + np.arange(128) * 2.0 ** -10, 4.0 + g.integers(0, 4096, ntiny - 128) * 2.0 ** -12,
                            3.0 + np.arange(BAND) * 2.0 ** -10])
        return S.place(case, np.concatenate([g.random(ntiny) * W, 60.0 + 80.0 * g.random(BAND)]),
                       np.concatenate([g.random(ntiny) * H, 40.0 + 56.0 * g.random(BAND)]), d)
    if name == "exact_fit":
        # batches 0, 1, 2 of the one group hold exactly 64, 960 and 1024 entries: batch 0 is 64 one-tile Gaussians, batch 1
        # 14 band Gaussians + 36 of one tile + 14 of two, batch 2 15 band + 34 of one tile + 15 of two; ~1400 one-tile ones behind
        W = H = 128
        ntiny, far = 64 + 50 + 49, 1400
        P = ntiny + far + 29
        case = S.axis_case(P, W, H, seed=P)
        _tiny(case, ntiny + far)
        case["sc"]["scaling"][ntiny + far:] = 6.0
        px, py = _interior(g, ntiny + far, W, H, corners=0.0)
        two = np.r_[64 + 36:64 + 50, 64 + 50 + 34:ntiny]  # on a vertical tile edge: two tiles
        px[two] = 16.0 * g.integers(1, W // 16, two.size) - 0.5
        step = 2.0 ** -10
        d = np.concatenate([2.0 + np.arange(64) * step, 2.25 + np.arange(14, 64) * step, 2.5 + np.arange(15, 64) * step,
                            4.0 + g.integers(0, 4096, far) * 2.0 ** -12, 2.25 + np.arange(14) * step, 2.5 + np.arange(15) * step])
        return S.place(case, np.concatenate([px, 40.0 + 48.0 * g.random(29)]), np.concatenate([py, 40.0 + 48.0 * g.random(29)]), d)
    if name == "hole":  # three groups side by side, the middle one (pixels 128 .. 255) empty
        P, W, H = 1200, 384, 128
        case = S.axis_case(P, W, H, seed=P)
        _tiny(case, P)
        px, py = _interior(g, P, 128, H, corners=0.0)
        px[P // 2:] += 256.0
        return S.place(case, px, py, 3.0 + g.integers(0, 8192, P) * 2.0 ** -12)
    raise KeyError(name)


def scene(name):
    if name == "four_groups_each":
        return S.scene(name)
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


def expectation(oracle, name):
    """The oracle's forward of a scene, computed once per process and left unchanged."""
    if name == "four_groups_each":
        return S.expectation(oracle, name)
    if name not in _oracle:
        _oracle[name] = oracle_forward(oracle, scene(name))
    return _oracle[name]


# ---- the census -------------------------------------------------------------------------------------------------------------
def tile_rects(f, W, H):
    """getRect (auxiliary.h:46-57) of every Gaussian from the forward's means2D and radii -> x0, y0, x1, y1 (exclusive)."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    m, r = f["means2D"].astype(np.float32), f["radii"].astype(np.float32)
    sixteen = np.float32(16.0)
    with np.errstate(invalid="ignore"):
        x0 = np.clip(((m[:, 0] - r) / sixteen).astype(np.int64), 0, gx)
        y0 = np.clip(((m[:, 1] - r) / sixteen).astype(np.int64), 0, gy)
        x1 = np.clip(((m[:, 0] + r + np.float32(15.0)) / sixteen).astype(np.int64), 0, gx)
        y1 = np.clip(((m[:, 1] + r + np.float32(15.0)) / sixteen).astype(np.int64), 0, gy)
    return x0, y0, x1, y1


def group_instances(f, W, H):
    """Per group, in group order: (Gaussian indices, tiles of rectangle ^ group) of its instances in the stable depth order
    of the visible Gaussians -> list over the sgx * sgy groups, R, G."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    sgx, sgy = (gx + GROUP_EDGE - 1) // GROUP_EDGE, (gy + GROUP_EDGE - 1) // GROUP_EDGE
    x0, y0, x1, y1 = tile_rects(f, W, H)
    visible = (f["radii"] > 0) & ((x1 - x0) * (y1 - y0) > 0)
    assert np.array_equal(np.where(visible, (x1 - x0) * (y1 - y0), 0), f["tiles_touched"].astype(np.int64))
    idx = np.flatnonzero(visible)
    idx = idx[np.argsort(f["depths"][idx].view(np.uint32), kind="stable")]  # (positive floats order like their bits)
    per = [([], []) for _ in range(sgx * sgy)]
    for i in idx.tolist():
        for sy in range(y0[i] // GROUP_EDGE, (y1[i] - 1) // GROUP_EDGE + 1):
            for sx in range(x0[i] // GROUP_EDGE, (x1[i] - 1) // GROUP_EDGE + 1):
                w = min(x1[i], (sx + 1) * GROUP_EDGE) - max(x0[i], sx * GROUP_EDGE)
                h = min(y1[i], (sy + 1) * GROUP_EDGE) - max(y0[i], sy * GROUP_EDGE)
                per[sy * sgx + sx][0].append(i)
                per[sy * sgx + sx][1].append(int(w * h))
    per = [(np.array(a, dtype=np.int64), np.array(b, dtype=np.int64)) for a, b in per]
    return per, int(sum(b.sum() for _, b in per)), int(sum(b.size for _, b in per))


def census(f, W, H, chunk, K):
    """What group_chunk_kernel<append, chunk / 64> and group_colscan_kernel meet on the forward `f` of a W x H view, from the
    oracle's forward alone.  K: kernel_constants()."""
    per, R, G = group_instances(f, W, H)
    assert R == f["num_rendered"]
    cap = K["CAP_SMALL"] if (R // G + 1) * chunk <= K["STAGE_BOUND"] else K["CAP_LARGE"]
    out = dict(NB=chunk // 64, cap=cap, R=R, G=G, nparts={1: 0, 2: 0, 4: 0}, mid_chunk_flushes=0, eq_batch=0, eq_half=0, eq_part=0,
               eq_staged=0, chunks_per_group=[], empty_groups=0, padding_batches=0, partial_batches=0, partial_later_batches=0,
               one_item_batches=0, full_segments=0, mixed_part_chunks=0, part_totals=[], batches=[])
    for _, tiles in per:
        n = tiles.size
        out["chunks_per_group"].append((n + chunk - 1) // chunk)
        out["empty_groups"] += n == 0
        out["full_segments"] += n > 0 and n % chunk == 0
        for c0 in range(0, n, chunk):
            staged, kinds = 0, set()
            for b in range(chunk // 64):
                t = tiles[c0 + 64 * b:min(n, c0 + 64 * b + 64)]
                if t.size == 0:  # (the kernel's `break`: counted once per chunk that ends in padding-only batches)
                    out["padding_batches"] += 1
                    break
                out["partial_batches"] += t.size < 64
                out["partial_later_batches"] += b > 0 and t.size < 64
                out["one_item_batches"] += t.size == 1
                tot_l, tot_h = int(t[:32].sum()), int(t[32:].sum())
                nparts = 1 if tot_l + tot_h <= cap else (2 if max(tot_l, tot_h) <= cap else 4)
                out["nparts"][nparts] += 1
                out["batches"].append((nparts, int(t.size), tot_l, tot_h))
                kinds.add(nparts)
                out["eq_batch"] += tot_l + tot_h == cap
                out["eq_half"] += nparts == 2 and max(tot_l, tot_h) == cap
                parts = {1: [t], 2: [t[:32], t[32:]], 4: [t[:16], t[16:32], t[32:48], t[48:]]}[nparts]
                for p in parts:
                    total = int(p.sum())
                    assert total <= cap
                    out["part_totals"].append((nparts, total))
                    out["eq_part"] += total == cap
                    if staged + total > cap:
                        out["mid_chunk_flushes"] += staged > 0
                        staged = 0
                    out["eq_staged"] += staged > 0 and staged + total == cap
                    staged += total
            out["mixed_part_chunks"] += len(kinds) > 1
    return out


def scene_census(oracle, name, chunk):
    if (name, chunk) not in _census:
        case = scene(name)
        _census[name, chunk] = census(expectation(oracle, name), case["W"], case["H"], chunk, kernel_constants())
    return _census[name, chunk]


def colscan_rows(chunks, K):
    """Rows (chunks) per wave of group_colscan_kernel for a group of `chunks` chunks."""
    per = (chunks + K["COLSCAN_WAVES"] - 1) // K["COLSCAN_WAVES"]
    return [min(chunks, w * per + per) - min(chunks, w * per) for w in range(K["COLSCAN_WAVES"])]


# ---- the GPU comparison -----------------------------------------------------------------------------------------------------
def check_scene(oracle, name, chunk, allocator=None):
    """test_gpu_round3._lists_match on a scene, bit for bit, + exactly the predicted count and append counters rose -> what the
    run left.  `allocator`: a context manager factory the forward runs under (guarded_alloc.GuardedAllocator)."""
    case = scene(name)
    f = expectation(oracle, name)
    cs = scene_census(oracle, name, chunk)
    before = launches()
    if allocator is None:
        R, color, radii, st, _ = S.forward(case)
    else:
        with allocator() as ga:
            R, color, radii, st, _ = S.forward(case)
        ga.assert_clean()
        assert len(ga) > 0
    rose = launches() - before
    assert R == f["num_rendered"] == cs["R"], name
    assert np.array_equal(st["point_list"], f["point_list"]) and np.array_equal(st["keys"], f["keys"]), name
    assert np.array_equal(st["ranges"], f["ranges"]), name
    assert np.array_equal(st["n_contrib"], f["n_contrib"]), name
    assert np.array_equal(color.view(np.uint32), f["color"].view(np.uint32)), name
    want = np.zeros(16, dtype=np.int64)
    want[count_index(chunk)] = want[append_index(chunk, cs["cap"])] = 1
    assert np.array_equal(rose, want), (name, S.counter_table(rose), S.counter_table(want))
    print(f"  {name}: {case['W']}x{case['H']} R {R} G {cs['G']} chunk {chunk} cap {cs['cap']}, parts {cs['nparts']}, "
          f"{cs['mid_chunk_flushes']} mid-chunk flushes, rose {S.counter_table(rose)}")
    return dict(point_list=st["point_list"], color=color)


__all__ = ["CHUNKS", "NEVER", "SCENES", "census", "scene", "expectation", "check_scene", "launches"]
