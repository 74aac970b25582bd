"""Without a GPU: every scene of tests/chunk_matrix_helpers.py reaches the regime of group_chunk_kernel / group_colscan_kernel
it is named for, at the chunk lengths it claims -- read off the census (chunk_matrix_helpers.census), which restates from the
CPU oracle's forward alone what the chunk kernels will meet.  Conditions, not measurements: nothing here looks at what the
library computes.

The constants the scenes were sized by -- GROUP_CHUNKS_TARGET, the 820 of the stage rule with its 1024 / 2048, COLSCAN_WAVES,
COLSCAN_REG -- and the text of the part, flush and chunk rules are parsed out of the sources, so that a change of one of them
fails here instead of moving a scene of tests/test_gpu_chunk_matrix.py out of its regime without a word.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import chunk_matrix_helpers as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = C.kernel_constants()
QUARTERS = (64, 128, 256)  # the chunk lengths at which the `mixed` views keep the stage of 1024 entries


def _cs(oracle, name, chunk):
    return C.scene_census(oracle, name, chunk)


def test_constants_are_the_ones_the_scenes_were_sized_by():
    assert K == dict(GROUP_CHUNKS_TARGET=16384, STAGE_BOUND=820, CAP_SMALL=1024, CAP_LARGE=2048, COLSCAN_WAVES=16, COLSCAN_REG=16)
    t = K["GROUP_CHUNKS_TARGET"]
    assert [C.natural_chunk(g, t) for g in (1, 64 * t, 64 * t + 1, 128 * t, 128 * t + 1, 256 * t, 256 * t + 1, 1 << 30)] == \
        [64, 64, 128, 128, 256, 256, 512, 512]
    # the indices no host code launches: a chunk of 512 never has the stage of 1024 entries (R >= G); the count pass has none
    assert min((r_over_g + 1) * 512 for r_over_g in (1, 2)) > K["STAGE_BOUND"]
    assert C.NEVER == (7, 8, 9, 10, 11) and C.append_index(512, 1024) == 7
    assert [C.reachable(c) for c in C.CHUNKS] == [(0, 4, 12), (1, 5, 13), (2, 6, 14), (3, 15)]


def test_knob_is_read_by_the_size_query_and_other_values_count_as_unset():
    """gsr_scratch_sizes in fresh processes (the knob is read once): the binning scratch holds `chunks * chunk` padded slots
    twice (keys, indices: 4 bytes each) and 64 counts + 64 prefixes per chunk (2 + 4 bytes), chunks = G / chunk + groups."""
    code = "from gaussianeditor_amd import _native; print(_native.scratch_sizes(1000, {R}, 640, 360, {G})[1])"

    def size(value, R, G):
        env = {k: v for k, v in os.environ.items() if k != "GSR_GROUP_CHUNK"}
        if value is not None:
            env["GSR_GROUP_CHUNK"] = value
        p = subprocess.run([sys.executable, "-c", code.format(R=R, G=G)], capture_output=True, text=True, cwd=ROOT, env=env, timeout=60)
        assert p.returncode == 0, p.stderr[-2000:]
        return int(p.stdout)

    groups = ((640 // 16 + 7) // 8) * (((360 + 15) // 16 + 7) // 8)  # 5 x 3

    def sections(G, chunk):  # the four sections that depend on the chunk length, each rounded up to 256 bytes
        chunks = G // chunk + groups
        up = lambda n: (n + 255) // 256 * 256  # noqa: E731
        return 2 * up(4 * chunks * chunk) + up(2 * 64 * chunks) + up(4 * 64 * chunks)

    R, G = 9000, 3000  # chunk 64 by its size
    unset = size(None, R, G)
    for value in ("64", "100", "0", "1024", "abc", ""):
        assert size(value, R, G) == unset, value
    for chunk in (128, 256, 512):
        assert size(str(chunk), R, G) - unset == sections(G, chunk) - sections(G, 64), chunk
    R, G = 9_000_000, 3_000_000  # chunk 256 by its size
    assert C.natural_chunk(G, K["GROUP_CHUNKS_TARGET"]) == 256
    unset = size(None, R, G)
    assert size("256", R, G) == unset and size("7", R, G) == unset
    assert size("64", R, G) - unset == sections(G, 64) - sections(G, 256)


@pytest.mark.parametrize("name", C.SCENES)
def test_unset_knob_means_chunk_64(oracle, name):
    """Every scene is far below the first natural threshold: with GSR_GROUP_CHUNK unset its chunk length is 64."""
    cs = _cs(oracle, name, 64)
    assert C.natural_chunk(cs["G"], K["GROUP_CHUNKS_TARGET"]) == 64 and 0 < cs["G"] <= cs["R"]


@pytest.mark.parametrize("name", ("mixed", "ragged", "exact_fit", "hole"))
def test_census_order_is_the_oracles_point_list(oracle, name):
    """The census's own reading of the forward -- getRect, stable depth order -- rebuilds the oracle's point_list."""
    case, f = C.scene(name), C.expectation(oracle, name)
    gx = (case["W"] + 15) // 16
    x0, y0, x1, y1 = C.tile_rects(f, case["W"], case["H"])
    per, R, G = C.group_instances(f, case["W"], case["H"])
    lists = {}
    for s, (idx, tiles) in enumerate(per):
        for i, n in zip(idx.tolist(), tiles.tolist()):
            sx, sy = s % ((gx + 7) // 8), s // ((gx + 7) // 8)
            mine = [(y, x) for y in range(max(y0[i], 8 * sy), min(y1[i], 8 * sy + 8)) for x in range(max(x0[i], 8 * sx), min(x1[i], 8 * sx + 8))]
            assert len(mine) == n
            for y, x in mine:
                lists.setdefault(y * gx + x, []).append(i)
    rebuilt = np.array([i for t in sorted(lists) for i in lists[t]], dtype=np.uint32)
    assert np.array_equal(rebuilt, f["point_list"]) and R == f["num_rendered"]


def test_mixed_quarters_halves_and_flushes(oracle):
    f, case = C.expectation(oracle, "mixed"), C.scene("mixed")
    (idx, tiles), = C.group_instances(f, case["W"], case["H"])[0]
    # 192 tiny ones, then exactly the 64 band Gaussians, each on all 64 tiles of the one group: a batch of its own at every length
    assert (tiles[192:256] == 64).all() and (tiles[:192] <= 4).all() and (tiles[256:] <= 4).all() and (idx[192:256] >= 2400).all()
    for chunk in C.CHUNKS:
        cs = _cs(oracle, "mixed", chunk)
        band = cs["batches"][3]
        if chunk in QUARTERS:  # four quarters of exactly 1024 entries = cap
            assert cs["cap"] == 1024 and band == (4, 64, 2048, 2048) and cs["nparts"] == {1: 38, 2: 0, 4: 1}
            assert cs["part_totals"].count((4, 1024)) == 4 and cs["eq_part"] == 4
        else:                  # chunk 512: two halves of exactly 2048 entries = cap
            assert cs["cap"] == 2048 and band == (2, 64, 2048, 2048) and cs["nparts"] == {1: 38, 2: 1, 4: 0}
            assert cs["part_totals"].count((2, 2048)) == 2 and cs["eq_half"] == 1
        if chunk >= 128:       # the band's batch is not the first of its chunk: the stage holds the tiny ones in front of it
            assert cs["mid_chunk_flushes"] >= 1 and cs["mixed_part_chunks"] == 1


def test_mixed_unaligned_and_few(oracle):
    f, case = C.expectation(oracle, "mixed_unaligned"), C.scene("mixed_unaligned")
    (_, tiles), = C.group_instances(f, case["W"], case["H"])[0]
    assert (tiles[200:264] == 64).all() and (tiles[:200] <= 4).all() and (tiles[264:] <= 4).all()
    for chunk in C.CHUNKS:
        cs = _cs(oracle, "mixed_unaligned", chunk)
        b3, b4 = cs["batches"][3], cs["batches"][4]  # 8 tiny + 56 band | 8 band + 56 tiny
        assert b3[2] > 1024 and b3[3] == 2048 and 512 < b4[2] + b4[3] <= 1024
        assert (b3[0], b4[0], cs["cap"]) == ((4, 1, 1024) if chunk in QUARTERS else (2, 1, 2048))
    for chunk in C.CHUNKS:  # few tiny ones: a heavy mean, the stage of 2048 entries at every length, halves
        cs = _cs(oracle, "mixed_few", chunk)
        assert cs["cap"] == 2048 and cs["nparts"] == {1: 2, 2: 1, 4: 0} and cs["batches"][0] == (2, 64, 2048, 2048)


def test_exact_fit_hits_both_equalities(oracle):
    """tot_l + tot_h == cap (one part, no split) and staged + total == cap with staged > 0 (no flush)."""
    for chunk in C.CHUNKS:
        cs = _cs(oracle, "exact_fit", chunk)
        assert [b[2] + b[3] for b in cs["batches"][:3]] == [64, 960, 1024] and cs["nparts"][2] == cs["nparts"][4] == 0
        assert cs["cap"] == (1024 if chunk in QUARTERS else 2048)
        assert cs["eq_batch"] == (1 if chunk in QUARTERS else 0)      # batch 2 alone fills the stage of 1024
        assert cs["eq_staged"] == (0 if chunk == 64 else 1)           # 64 + 960 = 1024; at 512: 64 + 960 + 1024 = 2048
        assert cs["mid_chunk_flushes"] == {64: 0, 128: 1, 256: 2, 512: 1}[chunk]


@pytest.mark.parametrize("chunk", C.CHUNKS)
def test_segments(oracle, chunk):
    nb = chunk // 64
    for P in (chunk - 63, chunk, chunk + 1) + ((65,) if chunk >= 128 else ()):
        cs = _cs(oracle, f"segment_{P}", chunk)
        assert cs["G"] == cs["R"] == P and cs["nparts"] == {1: (P + 63) // 64, 2: 0, 4: 0}  # every Gaussian visible, one tile each
        assert cs["cap"] == (1024 if chunk in QUARTERS else 2048)
    a, b, c = (_cs(oracle, f"segment_{P}", chunk) for P in (chunk - 63, chunk, chunk + 1))
    # chunk - 63: one chunk whose LAST batch holds one item -- no padding-only batch
    assert a["chunks_per_group"] == [1] and a["one_item_batches"] == 1 and a["padding_batches"] == 0 and a["batches"][-1][1] == 1
    assert len(a["batches"]) == nb and a["partial_later_batches"] == (1 if nb > 1 else 0)
    # chunk: no padding at all
    assert b["chunks_per_group"] == [1] and b["full_segments"] == 1 and b["partial_batches"] == b["padding_batches"] == 0
    # chunk + 1: a second chunk of one item whose later batches are all padding
    assert c["chunks_per_group"] == [2] and c["one_item_batches"] == 1 and c["padding_batches"] == (1 if nb > 1 else 0)
    assert c["partial_later_batches"] == 0
    if chunk >= 128:  # 65: the SECOND batch has one valid lane
        d = _cs(oracle, "segment_65", chunk)
        assert [x[1] for x in d["batches"]] == [64, 1] and d["partial_later_batches"] == 1 and d["padding_batches"] == (1 if nb > 2 else 0)


def test_long_column_colscan_rounds(oracle):
    at64, at512 = _cs(oracle, "long_column", 64), _cs(oracle, "long_column", 512)
    n = at64["chunks_per_group"][0]
    assert n > K["COLSCAN_WAVES"] * K["COLSCAN_REG"]  # the second round
    rows = C.colscan_rows(n, K)
    assert max(rows) >= K["COLSCAN_REG"] + 2  # (two rows in that round: the first one's count is carried into the second's prefix)
    assert 0 < rows[-1] < rows[0] and rows[-1] % K["COLSCAN_REG"] != 0 and sum(rows) == n
    rows = C.colscan_rows(at512["chunks_per_group"][0], K)
    assert rows.count(0) >= 2 and rows[0] > 1 and 0 < min(r for r in rows if r) < rows[0]  # waves without rows, a ragged one
    for chunk in C.CHUNKS:
        assert _cs(oracle, "long_column", chunk)["nparts"][1] == n


def test_ragged_hole_and_many_groups(oracle):
    case = C.scene("ragged")
    gx, gy = (case["W"] + 15) // 16, (case["H"] + 15) // 16
    assert (gx, gy) == (13, 9)  # 2 x 2 groups; (1, 0), (0, 1), (1, 1) have lanes without a tile (tile_ok false)
    for chunk in C.CHUNKS:
        cs = _cs(oracle, "ragged", chunk)
        assert len(cs["chunks_per_group"]) == 4 and min(cs["chunks_per_group"]) >= 1
        assert cs["nparts"][4 if chunk <= 128 else 2] >= 1 and cs["mid_chunk_flushes"] >= 1
        h = _cs(oracle, "hole", chunk)
        assert len(h["chunks_per_group"]) == 3 and h["chunks_per_group"][1] == 0 and h["empty_groups"] == 1
        assert h["chunks_per_group"][0] > 0 and h["chunks_per_group"][2] > 0
        m = _cs(oracle, "four_groups_each", chunk)
        assert len(m["chunks_per_group"]) == 289 > 256 and set(m["chunks_per_group"]) == {1} and m["partial_batches"] == 289
        assert m["padding_batches"] == (289 if chunk >= 128 else 0)


def test_every_reachable_append_instantiation_has_a_scene(oracle):
    got = {(chunk // 64, _cs(oracle, name, chunk)["cap"]) for name in C.SCENES for chunk in C.CHUNKS}
    assert got == {(1, 1024), (1, 2048), (2, 1024), (2, 2048), (4, 1024), (4, 2048), (8, 2048)}
    for chunk in C.CHUNKS:
        caps = {_cs(oracle, name, chunk)["cap"] for name in C.SCENES}
        assert {C.append_index(chunk, cap) for cap in caps} | {C.count_index(chunk)} == set(C.reachable(chunk))
