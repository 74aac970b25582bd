"""-m gpu: the grouped binning's chunk stage -- group_chunk_kernel<count | append, NB> with its 64 x 64 bit transpose, LDS stage
and per-batch split, and group_colscan_kernel (gsr_binning.hip) -- at EVERY chunk length (NB = 1, 2, 4, 8) and both stage
sizes, each run proving what it launched (gsr_debug_group_launches: exactly the predicted count and append counter rose) under
the comparison of test_gpu_round3.py::_lists_match: num_rendered, point_list, the 64-bit keys, ranges, n_contrib and the
colour image equal the CPU oracle's bit for bit (integers and exactly specified floats: no tolerance).
Scenes, the census that predicts each run's regime, counter indices and the indices no host code launches (7, 8 .. 11):
tests/chunk_matrix_helpers.py; that every scene is in the regime it claims: tests/test_cpu_chunk_matrix.py, without a GPU.

Scenes (128 x 128 = one group unless said; what each pins):
  mixed             2400 tiny Gaussians + a band of 64 screen-filling ones at sorted positions 192 .. 255: the band is one batch
                    at every chunk length.  Chunk 64 / 128 / 256: stage of 1024, the batch in FOUR quarters of exactly 1024
                    entries (the `m = 0xffff << 16 * (part & 1)` branch); chunk 512: stage of 2048, two halves of exactly 2048;
                    chunk >= 128: a flush in the middle of the chunk;
  mixed_unaligned   the band at 200 .. 263: two batches of tiny + band items, four parts and one part side by side;
  mixed_few         the band + 100 tiny ones: a heavy mean, stage of 2048 at chunk 64 already, halves;
  exact_fit         batches of exactly 64, 960 and 1024 entries: tot_l + tot_h == cap (one part) and staged + total == cap
                    (no flush) at cap 1024; 64 + 960 + 1024 == 2048 at chunk 512;
  segment_<P>       P = 1, 64, 65, 128, 129, 193, 256, 257, 449, 512, 513 one-tile Gaussians = chunk - 63, chunk, chunk + 1 of
                    every length, and 65: a last batch of one item, no padding at all, a chunk whose later batches are all
                    padding (the `break`), a second batch with one valid lane;
  long_column       17 600 tiny ones: 275 chunks of 64 in one group -- the column scan's second round with ragged slabs (18 rows
                    per wave, 5 in the last; 17 000 would give 17 rows, one row in that round, whose running sum nobody
                    reads); 35 chunks of 512: waves without rows;
  ragged            200 x 136 = 13 x 9 tiles in 2 x 2 groups, three of them hanging over the image's edge (lanes without a
                    tile), band + 1500 tiny ones;
  hole              384 x 128, three groups, the middle one empty: run under guarded_alloc.GuardedAllocator (patterns 0xFF and
                    0x5A, as test_gpu_guard_bands.py runs its cells), so that a tile_total entry the column scan did not
                    write cannot pass for zero;
  four_groups_each  sort_matrix_helpers': 2064 x 2064, 289 groups of 11-bit ids with <= 36 instances each: one chunk per
                    group, at chunk >= 128 every one ends in padding-only batches.

Processes:
  a. this one (GSR_GROUP_CHUNK unset: asserted): every scene at the chunk length its G picks, 64;
  b. THREE fresh processes, one after the other, under GSR_GROUP_CHUNK=128, 256, 512: every scene again, point lists and
     images byte-identical to the ones (a) left.  Their tests are defined only there and reached through the parent's test
     alone, which asserts their number.
  Coverage (last test of each process): every reachable counter of the process >= 1, every other one 0 -- in (a) as
  increments since the file's first test, since other files of the suite bin in this process too.

Measured on the MI355X (the file run alone; R instances, G group instances):
  mixed R 6 895 G 2 464      mixed_unaligned R 6 859 G 2 464   mixed_few R 4 208 G 164      exact_fit R 3 448 G 1 592
  segment_<P> R = G = P      long_column R 20 207 G 17 600     ragged R 10 005 G 1 845      hole R 1 200 G 1 200
  four_groups_each R 8 400 G 8 400
  stage: 1024 entries everywhere at chunk 64 / 128 / 256 except mixed_few (2048 throughout) and ragged at 256 (R / G = 5:
  6 x 256 > 820); 2048 everywhere at chunk 512.  Every run raised its count counter and its append counter by one.
  counters at the end of each process:
    a (64)  [0]=20 [4]=19 [12]=1      128  [1]=20 [5]=19 [13]=1      256  [2]=20 [6]=18 [14]=2      512  [3]=20 [15]=20
    (19 scenes, 20 forwards: hole runs under both patterns)
  time: the file 14.6 s, of which the fresh processes 3.8 s (128), 3.9 s (256) and 4.1 s (512), their 20 tests 2.3 - 2.4 s
    each; in-process tests: mixed 0.37 s (the oracle's and the library's first call), hole 0.18 s (two guarded runs),
    four_groups_each 0.04 s, long_column 0.03 s, every other one <= 0.01 s.

Mutants.  The tests were run once against four scratch builds of gsr_binning.hip (never committed).  Each keeps every store
in bounds and may reorder or drop entries but adds none; memory a mutant leaves unwritten was made to read as index 0 for
these runs (zero-filled allocations in place of stale bytes or poison), so that a dropped entry could not become a wild
Gaussian index in the blend.  No run faulted.  Every failure is the bit-for-bit comparison of point_list / keys.  The fresh
processes were run on the mutant with the parent on the real library (a parent whose own scene fails does not start them):
  1. the quarter mask uses !(part & 1)
       chunk 64: test_scene[mixed], [mixed_unaligned], [ragged];  128: the same three;  256: mixed, mixed_unaligned (ragged
       has the stage of 2048 there);  512: passes -- no view has quarters at 2048, as the census says.
  2. the two halves are taken in swapped order
       chunk 64: test_scene[mixed_few];  128: mixed_few;  256: mixed_few, ragged;  512: mixed, mixed_unaligned, mixed_few, ragged.
  3. the column scan's second round omits run += v[i]
       chunk 64: test_scene[long_column] alone;  128 / 256 / 512 pass: 138 chunks and fewer are at most 9 rows per wave, no
       second round.  (At 17 000 Gaussians -- 17 rows per wave, ONE row in the second round -- this mutant passed the census's
       "second round is entered" and would have passed here: the scene has 17 600 for its second row.)
  4. a later batch's items are skipped when its first lane is padding
       As worded this is the code itself: padding only follows the items of a chunk, so a batch whose first lane is padding is
       all padding, which is the kernel's `break`.  Built instead: a later batch is skipped when ANY lane is padding.
       chunk 64: passes (no later batch);  128: segment_65, segment_193, segment_449, ragged, hole;  256: those + mixed,
       mixed_unaligned, mixed_few, segment_129;  512: those + segment_257.
  Not built, on purpose: a mutant that skips a flush, widens a write or overruns the stage.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import chunk_matrix_helpers as C
from guarded_alloc import GuardedAllocator

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "GSR_GROUP_CHUNK"
#: set in the fresh processes: "<chunk>:<npz of process a's lists and images>"
CHILD = os.environ.get("GSR_CHUNK_MATRIX_CHILD")
CHUNK = 64 if CHILD is None else int(CHILD.split(":", 1)[0])
PATTERNS = (0xFF, 0x5A)
_state, _left = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _knob():
    """A chunk knob in the environment would turn this file into a test of something else, so it FAILS (a child runs under
    exactly the knob its parent gave it).  The counters of the file's start: other files bin in this process too."""
    assert os.environ.get(KNOB) == (None if CHILD is None else str(CHUNK)), f"{KNOB}={os.environ.get(KNOB)} in a process that runs chunk {CHUNK}"
    _state["start"] = C.launches()
    yield


def _run(oracle, name):
    if name != "hole":
        return C.check_scene(oracle, name, CHUNK)
    runs = [C.check_scene(oracle, name, CHUNK, allocator=lambda p=p: GuardedAllocator(p)) for p in PATTERNS]
    for k, v in runs[0].items():  # (nothing read depends on the poison)
        assert v.tobytes() == runs[1][k].tobytes(), k
    return runs[0]


def _coverage():
    rose = C.launches() - _state["start"]
    want = C.reachable(CHUNK)
    print(f"  chunk {CHUNK}: {C.S.counter_table(rose)}")
    assert all(rose[i] >= 1 for i in want), (want, C.S.counter_table(rose))
    assert not any(rose[i] for i in range(16) if i not in want), (want, C.S.counter_table(rose))


if CHILD is None:
    @pytest.mark.parametrize("name", C.SCENES)
    def test_scene(oracle, name):
        _left[name] = _run(oracle, name)

    @pytest.mark.parametrize("chunk", C.CHUNKS[1:])
    def test_scenes_in_a_fresh_process(oracle, tmp_path, chunk):
        for name in C.SCENES:  # (run alone: this test takes process a's runs itself)
            if name not in _left:
                _left[name] = _run(oracle, name)
        path = str(tmp_path / "chunk64.npz")
        np.savez(path, **{f"{n}.{k}": v for n, r in _left.items() for k, v in r.items()})
        env = {k: v for k, v in os.environ.items() if k != KNOB}
        t0 = time.time()
        p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", os.path.abspath(__file__), "-k", "chunk_child"],
                           capture_output=True, text=True, timeout=300, cwd=ROOT,
                           env=dict(env, GSR_CHUNK_MATRIX_CHILD=f"{chunk}:{path}", **{KNOB: str(chunk)}))
        assert p.returncode == 0, (p.stdout + p.stderr)[-6000:]
        assert f"{len(C.SCENES) + 1} passed" in p.stdout, p.stdout[-3000:]
        # (-q -s: pytest's progress dots sit in front of a test's first line)
        print("\n".join(ln.lstrip(".") for ln in p.stdout.splitlines() if ln.lstrip(".").startswith("  ") or "passed" in ln))
        print(f"  fresh process (chunk {chunk}): {time.time() - t0:.1f} s")

    def test_every_chunk_64_instantiation_of_this_process_was_launched():
        """Reachable with the knob unset on these sizes: the count pass and both stage sizes of the append pass at NB = 1
        (0, 4, 12).  Not in this process: every NB > 1 (the three fresh processes)."""
        _coverage()

else:
    @pytest.mark.parametrize("name", C.SCENES)
    def test_chunk_child_scene(oracle, name):
        got = _run(oracle, name)
        want = np.load(CHILD.split(":", 1)[1])  # against the chunk-64 run of the parent's process, byte for byte
        for k, v in got.items():
            assert v.tobytes() == want[f"{name}.{k}"].tobytes(), (name, k)

    def test_chunk_child_coverage():
        """128: 1, 5, 13; 256: 2, 6, 14; 512: 3, 15 (7 -- a chunk of 512 with the stage of 1024 -- is never launched)."""
        _coverage()
