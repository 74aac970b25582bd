"""-m gpu: every reachable instantiation of the binning's three stable radix scatter kernels -- sort_scatter_kernel<IOTA, K, TH>,
depth_scatter_kernel<LAST, IOTA, TH>, group_scatter_kernel<BITS, TH> (gsr_binning.hip), 20 in all -- and the carry round of
sort_scan_kernel, at BOTH block widths, each run proving what it launched (gsr_debug_sort_launches: exactly the expected
counters rose) under the comparison of test_gpu_round3.py::_lists_match: num_rendered, point_list, the 64-bit keys, ranges,
n_contrib and the colour image equal the CPU oracle's bit for bit (integers and exactly specified floats: no tolerance).
Scenes, counter indices and the indices that no host code launches (1, 5, 11, 15): tests/sort_matrix_helpers.py.

Scenes (depths and positions set by hand; what each pins):
  flat                P 8193 (blocks of 4096, 4096, 1), one plane: ALL depth keys tie -- the order is pure stability across
                      lanes, waves and blocks;
  two_depths          P 4097, even / odd indices at two depths: alternating digits in every ballot;
  deep                P 4095, depths 0.25 .. 60: four passes, last wave partial;
  culled_interleaved  P 4160, every third Gaussian behind the camera: culled keys sort last, among live ones;
  low_byte, high_byte P 5000, depth keys that differ in the lowest / the highest byte only: every other pass sees one bin
                      holding whole blocks;
  tiny1, 63, 64, 65   one partial wave;
  one_group_of_many   2064 x 2064 (289 groups: BITS = 11), everything inside group (8, 8): 2047 empty bins, padded segments;
  four_groups_each    the same image, P 2100 centred on the corners of the group grid: four group instances each, G = 8400
                      in three blocks;
  one_group           128 x 128: BITS = 8, one bin;
  tile_keys_32        4112 x 4096 = 65 792 tiles: the tile-pair sort by image size, 17-bit tile ids in three passes.

Processes:
  a. this one (no GSR_SORT_THREADS, no GSR_BIN_LEGACY: asserted): all scenes; wide counters only;
  b. ONE fresh process under GSR_SORT_THREADS=256: all scenes, narrow counters only, point lists and images byte-identical to
     the ones (a) left; it also runs test_gpu_parity.py -k "test_knn_bit_exact_vs_oracle or test_random_configuration_sweep
     or test_depth_key_ranges" and test_gpu_round3.py::test_grouped_binning_shapes under the knob;
  c. ONE fresh process under GSR_SORT_THREADS=256 GSR_BIN_LEGACY=1: the ten depth scenes on the pair-sort path (16-bit keys);
  d. ONE fresh process under GSR_BIN_LEGACY=1 alone: the depth scenes at the width the size picks (wide), and `scan_carry`:
     a 1080p view with R > 2048 x 4096 instances, whose pair sort is narrow by its size and whose per-bin scan takes a second
     round behind a carry; held to sort_matrix_helpers.assert_sorted_list_invariants (the checks of
     test_gpu_properties.py::test_full_size_sorted_list_invariants; the oracle is not used at this size).
  The children's tests are defined only there and reached through their parent test alone, which asserts their number.
  Coverage (last test of each process): every reachable counter of the process >= 1, every other one 0 -- in (a) as
  increments since the file's first test, since other files of the suite sort in this process too.

Measured on the MI355X (R; depth passes of the grouped path / of the pair-sort path; the pair sort itself is one pass on these
images, three on tile_keys_32):
  flat 22 352, 3 / 2        two_depths 10 390, 3 / 3    deep 41 459, 4 / 4       culled_interleaved 7 641, 3 / 3
  low_byte 13 376, 3 / 2    high_byte 44 770, 4 / 4     tiny1 2, 3 / 2           tiny63 182, tiny64 194, tiny65 191: 3 / 3
  one_group_of_many 18 305, 3   four_groups_each 8 400, 3   one_group 11 370, 3   tile_keys_32 30 169, - / 3
  a scene of the grouped path launches depth [IOTA] 1, [plain] passes - 2, [LAST] 1 and one group scatter; of the pair-sort
  path [IOTA, uint32] 1, [uint32] passes - 1 and the tile-pair passes (tile_keys_32: [uint32] 2 + 3 = 5).
  counters at the end of each process (the file run alone):
    a  [6]=5 [7]=1 [12]=15 [13]=13 [14]=13 [18]=11 [19]=2
    b  [2]=32 [3]=10 [8]=50 [9]=45 [10]=45 [16]=41 [17]=2     (44 tests: 29 of the two other files, 14 scenes, coverage)
    c  [0]=10 [2]=19 [3]=10
    d  [0]=2 [4]=10 [6]=21 [7]=11 [20]=2
  scan_carry: 500 000 Gaussians at s0 = 0.04, R = 16 758 528 = 4092 blocks (two rounds of the scan), 3 depth passes, rose
    [0]=2 [6]=2 [7]=1 [20]=2; scene + forward + export 0.1 s, the invariants 0.2 s.
  time: the file 18.5 s, of which the fresh processes 6.8 s (b; its 44 tests 4.7 s), 4.5 s (c) and 4.4 s (d); in-process tests:
    flat 0.26 s (the oracle's first call), tile_keys_32 0.13 s, every other one <= 0.04 s.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import sort_matrix_helpers as S
from helpers import make_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
#: set in the fresh processes ("narrow:<npz of process a's lists and images>", "legacy_narrow", "legacy")
CHILD = os.environ.get("GSR_SORT_MATRIX_CHILD")
MODE = None if CHILD is None else CHILD.split(":", 1)[0]
KNOBS = ("GSR_SORT_THREADS", "GSR_BIN_LEGACY")
CHILD_KNOBS = {None: {}, "narrow": dict(GSR_SORT_THREADS="256"), "legacy_narrow": dict(GSR_SORT_THREADS="256", GSR_BIN_LEGACY="1"),
               "legacy": dict(GSR_BIN_LEGACY="1")}
FORCED = 256 if MODE in ("narrow", "legacy_narrow") else 0
LEGACY = MODE in ("legacy_narrow", "legacy")
SCAN_CARRY_P = 500_000
_state, _left = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _knobs():
    """A width or path knob in the environment would turn this file into a test of something else, so it FAILS (a child runs
    under exactly the knobs its parent gave it).  The counters of the file's start: other files sort in this process too."""
    have = {k: os.environ[k] for k in KNOBS if k in os.environ}
    assert have == CHILD_KNOBS[MODE], f"{have}: this process of the sort matrix runs under {CHILD_KNOBS[MODE]}"
    _state["start"] = S.launches()
    yield


def _fresh(mode, arg, files, select, passed, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    t0 = time.time()
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu"] + files + [os.path.abspath(__file__), "-k", select],
                       capture_output=True, text=True, timeout=timeout, cwd=ROOT,
                       env=dict(env, GSR_SORT_MATRIX_CHILD=mode + arg, **CHILD_KNOBS[mode]))
    assert p.returncode == 0, (p.stdout + p.stderr)[-6000:]
    assert f"{passed} passed" in p.stdout, p.stdout[-3000:]
    # (-q -s: pytest's progress dots sit in front of a test's first line)
    print("\n".join(ln.lstrip(".") for ln in p.stdout.splitlines() if ln.lstrip(".").startswith("  ") or "passed" in ln))
    print(f"  fresh process ({mode}): {time.time() - t0:.1f} s")


def _coverage(c, reachable):
    print(f"  process {MODE or 'a'}: {S.counter_table(c)}")
    assert all(c[i] >= 1 for i in reachable), (sorted(reachable), S.counter_table(c))
    assert not any(c[i] for i in range(24) if i not in reachable), (sorted(reachable), S.counter_table(c))


if CHILD is None:
    # -----------------------------------------------------------------------------------------------------------------
    # a. every scene at the width its size picks: wide
    @pytest.mark.parametrize("name", S.SCENES)
    def test_scene(oracle, name):
        _left[name] = S.check_scene(oracle, name, legacy=False, forced=0)

    # -----------------------------------------------------------------------------------------------------------------
    # b. the narrow kernels: one fresh process under GSR_SORT_THREADS=256
    def test_narrow_scenes_in_a_fresh_process(oracle, tmp_path):
        for name in S.SCENES:  # (run alone: this test takes process a's runs itself)
            if name not in _left:
                _left[name] = S.check_scene(oracle, name, legacy=False, forced=0)
        path = str(tmp_path / "wide.npz")
        np.savez(path, **{f"{n}.{k}": v for n, r in _left.items() for k, v in r.items()})
        _fresh("narrow", ":" + path, [os.path.join(TESTS, "test_gpu_parity.py"), os.path.join(TESTS, "test_gpu_round3.py")],
               "test_knn_bit_exact_vs_oracle or test_random_configuration_sweep or test_depth_key_ranges or "
               "test_grouped_binning_shapes or sort_child",
               12 + 9 + 3 + 5 + len(S.SCENES) + 1)  # sweep, KNN, depth key ranges, grouped shapes; this file's scenes + coverage

    # -----------------------------------------------------------------------------------------------------------------
    # c. the pair-sort path with 16-bit keys, narrow: one fresh process under GSR_SORT_THREADS=256 GSR_BIN_LEGACY=1
    def test_narrow_pair_sort_in_a_fresh_process():
        _fresh("legacy_narrow", "", [], "sort_child", len(S.DEPTH_SCENES) + 1)

    # -----------------------------------------------------------------------------------------------------------------
    # d. the same path at the width the size picks, and the scan's carry round: one fresh process under GSR_BIN_LEGACY=1
    def test_pair_sort_and_scan_carry_in_a_fresh_process():
        _fresh("legacy", "", [], "sort_child", len(S.DEPTH_SCENES) + 2)

    # -----------------------------------------------------------------------------------------------------------------
    # coverage of process a (last in the file)
    def test_every_wide_instantiation_of_this_process_was_launched():
        """Reachable here: the grouped depth sort's three (12, 13, 14), both group scatters (18, 19) and, through
        tile_keys_32, the 32-bit pair sort with and without IOTA (6, 7).  Not in this process: 4 (16-bit tile ids: needs
        GSR_BIN_LEGACY=1 on these image sizes -- process d), every narrow index (b, c, d) and 20 (d)."""
        wide = (S.depth_index(0, 0, 1), S.depth_index(1, 0, 1), S.depth_index(0, 1, 1), S.group_index(0, 1), S.group_index(1, 1),
                S.scatter_index(0, 1, 1), S.scatter_index(1, 1, 1))
        _coverage(S.launches() - _state["start"], wide)

else:
    CHILD_SCENES = S.SCENES if MODE == "narrow" else S.DEPTH_SCENES

    @pytest.mark.parametrize("name", CHILD_SCENES)
    def test_sort_child_scene(oracle, name):
        got = S.check_scene(oracle, name, legacy=LEGACY, forced=FORCED)
        if MODE == "narrow":  # against the wide run of the parent's process, byte for byte
            want = np.load(CHILD.split(":", 1)[1])
            for k, v in got.items():
                assert v.tobytes() == want[f"{name}.{k}"].tobytes(), (name, k)

    if MODE == "legacy":
        def test_sort_child_scan_carry():
            """BASELINE's view with larger splats: the pair sort of R > 2048 x 4096 (tile id, Gaussian) pairs is narrow by its
            size -- sort_scatter_kernel<false, uint16_t, 256> [0] -- and every bin's row of the block histogram is longer than
            one round of sort_scan_kernel [20]; the depth sort of the P Gaussians stays wide [6, 7]."""
            from gaussianeditor_amd.diff_gaussian_rasterization import _C  # noqa: F401  (the library, before the clock starts)

            P, W, H = SCAN_CARRY_P, 1920, 1080
            t0 = time.time()
            case = make_case(P, W, H, seed=0, s0=0.04, sh_degree=0)
            R, color, radii, st, rose = S.forward(case)
            t1 = time.time()
            assert R > 2048 * 4096, R
            S.assert_sorted_list_invariants(st, R, radii)
            nbits = int(int(st["depths"][radii > 0].view(np.uint32).max()) ^ int(st["depths"][radii > 0].view(np.uint32).min())).bit_length()
            want, passes = S.expected_launches(P, W, H, R, nbits, True, 0)
            assert want[S.SCAN_CARRY] == 2 and want[S.scatter_index(0, 0, 0)] == 2
            assert np.array_equal(rose, want), (S.counter_table(rose), S.counter_table(want))
            print(f"  scan_carry: P {P} {W}x{H} R {R} = {(R + 4095) // 4096} blocks, {passes} depth passes, rose {S.counter_table(rose)}; "
                  f"scene + forward + export {t1 - t0:.1f} s, invariants {time.time() - t1:.1f} s")

    def test_sort_child_coverage():
        """b: the grouped depth sort's three narrow kernels (8, 9, 10), both narrow group scatters (16, 17), the narrow
        32-bit pair sort without and with IOTA (2, 3: tile_keys_32, and the Morton sort of the KNN tests).  c: 16-bit pairs
        and the pair-sort path's depth order, narrow (0, 2, 3).  d: the same three wide (4, 6, 7), and scan_carry's narrow
        16-bit pair sort with the scan's carry round (0, 20)."""
        reachable = {"narrow": (8, 9, 10, 16, 17, 2, 3), "legacy_narrow": (0, 2, 3), "legacy": (4, 6, 7, 0, S.SCAN_CARRY)}[MODE]
        _coverage(S.launches(), reachable)
