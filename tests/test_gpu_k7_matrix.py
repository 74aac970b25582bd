"""-m gpu: every instantiation of the blend backward, blend_backward_kernel<FAST, SEG, DEPTH, ABS, ALPHA> (24: DEPTH excludes
SEG), against ONE builder of the expected gradients of <G, C> + <GA, A> + <GD, D> (tests/k7_matrix_helpers.py; held to float64
autograd by tests/test_cpu_k7_matrix.py), each run proving which kernel it launched (gsr_debug_blend_backward_launches: the
counter of exactly the intended index rises by one) and, for the SEG rows, that its work list held list-segment items
(gsr_debug_blend_backward_items).  A row is written FSDBL = (FAST, SEG, DEPTH, ABS, ALPHA), its counter index in brackets.

  a. the 16 rows without SEG in this process, on 2000 Gaussians / 64 x 64 (two rows again on 70 x 45);
  b. the 8 rows with SEG in ONE fresh process with GSR_CK_CHUNKS=4 GSR_BWD_SEG=1 (read once per process), on 20 000
     Gaussians / 64 x 64; that process also runs test_gpu_round2.py::test_fast_exp_flag_parity_and_flag_pinning under the
     knobs.  The FAST base (1,1,0,0,0) is compared with (1,0,0,0,0) of the same scene: forward image bit-identical, gradients
     within the bars.  (1,0,0,0,0) comes from a second fresh process with the same forward and GSR_BWD_SEG=0 (the backward
     never cuts a list): with default knobs a view whose lists are this long (R = 32 220 >= 1 200 x 16 tiles) leaves
     checkpoints and runs the SEG kernels in ANY process, this one included, so it cannot produce that base itself;
  c. the seeded shape sweep of test_gpu_parity.py (P = 1, 2, 63, 65, 255, 256, images down to 2 x 156 and 291 x 1) under
     abs-grad with <G,C>+<GA,A>+<GD,D> and with <G,C>+<GA,A>: the alpha image (its scalar path: W H not a multiple of 4) bit
     for bit, signed gradients, absgrad dominance and the one-pixel identity;
  d. coverage: all 16 counters of this process >= 1, the 8 impossible ones 0 (the fresh process: the same for its 8).

Bars: helpers.assert_grads_close with its defaults (1e-5 of the tensor's maximum + the per-row bar) everywhere.

Measured on the MI355X (worst |got - want| / max |want| over a row's tensors as a fraction of the 1e-5 bar, signed gradients /
absgrad against the per-pixel block expectation; work list as (items, list-segment items); two runs, which differ on two
figures by the order of the float atomics -- F----[1] 0.005 / 0.010, sweep seed 8 0.086 / 0.114 -- the larger is quoted):
  2000 Gaussians, 64 x 64, work list (19, 0):
    -----[0] 0.052          F----[1] 0.010          --D--[4] 0.047          F-D--[5] 0.038
    ---B-[8] 0.052 / 0.011  F--B-[9] 0.010 / 0.005  --DB-[12] 0.047 / 0.008 F-DB-[13] 0.038 / 0.022
    ----L[16] 0.042         F---L[17] 0.027         --D-L[20] 0.029         F-D-L[21] 0.024
    ---BL[24] 0.042 / 0.010 F--BL[25] 0.027 / 0.007 --DBL[28] 0.029 / 0.010 F-DBL[29] 0.024 / 0.016
  70 x 45, work list (13, 0): --DBL[28] 0.040 / 0.008, F-DBL[29] 0.025 / 0.004
  20 000 Gaussians, 64 x 64, fresh process under the knobs, work list (75, 59); the unsegmented base's (24, 0):
    -S---[2] 0.051          FS---[3] 0.006          -S-B-[10] 0.051 / 0.031 FS-B-[11] 0.006 / 0.004
    -S--L[18] 0.042         FS--L[19] 0.029         -S-BL[26] 0.042 / 0.043 FS-BL[27] 0.029 / 0.020
    FS---[3] against F----[1] of the other fresh process: forward image bit-identical, gradients 0.057 -- the largest figure
    of the 24 rows.  Counters of that process at its end: [2]=4 [3]=60 [10]=3 [11]=3 [18]=1 [19]=1 [26]=2 [27]=2, all others 0.
  test_fast_exp_flag_parity_and_flag_pinning passes under the knobs (every gradient within 4.3e-7 of its maximum, no row
  masked; it launched [3] twice); its scene (20 000 Gaussians, 512 x 512) gives a work list of (651, 0): the SEG kernel
  runs, but no tile of it is cut -- that test does not reach segment items, the rows above do.
  sweep, seeds 0..11, <G,C>+<GA,A>+<GD,D> / <G,C>+<GA,A>: 0 / 0 (nothing rendered, nothing launched), 0.033 / 0.018,
    0.019 / 0.066, 0.032 / 0.022, 0.609 / 0.109, 0.110 / 0.145, 0.075 / 0.065, 0.146 / 0.113, 0.114 / 0.109, 0.068 / 0.060,
    0.046 / 0.059, 0.041 / 0.046; one-pixel identity within 1.2e-7.  The three-term runs launched [28]; the two-term runs [24],
    on seeds 6 and 9 [26] with work lists (14, 12) and (9, 9): views that leave checkpoints by default.
  counters at the end of the file, run alone: [0]=5 [1]=198 [4]=2 [5]=2 [8]=4 [9]=4 [12]=4 [13]=4 [16]=2 [17]=2
    [20]=1 [21]=1 [24]=22 [25]=4 [26]=4 [28]=26 [29]=4, every other of the 24 (and the 8 impossible ones) 0.
  time: the file 16 s, of which the two fresh processes 2.4 s (base) + 7.3 s (SEG rows and the fast-exp test); no in-process
  test above 0.71 s.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import abs_helpers as AB
import k7_matrix_helpers as K
from helpers import assert_grads_close, make_case, seed_gradient
from test_gpu_alpha import _bits, _case, _one_pixel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
#: set (to the path of the (1,0,0,0,0) base) in the fresh process of test_seg_rows_in_a_fresh_process: the tests of part b are
#: defined there and only there -- under default knobs their scene runs other kernels than the ones they are about.  They are
#: reached through test_seg_rows_in_a_fresh_process alone (a direct `-k seg_child` selects nothing), which asserts their number.
CHILD_BASE = os.environ.get("GSR_K7_MATRIX_BASE")
SEG_KNOBS = dict(GSR_CK_CHUNKS="4", GSR_BWD_SEG="1")
_state = {}


def _plain_one_pixel(oracle):
    """A one-pixel colour-only backward of this process's scene: -----[0] on p2000, under the segment knobs -S---[2] on p20000."""
    case, G, _, _ = K.scene("p2000" if CHILD_BASE is None else "p20000")
    return K.run(case, (0, int(CHILD_BASE is not None), 0, 0, 0), G * _one_pixel(oracle, case))[0]


# ---------------------------------------------------------------------------------------------------------------------
# a. the 16 rows without SEG
@pytest.fixture(scope="module", autouse=True)
def _plain_backward_before_the_first_row(oracle):
    _state["before"] = _plain_one_pixel(oracle)
    yield


NOSEG = [(r, "p2000") for r in K.ROWS if not r[1]] + [((0, 0, 1, 1, 1), "ragged"), ((1, 0, 1, 1, 1), "ragged")]


@pytest.mark.parametrize("row,name", NOSEG, ids=[f"{K.row_id(r)}-{n}" for r, n in NOSEG])
def test_row_without_seg(oracle, row, name):
    case, G, GA, GD = K.scene(name)
    K.check_row(oracle, case, row, G, GA, GD, f"{K.row_id(row)} {name}")


def test_plain_backward_is_unchanged_after_the_rows(oracle):
    """A one-pixel gradient makes a backward deterministic (every accumulator cell receives at most one add): bit identity
    with the one taken before the first row (the module's autouse fixture) is a meaningful demand."""
    after = _plain_one_pixel(oracle)
    for k, v in _state["before"].items():
        assert np.array_equal(v.view(np.uint32), after[k].view(np.uint32)), (k, "not bit-identical")


# ---------------------------------------------------------------------------------------------------------------------
# b. the 8 rows with SEG: one fresh process under the segment knobs
def _fresh(cmd, env, timeout=600):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)


def test_seg_rows_in_a_fresh_process(tmp_path):
    base = str(tmp_path / "base_F.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("GSR_CK_CHUNKS", "GSR_BWD_SEG", "GSR_CK_DEBUG", "GSR_CK_SLOTS", "GSR_SORT_THREADS")}
    t0 = time.time()
    p = _fresh([sys.executable, "-c", f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import k7_matrix_helpers as K; "
                f"K.write_base({base!r})"], dict(env, GSR_CK_CHUNKS="4", GSR_BWD_SEG="0"))
    assert p.returncode == 0 and os.path.exists(base), (p.stdout + p.stderr)[-3000:]
    print(p.stdout[-400:])
    t1 = time.time()
    p = _fresh([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", os.path.join(TESTS, "test_gpu_round2.py"),
                os.path.abspath(__file__), "-k", "fast_exp_flag_parity or seg_child"],
               dict(env, GSR_K7_MATRIX_BASE=base, **SEG_KNOBS))
    assert p.returncode == 0, (p.stdout + p.stderr)[-6000:]
    assert "13 passed" in p.stdout, p.stdout[-3000:]  # (1 of test_gpu_round2.py, 12 of this file)
    # (-q -s: pytest's progress dots sit in front of a test's first line)
    print("\n".join(ln.lstrip(".") for ln in p.stdout.splitlines() if ln.lstrip(".").startswith("  ") or "passed" in ln))
    print(f"  fresh processes: base {t1 - t0:.1f} s, SEG rows {time.time() - t1:.1f} s")


if CHILD_BASE is not None:
    def test_seg_child_what_the_fast_exp_parity_test_launched():
        """test_gpu_round2.py::test_fast_exp_flag_parity_and_flag_pinning ran in front of this file: which kernels it
        launched under the knobs (reported; asserted only that FAST + SEG ran), and what the work list of its scene
        (20 000 Gaussians, 512 x 512) holds."""
        c = K.launches()
        print(f"  after fast_exp_flag_parity: {K.counter_table(c)}")
        assert c[K.index((1, 1, 0, 0, 0))] >= 1
        case = make_case(20000, 512, 512, seed=4, s0=0.02)
        _, out = K.run(case, (1, 1, 0, 0, 0), seed_gradient(512, 512, 4) * (512 * 512))
        print(f"  fast_exp_flag_parity's scene: items {out['items']}")

    def test_seg_child_fast_base_against_the_unsegmented_one():
        """SEG may change only the summation order: the forward image bit-identical, the gradients within the bars."""
        case, G, _, _ = K.scene("p20000")
        want = np.load(CHILD_BASE)
        assert int(want["items"][1]) == 0
        got, out = K.run(case, (1, 1, 0, 0, 0), G)
        assert out["items"][1] >= 1, out["items"]
        assert np.array_equal(_bits(out["color"]), _bits(want["color"]))
        worst = assert_grads_close(got, want, tag="(1,1,0,0,0) vs (1,0,0,0,0)", keys=list(got))
        print(f"  {K.row_id((1, 1, 0, 0, 0))} vs {K.row_id((1, 0, 0, 0, 0))} of another process: items {out['items']} vs "
              f"{tuple(int(v) for v in want['items'])}, worst {worst:.2e} = {worst / 1e-5:.3f} bar")

    @pytest.mark.parametrize("row", [r for r in K.ROWS if r[1]], ids=K.row_id)
    def test_seg_child_row(oracle, row):
        case, G, GA, GD = K.scene("p20000")
        K.check_row(oracle, case, row, G, GA, GD, f"{K.row_id(row)} p20000")

    def test_seg_child_plain_backward_is_unchanged_after_the_rows(oracle):
        """As part a: the one-pixel -S---[2] backward taken before this process's first test of this file, again."""
        after = _plain_one_pixel(oracle)
        assert K.acc_tables_are_zero()
        for k, v in _state["before"].items():
            assert np.array_equal(v.view(np.uint32), after[k].view(np.uint32)), (k, "not bit-identical")

    def test_seg_child_coverage():
        c = K.launches()
        print(f"  fresh process: {K.counter_table(c)}")
        assert all(c[K.index(r)] >= 1 for r in K.ROWS if r[1]), K.counter_table(c)
        assert not any(c[i] for i in range(32) if K.row_of(i) not in K.ROWS)


# ---------------------------------------------------------------------------------------------------------------------
# c. the shape sweep under the opt-in losses
@pytest.mark.parametrize("seed", range(12))
def test_shape_sweep_under_the_opt_in_losses(oracle, seed):
    s = K.sweep_expectation(oracle, seed)
    K.assert_sweep_discriminates(s, seed)
    case, G, GA, GD, kw, f = s["case"], s["G"], s["GA"], s["GD"], s["kw"], s["f"]
    H, W, P = case["H"], case["W"], case["sc"]["xyz"].shape[0]
    want_alpha = np.float32(1.0) - f["final_T"].astype(np.float32)
    p = int(np.abs(f["final_T"].reshape(-1).astype(np.float64) - 0.5).argmin())
    m = AB.pixel_mask(H, W, [(p // W, p % W)])
    for tag, gd, want in (("C+A+D", GD, s["want3"]), ("C+A", None, s["want2"])):
        row = (0, None, int(gd is not None), 1, 1)
        got, out = K.run(case, row, G, GA, gd, **kw)
        assert out["R"] == f["num_rendered"]
        assert np.array_equal(_bits(out["alpha"]), _bits(want_alpha)), (seed, tag, "alpha image")
        worst = assert_grads_close(got, want, tag=f"sweep seed {seed} {tag}", keys=list(got))
        a, sg = out["absgrad"].astype(np.float64), np.abs(got["dL_dmeans2D"][:, :2].astype(np.float64))
        assert a.shape == (P, 3) and (a[:, 2] == 0).all() and np.isfinite(a).all()
        assert (sg - a[:, :2]).max() <= 1e-5 * a.max(), (seed, tag, "dominance")
        line = f"  sweep seed {seed} {tag}: P {P} {W}x{H} R {out['R']}, launched {out['index']}, items {out['items']}, worst {worst:.2e} = {worst / 1e-5:.3f} bar"
        if out["R"] > 0:  # one pixel: every Gaussian has one term, absgrad == |grad|
            g1, o1 = K.run(case, row, G * m, GA * m, None if gd is None else gd * m, **kw)
            w1 = assert_grads_close(dict(absgrad=o1["absgrad"][:, :2]), dict(absgrad=np.abs(g1["dL_dmeans2D"][:, :2])),
                                    tag=f"sweep seed {seed} {tag}: one pixel")
            line += f", one pixel {w1:.1e}"
        else:
            assert not a.any() and all(not np.any(v) for v in got.values())
        print(line)
    assert K.acc_tables_are_zero()


# ---------------------------------------------------------------------------------------------------------------------
# d. coverage (last in the file)
def test_every_instantiation_without_seg_was_launched():
    c = K.launches()
    print(f"  this process: {K.counter_table(c)}")
    assert all(c[K.index(r)] >= 1 for r in K.ROWS if not r[1]), K.counter_table(c)
    assert not any(c[i] for i in range(32) if K.row_of(i) not in K.ROWS)
