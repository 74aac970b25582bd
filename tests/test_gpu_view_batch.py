"""`multiview_batch_step` on the GPU under every schedule of its view pipeline -- serial, pipelined with look-ahead 0 / 1 / 2
(2 / 3 / 4 view streams), and the L1 autograd route inside the pipeline -- with every view checked against ITS OWN oracle
gradients (tests/view_batch_helpers.py; tests/test_cpu_view_batch.py establishes the cases' premises without a GPU).

Every schedule runs four steps on one bucket: exact, speculated, a step whose 16-row speculation overflows (the pipelined
pass is discarded after it has run every backward into the bucket, and the step re-runs in its exact form), speculated.
After every step, for every pass: (1) each view as it was packed against that view's oracle gradients -- a view whose rows
the next view's K8+K9 overwrote too early, or that was packed before its own K8+K9 finished, fails here by orders of
magnitude, which the bit-equality of the sums cannot see; (2) the sums bit-equal to the packed views added in view order,
and within the per-view bars added up of the float64 sum of the oracle gradients; (3) colours, depths and radii bit-equal
to plain no-grad forwards on the default stream; (4) no NaN left of the fill the bucket started with; (5) FLAG_SHARED_SIMDS
on exactly the renders of a pipelined pass, the thread's flags restored; and the speculation's arithmetic (the next hint,
`last_exchange`, the passes taken).

Measured on an MI355X, worst per-view error as a fraction of the 1e-5 bar / worst batch-sum error as a fraction of its bar
(each test prints its own): 0.083 / 0.065 under each of the five schedules over K = 1, 2, 3, 5 (the same to three digits:
the schedule changes no arithmetic, only the order of K7's float atomics), 0.232 / 0.024 at K = 9, 0.070 / 0.019 at
P = 1025, 0.054 / 0.018 at P = 1."""
import pytest
import torch

import view_batch_helpers as vb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

#: (schedule, P, K): K in {1, 2, 3, 5} under every schedule (K = 5 wraps the view streams even with four of them); K = 9 -- more
#: than the accumulate kernel's 8-view batch -- P = 1025 and P = 1 in one schedule each
RUNS = [(s, vb.P_MAIN, K) for s in vb.SCHEDULES for K in (1, 2, 3, 5)] + [("ahead1", vb.P_MAIN, 9), ("ahead2", vb.P_EDGE, 3),
                                                                       ("ahead1", vb.P_ONE, 3)]


@pytest.mark.parametrize("schedule,P,K", RUNS)
def test_every_view_and_the_sums_match_the_oracle_under_the_schedule(monkeypatch, schedule, P, K):
    r = vb.Runner(monkeypatch, vb.Batch(P, K), DEV, schedule)
    # (a single Gaussian cannot overflow 16 rows: its third step stays speculated, tests/test_cpu_view_batch.py)
    passes = r.four_steps(may_overflow=P > vb.OVERFLOW_HINT)
    r.report()
    pipelined = schedule != "serial" and K > 1
    # the pipeline really ran: split forwards (or, on the L1 route, whole ones) carrying the shared-SIMDs flag in every
    # speculated pass, the discarded one included
    from gaussianeditor_amd import options

    shared = [all(f & options.FLAG_SHARED_SIMDS for _, f in p["renders"]) for step in passes for p in step]
    spec = [p["spec_cap"] is not None for step in passes for p in step]
    assert shared == [s and pipelined for s in spec]
    if pipelined and schedule != "autograd":
        assert len(r.spy.pending) == K * sum(spec) and all(pf.ticket is None for pf in r.spy.pending)


def test_the_callers_flags_reach_the_renders_and_are_restored(monkeypatch):
    """Inside a caller's options.override(FLAG_FAST_EXP): every render carries the caller's bits (plus FLAG_SHARED_SIMDS in a
    pipelined pass), and the override is what the thread is left with.  (Another exp: the oracle checks are off; the sums,
    the forwards -- rendered under the same override -- and the NaN check stay.)"""
    from gaussianeditor_amd import options

    r = vb.Runner(monkeypatch, vb.Batch(vb.P_MAIN, 3), DEV, "ahead1", caller_flags=options.FLAG_FAST_EXP, oracle_checks=False)
    with options.override(options.FLAG_FAST_EXP):
        r._reference_forwards()
    assert options.current_flags() == 0
    r.four_steps()
    assert options.current_flags() == 0
    flags = {f for p in r.spy.passes for _, f in p["renders"]}
    assert flags == {options.FLAG_FAST_EXP, options.FLAG_FAST_EXP | options.FLAG_SHARED_SIMDS}


@pytest.mark.parametrize("away", [(), (1, 2)])
def test_sparse_rows_bucket_in_a_pipelined_batch(monkeypatch, away):
    """GradBucket(sparse_rows=True): `row_valid` is the union of the messages' row lists, the valid rows are the sequential
    sums of the packed views bit for bit (Runner, check 2), and the accumulate kernel writes no other row: all six tensors are
    NaN-filled right in front of it (the views' messages are packed by then) and the other rows must still be NaN.  Three
    views of this scene together touch every row, so the batch is run a second time with two cameras turned away: the
    remaining view leaves some rows out (tests/test_cpu_view_batch.py)."""
    from gaussianeditor_amd import multiview as mv

    b = vb.Batch(vb.P_MAIN, 3, away)
    r = vb.Runner(monkeypatch, b, DEV, "ahead0", bucket_kw=dict(sparse_rows=True))
    orig = mv._C.view_messages_accumulate

    def accumulate(messages, P, cap, degree, M, means3D, dense, row_valid=None):
        assert row_valid is r.bucket.row_valid
        for t in dense:
            t.fill_(float("nan"))
        return orig(messages, P, cap, degree, M, means3D, dense, row_valid=row_valid)

    monkeypatch.setattr(mv._C, "view_messages_accumulate", accumulate)
    for step, hint, over in ((0, None, None), (1, None, None), (2, vb.OVERFLOW_HINT, True), (3, None, None)):
        passes = r.step(step, cap_hint=hint, must_overflow=over)
        union = torch.zeros(b.P, dtype=torch.bool)
        for pk in passes[-1]["packs"]:
            n, rows = vb.message_rows(pk["message"], b.P)
            assert n == rows.numel()
            union[rows] = True
        valid = r.bucket.row_valid.cpu().bool()
        assert torch.equal(valid, union) and vb.OVERFLOW_HINT < int(union.sum()) and (int(union.sum()) < b.P) == bool(away), step
        for name, t in r.bucket.views.items():
            rest = t.reshape(b.P, -1)[~r.bucket.row_valid.bool()]
            assert bool(torch.isnan(rest).all()), (step, name, "a row no view sent was written")
    r.report(" sparse_rows")


def test_persistent_rows_bucket_in_a_pipelined_batch(monkeypatch):
    """GradBucket(persistent_rows=True): every row is correct after every step (checks 1 and 2), across the discarded
    speculative pass, which has run every backward into the bucket and its row state; the contract check of the bucket
    (Runner.step calls check_persistent_rows() in front of every step) raises nothing."""
    r = vb.Runner(monkeypatch, vb.Batch(vb.P_MAIN, 3), DEV, "ahead1", bucket_kw=dict(persistent_rows=True))
    passes = r.four_steps()
    assert [len(p) for p in passes] == [1, 1, 2, 1]
    r.bucket.check_persistent_rows()
    r.report(" persistent_rows")


def test_a_view_that_sees_nothing(monkeypatch):
    """One of three cameras is turned away from the cloud (zero radii in the oracle forward, tests/test_cpu_view_batch.py):
    its message counts 0 rows, the sums are the other two views' (check 2: it adds exact zeros), `last_counts` has three
    entries."""
    b = vb.Batch(vb.P_MAIN, 3, away=(1,))
    assert not vb.oracle_view_forward(*b.specs[1])["radii"].any()
    r = vb.Runner(monkeypatch, b, DEV, "ahead0")
    for passes in r.four_steps():
        for p in passes:
            assert vb.message_rows(p["packs"][1]["message"], b.P)[0] == 0
            assert all(not t.any() for t in p["packs"][1]["g5"]) and not p["packs"][1]["rgb"].any()
    assert len(r.bucket.last_counts) == 3 and r.bucket.last_counts[1] == 0 and min(r.bucket.last_counts[0::2]) > vb.OVERFLOW_HINT
    r.report(" one empty view")


def test_a_batch_in_which_every_view_sees_nothing(monkeypatch):
    """All sums are exact zeros, the radii are zero, and the next step still speculates (on the smallest message)."""
    b = vb.Batch(vb.P_MAIN, 3, away=(0, 1, 2))
    r = vb.Runner(monkeypatch, b, DEV, "ahead0")
    for step in range(3):
        passes = r.step(step)
        assert len(passes) == 1 and (passes[0]["spec_cap"] is not None) == (step > 0)
        assert r.bucket.last_counts == [0, 0, 0] and r.bucket._cap_hint == 1024
        assert all(not t.any() for t in r.bucket.views.values())
        assert r.bucket.last_exchange["message_rows"] == (1024 if step else 1)


@pytest.mark.parametrize("raise_at", [0, 1])
def test_a_step_that_raises_leaves_nothing_pending(monkeypatch, raise_at):
    """A Python exception in the backward of view `raise_at` of 3 under look-ahead 1 (at view 0 the third view's forward has
    begun and is not finished; at view 1 every forward is): afterwards the bucket's hook is gone, the thread's flags are
    restored, every PendingForward has given its native ticket back, and the next step on the same bucket is right."""
    from gaussianeditor_amd import multiview as mv
    from gaussianeditor_amd import options

    r = vb.Runner(monkeypatch, vb.Batch(vb.P_MAIN, 3), DEV, "ahead1")
    r.step(0)
    orig, calls, seen = mv._view_backward, [], {}

    class Boom(Exception):
        pass

    def failing(*a):
        calls.append(1)
        if len(calls) - 1 == raise_at:
            seen["outstanding"] = [pf.ticket is not None for pf in r.spy.pending]
            raise Boom("injected")
        return orig(*a)

    n0 = len(r.spy.pending)
    with monkeypatch.context() as m:
        m.setattr(mv, "_view_backward", failing)
        with pytest.raises(Boom):
            r.call(1)
    r.sync()
    assert sum(seen["outstanding"]) == (1 if raise_at == 0 else 0)  # (the case at view 0 is the one with a forward pending)
    assert r.bucket.on_blend_done is None and options.current_flags() == 0
    assert len(r.spy.pending) - n0 == 3 and all(pf.ticket is None for pf in r.spy.pending)
    for step in (2, 3):
        r.step(step)
    r.report(f" after a step that raised at view {raise_at}")
