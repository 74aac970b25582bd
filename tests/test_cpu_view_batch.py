"""The view-batch tests' own premises, from the reference alone (no GPU): the cases of tests/test_gpu_view_batch.py touch
enough rows to overflow a 16-row speculation and span every header block of a view message, the turned-away camera sees
nothing, the oracle gradients have live rows in every tensor, the exact / speculated / overflowing / speculated sequence of
`multiview_batch_step` takes the expected passes on the CPU path (the oracle backend tests/test_cpu_multiview.py installs:
no streams, no pipeline), and `_relayout_message` round-trips a message between capacities."""
import numpy as np
import pytest
import torch

import view_batch_helpers as vb
from helpers import assert_grads_close

STEPS = range(4)


def _views(batches=vb.ALL_BATCHES):
    for P, K, away in batches:
        b = vb.Batch(P, K, away)
        for v in range(K):
            yield b, v


def test_every_seeing_view_touches_more_rows_than_the_overflowing_hint(oracle):
    """Step 3 of every schedule speculates on 16 rows and must overflow.  (The one exception is the single Gaussian, P = 1:
    one row at most, so that batch stays speculated and its test says so.)"""
    for b, v in _views():
        for step in STEPS:
            touched = int(b.oracle(v, step)[1].sum())
            if v in b.away:
                assert touched == 0, (b.P, b.K, v, step)
            elif b.P > vb.OVERFLOW_HINT:
                assert touched > vb.OVERFLOW_HINT, (b.P, b.K, v, step, touched)
            else:
                assert touched == 1 and b.P == vb.P_ONE, (b.P, b.K, v, step, touched)


def test_touched_rows_span_every_header_block(oracle):
    """P = 2500: rows in all three 1024-row blocks of the message header; P = 1025: the second block holds row 1024 alone,
    and some view of the batch must touch it."""
    for b, v in _views([c for c in vb.ALL_BATCHES if c[0] == vb.P_MAIN and not c[2]]):
        rows = np.nonzero(b.oracle(v, 0)[1])[0]
        assert {int(r) // 1024 for r in rows} == {0, 1, 2}, (b.K, v)
    b = vb.Batch(vb.P_EDGE, 3)
    assert any(b.oracle(v, step)[1][1024] for v in range(3) for step in STEPS)


def test_the_turned_away_camera_sees_nothing(oracle):
    for b, v in _views([c for c in vb.ALL_BATCHES if c[2]]):
        f = vb.oracle_view_forward(*b.specs[v])
        if v in b.away:
            assert int(f["num_rendered"]) == 0 and not f["radii"].any(), (b.away, v)
            assert all(not b.oracle(v, step)[0][k].any() for step in STEPS for k in vb.GRAD_KEYS)
        else:
            assert int((f["radii"] > 0).sum()) > vb.OVERFLOW_HINT


def test_oracle_gradients_have_live_rows_in_every_tensor(oracle):
    """assert_grads_close allows ROW_FRACTION of the LIVE rows to miss the per-row bar: with no live row the allowance would be
    satisfied vacuously.  Against themselves the gradients pass at zero error."""
    for b, v in _views():
        if v in b.away:
            continue
        for step in STEPS:
            g = b.oracle(v, step)[0]
            assert assert_grads_close(g, g, tol=vb.TOL, tag=(b.P, b.K, v, step)) == 0.0
            for k in vb.GRAD_KEYS:
                assert np.isfinite(g[k]).all() and int((np.abs(g[k]).max(axis=1) > 0).sum()) >= 1, (b.P, b.K, v, step, k)


@pytest.mark.parametrize("P,K,away", [(vb.P_MAIN, 3, ()), (vb.P_MAIN, 2, ()), (vb.P_ONE, 3, ()), (vb.P_MAIN, 3, (1,)), (vb.P_MAIN, 3, (0, 1, 2))])
def test_four_step_sequence_on_the_cpu_path(oracle, monkeypatch, P, K, away):
    """exact, speculated, overflowing (hint 16: discarded and re-run exact), speculated -- and every check of the GPU tests,
    through the oracle backend: per view, sums, forwards, NaN fill, flags, the speculation's arithmetic."""
    import oracle_backend

    oracle_backend.install(monkeypatch)
    b = vb.Batch(P, K, away)
    r = vb.Runner(monkeypatch, b, "cpu", "serial")
    overflows = P > vb.OVERFLOW_HINT and len(away) < K
    passes = r.four_steps(may_overflow=overflows)
    assert [len(p) for p in passes] == [1, 1, 2 if overflows else 1, 1]
    assert [p[-1]["spec_cap"] is not None for p in passes] == [False, True, not overflows, True]
    if away:
        assert [r.bucket.last_counts[v] == 0 for v in range(K)] == [v in away for v in range(K)]
    assert r.ratios["view"] == 0.0  # (the oracle backend IS the oracle)


def test_an_overwritten_view_fails_the_per_view_check_and_not_the_bit_equality(oracle, monkeypatch):
    """The hazard the pipeline's `bucket_free` event prevents, made deterministic: a block of view 1's rows holds view 2's
    gradients by the time view 1 is packed.  The clone taken at the pack and the message are wrong alike, so everything but
    the oracle checks passes; with them, view 1 of the step is what fails."""
    import oracle_backend
    from gaussianeditor_amd import multiview as mv

    oracle_backend.install(monkeypatch)
    b = vb.Batch(vb.P_MAIN, 3)
    for oracle_checks in (False, True):
        with monkeypatch.context() as m:
            r = vb.Runner(m, b, "cpu", "serial", oracle_checks=oracle_checks)
            spied, calls = mv._C.view_message_pack, []

            def pack(plan, grads5, rgb, campos, cap, message):
                calls.append(1)
                if len(calls) == 2:  # view 1 of step 0: the rows of its message in the second header block
                    rows = torch.from_numpy(np.nonzero(b.oracle(1, 0)[1][1024:2048])[0] + 1024)
                    for t, k in zip(grads5, vb.SEG_KEYS):
                        t.reshape(b.P, -1)[rows] = torch.from_numpy(b.oracle(2, 0)[0][k].copy())[rows]
                return spied(plan, grads5, rgb, campos, cap, message)

            m.setattr(mv._C, "view_message_pack", pack)
            if oracle_checks:
                with pytest.raises(AssertionError, match="step 0 view 1"):
                    r.step(0)
            else:
                r.step(0)
            assert len(calls) == 3


def test_sparse_and_persistent_buckets_on_the_cpu_path(oracle, monkeypatch):
    import oracle_backend

    oracle_backend.install(monkeypatch)
    b = vb.Batch(vb.P_MAIN, 3)
    r = vb.Runner(monkeypatch, b, "cpu", "serial", bucket_kw=dict(sparse_rows=True))
    r.four_steps()
    union = np.logical_or.reduce([b.oracle(v, 3)[1] for v in range(3)])
    assert np.array_equal(r.bucket.row_valid.numpy().astype(bool), union)
    # three views together touch every row of this scene; the GPU test sees rows NO view sends in the batch whose second and
    # third cameras are turned away: view 0 alone leaves some Gaussians out (hidden behind saturated pixels)
    assert union.all() and 0 < int(vb.Batch(vb.P_MAIN, 3, (1, 2)).oracle(0, 3)[1].sum()) < vb.P_MAIN
    vb.Runner(monkeypatch, b, "cpu", "serial", bucket_kw=dict(persistent_rows=True)).four_steps()


@pytest.mark.parametrize("P", [1, 1024, 1025, 2500])
def test_relayout_message_round_trips_between_capacities(P):
    """A message of `count` rows laid out for one capacity, moved to a larger one (cap_src < cap_dst), to a smaller one
    (cap_src > cap_dst >= count) and back: header and every row of every segment survive; pure torch."""
    from gaussianeditor_amd.multiview import _relayout_message

    head, widths = 4 + (P + 1023) // 1024, (1, 3, 3, 4, 3, 1, 3)
    words = lambda cap: head + 18 * cap  # noqa: E731
    count = min(P, 37)
    g = torch.Generator().manual_seed(P)

    def segments(msg, cap):
        out, off = [], head
        for w in widths:
            out.append(msg[off:off + w * cap].view(cap, w)[:count].clone())
            off += w * cap
        return out

    src = torch.randn(words(count), generator=g)
    want_head, want = src[:head].clone(), segments(src, count)
    for caps in ((count, count + 13, count), (count, 4 * count + 1, count + 2, count), (count + 5, count, 3 * count, count + 5)):
        cur = torch.randn(words(caps[0]), generator=g)
        _relayout_message(src, P, count, cur, caps[0])
        for a, c in zip(caps, caps[1:]):
            nxt = torch.full((words(c),), float("nan"))
            _relayout_message(cur, P, a, nxt, c)
            assert torch.equal(nxt[:head], want_head), (P, a, c)
            for got, w in zip(segments(nxt, c), want):
                assert torch.equal(got, w), (P, a, c)
            cur = nxt
