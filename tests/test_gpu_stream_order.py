"""-m gpu: the detector of tests/stream_order.py proved on test-owned torch operations (no kernel of the product runs here).

  precondition   a trivial operation on the side stream completes, and its result reaches the host, while the default
                 stream still sleeps: the platform does not serialise the two (stream_order.py says which streams it does);
  stray launch   a cell that computes part of its result under torch.cuda.stream(torch.cuda.default_stream()) is a mismatch;
  stray wait     a cell that calls torch.cuda.synchronize() before it returns is not conclusive;
  clean cell     a correct cell is conclusive and bit-identical;
  decoys         every decoy has the dtype, shape and domain of its true value; integer and bool decoys equal it.

The three cells print their verdicts in that order: mismatch, not conclusive, clean.  Every sleep here is SLEEP_MS = 100 ms
of the default stream (the cells take about a millisecond), so each test takes 0.1 to 0.3 s on the MI355X.
"""
import numpy as np
import pytest
import torch

import stream_order as SO
from guarded_alloc import GuardedAllocator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLEEP_MS = 100.0


def _inputs():
    gen = torch.Generator().manual_seed(3)
    return torch.randn(257, 3, generator=gen), torch.randn(1025, generator=gen), torch.randint(0, 257, (300,), generator=gen)


def _plain_put(t):
    out = t.detach().to(DEV).clone()
    return out.requires_grad_(True) if t.requires_grad else out


def _clean_cell(put):
    a, b, idx = _inputs()
    x, y, i = put(a.requires_grad_(True)), put(b), put(idx)
    rows = x[i] * 2.0 + 1.0
    total = (rows.sum(dim=1) * y[:300]).sum()
    total.backward()
    return dict(rows=rows, total=total, scaled=y * 3.0), dict(x=x.grad)


def _stray_launch_cell(put):
    """`scaled` is computed on the default stream, unordered with the stream the cell was called on."""
    a, b, idx = _inputs()
    x, y, i = put(a.requires_grad_(True)), put(b), put(idx)
    rows = x[i] * 2.0 + 1.0
    total = (rows.sum(dim=1) * y[:300]).sum()
    total.backward()
    scaled = torch.empty_like(y)
    with torch.cuda.stream(torch.cuda.default_stream()):
        torch.mul(y, 3.0, out=scaled)
    return dict(rows=rows, total=total, scaled=scaled), dict(x=x.grad)


def _stray_wait_cell(put):
    det, grads = _clean_cell(put)
    torch.cuda.synchronize()
    return det, grads


def _verdict(fn):
    out, side = SO.run_cell(fn, SLEEP_MS, allocator=lambda: GuardedAllocator(0x5A))
    det, grads = fn(_plain_put)
    torch.cuda.synchronize()
    plain, plain_grads = SO.host(det), SO.host(grads)
    v = SO.verdict(out[0], plain, side)
    print(f"  {fn.__name__}: {v}; {SO.report(side)}")
    return v, out, (plain, plain_grads), side


def test_precondition_a_side_stream_runs_underneath_the_default_streams_sleep():
    side = SO.SideStream(int(SLEEP_MS * SO.cycles_per_ms()))
    want = torch.arange(1024.0)
    with side:
        x = side.place(want)
        got, _ = side.finish(dict(y=x * 2.0), None, SO.host)
    print(f"  {SO.cycles_per_ms():.3e} sleep cycles per ms; {SO.report(side)}")
    assert np.array_equal(got["y"], want.numpy() * 2.0)
    assert side.conclusive, "the side stream waited for the default stream: this platform serialises the two"
    assert 0.9 * SLEEP_MS <= side.sleep_ms <= 1.5 * SLEEP_MS, side.sleep_ms  # (the calibration holds)
    assert side.window_ms < 0.5 * SLEEP_MS  # (entry to the result on the host)


def test_late_inputs_hold_the_decoy_first():
    """What an unordered reader sees: the decoy while the side stream sleeps in `place`, the true value afterwards.  (The
    reader's buffer exists beforehand: a first allocation on a stream can take longer than PLACE_SLEEP_MS.)"""
    side = SO.SideStream(int(SLEEP_MS * SO.cycles_per_ms()))
    want = torch.randn(257, 3, generator=torch.Generator().manual_seed(1))
    for _ in range(8):  # a reader's stream that shares a hardware queue with neither the default nor the side stream
        other = SO._vetted_stream(side.device)
        if SO._runs_underneath(other, side.device, blocked=side.stream):
            break
    else:
        pytest.fail("eight fresh streams in a row serialise with the side stream")
    with torch.cuda.stream(other):
        early = torch.zeros(257, 3, device=DEV)
        early.copy_(torch.ones(257, 3, device=DEV))
    torch.cuda.synchronize()
    with side:
        x = side.place(want)
        side.decoy_placed.synchronize()  # (the host waits for the decoy's store, about 20 us; the side stream then sleeps)
        with torch.cuda.stream(other):  # not ordered behind the side stream: a launch takes far less than PLACE_SLEEP_MS
            early.copy_(x.detach())
        late, _ = side.finish(dict(x=x), None, SO.host)
    early = early.cpu()
    assert np.array_equal(late["x"], want.numpy())
    assert torch.equal(early, SO.decoy(want)) and not torch.equal(early, want)


def test_stray_launch_is_a_mismatch():
    v, *_ = _verdict(_stray_launch_cell)
    assert v == "mismatch: scaled"


def test_stray_wait_is_not_conclusive():
    v, out, plain, side = _verdict(_stray_wait_cell)
    assert v == "not conclusive" and not side.conclusive
    assert side.window_ms >= 0.9 * SLEEP_MS  # (the cell waited the sleep out)


def test_clean_cell_is_conclusive_and_identical():
    v, out, plain, side = _verdict(_clean_cell)
    assert v == "clean" and side.conclusive and side.placed == 3
    assert SO.same_bits(out[1]["x"], plain[1]["x"])
    a, b, idx = _inputs()
    assert np.array_equal(out[0]["rows"], (a[idx] * 2.0 + 1.0).numpy())


DECOY_CASES = dict(
    rows=torch.randn(257, 3, generator=torch.Generator().manual_seed(2)),
    sh=torch.randn(5, 16, 3, generator=torch.Generator().manual_seed(3)),
    vector=torch.tensor([0.1, 0.2, 0.3]),
    matrix=torch.eye(4) + torch.arange(16.0).reshape(4, 4) * 0.01,
    mask01=(torch.rand(2, 9, 7, generator=torch.Generator().manual_seed(4)) > 0.5).float(),
    positive=torch.rand(300, 1, generator=torch.Generator().manual_seed(5)) + 0.5,
    half=torch.randn(6, 2, generator=torch.Generator().manual_seed(6)).half(),
    single_row=torch.randn(1, 7, generator=torch.Generator().manual_seed(7)),
    scalar=torch.tensor(3.5),
    int32=torch.randint(-1, 30, (300,), generator=torch.Generator().manual_seed(8), dtype=torch.int32),
    int64=torch.randint(0, 257, (2, 5), generator=torch.Generator().manual_seed(9)),
    uint8=torch.full((300,), 7, dtype=torch.uint8),
    bools=torch.rand(300, generator=torch.Generator().manual_seed(10)) > 0.5,
)


@pytest.mark.parametrize("name", list(DECOY_CASES))
def test_decoys_stay_in_the_domain_of_the_true_value(name):
    t = DECOY_CASES[name]
    for true in (t, t.to(DEV)):
        d = SO.decoy(true)
        assert d.dtype == true.dtype and d.shape == true.shape and d.device == true.device and d.is_contiguous()
        assert d.data_ptr() != true.data_ptr()
        if not true.dtype.is_floating_point or true.dim() == 0 or true.shape[0] < 2:
            assert torch.equal(d, true)  # integers (indices, counts), bools and masks of bytes, single rows: the true value
            continue
        # the true rows, each exactly once, in another order: finite, no poison, and whatever holds per row of the true
        # value -- a range, a sign, a unit norm, a 0 / 1 mask -- holds per row of the decoy
        assert bool(torch.isfinite(d).all()) and torch.equal(d, torch.roll(true, 1, 0)) and torch.equal(d[1:], true[:-1])
        assert torch.equal(d[0], true[-1]) and d.min() == true.min() and d.max() == true.max()
        if name in ("rows", "sh", "vector", "matrix", "positive", "half"):
            assert not torch.equal(d, true)  # ... and a reader that comes early computes something else
