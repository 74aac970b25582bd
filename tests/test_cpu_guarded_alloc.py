"""The guard-band allocator of guarded_alloc.py, proven on CPU tensors: what test_gpu_guard_bands.py relies on when it
says that no kernel wrote outside a buffer."""
import threading

import pytest
import torch

from guarded_alloc import ALIGN, NAMES, GuardedAllocator

CPU = torch.device("cpu")
DTYPES = [torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64]


def _alloc(pattern=0xFF, **kw):
    return GuardedAllocator(pattern, device=CPU, **kw)


def _raw_of(ga, i=-1):
    r = ga.records[i]
    return r["raw"], r["lo"], r["nbytes"]


def _this_line():
    import sys

    return sys._getframe(1).f_lineno


def test_clean_run_reports_nothing():
    with _alloc() as ga:
        a = torch.empty((3, 5), dtype=torch.float32)
        b = torch.zeros(7, dtype=torch.int32)
        c = torch.ones((2, 2))
        d = torch.full((4,), 2.5)
        e = torch.empty_like(a)
        f = torch.zeros_like(b)
        for t in (a, b, c, d, e, f):  # legitimate full writes
            t.fill_(3)
    assert len(ga) == 6
    assert ga.check() == []
    ga.assert_clean()


@pytest.mark.parametrize("side", ["back", "front"])
def test_one_byte_outside_is_reported_with_side_offset_and_site(side):
    with _alloc(0x5A) as ga:
        line = _this_line() + 1
        t = torch.empty((5, 3), dtype=torch.float32)
        other = torch.zeros(9, dtype=torch.int64)
    raw, lo, n = _raw_of(ga, 0)
    assert n == 60 and t.data_ptr() == raw.data_ptr() + lo
    raw[lo + n if side == "back" else lo - 1] = 0x00
    got = ga.check()
    assert got == [dict(site=f"tests/test_cpu_guarded_alloc.py:{line}", shape=(5, 3), dtype=torch.float32, side=side,
                        offset=0 if side == "back" else -1, count=1)]
    with pytest.raises(AssertionError) as e:
        ga.assert_clean()
    assert f"test_cpu_guarded_alloc.py:{line}" in str(e.value) and side in str(e.value)
    del other


def test_far_end_of_each_guard_is_watched():
    with _alloc(front=64, back=128) as ga:
        torch.empty(10, dtype=torch.uint8)
    raw, lo, n = _raw_of(ga)
    raw[0] = 1
    raw[lo + n + 127] = 1
    raw[lo + n + 5] = 1
    got = {v["side"]: v for v in ga.check()}
    assert got["front"]["offset"] == -lo and got["front"]["count"] == 1
    assert got["back"]["offset"] == 5 and got["back"]["count"] == 2


def test_understate_turns_a_full_legitimate_write_into_four_bytes_at_back():
    with _alloc() as ga:
        ga.understate(4)
        t = torch.empty((2, 8), dtype=torch.float32)
        u = torch.empty((2, 8), dtype=torch.float32)  # only the next allocation is understated
        assert ga.check() == []
        t.fill_(1.0)
        u.fill_(1.0)
    got = ga.check()
    assert len(got) == 1
    assert (got[0]["side"], got[0]["offset"], got[0]["count"], got[0]["shape"]) == ("back", 0, 4, (2, 8))


def test_understate_with_a_filling_allocation_starts_clean():
    with _alloc(0x5A) as ga:
        ga.understate(4)
        t = torch.zeros(8, dtype=torch.float32)
        assert ga.check() == []
        t.fill_(0.0)
    assert [(v["side"], v["count"]) for v in ga.check()] == [("back", 4)]


@pytest.mark.parametrize("pattern", [0xFF, 0x5A])
def test_interiors_empty_is_poison_and_the_others_hold_their_value(pattern):
    with _alloc(pattern) as ga:
        e = torch.empty((3, 7), dtype=torch.float32)
        el = torch.empty_like(e, dtype=torch.int32)
        z = torch.zeros((3, 7), dtype=torch.float32)
        zl = torch.zeros_like(e)
        o = torch.ones(5, dtype=torch.int64)
        f = torch.full((2, 3), 7, dtype=torch.int32)
        fb = torch.full((4,), True)
    assert (e.view(torch.uint8) == pattern).all() and (el.view(torch.uint8) == pattern).all()
    if pattern == 0xFF:
        assert torch.isnan(e).all() and (el == -1).all()
    assert (z == 0).all() and (zl == 0).all() and (o == 1).all() and (f == 7).all()
    assert fb.dtype == torch.bool and fb.all()
    ga.assert_clean()


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
def test_dtype_shape_alignment_and_tight_back_guard(dtype):
    with _alloc(front=4096, back=65536) as ga:
        for shape in [(1,), (257,), (3, 5, 7)]:
            t = torch.empty(shape, dtype=dtype)
            v = torch.zeros(*shape, dtype=dtype)  # sizes as separate arguments
            for x, i in ((t, -2), (v, -1)):
                assert x.dtype == dtype and tuple(x.shape) == shape and x.is_contiguous() and x.device == CPU
                assert x.data_ptr() % ALIGN == 0
                raw, lo, n = _raw_of(ga, i)
                assert n == x.numel() * x.element_size()  # no rounding: the guard starts at the first byte behind
                assert x.data_ptr() == raw.data_ptr() + lo and lo >= 4096 and raw.numel() - lo - n >= 65536
                assert (raw[:lo] == 0xFF).all() and (raw[lo + n:] == 0xFF).all()


def test_requires_grad_and_like_keywords_are_honoured():
    with _alloc() as ga:
        a = torch.zeros((4, 3), dtype=torch.float32, requires_grad=True)
        b = torch.empty((4, 3), requires_grad=True)
        src = torch.zeros((2, 3, 4, 5), dtype=torch.float32)
        c = torch.zeros_like(src, dtype=torch.float64, requires_grad=True)
        d = torch.empty_like(src, memory_format=torch.channels_last)
        e = torch.empty_like(src.permute(0, 2, 1, 3), memory_format=torch.contiguous_format)
        n = len(ga)
    assert a.requires_grad and a.is_leaf and b.requires_grad and b.is_leaf
    (a * 2).sum().backward()
    assert (a.grad == 2).all()
    assert c.dtype == torch.float64 and c.requires_grad and tuple(c.shape) == (2, 3, 4, 5)
    assert d.is_contiguous(memory_format=torch.channels_last) and tuple(d.shape) == (2, 3, 4, 5)
    assert e.is_contiguous() and tuple(e.shape) == (2, 4, 3, 5)
    assert n == 6
    ga.assert_clean()


def test_what_the_wrapper_does_not_understand_falls_through():
    with _alloc() as ga:
        z = torch.empty(0, dtype=torch.uint8)
        m = torch.empty(4, device="meta")
        out = torch.zeros(3)
        n = len(ga)
        torch.ones(3, out=out)
    assert n == 1 and z.numel() == 0 and m.device.type == "meta" and (out == 1).all()


def test_place_surrounds_a_callers_tensor_with_poison():
    src = torch.arange(15, dtype=torch.float32).reshape(5, 3).t()  # not contiguous
    src.requires_grad_(True)
    with _alloc(0x5A) as ga:
        p = ga.place(src)
    assert torch.equal(p.detach(), src.detach()) and p.is_contiguous() and p.requires_grad and p.is_leaf
    raw, lo, n = _raw_of(ga)
    assert n == 60 and (raw[:lo] == 0x5A).all() and (raw[lo + n:] == 0x5A).all() and p.data_ptr() % ALIGN == 0
    ga.assert_clean()


def test_the_six_functions_are_the_originals_again_after_exit():
    before = {n: getattr(torch, n) for n in NAMES}
    with _alloc():
        assert all(getattr(torch, n) is not before[n] for n in NAMES)
    assert all(getattr(torch, n) is before[n] for n in NAMES)
    with pytest.raises(KeyError):
        with _alloc():
            raise KeyError("x")
    assert all(getattr(torch, n) is before[n] for n in NAMES)


def test_allocations_from_a_second_thread_are_registered():
    made = []

    def work():
        for _ in range(50):
            made.append(torch.empty(33, dtype=torch.float32))

    with _alloc() as ga:
        th = threading.Thread(target=work)
        th.start()
        for _ in range(50):
            made.append(torch.zeros(17, dtype=torch.int32))
        th.join()
    assert len(ga) == 100 and len({t.data_ptr() for t in made}) == 100
    ga.assert_clean()
    raw, lo, n = _raw_of(ga, 37)
    raw[lo + n] ^= 0xFF
    assert len(ga.check()) == 1
