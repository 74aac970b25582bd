"""Guard bands and poison around every buffer the Python glue hands to the native library (a helper module, imported by
test_cpu_guarded_alloc.py, test_gpu_guard_bands.py and test_gpu_stream_order.py only).

The library never allocates: outputs, the three state buffers and every workspace are `torch.empty` / `torch.zeros` /
`torch.ones` / `torch.full` / `torch.empty_like` / `torch.zeros_like` calls of `gaussianeditor_amd/**`, looked up as
`torch.<name>` at call time.  While a `GuardedAllocator` is active those six names are replaced: an allocation on the
selected device becomes ONE raw uint8 tensor

    [ front guard | interior: numel * itemsize bytes | back guard ]        all filled with `pattern`

and the caller receives the interior viewed as the dtype and shape it asked for.  The interior starts 256-byte aligned
and the back guard starts at the very first byte behind it (no rounding).  `empty` / `empty_like` leave the interior
poisoned; `zeros` / `ones` / `full` set it to their value.  `check()` then finds every guard byte that no longer holds
the pattern: a store before the start or past the end of a buffer, which torch's caching allocator (512-byte rounding,
pooled blocks) would have absorbed in padding or in a neighbour's block.

Anything the wrappers do not understand -- another device, pin_memory, a sparse layout, `out=`, named tensors, a
zero-size tensor -- goes to the real function untouched.
"""
import operator
import os
import sys
import threading

import torch

ALIGN = 256
NAMES = ("empty", "zeros", "ones", "full", "empty_like", "zeros_like")

_HERE = os.path.abspath(__file__)
_TESTS = os.path.dirname(_HERE)
_ROOT = os.path.dirname(_TESTS)
_PRODUCT = os.path.join(_ROOT, "gaussianeditor_amd") + os.sep


def _site():
    """`file:line` of the first frame, walking outwards from the allocation call, that lies inside gaussianeditor_amd/ or
    in a test file (this module excluded)."""
    f = sys._getframe(1)
    while f is not None:
        path = os.path.abspath(f.f_code.co_filename)
        if path != _HERE and (path.startswith(_PRODUCT) or path.startswith(_TESTS + os.sep)):
            return f"{os.path.relpath(path, _ROOT)}:{f.f_lineno}"
        f = f.f_back
    return "?:0"


class GuardedAllocator:
    """Context manager; see the module docstring.  `device`: the device whose allocations are guarded (default: the
    current ROCm device where there is one, else the CPU)."""

    def __init__(self, pattern, front=4096, back=65536, device=None):
        if not 0 <= int(pattern) <= 255 or front < 0 or back < 0:
            raise ValueError("pattern must be a byte value, front and back non-negative")
        self.pattern, self.front, self.back = int(pattern), int(front), int(back)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = self._norm(torch.device(device))
        self._lock = threading.Lock()
        self.records = []      # dicts: raw, lo (byte offset of the interior in raw), nbytes (recorded), site, shape, dtype
        self._understate = 0
        self._saved = None

    # ---- patching ----------------------------------------------------------------------------------------------------
    def __enter__(self):
        if self._saved is not None:
            raise RuntimeError("GuardedAllocator is already active")
        self._saved = {n: getattr(torch, n) for n in NAMES}
        try:
            for n in NAMES:
                setattr(torch, n, self._wrap(n, self._saved[n]))
        except BaseException:
            self._restore()
            raise
        return self

    def __exit__(self, *exc):
        self._restore()
        return False

    def _restore(self):
        saved, self._saved = self._saved, None
        for n, fn in (saved or {}).items():
            setattr(torch, n, fn)

    def _wrap(self, name, real):
        like = name.endswith("_like")

        def guarded(*args, **kwargs):
            try:
                return (self._like if like else self._plain)(name, real, args, dict(kwargs))
            except _Fallthrough:
                return real(*args, **kwargs)

        guarded.__name__ = name
        guarded.__wrapped__ = real
        return guarded

    # ---- argument handling -------------------------------------------------------------------------------------------
    @staticmethod
    def _norm(dev):
        if dev.type == "cuda" and dev.index is None:
            return torch.device("cuda", torch.cuda.current_device())
        return dev

    def _common(self, kw, default_dtype, default_device):
        """Pops the keywords the wrappers understand -> (dtype, requires_grad); falls through on anything else."""
        dtype = kw.pop("dtype", None) or default_dtype
        device = kw.pop("device", None)
        device = default_device if device is None else torch.device(device)
        requires_grad = bool(kw.pop("requires_grad", False))
        if kw.pop("layout", torch.strided) not in (torch.strided, None) or kw.pop("pin_memory", False):
            raise _Fallthrough
        if kw:  # out=, names=, ...
            raise _Fallthrough
        if self._norm(device) != self.device or not isinstance(dtype, torch.dtype):
            raise _Fallthrough
        return dtype, requires_grad

    @staticmethod
    def _shape(args):
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            args = tuple(args[0])
        try:
            return tuple(operator.index(a) for a in args)
        except TypeError:
            raise _Fallthrough from None

    def _plain(self, name, real, args, kw):
        fill = None
        if name == "full":
            if "fill_value" in kw:
                fill = kw.pop("fill_value")
            elif len(args) == 2:
                args, fill = args[:1], args[1]
            else:
                raise _Fallthrough
            if "size" in kw:
                args = (kw.pop("size"),)
            if isinstance(fill, torch.Tensor) or not isinstance(fill, (bool, int, float)):
                raise _Fallthrough
            default_dtype = torch.tensor(fill).dtype
        else:
            if "size" in kw:
                if args:
                    raise _Fallthrough
                args = (kw.pop("size"),)
            default_dtype = torch.get_default_dtype()
            fill = {"zeros": 0, "ones": 1}.get(name)
        if kw.pop("memory_format", torch.contiguous_format) != torch.contiguous_format:
            raise _Fallthrough
        shape = self._shape(args)
        dtype, requires_grad = self._common(kw, default_dtype, _default_device())
        return self._make(shape, None, dtype, fill, requires_grad)

    def _like(self, name, real, args, kw):
        if len(args) != 1 or not isinstance(args[0], torch.Tensor):
            raise _Fallthrough
        src = args[0]
        if src.layout != torch.strided or src.is_quantized:
            raise _Fallthrough
        memory_format = kw.pop("memory_format", torch.preserve_format)
        dtype, requires_grad = self._common(kw, src.dtype, src.device)
        # the strides the real function would give (memory_format honoured), worked out on the meta device
        meta_src = torch.empty_strided(tuple(src.shape), tuple(src.stride()), dtype=src.dtype, device="meta")
        meta = self._saved["empty_like"](meta_src, dtype=dtype, memory_format=memory_format)
        return self._make(tuple(src.shape), tuple(meta.stride()), dtype, 0 if name == "zeros_like" else None, requires_grad)

    # ---- allocation --------------------------------------------------------------------------------------------------
    def _make(self, shape, strides, dtype, fill, requires_grad, site=None):
        numel = 1
        for s in shape:
            if s < 0:
                raise _Fallthrough
            numel *= s
        if numel == 0:
            raise _Fallthrough
        real_empty = self._saved["empty"] if self._saved is not None else torch.empty  # (place() also works outside `with`)
        nbytes = numel * real_empty((), dtype=dtype, device="meta").element_size()
        # (ALIGN spare bytes so that the interior can start on an ALIGN boundary whatever the raw block's address is: the
        #  front guard is then `front` .. `front + ALIGN - 1` bytes long, the back guard `back` or more)
        raw = real_empty(self.front + nbytes + self.back + ALIGN, dtype=torch.uint8, device=self.device)
        raw.fill_(self.pattern)
        lo = self.front + (-(raw.data_ptr() + self.front)) % ALIGN
        flat = raw[lo:lo + nbytes].view(dtype)
        out = flat.view(shape) if strides is None else flat.as_strided(shape, strides)
        if fill is not None:
            out.fill_(fill)
        with self._lock:
            under, self._understate = self._understate, 0
            if under:
                if not 0 < under <= nbytes:
                    raise ValueError("understate: more bytes than the allocation has")
                raw[lo + nbytes - under:lo + nbytes] = self.pattern
            self.records.append(dict(raw=raw, lo=lo, nbytes=nbytes - under, site=site or _site(), shape=shape,
                                     dtype=dtype))
        if requires_grad:
            out.requires_grad_(True)
        return out

    def place(self, tensor):
        """A copy of `tensor` (values, dtype, shape; contiguous) inside a guarded interior on the selected device, so that a
        test's own inputs are surrounded by poison.  requires_grad is carried over (the copy is a leaf)."""
        t = tensor.detach()
        if t.numel() == 0:
            out = t.to(self.device).clone()
        else:
            out = self._make(tuple(t.shape), None, t.dtype, None, False, site=_site())
            out.copy_(t)
        if tensor.requires_grad:
            out.requires_grad_(True)
        return out

    def understate(self, nbytes):
        """The next guarded allocation is RECORDED `nbytes` shorter than the tensor handed out: its last `nbytes` bytes
        count as back guard.  For the detector's self-tests: a kernel's legitimate full write then shows as a violation
        without a byte being written outside the allocation."""
        with self._lock:
            self._understate = int(nbytes)

    # ---- checking ----------------------------------------------------------------------------------------------------
    def check(self):
        """Synchronises, then -> one record per violated guard: dict(site, shape, dtype, side ('front' | 'back'), offset,
        count).  `offset`: of the first changed byte in address order, relative to the interior's edge -- 0 is the first
        byte behind the interior for 'back', -1 the byte just in front of it for 'front'.  `count`: changed bytes."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        with self._lock:
            records = list(self.records)
        guards, counts = [], []
        for r in records:
            raw, lo, n = r["raw"], r["lo"], r["nbytes"]
            for side, g in (("front", raw[:lo]), ("back", raw[lo + n:])):
                bad = g != self.pattern
                guards.append((r, side, bad))
                counts.append(bad.sum())
        if not counts:
            return []
        counts = torch.stack(counts).cpu().tolist()
        out = []
        for (r, side, bad), c in zip(guards, counts):
            if c:
                first = int(bad.nonzero()[0])
                out.append(dict(site=r["site"], shape=r["shape"], dtype=r["dtype"], side=side,
                                offset=first - r["lo"] if side == "front" else first, count=int(c)))
        return out

    def assert_clean(self):
        bad = self.check()
        if bad:
            lines = [f"  {v['site']} {tuple(v['shape'])} {v['dtype']}: {v['side']} guard, first changed byte at offset "
                     f"{v['offset']}, {v['count']} byte(s) changed" for v in bad]
            raise AssertionError(f"{len(bad)} guard band(s) written (pattern 0x{self.pattern:02X}):\n" + "\n".join(lines))

    def __len__(self):
        with self._lock:
            return len(self.records)


class _Fallthrough(Exception):
    pass


def _default_device():
    get = getattr(torch, "get_default_device", None)
    return get() if get is not None else torch.device("cpu")
