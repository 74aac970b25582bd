"""Densify / prune surgery on the tensors of a Gaussian model.

PRUNE = one stable row compaction for all tensors:

`GaussianModel.prune_points` / `_prune_optimizer` (gaussiansplatting/scene/gaussian_model.py:568-609) index six
parameters, their twelve Adam moment tensors and five bookkeeping tensors with the same boolean mask, one after the
other; every `tensor[mask]` runs its own nonzero + host sync + gather.  `compact_rows` scans the mask once (one host
readback for the number of survivors) and moves the surviving rows of ALL tensors with one launch of the HIP kernel
behind `gsr_compact_apply` (include/gsr.h).  The survivors keep their order, so each output equals `tensor[mask]` bit
for bit.  `prune_optimizer` is `_prune_optimizer` on top of it.

DENSIFY = rows appended to all tensors: `cat_tensors_to_optimizer` (:609-641), which `densification_postfix` (:643-671)
calls at the end of both `densify_and_clone` (:730-766) and `densify_and_split` (:673-728), runs `torch.cat` on each of
the six parameters and on their twelve Adam moments (the moments extended by `torch.zeros_like`): 18 cats + 12 fills.
`append_rows` writes every `[old rows ; new rows | zeros]` with ONE launch of the kernel behind `gsr_append_rows`;
`cat_tensors_to_optimizer` is the reference's method on top of it, `clone_rows` = select by mask (one compaction) +
append, i.e. the tensor side of `densify_and_clone`.  With these functions WHICH rows are cloned / how split samples
are drawn stays in torch with the caller, as in the reference.

The POLICY = which rows: `add_densification_stats` is the per-step bookkeeping of
`on_before_optimizer_step` (threestudio/systems/GassuianEditor.py:251-281) with `add_densification_stats` (:811-815) as
one launch without host synchronisation; `select_densification` the decision of `densify_and_prune` (:771-777),
`densify_and_clone` (:732-739) and `densify_and_split` (:676-683) with one readback (the quantile by a radix select, not
a sort); `split_positions` the children's positions (:685-691); `prune_keep_mask` the prune mask (:787-794).
`densify_and_prune` composes them with the surgery above into the reference's method: ONE append and ONE compaction
instead of two each.  The split's random numbers are still drawn with `torch.randn`, so seeding works as before.
No CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch
from torch.autograd.graph import increment_version

from . import _native

__all__ = ["compact_rows", "prune_optimizer", "append_rows", "cat_tensors_to_optimizer", "clone_rows",
           "add_densification_stats", "select_densification", "split_positions", "prune_keep_mask", "densify_and_prune",
           "DensifySelection"]


def compact_rows(tensors: Sequence[torch.Tensor], keep: torch.Tensor) -> List[torch.Tensor]:
    """[t[keep] for t in tensors] for tensors that share their leading dimension P with the (P,) bool mask `keep`."""
    if keep.dim() != 1 or keep.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("compact_rows: keep must be a 1-D bool / uint8 mask")
    if not keep.is_cuda:
        raise RuntimeError("compact_rows: tensors must live on the ROCm GPU; there is no CPU fallback")
    P = int(keep.numel())
    dev = keep.device
    srcs = []
    for t in tensors:
        if t.device != dev or t.dim() < 1 or int(t.shape[0]) != P:
            raise RuntimeError("compact_rows: every tensor needs the mask's device and leading dimension")
        srcs.append(t.detach().contiguous())
    if P == 0:
        return [s.clone() for s in srcs]
    k8 = keep.contiguous().view(torch.uint8) if keep.dtype == torch.bool else keep.contiguous()
    L = _native.lib()
    nbytes = ctypes.c_size_t(0)
    _native.check("gsr_compact_workspace_size", L.gsr_compact_workspace_size(P, ctypes.byref(nbytes)))
    work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    kept = ctypes.c_int64(0)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        _native.check("gsr_compact_plan", L.gsr_compact_plan(s, P, k8.data_ptr(), work.data_ptr(), ctypes.byref(kept)))
        n = int(kept.value)
        outs = [torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in srcs]
        if n > 0:
            for lo in range(0, len(srcs), 32):
                chunk = list(zip(srcs[lo:lo + 32], outs[lo:lo + 32]))
                arr = (_native.CompactTensor * len(chunk))()
                for i, (src, dst) in enumerate(chunk):
                    row_bytes = src.element_size() * (src.numel() // P)
                    if row_bytes == 0:
                        raise RuntimeError("compact_rows: tensors with empty rows are not supported")
                    arr[i] = _native.CompactTensor(src.data_ptr(), dst.data_ptr(), row_bytes)
                _native.check("gsr_compact_apply", L.gsr_compact_apply(s, P, k8.data_ptr(), work.data_ptr(), len(chunk), arr))
    return outs


def _prune_optimizer_and(optimizer: torch.optim.Optimizer, keep: torch.Tensor, also: Sequence[torch.Tensor] = ()):
    """`prune_optimizer` with further tensors (bookkeeping) moved by the same compaction: ({name: parameter}, [also[keep]])."""
    items = []  # (group, old param, state or None)
    flat: List[torch.Tensor] = []
    for group in optimizer.param_groups:
        assert len(group["params"]) == 1
        p = group["params"][0]
        st = optimizer.state.get(p, None)
        items.append((group, p, st))
        flat.append(p)
        if st is not None and "exp_avg" in st:
            flat += [st["exp_avg"], st["exp_avg_sq"]]
    outs = compact_rows(flat + list(also), keep)
    result: Dict[str, torch.nn.Parameter] = {}
    i = 0
    for group, p, st in items:
        new_p = torch.nn.Parameter(outs[i].requires_grad_(True))
        i += 1
        if st is not None and "exp_avg" in st:
            st["exp_avg"], st["exp_avg_sq"] = outs[i], outs[i + 1]
            i += 2
        if st is not None:
            del optimizer.state[p]
            optimizer.state[new_p] = st
        group["params"][0] = new_p
        result[group["name"]] = new_p
    return result, outs[i:]


def prune_optimizer(optimizer: torch.optim.Optimizer, keep: torch.Tensor) -> Dict[str, torch.nn.Parameter]:
    """`GaussianModel._prune_optimizer(mask)` (gaussian_model.py:568-591) with one compaction for all groups: every
    group's single parameter and its `exp_avg` / `exp_avg_sq` lose the rows where `keep` is False.  Returns
    {group["name"]: new parameter}."""
    return _prune_optimizer_and(optimizer, keep)[0]


def append_rows(tensors: Sequence[torch.Tensor], extensions: Sequence[Optional[torch.Tensor]], n: Optional[int] = None
                ) -> List[torch.Tensor]:
    """[torch.cat((t, e)) for t, e in zip(tensors, extensions)], an extension of None standing for `n` zero rows
    (torch.cat((t, zeros)) -- what the reference does to the Adam moments).  All tensors share their leading dimension P,
    all extensions theirs (n); trailing shapes and dtypes of a pair must agree."""
    if len(tensors) != len(extensions):
        raise RuntimeError("append_rows: one extension (or None) per tensor")
    if not tensors:
        return []
    dev = tensors[0].device
    if not tensors[0].is_cuda:
        raise RuntimeError("append_rows: tensors must live on the ROCm GPU; there is no CPU fallback")
    P = int(tensors[0].shape[0])
    for e in extensions:
        if e is not None:
            n = int(e.shape[0]) if n is None else n
            if int(e.shape[0]) != n:
                raise RuntimeError("append_rows: all extensions need the same number of rows")
    if n is None:
        raise RuntimeError("append_rows: give n when every extension is None")
    srcs, exts, outs = [], [], []
    for t, e in zip(tensors, extensions):
        if t.device != dev or t.dim() < 1 or int(t.shape[0]) != P:
            raise RuntimeError("append_rows: every tensor needs the same device and leading dimension")
        if e is not None and (e.device != dev or e.dtype != t.dtype or tuple(e.shape[1:]) != tuple(t.shape[1:])):
            raise RuntimeError("append_rows: an extension must match its tensor's device, dtype and row shape")
        srcs.append(t.detach().contiguous())
        exts.append(None if e is None else e.detach().contiguous())
        outs.append(torch.empty((P + n,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev))
    if P + n == 0:
        return outs
    L = _native.lib()
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        for lo in range(0, len(srcs), 32):
            chunk = list(zip(srcs[lo:lo + 32], exts[lo:lo + 32], outs[lo:lo + 32]))
            arr = (_native.AppendTensor * len(chunk))()
            for i, (src, ext, dst) in enumerate(chunk):
                row_bytes = dst.element_size() * (dst.numel() // (P + n))
                if row_bytes == 0:
                    raise RuntimeError("append_rows: tensors with empty rows are not supported")
                arr[i] = _native.AppendTensor(src.data_ptr() if P else None, None if ext is None or n == 0 else ext.data_ptr(),
                                              dst.data_ptr(), row_bytes)
            _native.check("gsr_append_rows", L.gsr_append_rows(s, P, n, len(chunk), arr))
    return outs


def cat_tensors_to_optimizer(optimizer: torch.optim.Optimizer, tensors_dict: Dict[str, torch.Tensor]
                             ) -> Dict[str, torch.nn.Parameter]:
    """`GaussianModel.cat_tensors_to_optimizer(tensors_dict)` (gaussian_model.py:609-641) with one launch for all groups:
    every group's single parameter gets `tensors_dict[group["name"]]` appended, its `exp_avg` / `exp_avg_sq` the same
    number of zero rows.  Returns {group["name"]: new parameter}."""
    items, flat, ext = [], [], []
    n = None
    for group in optimizer.param_groups:
        assert len(group["params"]) == 1
        p = group["params"][0]
        e = tensors_dict[group["name"]]
        n = int(e.shape[0]) if n is None else n
        st = optimizer.state.get(p, None)
        has_moments = st is not None and "exp_avg" in st
        items.append((group, p, st, has_moments))
        flat.append(p)
        ext.append(e)
        if has_moments:
            flat += [st["exp_avg"], st["exp_avg_sq"]]
            ext += [None, None]
    outs = append_rows(flat, ext, n=n)
    result: Dict[str, torch.nn.Parameter] = {}
    i = 0
    for group, p, st, has_moments in items:
        new_p = torch.nn.Parameter(outs[i].requires_grad_(True))
        i += 1
        if has_moments:
            st["exp_avg"], st["exp_avg_sq"] = outs[i], outs[i + 1]
            i += 2
        if st is not None:
            del optimizer.state[p]
            optimizer.state[new_p] = st
        group["params"][0] = new_p
        result[group["name"]] = new_p
    return result


def clone_rows(optimizer: torch.optim.Optimizer, selected: torch.Tensor) -> Dict[str, torch.nn.Parameter]:
    """The tensor side of `densify_and_clone` (gaussian_model.py:730-766): the rows of every group's parameter where
    `selected` is set are appended to it (moments: zero rows) -- `param[selected]` for all groups by one compaction,
    then `cat_tensors_to_optimizer`."""
    names = [g["name"] for g in optimizer.param_groups]
    picked = compact_rows([g["params"][0] for g in optimizer.param_groups], selected)
    return cat_tensors_to_optimizer(optimizer, dict(zip(names, picked)))


# ----------------------------------------------------------------------------------------------------------------------
# the densification policy (include/gsr.h: gsr_densify_*)
# ----------------------------------------------------------------------------------------------------------------------
def _need(what: str, *pairs) -> torch.device:
    """Every (tensor | None, dtype | tuple of dtypes) pair: the dtypes first, then one ROCm device for all.  Returns it."""
    pairs = [(t, d if isinstance(d, tuple) else (d,)) for t, d in pairs if t is not None]
    for t, dtypes in pairs:
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
            raise RuntimeError(f"{what}: expected a tensor of dtype {' / '.join(str(d) for d in dtypes)}, got "
                               f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
    dev = pairs[0][0].device
    for t, _ in pairs:
        if not t.is_cuda or t.device != dev:
            raise RuntimeError(f"{what}: tensors must live on one ROCm GPU; there is no CPU fallback")
    return dev


_MASK = (torch.bool, torch.uint8)


def _u8(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def add_densification_stats(xyz_gradient_accum: torch.Tensor, denom: torch.Tensor, max_radii2D: torch.Tensor,
                            grads: Sequence[torch.Tensor], radii: Sequence[torch.Tensor]) -> None:
    """The statistics of one optimizer step, in place, as one launch that never synchronises with the host
    (GassuianEditor.py:251-281, gaussian_model.py:811-815): `grads` = the 1..8 views' `viewspace_points.grad` (or
    `.absgrad`) (P,3), `radii` = their radii (P,) int32.  Rows no view sees (max radii <= 0) are neither read nor written;
    for the others `xyz_gradient_accum += norm(sum of the views' gradients [:2])`, `denom += 1` and
    `max_radii2D = max(max_radii2D, radii)`."""
    grads, radii = list(grads), list(radii)
    V = len(grads)
    if V < 1 or V > 8 or len(radii) != V:
        raise ValueError("add_densification_stats: 1..8 views, one radii tensor per gradient tensor")
    _need("add_densification_stats", *[(t, torch.float32) for t in (xyz_gradient_accum, denom, max_radii2D, *grads)],
          *[(r, torch.int32) for r in radii])
    dev = xyz_gradient_accum.device
    P = int(xyz_gradient_accum.numel())
    for t in (xyz_gradient_accum, denom, max_radii2D):
        if int(t.numel()) != P or not t.is_contiguous():
            raise RuntimeError("add_densification_stats: the statistics must be contiguous tensors of P elements (updated in place)")
    gs, rs = [], []
    for g, r in zip(grads, radii):
        if tuple(g.shape) != (P, 3) or int(r.numel()) != P:
            raise RuntimeError("add_densification_stats: gradients must be (P, 3), radii (P,)")
        gs.append(g.detach().contiguous())
        rs.append(r.contiguous())
    if P == 0:
        return
    gp = (ctypes.c_void_p * V)(*[g.data_ptr() for g in gs])
    rp = (ctypes.c_void_p * V)(*[r.data_ptr() for r in rs])
    L = _native.lib()
    increment_version((xyz_gradient_accum, denom, max_radii2D))  # updated through raw pointers: what `+=` does by itself
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        _native.check("gsr_densify_stats", L.gsr_densify_stats(s, P, V, gp, rp, xyz_gradient_accum.data_ptr(), denom.data_ptr(),
                                                               max_radii2D.data_ptr()))


class DensifySelection(NamedTuple):
    """What `select_densification` decided.  `workspace` keeps the plans of both masks alive for `split_positions` and the
    row copies of `densify_and_prune` (`clone_plan` / `split_plan` point into it)."""
    clone_sel: torch.Tensor   # (P,) bool
    split_sel: torch.Tensor   # (P,) bool
    nonzero: int              # rows with a non-zero statistic before the threshold
    n_clone: int
    n_split: int
    threshold: float          # the quantile (0.0 when max_densify_percent >= 1)
    workspace: Optional[torch.Tensor]
    clone_plan: Optional[int]
    split_plan: Optional[int]


def select_densification(xyz_gradient_accum: torch.Tensor, denom: torch.Tensor, mask: torch.Tensor, scaling: torch.Tensor, *,
                         max_grad: float, max_densify_percent: float, percent_dense: float, extent: float) -> DensifySelection:
    """Which rows `densify_and_prune` clones and splits (gaussian_model.py:771-777, :732-739, :676-683), decided on the GPU
    with one readback.  `scaling` is the ACTIVATED scaling (`get_scaling`), `mask` the edit mask (bool / uint8).  At most
    2**24 rows (torch.quantile's own limit); `max_grad` must be positive."""
    if not max_grad > 0:
        raise ValueError("select_densification: max_grad must be > 0 (0 would select rows outside the mask)")
    if not max_densify_percent >= 0:
        raise ValueError("select_densification: max_densify_percent must be >= 0")
    dev = _need("select_densification", (xyz_gradient_accum, torch.float32), (denom, torch.float32), (scaling, torch.float32),
                (mask, _MASK))
    P = int(xyz_gradient_accum.numel())
    if P > (1 << 24):
        raise ValueError("select_densification: at most 2**24 rows")
    if int(denom.numel()) != P or int(mask.numel()) != P or tuple(scaling.shape) != (P, 3):
        raise RuntimeError("select_densification: statistics and mask need P elements, scaling (P, 3)")
    clone_sel = torch.empty(P, dtype=torch.bool, device=dev)
    split_sel = torch.empty(P, dtype=torch.bool, device=dev)
    if P == 0:
        return DensifySelection(clone_sel, split_sel, 0, 0, 0, 0.0, None, None, None)
    L = _native.lib()
    nbytes = ctypes.c_size_t(0)
    _native.check("gsr_densify_workspace_size", L.gsr_densify_workspace_size(P, ctypes.byref(nbytes)))
    work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    a, d, m, sc = xyz_gradient_accum.detach().contiguous(), denom.detach().contiguous(), _u8(mask), scaling.detach().contiguous()
    res = _native.DensifyResult()
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        _native.check("gsr_densify_select", L.gsr_densify_select(
            s, P, a.data_ptr(), d.data_ptr(), m.data_ptr(), sc.data_ptr(), float(max_grad), float(max_densify_percent),
            float(percent_dense), float(extent), work.data_ptr(), clone_sel.data_ptr(), split_sel.data_ptr(), ctypes.byref(res)))
    cp, sp = ctypes.c_void_p(), ctypes.c_void_p()
    _native.check("gsr_densify_plans", L.gsr_densify_plans(work.data_ptr(), P, ctypes.byref(cp), ctypes.byref(sp)))
    return DensifySelection(clone_sel, split_sel, int(res.nonzero), int(res.n_clone), int(res.n_split), float(res.threshold),
                            work, int(cp.value), int(sp.value))


def _plan_of(sel: torch.Tensor):
    """(mask as uint8, plan workspace tensor, plan address, number of set rows) of a bare mask: one gsr_compact_plan."""
    P = int(sel.numel())
    k8 = _u8(sel)
    L = _native.lib()
    nbytes = ctypes.c_size_t(0)
    _native.check("gsr_compact_workspace_size", L.gsr_compact_workspace_size(P, ctypes.byref(nbytes)))
    work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=sel.device)
    kept = ctypes.c_int64(0)
    with torch.cuda.device(sel.device):
        s = torch.cuda.current_stream(sel.device).cuda_stream
        _native.check("gsr_compact_plan", L.gsr_compact_plan(s, P, k8.data_ptr(), work.data_ptr(), ctypes.byref(kept)))
    return k8, work, work.data_ptr(), int(kept.value)


def split_positions(xyz: torch.Tensor, scaling: torch.Tensor, rotation: torch.Tensor,
                    selection: Union[DensifySelection, torch.Tensor], noise: torch.Tensor, N: int = 2,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`new_xyz` of `densify_and_split` (gaussian_model.py:685-691): `build_rotation(rotation[sel]) @ (noise * scaling[sel])
    + xyz[sel]`, the N copies in `.repeat(N, 1)` order.  `scaling` is activated, `rotation` the raw quaternions, `noise`
    (N * n_split, 3) standard-normal numbers (`torch.randn` on the caller's generator); `selection` is what
    `select_densification` returned, or a bare (P,) mask."""
    if N < 1 or N > 8:
        raise ValueError("split_positions: N must be 1..8")
    dev = _need("split_positions", *[(t, torch.float32) for t in (xyz, scaling, rotation, noise)],
                (None if isinstance(selection, DensifySelection) else selection, _MASK))
    P = int(xyz.shape[0])
    if tuple(xyz.shape) != (P, 3) or tuple(scaling.shape) != (P, 3) or tuple(rotation.shape) != (P, 4):
        raise RuntimeError("split_positions: xyz and scaling must be (P, 3), rotation (P, 4)")
    if isinstance(selection, DensifySelection):
        sel8, keepalive, plan, n_split = _u8(selection.split_sel), selection.workspace, selection.split_plan, selection.n_split
        if int(sel8.numel()) != P:
            raise RuntimeError("split_positions: the selection belongs to another number of rows")
    else:
        if selection.dim() != 1 or int(selection.numel()) != P:
            raise RuntimeError("split_positions: the mask must be (P,)")
        sel8, keepalive, plan, n_split = _plan_of(selection) if P else (_u8(selection), None, None, 0)
    if tuple(noise.shape) != (N * n_split, 3):
        raise RuntimeError(f"split_positions: noise must be (N * n_split, 3) = ({N * n_split}, 3)")
    if out is None:
        out = torch.empty((N * n_split, 3), dtype=torch.float32, device=dev)
    elif out.device != dev or out.dtype != torch.float32 or tuple(out.shape) != (N * n_split, 3) or not out.is_contiguous():
        raise RuntimeError("split_positions: out must be a contiguous (N * n_split, 3) float32 tensor")
    if n_split == 0:
        return out
    increment_version(out)  # (a caller's `out=` is written through its raw pointer)
    x, sc, rot, nz = xyz.detach().contiguous(), scaling.detach().contiguous(), rotation.detach().contiguous(), noise.contiguous()
    L = _native.lib()
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        _native.check("gsr_densify_split_xyz", L.gsr_densify_split_xyz(
            s, P, x.data_ptr(), sc.data_ptr(), rot.data_ptr(), sel8.data_ptr(), plan, n_split, N, nz.data_ptr(), out.data_ptr()))
    del keepalive
    return out


def prune_keep_mask(opacity: torch.Tensor, scaling: torch.Tensor, mask: torch.Tensor, *, min_opacity: float,
                    max_screen_size: float, extent: float, max_radii2D: Optional[torch.Tensor] = None,
                    drop: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`~prune_mask` of `densify_and_prune` (gaussian_model.py:787-794) and not `drop`: a row is pruned if it is inside `mask`
    and faint (`opacity < min_opacity`), large on screen (`max_radii2D > max_screen_size`, when `max_radii2D` is given) or
    large in the world (`max(scaling) > 0.1 * extent`).  `opacity` and `scaling` are activated.  Returns a (P,) bool tensor."""
    dev = _need("prune_keep_mask", (opacity, torch.float32), (scaling, torch.float32), (max_radii2D, torch.float32),
                (mask, _MASK), (drop, _MASK))
    P = int(opacity.numel())
    if tuple(scaling.shape) != (P, 3) or int(mask.numel()) != P:
        raise RuntimeError("prune_keep_mask: opacity and mask need P elements, scaling (P, 3)")
    for t in (max_radii2D, drop):
        if t is not None and int(t.numel()) != P:
            raise RuntimeError("prune_keep_mask: max_radii2D and drop need P elements")
    keep = torch.empty(P, dtype=torch.bool, device=dev)
    if P == 0:
        return keep
    o, sc, m = opacity.detach().contiguous(), scaling.detach().contiguous(), _u8(mask)
    r = None if max_radii2D is None else max_radii2D.contiguous()
    d = None if drop is None else _u8(drop)
    L = _native.lib()
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        _native.check("gsr_densify_keep", L.gsr_densify_keep(
            s, P, o.data_ptr(), sc.data_ptr(), None if r is None else r.data_ptr(), m.data_ptr(),
            None if d is None else d.data_ptr(), float(min_opacity), float(max_screen_size), float(extent), keep.data_ptr()))
    return keep


def _gather_into(P: int, sel8: torch.Tensor, plan: int, pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]]) -> None:
    """dst[:] = src[sel] for every (src, dst) pair by one gsr_compact_apply under an existing plan of `sel8`."""
    if not pairs or int(pairs[0][1].shape[0]) == 0:
        return
    L = _native.lib()
    dev = sel8.device
    arr = (_native.CompactTensor * len(pairs))()
    for i, (src, dst) in enumerate(pairs):
        assert src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype
        arr[i] = _native.CompactTensor(src.data_ptr(), dst.data_ptr(), src.element_size() * (src.numel() // P))
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        _native.check("gsr_compact_apply", L.gsr_compact_apply(s, P, sel8.data_ptr(), plan, len(pairs), arr))


def densify_and_prune(optimizer: torch.optim.Optimizer, extra: Dict[str, torch.Tensor], *, max_grad: float,
                      max_densify_percent: float, min_opacity: float, extent: float, max_screen_size: Optional[float],
                      percent_dense: float, N: int = 2, scaling_activation: Callable = torch.exp,
                      scaling_inverse_activation: Callable = torch.log, opacity_activation: Callable = torch.sigmoid,
                      generation_num: Optional[int] = None, generator: Optional[torch.Generator] = None,
                      screen_prune: str = "reference"):
    """`GaussianModel.densify_and_prune` (gaussian_model.py:768-797) on an optimizer with the reference's six named groups
    (xyz, f_dc, f_rest, opacity, scaling, rotation) and the bookkeeping tensors `extra` = {"xyz_gradient_accum", "denom",
    "max_radii2D", "mask", optionally "generation"}: select, ONE append (`n_clone` clones followed by `N * n_split` split
    children), ONE compaction (the split parents and the pruned rows leave together).  The result equals the reference's,
    rows in its order: surviving originals, clones, children.  Every copied column, the Adam moments, the mask and the
    children's scaling are the reference's bits; the children's positions differ from its `bmm` by rounding only.  The
    split's noise is `torch.randn((N * n_split, 3), generator=generator)`, times the parents' scaling.

    The reference's `densification_postfix` has reset `max_radii2D` to zeros before the prune test, so its screen-size term
    never fires from here.  `screen_prune="reference"` (default) reproduces that; `"accumulated"` tests the `max_radii2D`
    gathered since the last densification (new rows: 0) against `max_screen_size`.  A false `max_screen_size` switches the
    screen AND world size terms off, as the reference's `if max_screen_size:` does.

    Returns ({name: new parameter}, new extra with the statistics reset to zeros, (before, n_clone, n_split, n_pruned)).
    `apply_grad_mask`, `update_anchor` and the anchor schedule stay with the caller."""
    if screen_prune not in ("reference", "accumulated"):
        raise ValueError("densify_and_prune: screen_prune is 'reference' or 'accumulated'")
    if N < 1 or N > 8:
        raise ValueError("densify_and_prune: N must be 1..8")
    groups = {g["name"]: g for g in optimizer.param_groups}
    names = [g["name"] for g in optimizer.param_groups]
    for k in ("xyz", "opacity", "scaling", "rotation"):
        if k not in groups:
            raise RuntimeError(f"densify_and_prune: the optimizer has no parameter group named {k!r}")
    par = {k: g["params"][0] for k, g in groups.items()}
    P = int(par["xyz"].shape[0])
    dev = par["xyz"].device
    mask = extra["mask"]
    with torch.no_grad():
        scaling = scaling_activation(par["scaling"].detach())
        sel = select_densification(extra["xyz_gradient_accum"], extra["denom"], mask, scaling, max_grad=max_grad,
                                   max_densify_percent=max_densify_percent, percent_dense=percent_dense, extent=extent)
        n_clone, n_split = sel.n_clone, sel.n_split
        n_new = n_clone + N * n_split
        # --- the appended rows: clones (:741-746), then the children copy by copy (:692-698)
        srcs = [par[k].detach().contiguous() for k in names] + [_u8(mask)]
        exts = [torch.empty((n_new,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in srcs]
        ext = dict(zip(names, exts))  # (the mask's rows stay in exts[-1])
        if n_clone:
            _gather_into(P, _u8(sel.clone_sel), sel.clone_plan, [(t, e[:n_clone]) for t, e in zip(srcs, exts)])
        if n_split:
            s8 = _u8(sel.split_sel)
            for c in range(N):
                lo = n_clone + c * n_split
                _gather_into(P, s8, sel.split_plan, [(t, e[lo:lo + n_split]) for t, e in zip(srcs, exts)])
            noise = torch.randn((N * n_split, 3), dtype=torch.float32, device=dev, generator=generator)
            split_positions(par["xyz"], scaling, par["rotation"], sel, noise, N, out=ext["xyz"][n_clone:])
            parents = torch.empty((n_split, 3), dtype=torch.float32, device=dev)
            _gather_into(P, s8, sel.split_plan, [(scaling.contiguous(), parents)])
            ext["scaling"][n_clone:] = scaling_inverse_activation(parents.repeat(N, 1) / (0.8 * N))
        new_mask = torch.cat((_u8(mask), exts[-1])).view(torch.bool) if mask.dtype == torch.bool else torch.cat((mask, exts[-1]))
        cat_tensors_to_optimizer(optimizer, ext)
        par = {g["name"]: g["params"][0] for g in optimizer.param_groups}
        P2 = P + n_new
        # --- the prune test on the new set (:787-794), the split parents leaving with it (:720-727)
        drop = torch.zeros(P2, dtype=torch.uint8, device=dev)
        drop[:P] = _u8(sel.split_sel)
        radii = None
        if screen_prune == "accumulated" and max_screen_size:
            radii = torch.zeros(P2, dtype=torch.float32, device=dev)
            radii[:P] = extra["max_radii2D"].reshape(-1)
        keep = prune_keep_mask(opacity_activation(par["opacity"].detach()).reshape(-1), scaling_activation(par["scaling"].detach()),
                               new_mask, min_opacity=min_opacity, max_screen_size=max_screen_size if max_screen_size else 0.0,
                               extent=extent if max_screen_size else float("inf"), max_radii2D=radii, drop=drop)
        # --- one compaction for parameters, moments and bookkeeping
        book = [new_mask]
        if extra.get("generation") is not None:
            gen = extra["generation"]
            fresh = torch.full((n_new,), 0 if generation_num is None else int(generation_num), dtype=gen.dtype, device=dev)
            book.append(torch.cat((gen, fresh)))
        result, book = _prune_optimizer_and(optimizer, keep, book)
        final = int(result["xyz"].shape[0])
        new_extra = dict(extra)
        new_extra["mask"] = book[0]
        if len(book) > 1:
            new_extra["generation"] = book[1]
        for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
            old = extra[k]
            new_extra[k] = torch.zeros((final,) + tuple(old.shape[1:]), dtype=old.dtype, device=dev)
    return result, new_extra, (P, n_clone, n_split, P2 - n_split - final)
