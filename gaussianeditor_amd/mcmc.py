"""The 3DGS-MCMC strategy (Kheradmand et al. 2024, "3D Gaussian Splatting as Markov Chain Monte Carlo") on the GPU, beside
the ADC policy of `densify.py` (include/gsr.h: gsr_mcmc_*).

Three properties make it the other strategy an editor wants: a FIXED BUDGET of Gaussians (`cap_max`: an edited scene does
not grow with every prompt), RELOCATION of dead Gaussians onto live ones with a correction of opacity and scale that
preserves the render (floaters are recycled, not pruned and re-grown; no gradient threshold to tune), and opacity-gated
positional NOISE every step.

  * `inject_noise` -- every training step, after the optimizer step: `xyz += Sigma (noise * gate * scaler)` in place, ONE
    launch over the raw parameters (activations, covariance and product inside the kernel), no workspace, no host
    synchronisation.  The noise is the caller's `torch.randn`, so seeding stays with torch, as in `split_positions`.
  * `classify_and_sample` -- which rows are dead, and opacity-weighted draws among the alive ones, as INTEGER arithmetic
    (weights truncated to 23 bits, 64-bit prefix sums, one 128-bit product per draw): the same bits on every run, one
    readback.  The uniform numbers are the caller's `torch.rand`.
  * `relocation_values` -- the new raw opacity and scaling of every draw, in binary64, rounded once.
  * `relocate` -- dead rows become copies of their sources, both get the new values, the sources' Adam moments are zeroed;
    in place, one launch per role (copy, value, zero) for all tensors.
  * `add_new` -- growth: the appended rows are copies of their sources with the new values and zero moments
    (`cat_tensors_to_optimizer`).
  * `mcmc_refine` composes them: at most two host synchronisations (one record per sampling).

Every in-place writer moves the version counters of what it writes; a parameter that is a view of an
arena shares the arena's counter, so that one moves too.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Dict, NamedTuple, Optional, Tuple

import torch
from torch.autograd.graph import increment_version

from . import _native
from .densify import cat_tensors_to_optimizer

__all__ = ["inject_noise", "classify_and_sample", "relocation_values", "relocate", "add_new", "mcmc_refine", "McmcSample",
           "RATIO_CAP"]

#: a source drawn more often than this is treated as drawn this often (3DGS-MCMC's N_max)
RATIO_CAP = 51
_MASK = (torch.bool, torch.uint8)


def _check(what: str, name: str, t, ref: torch.Tensor, shape: Tuple[int, ...], dtypes=(torch.float32,)) -> None:
    """`t` against the tensor everything is compared with (`xyz` / `opacity`): device, dtype, shape, contiguity -- by name."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: {name} must live on the ROCm GPU; there is no CPU fallback")
    if t.device != ref.device:
        raise RuntimeError(f"{what}: {name} is on {t.device}, expected {ref.device}")
    if t.dtype not in dtypes:
        raise RuntimeError(f"{what}: {name} has dtype {t.dtype}, expected {' / '.join(str(d) for d in dtypes)}")
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be contiguous")


def _u8(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def inject_noise(xyz: torch.Tensor, scaling_raw: torch.Tensor, rotation_raw: torch.Tensor, opacity_raw: torch.Tensor,
                 noise: torch.Tensor, *, scaler: float, mask: Optional[torch.Tensor] = None, k: float = 100.0,
                 x0: float = 0.995) -> None:
    """The positional noise of one step (3DGS-MCMC's `inject_noise_to_position`), in place on `xyz` (P,3), one launch that
    never synchronises with the host.  `scaling_raw` (P,3), `rotation_raw` (P,4) and `opacity_raw` (P,1) or (P,) are the RAW
    parameters, `noise` (P,3) standard-normal numbers (`torch.randn` on the caller's generator), `scaler` the noise learning
    rate times the current position learning rate.  Per row, in binary64, rounded once at the store:

        o = sigmoid(opacity_raw); Sigma = R diag(exp(scaling_raw)^2) R^T, R of rotation_raw / |rotation_raw|
        gate = 1 / (1 + exp(k (o - (1 - x0))));  xyz += Sigma (noise * gate * scaler)

    Rows where `mask` (P, bool / uint8) is False are not written (the editor freezes them)."""
    what = "inject_noise"
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2:
        raise RuntimeError(f"{what}: xyz must be a (P, 3) tensor")
    P = int(xyz.shape[0])
    _check(what, "xyz", xyz, xyz, (P, 3))
    _check(what, "scaling_raw", scaling_raw, xyz, (P, 3))
    _check(what, "rotation_raw", rotation_raw, xyz, (P, 4))
    _check(what, "opacity_raw", opacity_raw, xyz, (P, 1) if isinstance(opacity_raw, torch.Tensor) and opacity_raw.dim() == 2 else (P,))
    _check(what, "noise", noise, xyz, (P, 3))
    if mask is not None:
        _check(what, "mask", mask, xyz, (P,), _MASK)
    if P == 0:
        return
    dev = xyz.device
    rot = rotation_raw.detach()
    if rot.data_ptr() % 16:  # (a view at an odd offset: the kernel reads a quaternion as one 16-byte vector)
        rot = rot.clone()
    L = _native.lib()
    increment_version(xyz)  # written through its raw pointer: what `+=` does by itself
    with torch.cuda.device(dev):
        _native.check("gsr_mcmc_noise", L.gsr_mcmc_noise(
            _stream(dev), P, xyz.data_ptr(), scaling_raw.data_ptr(), rot.data_ptr(), opacity_raw.data_ptr(), noise.data_ptr(),
            None if mask is None else _u8(mask).data_ptr(), float(k), float(x0), float(scaler)))


class McmcSample(NamedTuple):
    """What `classify_and_sample` decided and drew."""
    dead_sel: torch.Tensor   # (P,) bool
    dead_idx: torch.Tensor   # (P,) int32: its first n_dead entries are the dead rows, ascending; the rest is unspecified
    src: torch.Tensor        # (n,) int32: the source row of every draw; -1 for r >= n_draws and when total == 0
    count: torch.Tensor      # (P,) int32: draws of every row
    ratio: torch.Tensor      # (n,) int32: min(count[src] + 1, RATIO_CAP); 0 where src == -1
    n_dead: int
    n_alive: int
    n_draws: int
    total: int               # the sum of the integer weights; 0 with draws requested means nothing could be drawn


def classify_and_sample(opacity: torch.Tensor, u: torch.Tensor, *, min_opacity: float = 0.005,
                        mask: Optional[torch.Tensor] = None, n_draws: Optional[int] = None) -> McmcSample:
    """Dead / alive and the draws, one readback.  `opacity` (P,) is ACTIVATED; a row inside `mask` is dead when
    `opacity <= float32(min_opacity)`, alive otherwise (a NaN is neither).  An alive row weighs `k = trunc(opacity * 2**23)`;
    draw r takes `u[r]` in [0, 1) (`torch.rand`), `t = (trunc(u * 2**24) * total) >> 24`, and returns the smallest row whose
    inclusive prefix sum exceeds t.  `n_draws=None` draws once per dead row (relocation; `u` must then hold at least as many
    numbers as there can be dead rows, P is always enough), otherwise `n_draws <= len(u)` times."""
    what = "classify_and_sample"
    if not isinstance(opacity, torch.Tensor) or opacity.dim() != 1:
        raise RuntimeError(f"{what}: opacity must be a (P,) tensor of activated opacities")
    P = int(opacity.numel())
    _check(what, "opacity", opacity, opacity, (P,))
    if not isinstance(u, torch.Tensor) or u.dim() != 1:
        raise RuntimeError(f"{what}: u must be a 1-D tensor of uniform numbers")
    _check(what, "u", u, opacity, (int(u.numel()),))
    if mask is not None:
        _check(what, "mask", mask, opacity, (P,), _MASK)
    n = int(u.numel()) if n_draws is None else int(n_draws)
    if n < 0 or n > int(u.numel()):
        raise ValueError(f"{what}: n_draws must be 0 .. len(u)")
    dev = opacity.device
    dead_sel = torch.zeros(P, dtype=torch.bool, device=dev)
    dead_idx = torch.empty(P, dtype=torch.int32, device=dev)
    src = torch.full((n,), -1, dtype=torch.int32, device=dev)
    count = torch.zeros(P, dtype=torch.int32, device=dev)
    ratio = torch.zeros(n, dtype=torch.int32, device=dev)
    if P == 0:
        return McmcSample(dead_sel, dead_idx, src, count, ratio, 0, 0, 0, 0)
    L = _native.lib()
    nbytes = ctypes.c_size_t(0)
    _native.check("gsr_mcmc_workspace_size", L.gsr_mcmc_workspace_size(P, ctypes.byref(nbytes)))
    work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    rec = _native.McmcRecord()
    with torch.cuda.device(dev):
        _native.check("gsr_mcmc_sample", L.gsr_mcmc_sample(
            _stream(dev), P, n, opacity.detach().data_ptr(), None if mask is None else _u8(mask).data_ptr(), float(min_opacity),
            u.data_ptr(), 1 if n_draws is None else 0, work.data_ptr(), dead_sel.data_ptr(), dead_idx.data_ptr(),
            src.data_ptr(), count.data_ptr(), ratio.data_ptr(), ctypes.byref(rec)))
    return McmcSample(dead_sel, dead_idx, src, count, ratio, int(rec.n_dead), int(rec.n_alive), int(rec.n_draws), int(rec.total))


def relocation_values(opacity: torch.Tensor, scaling_raw: torch.Tensor, src: torch.Tensor, ratio: torch.Tensor, *,
                      min_opacity: float = 0.005) -> Tuple[torch.Tensor, torch.Tensor]:
    """(new raw opacity (n,1), new raw scaling (n,3)) of every draw: with source s = src[r], N = ratio[r],

        o = min(opacity[s], 1 - 2**-24);  o' = 1 - (1 - o)**(1/N)
        denom = sum_{i=1..N} sum_{k=0..i-1} C(i-1,k) (-1)**k o'**(k+1) / sqrt(k+1);  scale' = exp(scaling_raw[s]) o / denom
        o' clamped to [min_opacity, 1 - 2**-23];  stored: log(o' / (1 - o')), log(scale')

    in binary64 from the float32 inputs, rounded at the store.  `opacity` (P,) is ACTIVATED and `scaling_raw` (P,3) RAW, both
    the values from BEFORE any row is written: the results go to draw-indexed tensors, so a source drawn several times gives
    every one of its draws the same numbers.  Rows of a draw with src == -1 are zero."""
    what = "relocation_values"
    if not isinstance(opacity, torch.Tensor) or opacity.dim() != 1:
        raise RuntimeError(f"{what}: opacity must be a (P,) tensor of activated opacities")
    P = int(opacity.numel())
    _check(what, "opacity", opacity, opacity, (P,))
    _check(what, "scaling_raw", scaling_raw, opacity, (P, 3))
    if not isinstance(src, torch.Tensor) or src.dim() != 1:
        raise RuntimeError(f"{what}: src must be a 1-D int32 tensor")
    n = int(src.numel())
    _check(what, "src", src, opacity, (n,), (torch.int32,))
    _check(what, "ratio", ratio, opacity, (n,), (torch.int32,))
    dev = opacity.device
    new_opacity = torch.zeros((n, 1), dtype=torch.float32, device=dev)
    new_scaling = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    if P == 0 or n == 0:
        return new_opacity, new_scaling
    L = _native.lib()
    with torch.cuda.device(dev):
        _native.check("gsr_mcmc_relocation_values", L.gsr_mcmc_relocation_values(
            _stream(dev), P, n, src.data_ptr(), ratio.data_ptr(), opacity.detach().data_ptr(), scaling_raw.detach().data_ptr(),
            float(min_opacity), new_opacity.data_ptr(), new_scaling.data_ptr()))
    return new_opacity, new_scaling


def _groups(what: str, optimizer: torch.optim.Optimizer):
    """[(name, parameter, exp_avg | None, exp_avg_sq | None)] of an optimizer with one parameter per named group."""
    out = []
    names = set()
    for group in optimizer.param_groups:
        assert len(group["params"]) == 1
        p = group["params"][0]
        st = optimizer.state.get(p, None)
        has = st is not None and "exp_avg" in st
        out.append((group["name"], p, st["exp_avg"] if has else None, st["exp_avg_sq"] if has else None))
        names.add(group["name"])
    for k in ("xyz", "opacity", "scaling"):
        if k not in names:
            raise RuntimeError(f"{what}: the optimizer has no parameter group named {k!r}")
    return out


def _row_bytes(what: str, name: str, t: torch.Tensor, xyz: torch.Tensor) -> int:
    P = int(xyz.shape[0])
    if not t.is_cuda or t.device != xyz.device:
        raise RuntimeError(f"{what}: {name} is on {t.device}, expected {xyz.device}; there is no CPU fallback")
    if t.dim() < 1 or int(t.shape[0]) != P:
        raise RuntimeError(f"{what}: {name} has shape {tuple(t.shape)}, expected {P} rows as xyz")
    if not t.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be contiguous (it is written in place)")
    rb = t.element_size() * (t.numel() // P) if P else 4
    if rb == 0 or rb % 4 or t.data_ptr() % 4:
        raise RuntimeError(f"{what}: {name} needs rows of a multiple of 4 bytes, 4-byte aligned")
    return rb


def _scatter(what: str, P: int, n: int, src: torch.Tensor, dst_idx: Optional[torch.Tensor], dst_rows: int, entries) -> None:
    """One gsr_mcmc_scatter (a launch per role) per 32 entries (base, dst | None, values | None, row_bytes, role)."""
    L = _native.lib()
    dev = src.device
    with torch.cuda.device(dev):
        for lo in range(0, len(entries), 32):
            chunk = entries[lo:lo + 32]
            arr = (_native.McmcTensor * len(chunk))()
            for i, (base, dst, values, rb, role) in enumerate(chunk):
                arr[i] = _native.McmcTensor(base.data_ptr(), None if dst is None else dst.data_ptr(),
                                            None if values is None else values.data_ptr(), rb, role)
            _native.check("gsr_mcmc_scatter", L.gsr_mcmc_scatter(_stream(dev), P, n, src.data_ptr(),
                                                                 None if dst_idx is None else dst_idx.data_ptr(), dst_rows,
                                                                 len(chunk), arr))


def _check_draws(what: str, xyz: torch.Tensor, src, new_opacity_raw, new_scaling_raw) -> int:
    if not isinstance(src, torch.Tensor) or src.dim() != 1:
        raise RuntimeError(f"{what}: src must be a 1-D int32 tensor")
    n = int(src.numel())
    _check(what, "src", src, xyz, (n,), (torch.int32,))
    _check(what, "new_opacity_raw", new_opacity_raw, xyz, (n, 1))
    _check(what, "new_scaling_raw", new_scaling_raw, xyz, (n, 3))
    return n


def relocate(optimizer: torch.optim.Optimizer, dead_idx: torch.Tensor, src: torch.Tensor, new_opacity_raw: torch.Tensor,
             new_scaling_raw: torch.Tensor) -> None:
    """3DGS-MCMC's `relocate_gs`, in place, three launches: for every draw r the dead row `dead_idx[r]` of every parameter
    becomes a copy of the source row `src[r]`; the opacity and the scaling of BOTH rows become `new_opacity_raw[r]` /
    `new_scaling_raw[r]` (`relocation_values`, computed from the old values before this call); `exp_avg` / `exp_avg_sq` of
    all groups are zeroed on the SOURCE rows, the dead rows' moments stay.  `dead_idx`, `src` (n,) int32 as
    `classify_and_sample` returns them (cut to the n draws): no source is a dead row."""
    what = "relocate"
    groups = _groups(what, optimizer)
    xyz = dict((g[0], g[1]) for g in groups)["xyz"]
    P = int(xyz.shape[0])
    n = _check_draws(what, xyz, src, new_opacity_raw, new_scaling_raw)
    _check(what, "dead_idx", dead_idx, xyz, (n,), (torch.int32,))
    if P == 0 or n == 0:
        return
    entries, written = [], []
    for name, p, m1, m2 in groups:
        d = p.detach()
        rb = _row_bytes(what, name, d, xyz)
        if name == "opacity":
            if rb != 4:
                raise RuntimeError(f"{what}: opacity has shape {tuple(p.shape)}, expected ({P}, 1)")
            entries.append((d, d, new_opacity_raw, rb, _native.MCMC_VALUE))
        elif name == "scaling":
            if rb != 12:
                raise RuntimeError(f"{what}: scaling has shape {tuple(p.shape)}, expected ({P}, 3)")
            entries.append((d, d, new_scaling_raw, rb, _native.MCMC_VALUE))
        else:
            entries.append((d, d, None, rb, _native.MCMC_COPY))
        written.append(p)
        for m, tag in ((m1, "exp_avg"), (m2, "exp_avg_sq")):
            if m is not None:
                entries.append((m, None, None, _row_bytes(what, f"{name}.{tag}", m, xyz), _native.MCMC_ZERO))
                written.append(m)
    increment_version(written)  # parameters and moments are written through raw pointers
    _scatter(what, P, n, src, dead_idx, P, entries)


def add_new(optimizer: torch.optim.Optimizer, extra: Dict[str, torch.Tensor], src: torch.Tensor, new_opacity_raw: torch.Tensor,
            new_scaling_raw: torch.Tensor, *, mask: Optional[torch.Tensor] = None, generation_num: Optional[int] = None):
    """3DGS-MCMC's `add_new_gs` after the draws: the sources get the new raw opacity and scaling in place (their moments are
    kept), and `len(src)` rows are appended through `cat_tensors_to_optimizer`: copies of their sources with those values
    and zero moments.  Of `extra`, `mask` (or the `mask` given) is extended by the sources' mask, `generation` by
    `generation_num` (0 when None), every other tensor with P rows by zeros.  Every src must be a row (total > 0).
    Returns ({name: new parameter}, new extra)."""
    what = "add_new"
    groups = _groups(what, optimizer)
    xyz = dict((g[0], g[1]) for g in groups)["xyz"]
    P = int(xyz.shape[0])
    dev = xyz.device
    n = _check_draws(what, xyz, src, new_opacity_raw, new_scaling_raw)
    if mask is None:
        mask = extra.get("mask")
    if mask is not None:
        _check(what, "mask", mask, xyz, (P,), _MASK)
    ext: Dict[str, torch.Tensor] = {}
    entries, written = [], []
    for name, p, _, _ in groups:
        d = p.detach()
        rb = _row_bytes(what, name, d, xyz)
        e = torch.empty((n,) + tuple(d.shape[1:]), dtype=d.dtype, device=dev)
        ext[name] = e
        if name in ("opacity", "scaling"):
            if rb != (4 if name == "opacity" else 12):
                raise RuntimeError(f"{what}: {name} has shape {tuple(p.shape)}, expected ({P}, {1 if name == 'opacity' else 3})")
            entries.append((d, e, new_opacity_raw if name == "opacity" else new_scaling_raw, rb, _native.MCMC_VALUE))
            written.append(p)
        else:
            entries.append((d, e, None, rb, _native.MCMC_COPY))
    new_extra = dict(extra)
    if P > 0 and n > 0:
        increment_version(written)  # the sources' opacity and scaling are written through raw pointers
        _scatter(what, P, n, src, None, n, entries)
    rows = src.long()
    for key, t in extra.items():
        if not isinstance(t, torch.Tensor) or t.dim() < 1 or int(t.shape[0]) != P:
            continue
        if key == "mask":
            new_extra[key] = torch.cat((t, t[rows]))
        elif key == "generation":
            fresh = torch.full((n,) + tuple(t.shape[1:]), 0 if generation_num is None else int(generation_num), dtype=t.dtype, device=dev)
            new_extra[key] = torch.cat((t, fresh))
        else:
            new_extra[key] = torch.cat((t, torch.zeros((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)))
    if "mask" not in extra and mask is not None:
        new_extra["mask"] = torch.cat((mask, mask[rows]))
    params = cat_tensors_to_optimizer(optimizer, ext)
    return params, new_extra


def mcmc_refine(optimizer: torch.optim.Optimizer, extra: Dict[str, torch.Tensor], *, cap_max: int, min_opacity: float = 0.005,
                grow: float = 1.05, mask: Optional[torch.Tensor] = None, generation_num: Optional[int] = None,
                generator: Optional[torch.Generator] = None):
    """One refine of 3DGS-MCMC's strategy (`MCMCStrategy.step_post_backward` at a refine step) on an optimizer with the
    reference's six named groups (xyz, f_dc, f_rest, opacity, scaling, rotation) and the bookkeeping tensors `extra`, as
    `densify_and_prune` takes them:

      1. relocation: `u = torch.rand(P, generator=generator)`; every dead row inside the mask (`mask`, else
         `extra["mask"]`, else all rows) is relocated onto a source drawn among the alive ones (`relocate`);
      2. growth: `n_new = max(0, min(cap_max, int(grow * P)) - P)`; `u = torch.rand(n_new, generator=generator)` draws the
         sources among the alive rows of the state AFTER relocation (`add_new`).  P never exceeds `cap_max`.

    New rows inherit their source's mask, get `generation_num` in `extra["generation"]`, and zeros in the statistics.  At
    most two host synchronisations: the record of each sampling.  Nothing happens where nothing can be drawn (no alive row).
    Returns ({name: parameter}, new extra, (P before, n_dead, n_relocated, n_added))."""
    what = "mcmc_refine"
    groups = _groups(what, optimizer)
    par = {g[0]: g[1] for g in groups}
    xyz = par["xyz"]
    P = int(xyz.shape[0])
    if not xyz.is_cuda:
        raise RuntimeError(f"{what}: the parameters must live on the ROCm GPU; there is no CPU fallback")
    dev = xyz.device
    if mask is None:
        mask = extra.get("mask")
    _check(what, "opacity", par["opacity"], xyz, (P, 1))
    _check(what, "scaling", par["scaling"], xyz, (P, 3))
    n_dead = n_relocated = n_added = 0
    new_extra = dict(extra)
    with torch.no_grad():
        if P > 0:
            opacity = torch.sigmoid(par["opacity"].detach()).reshape(-1)
            u = torch.rand(P, dtype=torch.float32, device=dev, generator=generator)
            smp = classify_and_sample(opacity, u, min_opacity=min_opacity, mask=mask)
            n_dead = smp.n_dead
            if smp.n_draws > 0 and smp.total > 0:
                n_relocated = smp.n_draws
                src, ratio = smp.src[:n_relocated], smp.ratio[:n_relocated]
                new_o, new_s = relocation_values(opacity, par["scaling"].detach(), src, ratio, min_opacity=min_opacity)
                relocate(optimizer, smp.dead_idx[:n_relocated], src, new_o, new_s)
        n_new = max(0, min(int(cap_max), int(grow * P)) - P)
        if n_new > 0 and P > 0:
            opacity = torch.sigmoid(par["opacity"].detach()).reshape(-1)
            u = torch.rand(n_new, dtype=torch.float32, device=dev, generator=generator)
            smp = classify_and_sample(opacity, u, min_opacity=min_opacity, mask=mask, n_draws=n_new)
            if smp.total > 0:
                new_o, new_s = relocation_values(opacity, par["scaling"].detach(), smp.src, smp.ratio, min_opacity=min_opacity)
                result, new_extra = add_new(optimizer, extra, smp.src, new_o, new_s, mask=mask, generation_num=generation_num)
                n_added = n_new
    result = {g["name"]: g["params"][0] for g in optimizer.param_groups}
    return result, new_extra, (P, n_dead, n_relocated, n_added)
