"""Per-Gaussian contribution statistics and the per-pixel pick buffer.

`GaussianModel.apply_weights` (the reference's semantic tracing, K12) gives every Gaussian a pixel blends the same vote:
`weights[i] += mask`, `cnt[i] += 1` -- a haze Gaussian of blending weight 0.004 in front of a surface counts like the
surface Gaussian of weight 0.9 behind it.  `trace_view` keeps the blending weight w = alpha T the forward composites with
(gsr_trace_contributions, include/gsr.h), which gives

* contribution-weighted lifting of 2D masks to 3D, sum w mask / sum w per Gaussian (`ContributionStats.label`), the label of
  SAGA, FlashSplat and Gaussian Grouping;
* contribution-based pruning scores, max over rays of w and sum of w (`ContributionStats.low_contribution`), as in RadSplat
  and LightGaussian;
* picking: the Gaussian under every pixel (`return_pixels=True`).

The table is accumulated in integers (units of 2^-32): the same bits on every run, on every launch grid and in every order
of the views, and two ranks' tables merge exactly (`ContributionStats.merge`).  Nothing here is differentiable.
"""
from __future__ import annotations

import torch

__all__ = ["ContributionStats", "trace_view", "patch_gaussian_model", "Q_ONE"]

#: one unit of blending weight in the sum columns of the table: q(w) = trunc(w * 2^32)
Q_ONE = float(1 << 32)
#: columns of the table in front of the per-channel sums (include/gsr.h: total_q, top_count, max_bits)
_TOTAL, _TOP, _MAX, _FIRST_CHANNEL = 0, 1, 2, 3


class ContributionStats:
    """The int64 (P, 3 + channels) table `trace_view` accumulates into, and the number of views traced so far.

    `total` (P) float64: the sum over all traced pixels of the Gaussian's blending weight; `weighted` (P, channels) float64:
    the same sum with every weight multiplied by the pixel's mask value (clamped to [0, 1]); `max_weight` (P) float32: the
    largest weight the Gaussian reached in any pixel; `top_count` (P) int64: pixels in which it was the top contributor."""

    def __init__(self, P: int, channels: int = 0, device="cuda"):
        if not 0 <= int(channels) <= 3:
            raise ValueError("ContributionStats: channels must be 0, 1, 2 or 3")
        if int(P) < 0:
            raise ValueError("ContributionStats: P must be >= 0")
        self.channels = int(channels)
        self.table = torch.zeros((int(P), _FIRST_CHANNEL + self.channels), dtype=torch.int64, device=device)
        self.views = 0

    def __len__(self) -> int:
        return int(self.table.size(0))

    @property
    def device(self) -> torch.device:
        return self.table.device

    @property
    def total(self) -> torch.Tensor:
        return self.table[:, _TOTAL].to(torch.float64) / Q_ONE

    @property
    def weighted(self) -> torch.Tensor:
        return self.table[:, _FIRST_CHANNEL:].to(torch.float64) / Q_ONE

    @property
    def max_weight(self) -> torch.Tensor:
        # (the column holds binary32 bit patterns, zero-extended: below 2^31 for weights <= 0.99)
        return self.table[:, _MAX].to(torch.int32).view(torch.float32)

    @property
    def top_count(self) -> torch.Tensor:
        return self.table[:, _TOP].clone()

    @torch.no_grad()
    def label(self, eps: float = 1e-7) -> torch.Tensor:
        """(P, channels) float64 in [0, 1]: weighted / (total + eps), the contribution-weighted counterpart of
        `weights / (cnt + 1e-7)` of the reference's update_mask."""
        return self.weighted / (self.total + eps).unsqueeze(1)

    @torch.no_grad()
    def select(self, thres: float, eps: float = 1e-7) -> torch.Tensor:
        """(P) bool: the Gaussians whose label of channel 0 exceeds `thres` (the reference's `weights > thres` selection)."""
        if self.channels < 1:
            raise RuntimeError("ContributionStats.select needs a table with at least one mask channel")
        return self.label(eps)[:, 0] > thres

    @torch.no_grad()
    def low_contribution(self, max_weight_below: float = 1.0 / 255.0, total_below=None) -> torch.Tensor:
        """(P) bool prune mask: Gaussians whose largest weight over all traced rays is below `max_weight_below` (default
        1/255, the alpha below which the rasterizer itself skips an entry; the Gaussians no pixel blended are always among
        them) or, with `total_below`, whose summed weight is below that."""
        low = self.max_weight < max_weight_below
        if total_below is not None:
            low = low | (self.total < total_below)
        return low

    def reset(self) -> None:
        self.table.zero_()
        self.views = 0

    @torch.no_grad()
    def merge(self, other: "ContributionStats") -> "ContributionStats":
        """Adds the table of `other` (a rank that traced different views of the same Gaussians): the sum columns and the
        count add, the largest weight is the larger of the two.  Exact, and independent of the order of the merges."""
        if other.table.shape != self.table.shape:
            raise ValueError(f"ContributionStats.merge: tables of {tuple(self.table.shape)} and {tuple(other.table.shape)}")
        o = other.table.to(self.table.device)
        mx = torch.maximum(self.table[:, _MAX], o[:, _MAX])
        self.table += o
        self.table[:, _MAX] = mx
        self.views += other.views
        return self


@torch.no_grad()
def trace_view(viewpoint_camera, pc, stats: ContributionStats, mask=None, scaling_modifier: float = 1.0,
               return_pixels: bool = False):
    """Traces one view into `stats`, as GaussianModel.apply_weights traces one into `weights` and `cnt`
    (scene/gaussian_model.py:817-832): `camera2rasterizer` with a black background, `pc.get_xyz`, `get_opacity`,
    `get_scaling`, `get_rotation`.  `mask`: None for a table without channels, else (H,W) or (channels,H,W), any dtype;
    values are clamped to [0, 1].  -> (top_id (H,W) int32, top_weight (H,W) float32) with `return_pixels`, else None."""
    from .gaussian_renderer import _settings
    from .diff_gaussian_rasterization import GaussianRasterizer

    xyz = pc.get_xyz
    dev = xyz.device
    if len(stats) != int(xyz.shape[0]):
        raise ValueError(f"trace_view: the table has {len(stats)} rows, the model {int(xyz.shape[0])} Gaussians")
    if (mask is None) != (stats.channels == 0):
        raise ValueError(f"trace_view: a table of {stats.channels} channels needs "
                         + ("no mask" if stats.channels == 0 else f"a mask of {stats.channels} channels"))
    if mask is not None:
        mask = torch.as_tensor(mask, device=dev).to(torch.float32)
        if mask.dim() == 2:
            mask = mask.unsqueeze(0)
        if mask.dim() != 3 or int(mask.size(0)) != stats.channels:
            raise ValueError(f"trace_view: the mask must be (H,W) or ({stats.channels},H,W), got {tuple(mask.shape)}")
    bg = torch.zeros(3, dtype=torch.float32, device=dev)
    rasterizer = GaussianRasterizer(raster_settings=_settings(viewpoint_camera, bg, scaling_modifier, 0))
    out = rasterizer.trace_contributions(xyz.float(), pc.get_opacity.float(), scales=pc.get_scaling.float(),
                                         rotations=pc.get_rotation.float(), stats=stats.table, image_weights=mask,
                                         return_pixels=return_pixels)
    stats.views += 1
    return out


def patch_gaussian_model(cls) -> None:
    """Bind `trace_view` as `cls.apply_contributions(camera, stats, mask=None, ...)` (cls: the reference's GaussianModel),
    beside its `apply_weights`; INTEGRATION.md."""

    def _method(self, camera, stats, mask=None, scaling_modifier: float = 1.0, return_pixels: bool = False):
        return trace_view(camera, self, stats, mask, scaling_modifier, return_pixels)

    cls.apply_contributions = _method
