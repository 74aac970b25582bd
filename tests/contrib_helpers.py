"""Expected contribution statistics and pick buffers (include/gsr.h gsr_trace_contributions), from the CPU oracle alone.

The blending weight w = alpha T of a (Gaussian, pixel) pair comes EXACTLY from `oracle.cpu.blend_forward`: on background 0,
with a colour column that is 1 for one Gaussian and 0 for every other, the pixel's colour is a sum with one non-zero term,
(1 * alpha) * T -- w itself -- and three columns serve three Gaussians per call.  On top of those weights the definitions
are restated in numpy: integer sums of floor(w 2^32), the largest weight's bit pattern, the per-pixel argmax with the
front-most entry of the tile's list winning a tie, and its histogram.
"""
import numpy as np
import torch

from helpers import make_case

#: the exhaustive cases (make_case arguments): every Gaussian's weight image is computed
EXHAUSTIVE = {"six_tiles": (256, 40, 24, 3, 0.15), "ragged": (256, 33, 17, 4, 0.4), "one_tile": (200, 16, 16, 5, 0.3),
              "fifteen_tiles": (256, 70, 45, 6, 0.1)}
Q_ONE = float(1 << 32)
_cache = {}


def contrib_case(P, W, H, seed, s0, view=0):
    return make_case(P, W, H, seed=seed, s0=s0, view=view, sh_degree=0)


def oracle_state(O, case):
    """(geom, binning) of the view as apply_weights prepares it: no colours."""
    sc, cam = case["sc"], case["cam"]
    P = sc["xyz"].shape[0]
    geom = O.preprocess(sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], None, None, np.zeros((P, 3), np.float32),
                        cam.world_view_transform, cam.full_proj_transform, cam.camera_center, case["W"], case["H"],
                        case["tfx"], case["tfy"], 1.0, 0, False)
    return geom, O.bin_tiles(geom, case["W"], case["H"])


def oracle_weights(O, case, ids, state=None):
    """(len(ids), H*W) float32: w of Gaussian ids[k] at every pixel (0 where the pixel does not blend it), and the final
    transmittance (H*W) of the view -> (weights, final_T)."""
    geom, binning = state if state is not None else oracle_state(O, case)
    P, W, H = case["sc"]["xyz"].shape[0], case["W"], case["H"]
    ids = [int(i) for i in ids]
    out = np.zeros((len(ids), H * W), np.float32)
    final_T = None
    for k in range(0, len(ids), 3):
        cols = np.zeros((P, 3), np.float32)
        for c, g in enumerate(ids[k:k + 3]):
            cols[g, c] = 1.0
        f = O.blend_forward(geom, binning, cols, np.zeros(3, np.float32), W, H)
        n = len(ids[k:k + 3])
        out[k:k + n] = f["color"][:n].reshape(n, -1)
        final_T = f["final_T"]
    return out, final_T


def clamp_mask(mask):
    """m = min(max(x, 0), 1) with NaN -> 0, float32."""
    m = np.asarray(mask, np.float32).copy()
    m[~(m > 0)] = 0.0
    return np.minimum(m, np.float32(1.0))


def q(x):
    """q(x) = (uint32) trunc(x 2^32) of float32 values in [0, 1), as uint64 (the product by a power of two is exact)."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    return np.floor(x.astype(np.float64) * Q_ONE).astype(np.uint64)


def expected_rows(weights, masks=None):
    """The sum and max columns of the rows whose weight images are `weights` (n, H*W): int64 (n, 3 + C) with column 1
    (top_count) left 0.  masks: (C, H*W) or None."""
    n = weights.shape[0]
    C = 0 if masks is None else masks.shape[0]
    rows = np.zeros((n, 3 + C), np.int64)
    rows[:, 0] = q(weights).sum(axis=1).astype(np.int64)
    rows[:, 2] = weights.view(np.uint32).max(axis=1).astype(np.int64)  # (w >= 0: the patterns order as the floats)
    for c in range(C):
        m = clamp_mask(masks[c])
        rows[:, 3 + c] = q(weights * m[None, :]).sum(axis=1).astype(np.int64)  # one binary32 multiply per pair
    return rows


def expected_top(weights, ids, ranges, point_list, W, H):
    """Per pixel the largest weight among the Gaussians `ids` (rows of `weights`) and that Gaussian's index; equal weights:
    the front-most entry of the pixel's tile list wins -> (top_id (H*W) int32, top_weight (H*W) float32, tied pixels)."""
    ids = np.asarray(ids, np.int64)
    top_w = weights.max(axis=0)
    is_max = (weights == top_w[None, :]) & (weights > 0)
    tied = int((is_max.sum(axis=0) > 1).sum())
    gx = (W + 15) // 16
    pix = np.arange(H * W)
    tile = (pix // W // 16) * gx + (pix % W) // 16
    rank = np.full((ranges.shape[0], int(ids.max()) + 1 if ids.size else 1), np.iinfo(np.int64).max, np.int64)
    for t, (lo, hi) in enumerate(ranges):
        lst = point_list[int(lo):int(hi)].astype(np.int64)
        # (a Gaussian appears once per tile; first occurrence = its list position)
        keep = lst <= ids.max() if ids.size else lst < 0
        rank[t, lst[keep]] = np.nonzero(keep)[0]
    r = rank[tile[None, :], ids[:, None]]  # (n, H*W) list position of Gaussian k in the pixel's tile
    r = np.where(is_max, r, np.iinfo(np.int64).max)
    k = r.argmin(axis=0)
    top_id = np.where(top_w > 0, ids[k], -1).astype(np.int32)
    return top_id, top_w.astype(np.float32), tied


def exhaustive_expectation(O, name):
    """Everything of an exhaustive case, computed once and never modified: dict(case, weights (P, H*W), final_T, state,
    top_id, top_weight, tied, top_count)."""
    if name not in _cache:
        P, W, H, seed, s0 = EXHAUSTIVE[name]
        case = contrib_case(P, W, H, seed, s0)
        state = oracle_state(O, case)
        weights, final_T = oracle_weights(O, case, range(P), state)
        top_id, top_w, tied = expected_top(weights, np.arange(P), state[1]["ranges"], state[1]["point_list"], W, H)
        _cache[name] = dict(case=case, weights=weights, final_T=final_T, state=state, top_id=top_id, top_weight=top_w,
                            tied=tied, top_count=np.bincount(top_id[top_id >= 0], minlength=P).astype(np.int64))
    return _cache[name]


def expected_table(exp, masks=None):
    """The full int64 (P, 3 + C) table of one traced view of an exhaustive case."""
    rows = expected_rows(exp["weights"], masks)
    rows[:, 1] = exp["top_count"]
    return rows


def make_masks(H, W, C, seed=12):
    """(C,H,W) float32: channel 0 binary; further channels uniform in [-0.5, 1.5] with values below 0, above 1, exact zeros and
    exact ones."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(C, H, W, generator=g) * 2.0 - 0.5
    if C > 0:
        m[0] = (m[0] > 0.5).float()
    for c in range(1, C):
        flat = m[c].reshape(-1)
        flat[0::7] = 0.0
        flat[3::7] = 1.0
    return m.contiguous()


def merge_tables(a, b):
    """Column-wise add of two tables, max of column 2."""
    out = a + b
    out[:, 2] = np.maximum(a[:, 2], b[:, 2])
    return out
