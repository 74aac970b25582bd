"""What the bilateral-grid tests share (tests/test_cpu_bilagrid.py, tests/test_gpu_bilagrid.py): the mathematics of the
gsr_bilagrid_* entry points (include/gsr.h) restated twice, and the seeded cases.

  * slice_torch: torch.nn.functional.grid_sample (align_corners=True, border padding) on the CPU with autograd, in the dtype
    of its inputs.  In float64 it is the yardstick; run in float32 its error against float64 sets the bar (`bar`).
  * slice_numpy: an explicit eight-corner loop in float64 numpy, forward and both gradients written out.
  * tv_torch: gsplat's total_variation_loss, the formula as written.
  * make_case / CASES: images in [-0.2, 1.3] whose luminance is spread over that whole range (both clamps of `gray` are
    active on well over 5 % of the pixels), grids = identity + 0.3 randn, dL/dout = randn / pixels.  The guidance term of
    dL/dimage jumps where gz crosses an integer and where gray crosses 0 or 1, so the generator redraws every pixel whose
    float64 gz lies within MARGIN of an integer or whose gray lies within MARGIN of 0 or 1 (`margin_violations` counts them:
    0 in every case, asserted on the CPU): a condition on the inputs, not a tolerance.
"""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 1e-4
LUMA = (0.299, 0.587, 0.114)
N_GRIDS = 3

#: name -> image shape
IMAGES = {"5x7": (3, 5, 7), "45x70": (3, 45, 70), "33x130": (3, 33, 130), "64x64": (3, 64, 64), "batch": (2, 3, 45, 70)}
#: name -> (GX, GY, GZ); 3 x 5 x 4 tells a transposition of the axes
GRIDS = {"g2": (2, 2, 2), "g354": (3, 5, 4), "g16": (16, 16, 8), "g32": (32, 32, 16)}
#: idx per image name: a Python int for single images, the two tensors for the batch
INDICES = {"5x7": (2,), "45x70": (2,), "33x130": (2,), "64x64": (2,), "batch": ([0, 2], [1, 1])}


def _cases():
    out = {}
    for (iname, shape), (gname, grid) in itertools.product(IMAGES.items(), GRIDS.items()):
        for idx in INDICES[iname]:
            tag = "" if isinstance(idx, int) else "_i" + "".join(str(i) for i in idx)
            out[f"{iname}_{gname}{tag}"] = (shape, grid, idx)
    return out


CASE_SPECS = _cases()
CASES = list(CASE_SPECS)


def gray64(image):
    """float64 luminance of a float32 / float64 numpy image (..., 3, H, W)"""
    im = np.asarray(image, dtype=np.float64)
    return LUMA[0] * im[..., 0, :, :] + LUMA[1] * im[..., 1, :, :] + LUMA[2] * im[..., 2, :, :]


def margin_violations(image, GZ):
    """pixels whose gz = clamp(gray, 0, 1) (GZ - 1) lies within MARGIN of an integer, or whose gray lies within MARGIN of 0 or 1"""
    gray = gray64(image)
    gz = np.clip(gray, 0.0, 1.0) * (GZ - 1)
    inside = (gray > 0.0) & (gray < 1.0)
    near_face = inside & (np.abs(gz - np.round(gz)) < MARGIN)
    near_clamp = (np.abs(gray) < MARGIN) | (np.abs(gray - 1.0) < MARGIN)
    return near_face | near_clamp


def _draw_image(rng, shape):
    """float32 pixels in [-0.2, 1.3]: a luminance uniform over the range plus a little colour"""
    lum = rng.uniform(-0.2, 1.3, size=shape[:-3] + (1,) + shape[-2:])
    return np.clip(lum + rng.uniform(-0.1, 0.1, size=shape), -0.2, 1.3).astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """dict(grids (3,12,GZ,GY,GX) f32, image f32, idx (int | list), dout f32 like image): numpy, seeded by the name"""
    shape, (GX, GY, GZ), idx = CASE_SPECS[name]
    rng = np.random.default_rng(1000 + CASES.index(name))
    eye = np.eye(3, 4).reshape(1, 12, 1, 1, 1)
    grids = (eye + 0.3 * rng.standard_normal((N_GRIDS, 12, GZ, GY, GX))).astype(np.float32)
    image = _draw_image(rng, shape)
    for _ in range(100):
        bad = margin_violations(image, GZ)
        if not bad.any():
            break
        fresh = _draw_image(rng, shape)
        image = np.where(np.expand_dims(bad, -3), fresh, image)
    else:
        raise AssertionError(f"{name}: the redraw did not converge")
    pixels = shape[-1] * shape[-2] * (shape[0] if len(shape) == 4 else 1)
    dout = (rng.standard_normal(shape) / pixels).astype(np.float32)
    for a in (grids, image, dout):
        a.setflags(write=False)
    return dict(grids=grids, image=image, idx=idx, dout=dout, grid=(GX, GY, GZ))


def index_list(idx, B):
    return [int(idx)] * B if isinstance(idx, int) else [int(i) for i in idx]


# ---- restatement one: grid_sample ------------------------------------------------------------------------------------
def affine_field(grids, image, idx, detach_guidance=False):
    """A (B,12,H,W): the grids sliced at (x, y, luminance) with grid_sample.  grids (N,12,GZ,GY,GX), image (B,3,H,W), one
    dtype, CPU; idx: list of B ints.  detach_guidance: no gradient flows through the luminance coordinate."""
    B, _, H, W = image.shape
    dt = image.dtype
    u = (torch.arange(W, dtype=dt) + 0.5) / W
    v = (torch.arange(H, dtype=dt) + 0.5) / H
    gray = LUMA[0] * image[:, 0] + LUMA[1] * image[:, 1] + LUMA[2] * image[:, 2]
    gray = torch.clamp(gray, 0.0, 1.0)
    if detach_guidance:
        gray = gray.detach()
    xy = torch.stack(torch.meshgrid(v, u, indexing="ij")[::-1], dim=-1)  # (H,W,2): (u, v)
    coords = torch.cat([xy.expand(B, H, W, 2), gray[..., None]], dim=-1) * 2.0 - 1.0  # normalised (x, y, z)
    field = F.grid_sample(grids[idx], coords[:, None], mode="bilinear", padding_mode="border", align_corners=True)
    return field[:, :, 0]


def slice_torch(grids, image, idx, detach_guidance=False):
    """out (B,3,H,W) = A [rgb; 1]"""
    A = affine_field(grids, image, idx, detach_guidance)
    B, _, H, W = image.shape
    A = A.reshape(B, 3, 4, H, W)
    return (A[:, :, :3] * image[:, None]).sum(2) + A[:, :, 3]


def tv_torch(grids):
    """gsplat's total_variation_loss: the mean over the grids of the three mean squared forward differences"""
    N = grids.shape[0]
    dz = grids[:, :, 1:] - grids[:, :, :-1]
    dy = grids[:, :, :, 1:] - grids[:, :, :, :-1]
    dx = grids[..., 1:] - grids[..., :-1]
    per_grid = lambda d: d.numel() // N  # noqa: E731  (count_d: the differenced elements of ONE grid)
    return ((dz ** 2).sum() / per_grid(dz) + (dy ** 2).sum() / per_grid(dy) + (dx ** 2).sum() / per_grid(dx)) / N


def run_torch(case, dtype):
    """dict(out, d_image, d_grids, d_image_direct) as float64 numpy, evaluated in `dtype` with slice_torch and autograd"""
    c = make_case(case) if isinstance(case, str) else case
    image = torch.tensor(c["image"]).to(dtype)
    batched = image.ndimension() == 4
    image = (image if batched else image[None]).clone().requires_grad_(True)
    grids = torch.tensor(c["grids"]).to(dtype).requires_grad_(True)
    dout = torch.tensor(c["dout"]).to(dtype).reshape(image.shape)
    idx = index_list(c["idx"], image.shape[0])
    out = slice_torch(grids, image, idx)
    d_grids, d_image = torch.autograd.grad(out, (grids, image), dout)
    direct, = torch.autograd.grad(slice_torch(grids.detach(), image, idx, detach_guidance=True), image, dout)
    shape = c["image"].shape
    f = lambda t: t.detach().double().numpy()  # noqa: E731
    return dict(out=f(out).reshape(shape), d_image=f(d_image).reshape(shape), d_grids=f(d_grids),
                d_image_direct=f(direct).reshape(shape))


@functools.lru_cache(maxsize=None)
def expectation(case):
    """the float64 results of a named case, with d_image_guidance = d_image - d_image_direct"""
    e = run_torch(case, torch.float64)
    e["d_image_guidance"] = e["d_image"] - e["d_image_direct"]
    return e


@functools.lru_cache(maxsize=None)
def bar(case):
    """per quantity: max(2 x the error of the float32 run of slice_torch against float64, 1e-6 of the largest entry)"""
    e, s = expectation(case), run_torch(case, torch.float32)
    return {k: max(2.0 * float(np.abs(s[k] - e[k]).max()), 1e-6 * float(np.abs(e[k]).max())) for k in ("out", "d_image", "d_grids")}


@functools.lru_cache(maxsize=None)
def tv_case(N, grid):
    GX, GY, GZ = grid
    rng = np.random.default_rng(7 + N + 10 * GX + 100 * GY + 1000 * GZ)
    g = (np.eye(3, 4).reshape(1, 12, 1, 1, 1) + 0.3 * rng.standard_normal((N, 12, GZ, GY, GX))).astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def tv_expectation(N, grid):
    """(tv, gradient) in float64, and the bar of each from the float32 run of tv_torch"""
    res = {}
    for dt in (torch.float64, torch.float32):
        g = torch.tensor(tv_case(N, grid)).to(dt).requires_grad_(True)
        tv = tv_torch(g)
        grad, = torch.autograd.grad(tv, g)
        res[dt] = (float(tv.detach().double()), grad.double().numpy())
    (tv, grad), (tv32, grad32) = res[torch.float64], res[torch.float32]
    bars = dict(tv=max(2.0 * abs(tv32 - tv), 1e-6 * abs(tv)),
                grad=max(2.0 * float(np.abs(grad32 - grad).max()), 1e-6 * float(np.abs(grad).max())))
    return dict(tv=tv, grad=grad), bars


# ---- restatement two: eight corners in numpy --------------------------------------------------------------------------
def slice_numpy(grids, image, idx, dout=None):
    """float64.  grids (N,12,GZ,GY,GX), image (B,3,H,W), idx: list of B ints, dout like image or None ->
    (out, d_image, d_grids) (the last two None without dout)"""
    grids, image = np.asarray(grids, dtype=np.float64), np.asarray(image, dtype=np.float64)
    N, _, GZ, GY, GX = grids.shape
    B, _, H, W = image.shape
    out = np.zeros_like(image)
    d_image = d_grids = None
    if dout is not None:
        dout = np.asarray(dout, dtype=np.float64)
        d_image, d_grids = np.zeros_like(image), np.zeros_like(grids)
    gx = np.broadcast_to(((np.arange(W) + 0.5) / W * (GX - 1))[None, :], (H, W))
    gy = np.broadcast_to(((np.arange(H) + 0.5) / H * (GY - 1))[:, None], (H, W))
    x0 = np.minimum(np.floor(gx), GX - 2).astype(np.int64)
    y0 = np.minimum(np.floor(gy), GY - 2).astype(np.int64)
    fx, fy = gx - x0, gy - y0
    for b in range(B):
        G = grids[idx[b]]
        gray = gray64(image[b])
        gz = np.clip(gray, 0.0, 1.0) * (GZ - 1)
        z0 = np.minimum(np.floor(gz), GZ - 2).astype(np.int64)
        fz = gz - z0
        inside = (gray > 0.0) & (gray < 1.0)
        rgb1 = np.concatenate([image[b], np.ones((1, H, W))], axis=0)
        A, dA_dgz = np.zeros((12, H, W)), np.zeros((12, H, W))
        corners = []
        for dz, dy, dx in itertools.product((0, 1), repeat=3):
            wxy = (fy if dy else 1.0 - fy) * (fx if dx else 1.0 - fx)
            w = (fz if dz else 1.0 - fz) * wxy
            at = (slice(None), z0 + dz, y0 + dy, x0 + dx)
            A += w * G[at]
            dA_dgz += (wxy if dz else -wxy) * G[at]
            corners.append((at, w))
        for c in range(3):
            out[b, c] = (A[4 * c:4 * c + 4] * rgb1).sum(0)
        if dout is not None:
            dL_dA = np.stack([dout[b, k // 4] * rgb1[k % 4] for k in range(12)])
            for at, w in corners:
                np.add.at(d_grids[idx[b]], at, w * dL_dA)
            guide = (GZ - 1) * inside * (dA_dgz * dL_dA).sum(0)
            for m in range(3):
                d_image[b, m] = sum(dout[b, c] * A[4 * c + m] for c in range(3)) + LUMA[m] * guide
    return out, d_image, d_grids
