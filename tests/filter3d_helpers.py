"""What the 3D-filter tests share (tests/test_cpu_filter3d.py, tests/test_gpu_filter3d.py): the mathematics of the
gsr_filter3d_* entry points (include/gsr.h) restated on the CPU, and the seeded cases.

  * sweep_ref: numpy binary64 on the binary32 inputs, one IEEE operation per operator in the stated order (numpy's ufuncs do
    not contract a product and a sum).  The product is held to it BIT FOR BIT, so it takes everything the kernel takes from
    the host -- focal lengths, half sizes, screen bounds -- from `camera_table`, which restates the record layout itself.
  * apply_ref: plain torch operators with autograd, Mip-Splatting's get_scaling_with_3D_filter /
    get_opacity_with_3D_filter, in the dtype of their inputs.  In float64 they are the yardstick; run in float32 their error
    against float64 sets the bar, max(2 x that error, 1e-6 of the tensor's largest entry): the project's rule for fused
    stages (normals_helpers.bar_of).
  * sweep_case / apply_case: seeded inputs.  A sweep case meets its input condition ITSELF: no decision (near plane, the
    four screen bounds) within REL_MARGIN relative of its threshold -- `sweep_offenders` counts, 0 in every case, asserted on
    the CPU.
"""
import functools
import math

import numpy as np
import torch

from normals_helpers import bar_of

F64 = torch.float64
NEAR = float(np.float32(0.2))   # (double)0.2f, the rasterizer's near plane
ZZ_MIN = 0.001
UNSEEN = 100000.0
SQRT_0_2 = math.sqrt(0.2)
REL_MARGIN = 1e-9
ROWS = 256                      # filter3d.ROWS_PER_BLOCK (asserted by the CPU tests)
CHUNK = 32                      # filter3d.CAMERAS_PER_CHUNK (likewise)
LADDER = (1, 63, 64, 65, ROWS - 1, ROWS, ROWS + 1, 1000, 100_003)
VIEWS = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
SWEEP_CASES = [(P, V) for P in LADDER for V in VIEWS if P != 100_003 or V in (1, CHUNK + 1)]


class Cam:
    """the attributes the module reads of a camera"""

    def __init__(self, V, W, H, fovx, fovy):
        self.world_view_transform = torch.as_tensor(np.asarray(V, dtype=np.float32)).contiguous()
        self.image_width, self.image_height, self.FoVx, self.FoVy = W, H, fovx, fovy


# ---- the sweep ----------------------------------------------------------------------------------------------------------
def camera_table(cameras):
    """list of dict(M (4,4) f64 of the f32 matrix, fx, fy, W, H): doubles, as Python computes them"""
    out = []
    for c in cameras:
        W, H = float(int(c.image_width)), float(int(c.image_height))
        out.append(dict(M=c.world_view_transform.detach().cpu().float().numpy().astype(np.float64), W=W, H=H,
                        fx=W / (2.0 * math.tan(float(c.FoVx) / 2.0)), fy=H / (2.0 * math.tan(float(c.FoVy) / 2.0))))
    return out


def project(xyz, cam):
    """(zc, u, v) float64 (P,) of one camera of camera_table, in the stated order"""
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    M = cam["M"]
    p = [((x * M[0, k] + y * M[1, k]) + z * M[2, k]) + M[3, k] for k in range(3)]
    zc = p[2]
    zz = np.maximum(zc, ZZ_MIN)
    with np.errstate(all="ignore"):
        u = (p[0] / zz) * cam["fx"] + 0.5 * cam["W"]
        v = (p[1] / zz) * cam["fy"] + 0.5 * cam["H"]
    return zc, u, v


def bounds(cam):
    return -0.15 * cam["W"], 1.15 * cam["W"], -0.15 * cam["H"], 1.15 * cam["H"]


def sees(xyz, cam):
    """((P,) bool: the camera sees the row, zc)"""
    zc, u, v = project(xyz, cam)
    lo_u, hi_u, lo_v, hi_v = bounds(cam)
    return (zc > NEAR) & (u >= lo_u) & (u <= hi_u) & (v >= lo_v) & (v <= hi_v), zc


def sweep_ref(xyz, cameras):
    """(filter_3D (P,1) float32, valid (P,) bool): the restatement"""
    xyz = np.asarray(xyz, dtype=np.float32)
    table = camera_table(cameras)
    P = xyz.shape[0]
    d = np.full(P, np.inf)
    valid = np.zeros(P, dtype=bool)
    for cam in table:
        seen, zc = sees(xyz, cam)
        d = np.where(seen, np.minimum(d, zc), d)
        valid |= seen
    d = np.where(valid, d, d[valid].max() if valid.any() else UNSEEN)
    f_max = max(c["fx"] for c in table)
    return ((d / f_max) * SQRT_0_2).astype(np.float32).reshape(P, 1), valid


def offender_rows(xyz, cameras, rel=REL_MARGIN):
    """(P,) int: per row, how many of its decisions over all cameras lie within `rel` relative of their threshold.  The
    near plane always decides; a screen bound only decides where the row is beyond the near plane."""
    xyz = np.asarray(xyz, dtype=np.float32)
    n = np.zeros(xyz.shape[0], dtype=np.int64)
    for cam in camera_table(cameras):
        zc, u, v = project(xyz, cam)
        n += np.abs(zc - NEAR) <= rel * NEAR
        front = zc > NEAR
        lo_u, hi_u, lo_v, hi_v = bounds(cam)
        for val, b in ((u, lo_u), (u, hi_u), (v, lo_v), (v, hi_v)):
            n += front & (np.abs(val - b) <= rel * abs(b))
    return n


def sweep_offenders(xyz, cameras, rel=REL_MARGIN):
    return int(offender_rows(xyz, cameras, rel).sum())


def look_at(eye, target, roll_deg=0.0):
    """(4,4) float64: the transposed view matrix (row 3 the translation) of a camera at `eye` looking at `target`, rolled"""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    a = math.radians(roll_deg)
    r2, d2 = math.cos(a) * right + math.sin(a) * down, -math.sin(a) * right + math.cos(a) * down
    R = np.stack([r2, d2, fwd])          # world-to-camera rotation, rows = camera axes
    M = np.eye(4)
    M[:3, :3] = R.T
    M[3, :3] = -R @ eye
    return M


@functools.lru_cache(maxsize=None)
def seeded_cameras(V, seed=0):
    """V general cameras around the origin: roll, unequal focal lengths, image sizes that are multiples of nothing; a
    narrow field of view, so that a good share of the rows is seen by few cameras or none"""
    rng = np.random.default_rng(4000 + 17 * V + seed)
    cams = []
    for _ in range(V):
        eye = rng.standard_normal(3)
        eye *= rng.uniform(2.0, 6.0) / np.linalg.norm(eye)
        M = look_at(eye, rng.uniform(-1.5, 1.5, size=3), roll_deg=rng.uniform(-40.0, 40.0))
        W, H = int(rng.integers(37, 700)), int(rng.integers(29, 500))
        cams.append(Cam(M, W, H, math.radians(rng.uniform(12.0, 40.0)), math.radians(rng.uniform(10.0, 35.0))))
    return tuple(cams)


@functools.lru_cache(maxsize=None)
def sweep_case(P, V):
    """dict(xyz (P,3) f32 read-only, cameras): rows within REL_MARGIN of a threshold are redrawn"""
    rng = np.random.default_rng(5000 + P + 1_000_003 * V)
    cams = seeded_cameras(V)
    xyz = (3.0 * rng.standard_normal((P, 3))).astype(np.float32)
    for _ in range(20):
        bad = offender_rows(xyz, cams) > 0
        if not bad.any():
            break
        xyz[bad] = (3.0 * rng.standard_normal((int(bad.sum()), 3))).astype(np.float32)
    xyz.setflags(write=False)
    return dict(xyz=xyz, cameras=cams, P=P, V=V)


@functools.lru_cache(maxsize=None)
def sweep_expectation(P, V):
    c = sweep_case(P, V)
    return sweep_ref(c["xyz"], c["cameras"])


def identity_camera(W=640, H=480, fovx=1.0, fovy=0.8, t=(0.0, 0.0, 0.0)):
    M = np.eye(4)
    M[3, :3] = t
    return Cam(M, W, H, fovx, fovy)


def boundary_rows(cam, z=2.0):
    """For the identity-rotation camera `cam` (p = xyz exactly): rows (xyz (N,3) f32, expected seen (N,) bool, names) that
    straddle the near plane and each of the four screen bounds by one float32 step.  z = 2 makes p / z exact; the x (or y)
    that lands on a bound is found by bisection over float32 values on the restatement's own u (monotone in x)."""
    t = camera_table([cam])[0]
    rows, names = [], []
    at = np.float32(0.2)  # zc == 0.2f is NOT beyond the near plane (the comparison is strict); its successor is
    rows += [(0.0, 0.0, np.nextafter(at, np.float32(0.0))), (0.0, 0.0, at), (0.0, 0.0, np.nextafter(at, np.float32(1.0)))]
    names += ["near/below", "near/at", "near/above"]
    lo_u, hi_u, lo_v, hi_v = bounds(t)
    for axis, bound, upper in ((0, lo_u, False), (0, hi_u, True), (1, lo_v, False), (1, hi_v, True)):
        def coord(c, axis=axis):
            p = np.zeros((1, 3), dtype=np.float32)
            p[0, 2], p[0, axis] = z, c
            return project(p, t)[1 + axis][0]
        lo, hi = np.float32(-50.0), np.float32(50.0)   # coord(lo) < bound <= coord(hi); float32 bisection on the bit pattern
        assert coord(lo) < bound <= coord(hi)
        while np.nextafter(lo, np.float32(np.inf)) != hi:
            mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
            if mid == lo or mid == hi:
                break
            if coord(mid) < bound:
                lo = mid
            else:
                hi = mid
        # lo: the last float32 whose image lies below the bound, hi: the first at or above it
        if upper:   # inclusive upper bound: the first value ABOVE it is out; step to it
            inside, outside = (hi, np.nextafter(hi, np.float32(np.inf))) if coord(hi) == bound else (lo, hi)
        else:       # inclusive lower bound: lo is out, hi is in
            inside, outside = hi, lo
        for c, name in ((inside, "in"), (outside, "out")):
            p = [0.0, 0.0, z]
            p[axis] = c
            rows.append(tuple(p))
            names.append(f"{'uv'[axis]}{'hi' if upper else 'lo'}/{name}")
    xyz = np.array(rows, dtype=np.float32)
    want = np.array([n.endswith(("above", "in")) for n in names])
    return xyz, want, names


# ---- the apply ----------------------------------------------------------------------------------------------------------
def apply_ref(scales, opacity, filter_3D, from_raw=False):
    """(scales_eff, opacity_eff): Mip-Splatting's two getters in torch operators, in the dtype of the inputs"""
    s = torch.exp(scales) if from_raw else scales
    o = torch.sigmoid(opacity) if from_raw else opacity
    f2 = torch.square(filter_3D)
    s2 = torch.square(s)
    det1 = s2.prod(dim=1)
    e = s2 + f2
    det2 = e.prod(dim=1)
    coef = torch.sqrt(det1 / det2)
    return torch.sqrt(e), o * coef[..., None]


@functools.lru_cache(maxsize=None)
def apply_case(P, from_raw, wide=False):
    """dict(scales (P,3), opacity (P,1), filter (P,1), g_s (P,3), g_o (P,1)): f32 numpy, read-only.

    A row is a Gaussian, not three independent numbers: its size b is log-uniform over 1e-4 .. 1, its three scales lie
    within half a decade of b (clipped to 1e-4 .. 1), and its filter is 0 (15 % of the rows) or b times 10^U(-1, 1) clipped
    to 1e-4 .. 1e-1 -- what the sweep gives: the filter of a Gaussian is of the order of the pixel footprint at its depth,
    and so is a trained Gaussian.  Opacity across (0, 1).  from_raw: the logarithm of such scales (-9.2 .. 0) and raw opacity
    across +-8.  wide: raw scales uniform over +-8 instead, every row independent (scales up to e^8 = 2981): their
    gradients set the largest entry of the tensor and with it the bar, so the share condition on the cross term is not
    asked of that case; the bar is."""
    rng = np.random.default_rng(6000 + 2 * P + int(from_raw) + 100 * int(wide))
    b = 10.0 ** rng.uniform(-4.0, 0.0, size=(P, 1))
    scales = np.clip(b * 10.0 ** rng.uniform(-0.5, 0.5, size=(P, 3)), 1e-4, 1.0)
    opacity = rng.uniform(0.001, 0.999, size=(P, 1))
    f = np.clip(b * 10.0 ** rng.uniform(-1.0, 1.0, size=(P, 1)), 1e-4, 1e-1)
    f[rng.uniform(size=(P, 1)) < 0.15] = 0.0
    f[0] = np.clip(b[0], 1e-4, 1e-1)  # (every case has a row with a filter of its own size, and from two rows on one without)
    f[1:2] = 0.0
    if from_raw:
        scales = rng.uniform(-8.0, 8.0, size=(P, 3)) if wide else np.log(scales)
        opacity = rng.uniform(-8.0, 8.0, size=(P, 1))
    out = dict(scales=scales, opacity=opacity, filter=f, g_s=rng.standard_normal((P, 3)), g_o=rng.standard_normal((P, 1)))
    out = {k: v.astype(np.float32) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return dict(out, P=P, from_raw=from_raw, wide=wide)


def run_apply(case, dtype):
    """dict(s_eff, o_eff, d_scales, d_opacity) float64 numpy: apply_ref and autograd in `dtype`"""
    t = lambda k, g=False: torch.tensor(case[k]).to(dtype).requires_grad_(g)  # noqa: E731
    s, o = t("scales", True), t("opacity", True)
    s_eff, o_eff = apply_ref(s, o, t("filter"), case["from_raw"])
    gs, go = torch.autograd.grad([s_eff, o_eff], [s, o], [t("g_s"), t("g_o")])
    n = lambda x: x.detach().double().numpy()  # noqa: E731
    return dict(s_eff=n(s_eff), o_eff=n(o_eff), d_scales=n(gs), d_opacity=n(go))


def cross_term(case):
    """(P,3) float64: the share of d_scales that comes through o_eff, dL/do_eff d o_eff / d s_k (times s_k with from_raw)"""
    t = lambda k, g=False: torch.tensor(case[k]).to(F64).requires_grad_(g)  # noqa: E731
    s = t("scales", True)
    _, o_eff = apply_ref(s, t("opacity"), t("filter"), case["from_raw"])
    g, = torch.autograd.grad(o_eff, s, t("g_o"))
    return g.numpy()


@functools.lru_cache(maxsize=None)
def apply_expectation(P, from_raw, wide=False):
    case = apply_case(P, from_raw, wide)
    e, s = run_apply(case, F64), run_apply(case, torch.float32)
    return e, {k: bar_of(s[k], e[k]) for k in e}
