"""A float64 restatement of the similarity transform of Gaussians (a helper module, imported by test_cpu_transform.py and
test_gpu_transform.py only): quaternion product, matrix <-> quaternion, the SH rotation matrices D^l and the row transform.

D^l is obtained from its DEFINITION, independently of how the library builds it: Y(R d) = D^l Y(d) for every unit d, with Y
evaluated by `oracle.torch_ref._sh_to_rgb` (one-hot coefficients), solved in the least-squares sense over 40 seeded sample
directions.  The row transform states every sum in the order include/gsr.h gives, so that its binary64 results differ from
the library's only by what the two D^l and the two exp / log implementations differ.
"""
import math

import numpy as np
import torch

from oracle.torch_ref import _sh_to_rgb

F64 = torch.float64
PI_MATRIX = torch.tensor([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]], dtype=F64)  # D1 = PI R PI^T


def quat_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The Hamilton product a (x) b of quaternions (..., 4) in (w, x, y, z) order."""
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([((w1 * w2 - x1 * x2) - y1 * y2) - z1 * z2,
                        ((w1 * x2 + x1 * w2) + y1 * z2) - z1 * y2,
                        ((w1 * y2 - x1 * z2) + y1 * w2) + z1 * x2,
                        ((w1 * z2 + x1 * y2) - y1 * x2) + z1 * w2], -1)


def quat_from_matrix(R) -> torch.Tensor:
    """Shepperd's method: the unit quaternion (w, x, y, z), w >= 0, of a (3,3) rotation (x' = R x), float64."""
    r = torch.as_tensor(np.asarray(R, dtype=np.float64)).tolist()
    r00, r11, r22 = r[0][0], r[1][1], r[2][2]
    tr = r00 + r11 + r22
    if tr >= r00 and tr >= r11 and tr >= r22:
        q = [1.0 + tr, r[2][1] - r[1][2], r[0][2] - r[2][0], r[1][0] - r[0][1]]
    elif r00 >= r11 and r00 >= r22:
        q = [r[2][1] - r[1][2], 1.0 + r00 - r11 - r22, r[0][1] + r[1][0], r[0][2] + r[2][0]]
    elif r11 >= r22:
        q = [r[0][2] - r[2][0], r[0][1] + r[1][0], 1.0 - r00 + r11 - r22, r[1][2] + r[2][1]]
    else:
        q = [r[1][0] - r[0][1], r[0][2] + r[2][0], r[1][2] + r[2][1], 1.0 - r00 - r11 + r22]
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    sgn = -1.0 if q[0] < 0.0 else 1.0
    return torch.tensor([sgn * v / n for v in q], dtype=F64)


def matrix_from_quat(q: torch.Tensor) -> torch.Tensor:
    """(3,3) float64 rotation of the unit quaternion (w, x, y, z): the rasterizer's build_rotation."""
    w, x, y, z = (float(v) for v in q)
    return torch.tensor([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                         [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                         [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]], dtype=F64)


def rotation_hat(R) -> torch.Tensor:
    """matrix(quaternion(R)): the exactly orthonormal rotation the specification uses for everything."""
    return matrix_from_quat(quat_from_matrix(R))


def axis_angle(axis, angle: float) -> torch.Tensor:
    """(3,3) float64 rotation by `angle` about `axis` (Rodrigues)."""
    a = torch.tensor(axis, dtype=F64)
    a = a / a.norm()
    K = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=F64)
    return torch.eye(3, dtype=F64) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def random_rotation(seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(4, dtype=F64, generator=g)
    q = q / q.norm()
    return matrix_from_quat(q if q[0] >= 0 else -q)


def unit_directions(n: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, dtype=F64, generator=g)
    return d / d.norm(dim=1, keepdim=True)


def sh_basis(dirs: torch.Tensor) -> torch.Tensor:
    """(n, 16) float64: Y_m(d) of the rasterizer's basis for m = 0..15, read off `_sh_to_rgb` with one-hot coefficients."""
    n = dirs.shape[0]
    cols = []
    for m in range(16):
        sh = torch.zeros(n, 16, 3, dtype=F64)
        sh[:, m, :] = 1.0
        cols.append(_sh_to_rgb(3, sh, dirs)[:, 0])
    return torch.stack(cols, 1)


BANDS = ((1, 4), (4, 9), (9, 16))  # coefficient ranges of bands 1..3 among the 16


def sh_rotation_matrices(R: torch.Tensor, n_dirs: int = 40, seed: int = 20240) -> list:
    """[D1 (3,3), D2 (5,5), D3 (7,7)] float64 with Y_l(R d) = D^l Y_l(d): the least-squares solution of
    Y(S) (D^l)^T = Y(S R^T) over the sample directions S (rows)."""
    S = unit_directions(n_dirs, seed)
    Y0, Y1 = sh_basis(S), sh_basis(S @ R.T)
    out = []
    for lo, hi in BANDS:
        Dt = torch.linalg.lstsq(Y0[:, lo:hi], Y1[:, lo:hi]).solution
        out.append(Dt.T.contiguous())
    return out


def rotate_sh_rest(rest: torch.Tensor, D: list) -> torch.Tensor:
    """features_rest (P, M-1, 3) float64 -> c' = D^l c per band and channel; sums over k in ascending order."""
    out = rest.clone()
    n = rest.shape[1]
    for (lo, hi), Dl in zip(BANDS, D):
        lo, hi = lo - 1, hi - 1  # (the rest starts behind the DC term)
        if hi > n:
            break
        for m in range(hi - lo):
            acc = Dl[m, 0] * rest[:, lo, :]
            for k in range(1, hi - lo):
                acc = acc + Dl[m, k] * rest[:, lo + k, :]
            out[:, lo + m, :] = acc
    return out


def effective_translation(R_hat: torch.Tensor, t, s: float, pivot) -> torch.Tensor:
    t = torch.zeros(3, dtype=F64) if t is None else torch.as_tensor(np.asarray(t, dtype=np.float64))
    if pivot is None:
        return t
    p = torch.as_tensor(np.asarray(pivot, dtype=np.float64))
    Rp = torch.stack([(R_hat[i, 0] * p[0] + R_hat[i, 1] * p[1]) + R_hat[i, 2] * p[2] for i in range(3)])
    return (t + p) - s * Rp


def transform_rows_ref(xyz=None, rotation_raw=None, scaling_raw=None, features_rest=None, *, rotation=None, translation=None,
                       scale=1.0, pivot=None, mask=None, rotate_sh=True, scale_eps=0.0):
    """The specification on CPU tensors: float32 in, binary64 arithmetic, ONE rounding to float32 -> a tuple of new tensors
    (None where the input was None).  Rows outside `mask` keep their bits."""
    R_in = torch.eye(3, dtype=F64) if rotation is None else torch.as_tensor(np.asarray(rotation, dtype=np.float64))
    q = quat_from_matrix(R_in)
    Rh = matrix_from_quat(q)
    s = float(scale)
    t = effective_translation(Rh, translation, s, pivot)
    sel = None if mask is None else mask.bool()

    def keep(old, new32):
        return new32 if sel is None else torch.where(sel.view(-1, *([1] * (old.dim() - 1))), new32, old)

    out = []
    if xyz is None:
        out.append(None)
    else:
        x, y, z = xyz.double().unbind(1)
        new = torch.stack([s * ((Rh[i, 0] * x + Rh[i, 1] * y) + Rh[i, 2] * z) + t[i] for i in range(3)], 1)
        out.append(keep(xyz, new.float()))
    out.append(None if rotation_raw is None else keep(rotation_raw, quat_mul(q.expand_as(rotation_raw), rotation_raw.double()).float()))
    out.append(None if scaling_raw is None else keep(scaling_raw, torch.log(torch.exp(scaling_raw.double()) * s + scale_eps).float()))
    if features_rest is None:
        out.append(None)
    elif not rotate_sh or features_rest.shape[1] == 0:
        out.append(features_rest.clone())
    else:
        out.append(keep(features_rest, rotate_sh_rest(features_rest.double(), sh_rotation_matrices(Rh)).float()))
    return tuple(out)


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Elementwise distance of two float32 tensors in units in the last place (0 for equal bits; +0 and -0 are 0 apart)."""
    def ordered(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (ordered(a) - ordered(b)).abs()
