"""Similarity transforms of Gaussians on the GPU: move, rotate and scale what was selected (DESIGN.md section 25;
include/gsr.h: gsr_sh_rotation, gsr_transform_rows).

The reference's Add flow places the generated object with `rotate_gaussians`, `scale_gaussians` and `translate_gaussians`
of `threestudio/utils/transform.py`: a handful of torch operations that need kornia and scipy for one quaternion product
and that rotate positions and orientations but leave the spherical-harmonic coefficients where they were -- after a
rotation every view-dependent colour of the moved object points in the old direction.  Here the transform
T: x -> s R x + t is ONE launch over the raw parameters, in place:

    xyz'          = s R^ xyz + t
    rotation_raw' = q_R (x) rotation_raw        (Hamilton product, w x y z; the raw norm is kept: the activation normalises
                                                 anyway, and Adam's scale stays what it was)
    scaling_raw'  = log(exp(scaling_raw) s + eps)
    features_rest'= D^l(R^) c  per band l = 1..3 and channel (band 0, `features_dc`, is invariant)

every row in binary64, rounded once at the store.  q_R is the unit quaternion of the caller's matrix (Shepperd's method in
binary64, w >= 0) and R^ = matrix(q_R) is what positions, orientations and SH coefficients all see: an exactly orthonormal
rotation even where the caller's matrix was a float32 `cam.R`.  D^l is defined by
sum_m c'_m Y_m(R^ d) = sum_m c_m Y_m(d) for every unit d, Y the basis of `gaussian_renderer.eval_sh`.

  * `transform_rows` -- the tensors; `transform_gaussians` -- a reference-style model (and its optimizer's moments);
  * `rotate_gaussians`, `translate_gaussians`, `scale_gaussians` -- the reference's names, signatures and semantics;
    `install()` registers them as `threestudio.utils.transform`, without kornia or scipy;
  * `sh_rotation` -- the three D^l of a rotation, on the host.

Out of scope, refused with a ValueError: non-uniform scale (it needs a covariance re-decomposition), reflections,
`scale <= 0`, a matrix further than 1e-4 from a rotation.  Every in-place writer moves the version counters of what it
writes; a parameter that is a view of an arena shares the arena's counter.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
import sys
import types
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.autograd.graph import increment_version

from . import _native

__all__ = ["transform_rows", "transform_gaussians", "rotate_gaussians", "translate_gaussians", "scale_gaussians",
           "sh_rotation", "rotation_hat", "effective_translation", "install", "ROWS_PER_BLOCK"]

#: rows one block of the kernel transforms (gsr_transform.hip: TR_BLOCK); the tests size their cases around it
ROWS_PER_BLOCK = 256
_MASK = (torch.bool, torch.uint8)
_REST = (0, 3, 8, 15)
_EYE = np.eye(3)


def _check(what: str, name: str, t, ref: torch.Tensor, shape: Tuple[int, ...], dtypes=(torch.float32,)) -> None:
    """`t` against the first tensor of the call: dtype, shape, contiguity -- by name (then `_check_device` for all)."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise RuntimeError(f"{what}: {name} has dtype {t.dtype}, expected {' / '.join(str(d) for d in dtypes)}")
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be contiguous")


def _check_device(what: str, name: str, t: torch.Tensor, ref: torch.Tensor) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: {name} must live on the ROCm GPU; there is no CPU fallback")
    if t.device != ref.device:
        raise RuntimeError(f"{what}: {name} is on {t.device}, expected {ref.device}")


def _host(what: str, name: str, v, shape: Tuple[int, ...]) -> np.ndarray:
    """A tensor (on any device: one small readback), numpy array or list as binary64 numbers on the host."""
    if isinstance(v, torch.Tensor):
        v = v.detach().to(device="cpu", dtype=torch.float64).numpy()
    a = np.array(v, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{what}: {name} has shape {a.shape}, expected {shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what}: {name} holds a number that is not finite")
    return a


def _scalar(what: str, scale) -> float:
    if isinstance(scale, torch.Tensor):
        scale = scale.detach().to(device="cpu", dtype=torch.float64).numpy()
    a = np.asarray(scale, dtype=np.float64)
    if a.size != 1:
        raise ValueError(f"{what}: scale must be one number: a non-uniform scale needs a covariance re-decomposition and is "
                         "not supported")
    s = float(a.reshape(()))
    if not (s > 0.0 and math.isfinite(s)):
        raise ValueError(f"{what}: scale must be positive and finite, got {s}")
    return s


def _dbl(values: Sequence[float]):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def sh_rotation(rotation, what: str = "sh_rotation") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(D1 (3,3), D2 (5,5), D3 (7,7)) float64: the matrices that rotate the SH coefficients of bands 1..3, c' = D^l c, for
    the rotation nearest to `rotation` (3,3; x' = rotation x).  Host only.  ValueError unless `rotation` is a proper
    rotation within 1e-4."""
    rot = _host(what, "rotation", rotation, (3, 3))
    out = (ctypes.c_double * 83)()
    if _native.lib().gsr_sh_rotation(_dbl(rot.reshape(-1)), out) != 0:
        raise ValueError(f"{what}: rotation is not a proper rotation matrix (reflections and matrices further than 1e-4 "
                         "from orthonormal are refused)")
    d = np.array(out[:], dtype=np.float64)
    return d[:9].reshape(3, 3).copy(), d[9:34].reshape(5, 5).copy(), d[34:].reshape(7, 7).copy()


def rotation_hat(rotation, what: str = "rotation_hat") -> Tuple[np.ndarray, np.ndarray]:
    """(q_R (4,) w x y z, R^ (3,3)) float64 of `rotation` as the library sees it: Shepperd's method in binary64, normalised,
    w >= 0, and the matrix of that quaternion (the same operations as gsr_transform.hip: rotation_of)."""
    r = _host(what, "rotation", rotation, (3, 3))
    sh_rotation(r, what)  # (the library decides what counts as a rotation)
    r00, r11, r22 = float(r[0, 0]), float(r[1, 1]), float(r[2, 2])
    tr = r00 + r11 + r22
    if tr >= r00 and tr >= r11 and tr >= r22:
        q = [1.0 + tr, r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]]
    elif r00 >= r11 and r00 >= r22:
        q = [r[2, 1] - r[1, 2], 1.0 + r00 - r11 - r22, r[0, 1] + r[1, 0], r[0, 2] + r[2, 0]]
    elif r11 >= r22:
        q = [r[0, 2] - r[2, 0], r[0, 1] + r[1, 0], 1.0 - r00 + r11 - r22, r[1, 2] + r[2, 1]]
    else:
        q = [r[1, 0] - r[0, 1], r[0, 2] + r[2, 0], r[1, 2] + r[2, 1], 1.0 - r00 - r11 + r22]
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(((w * w + x * x) + y * y) + z * z)
    sgn = -1.0 if w < 0.0 else 1.0
    w, x, y, z = sgn * w / n, sgn * x / n, sgn * y / n, sgn * z / n
    R = np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                  [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                  [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]], dtype=np.float64)
    return np.array([w, x, y, z], dtype=np.float64), R


def effective_translation(rotation, translation, scale, pivot, what: str = "transform_rows") -> np.ndarray:
    """t_eff (3,) float64 of x -> s R^ (x - p) + p + t: t + p - s R^ p, on the host in binary64."""
    return _fold(what, _EYE if rotation is None else rotation_hat(rotation, what)[1], translation, _scalar(what, scale), pivot)


def _fold(what: str, R: np.ndarray, translation, s: float, pivot) -> np.ndarray:
    t = np.zeros(3) if translation is None else _host(what, "translation", translation, (3,))
    if pivot is None:
        return t
    p = _host(what, "pivot", pivot, (3,))
    Rp = np.array([(R[i, 0] * p[0] + R[i, 1] * p[1]) + R[i, 2] * p[2] for i in range(3)])
    return (t + p) - s * Rp


def _transform(what: str, xyz, rotation_raw, scaling_raw, features_rest, rotation, translation, scale, pivot, mask,
               rotate_sh: bool, scale_eps: float) -> List[torch.Tensor]:
    """Validates, launches, and returns the tensors the kernel wrote."""
    # the transform itself first: what is out of scope is a ValueError whatever the tensors are
    s = _scalar(what, scale)
    eps = float(scale_eps)
    if not (eps >= 0.0 and math.isfinite(eps)):
        raise ValueError(f"{what}: scale_eps must be non-negative and finite")
    rot, Rh, rotates = _EYE, _EYE, False
    if rotation is not None:
        rot = _host(what, "rotation", rotation, (3, 3))
        q, Rh = rotation_hat(rot, what)
        rotates = not (q[0] == 1.0 and q[1] == 0.0 and q[2] == 0.0 and q[3] == 0.0)  # (the identity leaves everything alone)
    t_eff = _fold(what, Rh, translation, s, pivot)
    given = [(n, t) for n, t in (("xyz", xyz), ("rotation_raw", rotation_raw), ("scaling_raw", scaling_raw),
                                 ("features_rest", features_rest)) if t is not None]
    if not given:
        raise RuntimeError(f"{what}: no tensor to transform")
    ref = given[0][1]
    if not isinstance(ref, torch.Tensor) or ref.dim() < 1:
        raise RuntimeError(f"{what}: {given[0][0]} must be a tensor with one row per Gaussian")
    P = int(ref.shape[0])
    rest = 0
    for name, t in given:
        if name == "features_rest":
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or int(t.shape[1]) not in _REST:
                raise RuntimeError(f"{what}: features_rest must be a (P, M - 1, 3) tensor with M - 1 in {_REST} (SH degree 0 to 3)")
            rest = int(t.shape[1])
            _check(what, name, t, ref, (P, rest, 3))
        else:
            _check(what, name, t, ref, (P, 4 if name == "rotation_raw" else 3))
    if mask is not None:
        _check(what, "mask", mask, ref, (P,), _MASK)
        given.append(("mask", mask))
    for name, t in given:
        _check_device(what, name, t, ref)
    # what the transform leaves alone is not handed to the kernel (and its version counter does not move)
    moves = rotates or s != 1.0 or bool(np.any(t_eff != 0.0))
    k_xyz = xyz if moves else None
    k_rot = rotation_raw if rotates else None
    k_scl = scaling_raw if (s != 1.0 or eps != 0.0) else None
    k_sh = features_rest if (rotates and rotate_sh and rest > 0) else None
    written = [t for t in (k_xyz, k_rot, k_scl, k_sh) if t is not None]
    if P == 0 or not written:
        return []
    dev = ref.device
    m8 = None if mask is None else (mask.view(torch.uint8) if mask.dtype == torch.bool else mask)
    increment_version(written)  # written through raw pointers
    with torch.cuda.device(dev):
        _native.check("gsr_transform_rows", _native.lib().gsr_transform_rows(
            torch.cuda.current_stream(dev).cuda_stream, P, rest if k_sh is not None else 0,
            None if k_xyz is None else k_xyz.data_ptr(), None if k_rot is None else k_rot.data_ptr(),
            None if k_scl is None else k_scl.data_ptr(), None if k_sh is None else k_sh.data_ptr(),
            None if m8 is None else m8.data_ptr(), _dbl(rot.reshape(-1)), _dbl(t_eff), s, eps))
    return written


def transform_rows(xyz: Optional[torch.Tensor], rotation_raw: Optional[torch.Tensor] = None,
                   scaling_raw: Optional[torch.Tensor] = None, features_rest: Optional[torch.Tensor] = None, *,
                   rotation=None, translation=None, scale=1.0, pivot=None, mask: Optional[torch.Tensor] = None,
                   rotate_sh: bool = True, scale_eps: float = 0.0) -> None:
    """x -> s R (x - pivot) + pivot + t on the rows where `mask` is set, in place, one launch on the current stream that
    never synchronises with the host.  `xyz` (P,3), `rotation_raw` (P,4; w x y z), `scaling_raw` (P,3) and `features_rest`
    (P, M-1, 3), M-1 in {0, 3, 8, 15}, are the RAW float32 parameters, contiguous, at any 4-byte-aligned address (views of
    a `RowArena` included); any of them may be None (a tensor that is not given is not transformed).  `rotation` (3,3),
    `translation` (3,) and `pivot` (3,) may be tensors on any device, numpy arrays or lists (a device tensor costs one small
    readback); `scale` is one positive number.  `mask` (P,) bool / uint8: rows outside it are never written, not even with
    their own values.  `rotate_sh=False` leaves `features_rest` alone (the reference's result).  `scale_eps`:
    scaling_raw' = log(exp(scaling_raw) s + scale_eps); the reference's `scale_gaussians` uses 1e-7.

    Tensors the transform leaves alone are not touched at all: a pure translation writes `xyz` only, a pure rotation leaves
    `scaling_raw`.  The version counter of every tensor written moves."""
    _transform("transform_rows", xyz, rotation_raw, scaling_raw, features_rest, rotation, translation, scale, pivot, mask,
               rotate_sh, scale_eps)


def transform_gaussians(model, *, rotation=None, translation=None, scale=1.0, pivot=None,
                        mask: Optional[torch.Tensor] = None, rotate_sh: bool = True,
                        optimizer: Optional[torch.optim.Optimizer] = None, scale_eps: float = 0.0) -> None:
    """`transform_rows` on a reference-style model: `_xyz`, `_rotation`, `_scaling`, `_features_rest` (a missing attribute
    is skipped).  With `optimizer`, the Adam moments `exp_avg` / `exp_avg_sq` of the tensors that were written are zeroed on
    the selected rows: a moved Gaussian does not keep the momentum of where it was.

        stats = ContributionStats(P, 1); trace_view(cam, model, stats, mask=mask2d)   # lift a 2D selection
        transform_gaussians(model, translation=[0.0, 0.1, 0.0], mask=stats.select(0.5), optimizer=opt)
    """
    what = "transform_gaussians"
    xyz = getattr(model, "_xyz", None)
    if xyz is None:
        raise RuntimeError(f"{what}: the model has no _xyz")
    tensors = [xyz, getattr(model, "_rotation", None), getattr(model, "_scaling", None), getattr(model, "_features_rest", None)]
    with torch.no_grad():
        written = _transform(what, *tensors, rotation, translation, scale, pivot, mask, rotate_sh, scale_eps)
        if optimizer is None:
            return
        rows = None if mask is None else mask.bool()
        for t in written:
            st = optimizer.state.get(t)
            if not st:
                continue
            for key in ("exp_avg", "exp_avg_sq"):
                m = st.get(key)
                if m is None:
                    continue
                if rows is None:
                    m.zero_()
                else:
                    m[rows] = 0


# ---------------------------------------------------------------------------------------------------------------------
# the reference's names (threestudio/utils/transform.py): same signatures, same semantics, one launch each
# ---------------------------------------------------------------------------------------------------------------------
def rotate_gaussians(gaussian, rotmat, rotate_sh: bool = False) -> None:
    """xyz' = rotmat xyz, rotation' = q(rotmat) (x) rotation.  `rotate_sh=False` is the reference's result (the SH
    coefficients stay); True also rotates `_features_rest`.  Unlike the reference the raw quaternion keeps its norm."""
    transform_gaussians(gaussian, rotation=rotmat, rotate_sh=rotate_sh)


def translate_gaussians(gaussian, tvec) -> None:
    """xyz' = xyz + tvec."""
    transform_gaussians(gaussian, translation=tvec)


def scale_gaussians(gaussian, scale) -> None:
    """xyz' = xyz scale (about the origin), scaling' = log(get_scaling scale + 1e-7): the reference's formula."""
    transform_gaussians(gaussian, scale=scale, scale_eps=1e-7)


def install(rotate_sh: bool = True) -> types.ModuleType:
    """Registers a stand-in for `threestudio.utils.transform` that needs neither kornia nor scipy: `rotate_gaussians`
    (rotating the SH coefficients too unless `rotate_sh=False`), `translate_gaussians`, `scale_gaussians` and
    `default_model_mtx`, the rotation by -pi/2 about x as a float32 tensor on the GPU, created when it is first read.
    Where no `threestudio` package can be imported, empty parent packages are registered with it.  -> the module."""
    import importlib.util

    name = "threestudio.utils.transform"
    mod = types.ModuleType(name, "gaussianeditor_amd.transform under the reference's name")
    default_sh = bool(rotate_sh)

    def _rotate(gaussian, rotmat, rotate_sh=default_sh):
        rotate_gaussians(gaussian, rotmat, rotate_sh=rotate_sh)

    _rotate.__name__ = "rotate_gaussians"
    _rotate.__doc__ = rotate_gaussians.__doc__
    mod.rotate_gaussians = _rotate
    mod.translate_gaussians = translate_gaussians
    mod.scale_gaussians = scale_gaussians

    def _lazy(attr):
        if attr == "default_model_mtx":
            mtx = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]], dtype=torch.float32, device="cuda")
            mod.default_model_mtx = mtx
            return mtx
        raise AttributeError(f"module {name!r} has no attribute {attr!r}")

    mod.__getattr__ = _lazy
    if "threestudio" not in sys.modules and importlib.util.find_spec("threestudio") is None:
        for pkg in ("threestudio", "threestudio.utils"):
            stub = types.ModuleType(pkg)
            stub.__path__ = []  # a package without files: only what is registered under it can be imported
            sys.modules[pkg] = stub
        sys.modules["threestudio"].utils = sys.modules["threestudio.utils"]
    parent = sys.modules.get("threestudio.utils")
    if parent is not None:
        parent.transform = mod
    sys.modules[name] = mod
    return mod
