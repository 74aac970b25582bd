"""CPU: the host half of the similarity transform of Gaussians (no device is touched): gsr_sh_rotation against the
definition of the SH rotation matrices, the argument validation of gsr_transform_rows, the Python layer's refusals and
pivot folding, and the `threestudio.utils.transform` stand-in."""
import ctypes
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

import transform_helpers as TH
from oracle.torch_ref import _sh_to_rgb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _f32_rounded(R):
    return R.float().double()


ROTATIONS = {
    "identity": torch.eye(3, dtype=F64),
    "z90": TH.axis_angle([0.0, 0.0, 1.0], math.pi / 2),
    "x180": TH.axis_angle([1.0, 0.0, 0.0], math.pi),
    "near180": TH.axis_angle([1.0, 2.0, 3.0], math.pi - 1e-6),  # trace < every diagonal entry but one: Shepperd's other branches
    "random1": TH.random_rotation(11),
    "random2": TH.random_rotation(12),
    "float32": _f32_rounded(TH.random_rotation(13)),
}


def _dbl(values):
    flat = [float(v) for v in np.asarray(values, dtype=np.float64).reshape(-1)]
    return (ctypes.c_double * len(flat))(*flat)


def _lib_D(R):
    from gaussianeditor_amd import _native

    out = (ctypes.c_double * 83)()
    assert _native.lib().gsr_sh_rotation(_dbl(R), out) == 0
    d = torch.tensor(out[:], dtype=F64)
    return [d[:9].reshape(3, 3), d[9:34].reshape(5, 5), d[34:].reshape(7, 7)]


def _identity_gap(D, Rh, seed):
    """max | sum_m c'_m Y_m(R^ d) - sum_m c_m Y_m(d) | over 64 seeded directions and random coefficients, c' = D c."""
    dirs = TH.unit_directions(64, seed)
    g = torch.Generator().manual_seed(seed + 1)
    c = torch.randn(64, 16, 3, dtype=F64, generator=g)
    c2 = c.clone()
    c2[:, 1:] = TH.rotate_sh_rest(c[:, 1:], D)
    return float((_sh_to_rgb(3, c2, dirs @ Rh.T) - _sh_to_rgb(3, c, dirs)).abs().max())


@pytest.mark.parametrize("name", list(ROTATIONS))
def test_sh_rotation_meets_its_definition(name):
    """The bars are 1e-12: a thousand times the 2.5e-15 the identity was measured at in float64."""
    R = ROTATIONS[name]
    Rh = TH.rotation_hat(R)
    D = _lib_D(R)
    eye = [torch.eye(n, dtype=F64) for n in (3, 5, 7)]
    if name == "identity":
        for Dl, I in zip(D, eye):
            assert torch.equal(Dl, I), "the identity must give exactly I"
    for Dl, I in zip(D, eye):
        assert float((Dl @ Dl.T - I).abs().max()) <= 1e-12
    assert float((D[0] - TH.PI_MATRIX @ Rh @ TH.PI_MATRIX.T).abs().max()) <= 1e-12
    # a homomorphism: D(R1 R2) = D(R1) D(R2), R2 a fixed seeded rotation
    R2 = TH.random_rotation(99)
    D2, D12 = _lib_D(R2), _lib_D(Rh @ R2)
    for a, b, ab in zip(D, D2, D12):
        assert float((ab - a @ b).abs().max()) <= 1e-12
    # the definition itself, and against the helper's independent construction
    gap = _identity_gap(D, Rh, seed=5)
    print(f"{name}: defining identity {gap:.3e}")
    assert gap <= 1e-12
    for Dl, Hl in zip(D, TH.sh_rotation_matrices(Rh)):
        assert float((Dl - Hl).abs().max()) <= 1e-12
    if name != "identity":  # the check discriminates: without the SH rotation the colour is off by O(1)
        assert _identity_gap(eye, Rh, seed=5) > 0.1


def test_sh_rotation_refuses_what_is_no_rotation():
    from gaussianeditor_amd import _native

    L = _native.lib()
    out = (ctypes.c_double * 83)()
    assert L.gsr_sh_rotation(None, out) == -1 and L.gsr_sh_rotation(_dbl(np.eye(3)), None) == -1
    assert L.gsr_sh_rotation(_dbl(np.diag([1.0, 1.0, -1.0])), out) == -1  # a reflection
    assert L.gsr_sh_rotation(_dbl(np.diag([1.0, 1.0, 1.001])), out) == -1  # 2e-3 from orthonormal
    assert L.gsr_sh_rotation(_dbl(np.full((3, 3), np.nan)), out) == -1
    assert L.gsr_sh_rotation(_dbl(np.eye(3) + 1e-6), out) == 0  # within 1e-4: the nearest rotation is used


def test_transform_rows_argument_validation_needs_no_gpu():
    """Every refusal of gsr_transform_rows comes back as GSR_ERR_BAD_ARGUMENT (-1) before the device is touched."""
    from gaussianeditor_amd import _native

    L = _native.lib()
    one = ctypes.c_void_p(256)  # never dereferenced
    I, t0 = _dbl(np.eye(3)), _dbl(np.zeros(3))
    call = L.gsr_transform_rows
    assert call(None, 0, 0, None, None, None, None, None, I, t0, 1.0, 0.0) == 0  # P = 0: nothing to do
    assert call(None, 0, 15, None, None, None, None, None, I, t0, 2.0, 1e-7) == 0
    assert call(None, 10, 15, None, None, None, None, None, I, t0, 1.0, 0.0) == -1  # all four tensors NULL
    assert call(None, -1, 0, one, None, None, None, None, I, t0, 1.0, 0.0) == -1
    for rest in (-1, 1, 2, 4, 9, 16, 24, 45):
        assert call(None, 10, rest, one, one, one, one, None, I, t0, 1.0, 0.0) == -1, rest
    assert call(None, 10, 0, one, None, None, one, None, I, t0, 1.0, 0.0) == -1  # sh_rest with rest == 0
    assert call(None, 10, 15, one, one, one, one, None, _dbl(2.0 * np.eye(3)), t0, 1.0, 0.0) == -1  # no rotation
    assert call(None, 10, 15, one, one, one, one, None, _dbl(np.diag([1.0, 2.0, 0.5])), t0, 1.0, 0.0) == -1  # non-uniform scale
    assert call(None, 10, 15, one, one, one, one, None, _dbl(np.diag([1.0, -1.0, 1.0])), t0, 1.0, 0.0) == -1  # a reflection
    assert call(None, 10, 15, one, one, one, one, None, None, t0, 1.0, 0.0) == -1
    assert call(None, 10, 15, one, one, one, one, None, I, None, 1.0, 0.0) == -1
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert call(None, 10, 15, one, one, one, one, None, I, t0, scale, 0.0) == -1, scale
    assert call(None, 10, 15, one, one, one, one, None, I, t0, 1.0, -1e-7) == -1
    assert call(None, 10, 15, ctypes.c_void_p(258), one, one, one, None, I, t0, 1.0, 0.0) == -1  # not 4-byte aligned


def test_python_layer_refuses_by_name():
    from gaussianeditor_amd import transform as T

    P = 6
    xyz, rot, scl, sh = torch.zeros(P, 3), torch.zeros(P, 4), torch.zeros(P, 3), torch.zeros(P, 15, 3)
    R = TH.random_rotation(3).numpy()
    with pytest.raises(RuntimeError, match="xyz.*no CPU fallback"):
        T.transform_rows(xyz, rot, scl, sh, rotation=R)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.transform_gaussians(type("M", (), {"_xyz": xyz, "_rotation": rot, "_scaling": scl, "_features_rest": sh})(), rotation=R)
    with pytest.raises(RuntimeError, match="rotation_raw has shape"):
        T.transform_rows(xyz, torch.zeros(P, 3), rotation=R)
    with pytest.raises(RuntimeError, match="scaling_raw has dtype"):
        T.transform_rows(xyz, rot, scl.double(), rotation=R)
    with pytest.raises(RuntimeError, match="xyz must be contiguous"):
        T.transform_rows(torch.zeros(3, P).T, rotation=R)
    with pytest.raises(RuntimeError, match="features_rest must be"):
        T.transform_rows(xyz, features_rest=torch.zeros(P, 7, 3), rotation=R)
    with pytest.raises(RuntimeError, match="mask has dtype"):
        T.transform_rows(xyz, rotation=R, mask=torch.zeros(P))
    with pytest.raises(RuntimeError, match="mask has shape"):
        T.transform_rows(xyz, rotation=R, mask=torch.zeros(P + 1, dtype=torch.bool))
    # out of scope: a ValueError, whatever the tensors are
    with pytest.raises(ValueError, match="proper rotation"):
        T.transform_rows(xyz, rotation=np.diag([1.0, 1.0, -1.0]))
    with pytest.raises(ValueError, match="non-uniform"):
        T.transform_rows(xyz, scale=[1.0, 2.0, 1.0])
    with pytest.raises(ValueError, match="positive"):
        T.transform_rows(xyz, scale=-2.0)
    with pytest.raises(ValueError, match="positive"):
        T.transform_rows(xyz, scale=0.0)
    with pytest.raises(ValueError, match="translation has shape"):
        T.transform_rows(xyz, translation=[1.0, 2.0])


@pytest.mark.parametrize("name", ["z90", "near180", "random1", "float32"])
def test_rotation_hat_and_pivot_folding(name):
    from gaussianeditor_amd import transform as T

    R = ROTATIONS[name]
    q, Rh = T.rotation_hat(R.float() if name == "float32" else R.numpy())  # (a float32 tensor, like cam.R, or an array)
    assert np.array_equal(q, TH.quat_from_matrix(R).numpy()) and q[0] >= 0.0
    assert np.array_equal(Rh, TH.rotation_hat(R).numpy())
    # orthonormal to the precision of binary64: an entry of R^ is a sum of products of the rounded unit quaternion (a few
    # eps each), an entry of R^ R^T three products of those: 16 eps bounds it with room
    assert float(np.abs(Rh @ Rh.T - np.eye(3)).max()) <= 16 * 2.0 ** -52
    t, p, s = [0.3, -1.2, 2.5], [1.5, 0.25, -0.75], 1.7
    got = T.effective_translation(R.numpy(), t, s, p)
    want = TH.effective_translation(TH.rotation_hat(R), t, s, p).numpy()
    assert float(np.abs(got - want).max()) <= 1e-15
    # the pivot is a fixed point of x -> s R^ x + t_eff - t
    assert float(np.abs(s * Rh @ np.array(p) + got - np.array(t) - np.array(p)).max()) <= 1e-14
    assert np.array_equal(T.effective_translation(None, t, 1.0, None), np.array(t))
    assert np.array_equal(T.effective_translation(None, None, 1.0, [1.0, 2.0, 3.0]), np.zeros(3))  # nothing to pivot about


def test_install_registers_a_stand_in_without_kornia_or_scipy(monkeypatch):
    import gaussianeditor_amd
    from gaussianeditor_amd import transform as T

    # (a real threestudio package on the path would be imported as the stand-in's parent: keep this test to the stand-in)
    monkeypatch.setattr(sys, "path", [p for p in sys.path if not os.path.isdir(os.path.join(p or ".", "threestudio"))])
    # the package's own install() registers what it always did, and no stand-in for threestudio
    for k in [k for k in sys.modules if k == "threestudio" or k.startswith("threestudio.")]:
        monkeypatch.delitem(sys.modules, k)
    for k in ("diff_gaussian_rasterization", "diff_gaussian_rasterization._C", "simple_knn", "simple_knn._C", "plyfile"):
        monkeypatch.delitem(sys.modules, k, raising=False)
    before = set(sys.modules)
    gaussianeditor_amd.install()
    added = {k for k in set(sys.modules) - before if not k.startswith("gaussianeditor_amd")}
    assert added == {"diff_gaussian_rasterization", "diff_gaussian_rasterization._C", "simple_knn", "simple_knn._C", "plyfile"}
    assert "threestudio.utils.transform" not in sys.modules

    # with kornia and scipy unimportable the module still imports, and install() registers the stand-in
    monkeypatch.setitem(sys.modules, "kornia", None)
    monkeypatch.setitem(sys.modules, "scipy", None)
    with pytest.raises(ImportError):
        importlib.import_module("kornia")
    try:
        importlib.reload(T)
        mod = T.install()
        monkeypatch.setitem(sys.modules, "threestudio.utils.transform", mod)  # (undone with the others at teardown)
        from threestudio.utils.transform import rotate_gaussians, scale_gaussians, translate_gaussians

        assert sys.modules["threestudio.utils.transform"] is mod
        assert rotate_gaussians is mod.rotate_gaussians and translate_gaussians is T.translate_gaussians
        assert scale_gaussians is T.scale_gaussians
        import inspect

        assert inspect.signature(rotate_gaussians).parameters["rotate_sh"].default is True
        assert inspect.signature(T.install(rotate_sh=False).rotate_gaussians).parameters["rotate_sh"].default is False
        assert inspect.signature(T.rotate_gaussians).parameters["rotate_sh"].default is False  # the reference's result
        assert "default_model_mtx" not in vars(mod)  # created on the GPU when it is first read, not here
        src = open(os.path.join(ROOT, "gaussianeditor_amd", "transform.py")).read()
        assert "import kornia" not in src and "import scipy" not in src and "from scipy" not in src and "from kornia" not in src
    finally:
        for k in [k for k in sys.modules if k == "threestudio" or k.startswith("threestudio.")]:
            sys.modules.pop(k)  # (the stubs install() made; what was there before the test comes back with undo())
        monkeypatch.undo()
        importlib.reload(T)
    assert gaussianeditor_amd.transform_rows is T.transform_rows
