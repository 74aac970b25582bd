"""Camera pose gradients (opt-in, gaussianeditor_amd.set_pose_grad; include/gsr.h gsr_pose_backward) without a GPU: the
pose helper against the reference fixture, the switch and its per-thread override, the binding-only bit, argument
validation of the two entry points, and the yardstick of the GPU tests -- float64 autograd with the camera tensors as
leaves -- against the translation identity (pose_helpers)."""
import ctypes
import os
import threading

import numpy as np
import pytest
import torch

import pose_helpers as PH
from helpers import oracle_forward, seed_gradient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ctypes.c_void_p(256)
ACC = ctypes.c_void_p(1 << 12)  # (64-byte aligned)
POSE = 65536


def test_camera_tensors_match_the_reference_fixture():
    """pose.camera_tensors on the (R, T, projection) of tests/golden/cameras.npz: the reference's world_view_transform,
    full_proj_transform and camera_center.  Evaluated in float64 and compared with the float32 fixture within 4 float32
    roundings of each tensor's largest entry (the fixture's product and inverse were rounded in float32); the view matrix,
    which is a placement of the inputs, exactly in float32."""
    from gaussianeditor_amd.pose import camera_tensors

    g = np.load(os.path.join(ROOT, "tests", "golden", "cameras.npz"))
    eps = 4 * 2.0 ** -24
    for i in range(4):
        R, T, proj = torch.from_numpy(g[f"R{i}"]), torch.from_numpy(g[f"T{i}"]), torch.from_numpy(g[f"proj{i}"]).double()
        view, full, center = camera_tensors(R, T, proj)
        assert view.dtype == torch.float64 and view.shape == (4, 4) and full.shape == (4, 4) and center.shape == (3,)
        for got, name in ((view, "world_view"), (full, "full_proj"), (center, "center")):
            want = g[f"{name}{i}"].astype(np.float64)
            assert np.abs(got.numpy() - want).max() <= eps * np.abs(want).max(), (i, name)
        v32 = camera_tensors(R.float(), T.float(), proj.float())[0]
        assert v32.dtype == torch.float32 and np.array_equal(v32.numpy(), g[f"world_view{i}"])
    # differentiable: a translation of the camera reaches all three tensors
    R, T = torch.from_numpy(g["R0"]), torch.from_numpy(g["T0"]).clone().requires_grad_(True)
    view, full, center = camera_tensors(R, T, torch.from_numpy(g["proj0"]).double())
    (view.sum() + full.sum() + center.sum()).backward()
    assert T.grad is not None and np.abs(T.grad.numpy()).min() > 0
    with pytest.raises(ValueError):
        camera_tensors(torch.eye(4), torch.zeros(3), torch.eye(4))


def test_flag_value_setter_and_per_thread_override():
    import gaussianeditor_amd
    from gaussianeditor_amd import options

    assert options.FLAG_POSE_GRAD == POSE and options.FLAG_ALL & options.FLAG_POSE_GRAD
    assert not gaussianeditor_amd.get_pose_grad() and options.current_flags() == 0
    gaussianeditor_amd.set_pose_grad(True)
    gaussianeditor_amd.set_antialiasing(True)
    try:
        assert gaussianeditor_amd.get_pose_grad()
        assert options.current_flags() == options.FLAG_POSE_GRAD | options.FLAG_ANTIALIAS
        gaussianeditor_amd.set_pose_grad(False)
        assert not gaussianeditor_amd.get_pose_grad() and options.current_flags() == options.FLAG_ANTIALIAS
    finally:
        gaussianeditor_amd.set_pose_grad(False)
        gaussianeditor_amd.set_antialiasing(False)
    assert options.current_flags() == 0
    seen = {}
    with options.override(options.FLAG_POSE_GRAD):
        assert options.current_flags() == POSE and not gaussianeditor_amd.get_pose_grad()
        t = threading.Thread(target=lambda: seen.setdefault("other", options.current_flags()))
        t.start()
        t.join()
    assert seen["other"] == 0 and options.current_flags() == 0
    # unknown bits still raise, next to the new one too
    for bad in (128, 256, 512, 2048, 8192, 32768, 131072, POSE | 2048, POSE | 32768):
        with pytest.raises(ValueError):
            options.set_default_flags(bad)
        with pytest.raises(ValueError):
            with options.override(bad):
                pass


def test_binding_keeps_the_bit_to_itself_and_the_library_refuses_it():
    from gaussianeditor_amd import _native, options
    from gaussianeditor_amd.diff_gaussian_rasterization import _C, _reuse

    assert _C._flags(options.FLAG_POSE_GRAD) == 0
    assert _C._flags(options.FLAG_POSE_GRAD | options.FLAG_ANTIALIAS | options.FLAG_DEPTH_GRAD) == options.FLAG_ANTIALIAS
    with options.override(options.FLAG_POSE_GRAD | options.FLAG_FAST_EXP):
        assert _C._flags(None) == options.FLAG_FAST_EXP
    assert _reuse._IGNORED_FLAGS & options.FLAG_POSE_GRAD  # (the state a render leaves is the same)
    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "#define GSR_ABI_VERSION 6" in hdr and "#define GSR_FLAG_ALL (127u | GSR_FLAG_ANTIALIAS)" in hdr
    assert "65536" not in hdr  # (no library bit)
    for name in ("gsr_pose_workspace_size", "gsr_pose_backward"):
        assert f"int {name}(" in hdr and name in _native.SIGNATURES and hasattr(_native.lib(), name)
    L = _native.lib()
    r = (ctypes.c_int64 * 2)()
    assert L.gsr_blend_forward(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ONE, POSE) == -1
    assert L.gsr_blend_backward(None, 10, 0, 64, 64, ONE, ONE, ONE, ONE, ONE, ACC, None, POSE) == -1
    assert L.gsr_preprocess(None, 10, 3, 16, ONE, ONE, 1.0, ONE, ONE, ONE, None, None, ONE, ONE, ONE, 64, 64, 1.0, 1.0, 0, 0,
                            POSE, ONE, ONE, r) == -1
    assert L.gsr_preprocess_backward(None, 10, 3, 16, 64, 64, ONE, ONE, ONE, 1.0, ONE, None, ONE, ONE, ONE, 1.0, 1.0, ONE, ONE,
                                     ACC, ONE, ONE, None, ONE, None, ONE, ONE, ONE, POSE) == -1


def test_render_without_the_flag_or_without_a_learnable_camera_adds_no_inputs():
    """`_pose_inputs` decides the arity of the autograd call: () unless the flag is on AND a camera tensor requires a
    gradient."""
    from gaussianeditor_amd import options
    from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, _pose_inputs

    def rs(grad):
        V = torch.eye(4, requires_grad=grad)
        return GaussianRasterizationSettings(32, 32, 1.0, 1.0, torch.zeros(3), 1.0, V, torch.eye(4), 0, torch.zeros(3), False, False)
    assert _pose_inputs(rs(True)) == () and _pose_inputs(rs(False)) == ()
    with options.override(options.FLAG_POSE_GRAD):
        assert _pose_inputs(rs(False)) == ()
        s = rs(True)
        got = _pose_inputs(s)
        assert len(got) == 3 and got[0] is s.viewmatrix and got[1] is s.projmatrix and got[2] is s.campos


def test_entry_points_validate_arguments_without_a_gpu():
    """No call here reaches the device: everything is refused before a kernel or a memset is issued."""
    from gaussianeditor_amd import _native

    L = _native.lib()
    sz = ctypes.c_size_t(0)
    ws = L.gsr_pose_workspace_size
    assert ws(0, ctypes.byref(sz)) == 0 and sz.value == 128  # one row of 32 floats
    assert ws(1, ctypes.byref(sz)) == 0 and sz.value == 128
    assert ws(257, ctypes.byref(sz)) == 0 and sz.value == 2 * 128
    assert ws(300_000, ctypes.byref(sz)) == 0 and sz.value == 1024 * 128  # capped: the kernel strides beyond 1024 blocks
    assert ws(-1, ctypes.byref(sz)) == -1 and ws(10, None) == -1

    def call(P=10, D=3, M=16, W=64, H=64, means=ONE, scales=ONE, rots=ONE, cov=None, view=ONE, proj=ONE, campos=ONE, radii=ONE,
             geom=ONE, acc=ACC, wsp=ONE, out=ONE, flags=0):
        return L.gsr_pose_backward(None, P, D, M, W, H, means, scales, 1.0, rots, cov, view, proj, campos, 1.0, 1.0, radii, geom,
                                   acc, wsp, out, flags)
    # flags: the depth and antialiasing bits and nothing else
    for bad in (1, 2, 4, 8, 16, 32, 128, 256, 512, 2048, 4096, 8192, 16384, 32768, POSE, 64 | 4096):
        assert call(flags=bad) == -1, bad
        assert call(P=0, flags=bad) == -1, bad
    assert call(P=-1) == -1 and call(out=None) == -1 and call(P=0, out=None) == -1 and call(out=ctypes.c_void_p(258)) == -1
    assert call(W=0) == -1 and call(H=-4) == -1 and call(D=4) == -1 and call(D=-1) == -1 and call(M=-1) == -1
    assert call(D=3, M=9) == -1  # fewer coefficients than the degree needs
    assert call(means=None) == -1 and call(view=None) == -1 and call(proj=None) == -1 and call(radii=None) == -1
    assert call(geom=None) == -1 and call(geom=ctypes.c_void_p(256 + 16)) == -1
    assert call(campos=None) == -1  # SH colours need the camera centre ...
    assert call(acc=None) == -1 and call(acc=ctypes.c_void_p(4096 + 16)) == -1
    assert call(wsp=None) == -1 and call(wsp=ctypes.c_void_p(256 + 4)) == -1
    assert call(scales=None) == -1 and call(rots=None) == -1  # neither a covariance nor what it is computed from


def test_float64_expectation_satisfies_the_translation_identity():
    """The yardstick checks itself: raw partials out of render_f64 with V, PV, C as float64 leaves, composed by autograd
    through the moved-camera construction, equal - sum dL/dmu to 1e-12 of sum |dL/dmu| (measured: 4e-16)."""
    from oracle import cpu
    from oracle.torch_ref import render_f64

    cpu.build()
    case = PH.identity_case()
    H, W = case["H"], case["W"]
    G = seed_gradient(H, W, 19) * H * W
    f = oracle_forward(cpu, case)
    assert int((f["radii"] > 0).sum()) > 200
    sc, d = case["sc"], torch.float64
    xyz = sc["xyz"].to(d).clone().requires_grad_(True)
    c, V, PV, C = PH.moved_camera(case["cam"], d)
    # the construction reproduces the camera
    assert np.abs(V.detach().numpy() - case["cam"].world_view_transform.double().numpy()).max() < 1e-6
    assert np.abs(PV.detach().numpy() - case["cam"].full_proj_transform.double().numpy()).max() < 1e-6
    render_f64(f, xyz, None, sc["opacity"].to(d), sc["scaling"].to(d), sc["rotation"].to(d), sc["features"].to(d), None, None,
               V, PV, C, case["bg"], W, H, case["tfx"], case["tfy"], 1.0, 3, dL_dimage=G.to(d))
    PH.assert_identity(c.grad.numpy(), xyz.grad.numpy(), "float64 self-check", tol=1e-12)
