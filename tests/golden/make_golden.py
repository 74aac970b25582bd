#!/usr/bin/env python3
"""Generates the golden fixtures in this directory by IMPORTING THE REFERENCE'S OWN PYTHON
modules (only possible where /root/reference exists; the fixtures themselves are committed).

    sh_eval.npz   reference `eval_sh` (gaussiansplatting/utils/sh_utils.py:57-112) on seeded inputs,
                  degrees 0..3  -> pins the oracle's SH -> RGB step (forward.cu:20-71 is the same maths)
    cameras.npz   reference `getWorld2View2` / `getProjectionMatrix` (utils/graphics_utils.py:40-87) and the
                  Simple_Camera composition (scene/cameras.py:92-95) -> pins the host-side matrix conventions
    near_points.npz  reference `K_nearest_neighbors` (gaussiansplatting/knn.py, scipy KDTree) and the reference's own
                  `GaussianModel.get_near_gaussians_by_mask` (scene/gaussian_model.py:865-898; the method's source is
                  compiled out of the reference file and run on a stub holding `_xyz`, so none of the module's GPU-only
                  imports are needed) -> pins the oracle's near_points / get_near_gaussians_by_mask
    near_method.npz  the same method of the reference on two more seeded clouds (tests/test_cpu_near.py)
    cov3d.npz     reference `build_rotation` / `build_scaling_rotation` / `strip_symmetric` (utils/general_utils.py), composed
                  as GaussianModel.setup_functions does (scene/gaussian_model.py:42-46), in float64 on the CPU, on seeded
                  unit quaternions and scales with scaling_modifier 0.5, 1 and 1.7 -> pins the 3D covariance of K1 and
                  gsr_debug_cov3d
    sh_clamped.npz  the colour the reference's renderer computes when it evaluates the SHs in Python,
                  clamp_min(eval_sh + 0.5, 0) (gaussian_renderer/__init__.py:112-118), degrees 0..3, on seeded inputs
                  whose DC term clamps a good share of the channels -> pins K1's rgb and its `clamped` flags
    reference_{render,point_cloud_render,optimizer_surgery}.npz, reference_save_ply.ply
                  the reference's render / point_cloud_render / camera2rasterizer, optimizer surgery and save_ply run as
                  written on the drop-in (tests/test_cpu_reference_modules.py holds the functions that ran them)
"""
import ast
import importlib.util
import sys as _sys

_sys.dont_write_bytecode = True  # the reference tree is read-only input: no __pycache__ there
import math
import os

import numpy as np
import torch

REF = "/root/reference/gaussiansplatting"
HERE = os.path.dirname(os.path.abspath(__file__))


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    sh_utils = load(os.path.join(REF, "utils", "sh_utils.py"), "ref_sh_utils")
    gfx = load(os.path.join(REF, "utils", "graphics_utils.py"), "ref_graphics_utils")

    g = torch.Generator().manual_seed(2024)
    P = 512
    shs = torch.randn(P, 16, 3, generator=g) * 0.4          # (P, M, 3) as the rasterizer receives them
    dirs = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    out = {"shs": shs.numpy(), "dirs": dirs.numpy()}
    for deg in range(4):
        # reference layout for eval_sh is (P, 3, M): gaussian_renderer/__init__.py:112-114
        out[f"rgb_deg{deg}"] = sh_utils.eval_sh(deg, shs.transpose(1, 2), dirs).numpy()
    np.savez(os.path.join(HERE, "sh_eval.npz"), **out)

    cams = {}
    rng = np.random.default_rng(7)
    for i in range(4):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        # world-to-camera rotation; the reference stores R = its transpose (dataset_readers.py:85)
        Rw2c = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        R = Rw2c.T
        T = rng.normal(size=3) * 2.0
        fovx, fovy = math.radians(40 + 10 * i), math.radians(30 + 7 * i)
        wv = torch.tensor(gfx.getWorld2View2(R, T, np.array([0.0, 0.0, 0.0]), 1.0)).transpose(0, 1)
        proj = gfx.getProjectionMatrix(znear=0.01, zfar=100.0, fovX=fovx, fovY=fovy).transpose(0, 1)
        full = (wv.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0)
        center = wv.inverse()[3, :3]
        cams[f"R{i}"], cams[f"T{i}"] = R, T
        cams[f"fov{i}"] = np.array([fovx, fovy])
        cams[f"world_view{i}"], cams[f"proj{i}"] = wv.numpy(), proj.numpy()
        cams[f"full_proj{i}"], cams[f"center{i}"] = full.numpy(), center.numpy()
    np.savez(os.path.join(HERE, "cameras.npz"), **cams)
    print("wrote", os.path.join(HERE, "sh_eval.npz"), os.path.join(HERE, "cameras.npz"))
    near_points_fixture()
    near_method_fixture()
    cov3d_fixture()
    sh_clamped_fixture(sh_utils)
    reference_modules_fixtures()


def reference_method(path, name, globs):
    """The function `name` of the class body in `path`, compiled from the reference's source as it lies there."""
    tree = ast.parse(open(path).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            mod = ast.Module(body=[node], type_ignores=[])
            exec(compile(mod, path, "exec"), globs)
            return globs[name]
    raise KeyError(name)


def near_points_fixture():
    knn = load(os.path.join(REF, "knn.py"), "ref_knn")
    fn = reference_method(os.path.join(REF, "scene", "gaussian_model.py"), "get_near_gaussians_by_mask",
                          {"torch": torch, "K_nearest_neighbors": knn.K_nearest_neighbors})

    class Stub:
        pass

    g = torch.Generator().manual_seed(99)
    N = 6000
    centres = torch.randn(12, 3, generator=g) * 1.5
    xyz = centres[torch.randint(0, 12, (N,), generator=g)] + torch.randn(N, 3, generator=g) * 0.35
    # the "object": three of the clusters' neighbourhoods, ragged
    mask = ((xyz - centres[0]).norm(dim=1) < 0.45) | ((xyz - centres[5]).norm(dim=1) < 0.3) | \
           ((xyz - centres[9]).norm(dim=1) < 0.5)
    xyz[7] = xyz[mask.nonzero()[0, 0]]  # a duplicate of an object point among the remaining ones: distance 0
    mask[7] = False
    out = {"xyz": xyz.numpy(), "mask": mask.numpy()}
    stub = Stub()
    stub._xyz = xyz
    for i, th in enumerate((0.1, 0.2, 0.05)):
        out[f"thresh{i}"] = np.float64(th)
        out[f"near{i}"] = fn(stub, mask.unsqueeze(1), dist_thresh=th).numpy()
    ref, qry = xyz[mask], xyz[~mask]
    _, idx, dist = knn.K_nearest_neighbors(ref, 1, query=qry, return_dist=True)
    out["nn_dist"], out["nn_idx"] = dist.numpy(), idx.numpy()
    np.savez_compressed(os.path.join(HERE, "near_points.npz"), **out)
    print("wrote", os.path.join(HERE, "near_points.npz"), {k: int(out[k].sum()) for k in ("mask", "near0", "near1", "near2")})


COV3D_MODIFIERS = (0.5, 1.0, 1.7)


def cov3d_fixture():
    """cov3d.npz: the reference's covariance composition on the CPU in float64.  Its helpers allocate with
    device="cuda" and dtype=torch.float; the shim they are compiled against allocates float64 CPU tensors instead."""
    import types

    path = os.path.join(REF, "utils", "general_utils.py")
    shim = types.SimpleNamespace(zeros=lambda *shape, dtype=None, device=None: torch.zeros(*shape, dtype=torch.float64),
                                 sqrt=torch.sqrt, float=torch.float64)
    globs = {"torch": shim}
    for name in ("strip_lowerdiag", "strip_symmetric", "build_rotation", "build_scaling_rotation"):
        reference_method(path, name, globs)
    build_cov = reference_method(os.path.join(REF, "scene", "gaussian_model.py"), "setup_functions", dict(
        torch=torch, build_scaling_rotation=globs["build_scaling_rotation"], strip_symmetric=globs["strip_symmetric"],
        inverse_sigmoid=None))

    class Stub:
        pass

    stub = Stub()
    build_cov(stub)
    g = torch.Generator().manual_seed(31)
    P = 1024
    rot = torch.nn.functional.normalize(torch.randn(P, 4, generator=g, dtype=torch.float64), dim=-1).float()
    scl = torch.exp(math.log(0.03) + 0.8 * torch.randn(P, 3, generator=g, dtype=torch.float64)).float()
    out = {"rotation": rot.numpy(), "scaling": scl.numpy(), "modifiers": np.array(COV3D_MODIFIERS)}
    for i, sm in enumerate(COV3D_MODIFIERS):
        # (the float32 inputs the kernels read, widened: the fixture is the float64 covariance of exactly those)
        out[f"cov3D_{i}"] = stub.covariance_activation(scl.double(), sm, rot.double()).numpy()
    np.savez_compressed(os.path.join(HERE, "cov3d.npz"), **out)
    print("wrote", os.path.join(HERE, "cov3d.npz"))


def sh_clamped_fixture(sh_utils):
    """sh_clamped.npz: clamp_min(eval_sh + 0.5, 0), the Python colour path of the reference's renderer."""
    g = torch.Generator().manual_seed(2025)
    P = 512
    shs = torch.randn(P, 16, 3, generator=g) * 0.4
    shs[:, 0] = torch.randn(P, 3, generator=g) * 2.0  # DC: rgb = 0.28 * dc + 0.5 + ... is negative for ~20 % of the channels
    dirs = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    out = {"shs": shs.numpy(), "dirs": dirs.numpy()}
    for deg in range(4):
        sh2rgb = sh_utils.eval_sh(deg, shs.transpose(1, 2), dirs)
        out[f"rgb_clamped_deg{deg}"] = torch.clamp_min(sh2rgb + 0.5, 0.0).numpy()
        out[f"rgb_deg{deg}"] = sh2rgb.numpy()
    np.savez_compressed(os.path.join(HERE, "sh_clamped.npz"), **out)
    print("wrote", os.path.join(HERE, "sh_clamped.npz"))


NEAR_METHOD_CASES = ((2000, 0.1), (5000, 0.04))


def near_method_inputs():
    """-> [(xyz, mask, dist_thresh)] of near_method.npz: seeded, regenerated by tests/test_cpu_near.py."""
    rng = np.random.default_rng(5)
    cases = []
    for n, th in NEAR_METHOD_CASES:
        xyz = (rng.standard_normal((n, 3)) * 0.6).astype(np.float32)
        cases.append((xyz, np.linalg.norm(xyz, axis=1) < 0.5, th))
    return cases


def near_method_fixture():
    """near_method.npz: the reference's `get_near_gaussians_by_mask` on the seeded clouds of near_method_inputs()."""
    knn = load(os.path.join(REF, "knn.py"), "ref_knn")
    fn = reference_method(os.path.join(REF, "scene", "gaussian_model.py"), "get_near_gaussians_by_mask",
                          {"torch": torch, "K_nearest_neighbors": knn.K_nearest_neighbors})
    out = {}
    for i, (xyz, mask, th) in enumerate(near_method_inputs()):
        class Stub:
            _xyz = torch.from_numpy(xyz)

        out[f"near{i}"] = fn(Stub(), torch.from_numpy(mask)[:, None], dist_thresh=th).numpy()
    np.savez_compressed(os.path.join(HERE, "near_method.npz"), **out)
    print("wrote", os.path.join(HERE, "near_method.npz"), {k: int(v.sum()) for k, v in out.items()})


def reference_modules_fixtures():
    """reference_{render,point_cloud_render,optimizer_surgery}.npz + reference_save_ply.ply: the reference's render / point_cloud_render / camera2rasterizer,
    GaussianModel.cat_tensors_to_optimizer / _prune_optimizer and GaussianModel.save_ply, imported unmodified after
    gaussianeditor_amd.install() and run on the drop-in (native calls routed to the oracle, tests/oracle_backend.py) by the
    functions of tests/test_cpu_reference_modules.py."""
    import pytest

    tests = os.path.dirname(HERE)
    for p in (os.path.dirname(tests), tests):
        if p not in _sys.path:
            _sys.path.insert(0, p)
    import oracle_backend
    import test_cpu_reference_modules as T

    import gaussianeditor_amd
    from oracle import cpu

    cpu.build()
    gaussianeditor_amd.install()
    with pytest.MonkeyPatch.context() as mp:
        mp.syspath_prepend(os.path.dirname(REF))
        import gaussiansplatting.gaussian_renderer as ref_renderer  # the reference's file, unmodified
        from gaussiansplatting.scene.gaussian_model import GaussianModel

        assert ref_renderer.GaussianRasterizer is _sys.modules["gaussianeditor_amd.diff_gaussian_rasterization"].GaussianRasterizer
        T.cpu_zeros_like(mp)
        oracle_backend.install(mp)
        out = T.render_outputs(ref_renderer.render, ref_renderer.camera2rasterizer)
        out.update(T.point_cloud_outputs(ref_renderer.point_cloud_render))
        out.update(T.surgery_outputs(GaussianModel.cat_tensors_to_optimizer, GaussianModel._prune_optimizer))
        gm = GaussianModel.__new__(GaussianModel)
        for k, t in T.ply_model().items():
            setattr(gm, k, t)
        gm.save_ply(T.PLY_FIXTURE)
    for path, prefixes in T.FIXTURES.items():
        np.savez_compressed(path, **{k: v for k, v in out.items() if k.startswith(prefixes)})
    assert all(k.startswith(sum(T.FIXTURES.values(), ())) for k in out)  # (every array went into one of the files)
    print("wrote", *T.FIXTURES, T.PLY_FIXTURE)


if __name__ == "__main__":
    main()
