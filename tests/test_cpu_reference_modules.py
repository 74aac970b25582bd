"""CPU: what the REFERENCE'S OWN Python modules returned when they were imported unmodified after
`gaussianeditor_amd.install()` and executed against the drop-in -- recorded by tests/golden/make_golden.py (which needs the
reference checkout) in tests/golden/reference_{render,point_cloud_render,optimizer_surgery}.npz and
tests/golden/reference_save_ply.ply -- against the mirror and the oracle.

  * gaussiansplatting/gaussian_renderer/__init__.py (`render` :45-150, `camera2rasterizer` :21-42) ran on the drop-in's L1
    API; the mirror gaussianeditor_amd/gaussian_renderer.py returns the same bits, and both equal the oracle (SURVEY.md
    row a1: the L2 boundary itself, not a restatement of it);
  * gaussiansplatting/scene/gaussian_model.py imported (it needs `simple_knn._C` and `plyfile` at import time: the shims),
    and its optimizer surgery -- `cat_tensors_to_optimizer` :609-641, `_prune_optimizer` :568-591 -- run as written pins
    the numpy restatements (`oracle.cpu.append_rows` / `compact_rows`) that the GPU tests check the HIP kernels against;
    its `save_ply` wrote the file that scene_ply reads and writes byte for byte.

The native library is replaced by the oracle stand-in (tests/oracle_backend.py), here and when the fixtures were recorded;
`torch.zeros_like(..., device="cuda")` in the reference's render() was redirected to the CPU.  The functions below that
take the renderer / the model class are the ones make_golden.py ran on the reference's modules.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle_backend
from helpers import make_case, oracle_backward, oracle_forward, rel_err, seed_gradient

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# fixture file -> the prefixes of the arrays it holds (one file per test: each stays far below the size limit of a file)
FIXTURES = {os.path.join(GOLD, "reference_render.npz"): ("render_", "override_", "apply_weights_"),
            os.path.join(GOLD, "reference_point_cloud_render.npz"): ("pcr_",),
            os.path.join(GOLD, "reference_optimizer_surgery.npz"): ("cat_", "prune_")}
PLY_FIXTURE = os.path.join(GOLD, "reference_save_ply.ply")
GETTERS = (("get_xyz", "dL_dmeans3D"), ("get_features", "dL_dsh"), ("get_opacity", "dL_dopacity"),
           ("get_scaling", "dL_dscales"), ("get_rotation", "dL_drotations"))
OUT_KEYS = ("render", "depth_3dgs", "radii", "visibility_filter")


def cpu_zeros_like(monkeypatch):
    """The reference hard-codes device="cuda" in zeros_like (gaussian_renderer/__init__.py:62): keep it on the CPU."""
    real = torch.zeros_like

    def zeros_like_on_cpu(t, *a, **kw):
        kw.pop("device", None)
        return real(t, *a, **kw)

    monkeypatch.setattr(torch, "zeros_like", zeros_like_on_cpu)


class _PC:
    """Duck-typed GaussianModel getters (scene/gaussian_model.py:221-258)."""

    def __init__(self, sc):
        self._sc = {k: v.clone().requires_grad_(True) for k, v in sc.items() if isinstance(v, torch.Tensor) and k != "bg"}
        self.active_sh_degree = 3
        self.max_sh_degree = 3

    get_xyz = property(lambda s: s._sc["xyz"])
    get_opacity = property(lambda s: s._sc["opacity"])
    get_scaling = property(lambda s: s._sc["scaling"])
    get_rotation = property(lambda s: s._sc["rotation"])
    get_features = property(lambda s: s._sc["features"])


def render_case():
    case = make_case(3000, 96, 64, seed=3, s0=0.05)
    G = seed_gradient(64, 96, 2) * 64 * 96
    mask = (torch.rand(3000, 1, generator=torch.Generator().manual_seed(1)) > 0.5).float().repeat(1, 3)
    m = (torch.rand(1, 64, 96, generator=torch.Generator().manual_seed(2)) > 0.3).float()
    return case, G, mask, m


def render_outputs(render, camera2rasterizer):
    """`render` (+ backward of <image, G>), `render(override_color=...)` and camera2rasterizer(...).apply_weights as
    GaussianModel.apply_weights calls them (scene/gaussian_model.py:817-832) on the fixed case -> numpy arrays."""
    case, G, mask, m = render_case()
    pipe = SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    pc = _PC(case["sc"])
    out = render(case["cam"], pc, pipe, case["bg"])
    (out["render"] * G).sum().backward()
    res = {"render_keys": np.array(sorted(out))}
    res.update({f"render_{k}": out[k].detach().numpy() for k in OUT_KEYS})
    res.update({f"render_grad_{getter}": getattr(pc, getter).grad.numpy() for getter, _ in GETTERS})
    res["render_grad_viewspace_points"] = out["viewspace_points"].grad.numpy()
    # override_color and SH evaluated in Python.  (pipe.convert_SHs_python=True cannot be exercised through the reference:
    # its render() dereferences `shs = None` at gaussian_renderer/__init__.py:125; the mirror keeps that path working and is
    # tested on its own)
    res["override_render"] = render(case["cam"], _PC(case["sc"]), pipe, case["bg"], override_color=mask)["render"].detach().numpy()
    w, cnt = torch.zeros(3000, 1), torch.zeros(3000, 1, dtype=torch.int32)
    sc = case["sc"]
    camera2rasterizer(case["cam"], torch.zeros(3)).apply_weights(sc["xyz"], None, sc["opacity"], None, w, sc["scaling"],
                                                                 sc["rotation"], None, cnt, m)
    res["apply_weights_w"], res["apply_weights_cnt"] = w.numpy(), cnt.numpy()
    return res


def point_cloud_outputs(point_cloud_render):
    """`point_cloud_render` (gaussian_renderer/__init__.py:156-250, imported by webui.py:39) + backward -> numpy arrays."""
    case = make_case(2000, 80, 48, seed=5, s0=0.05)
    G = seed_gradient(48, 80, 1) * 48 * 80
    xyz = case["sc"]["xyz"].clone().requires_grad_(True)
    out = point_cloud_render(case["cam"], xyz, None, case["bg"])
    (out["render"] * G).sum().backward()
    res = {"pcr_keys": np.array(sorted(out))}
    res.update({f"pcr_{k}": out[k].detach().numpy() for k in OUT_KEYS})
    res["pcr_grad_xyz"], res["pcr_grad_viewspace_points"] = xyz.grad.numpy(), out["viewspace_points"].grad.numpy()
    return res


def _adam_with_state(P, seed):
    gen = torch.Generator().manual_seed(seed)
    shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, 15, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
    params = {k: torch.nn.Parameter(torch.randn(s, generator=gen)) for k, s in shapes.items()}
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-3, "name": k} for k, p in params.items()], lr=0.0, eps=1e-15)
    for p in params.values():
        p.grad = torch.randn(p.shape, generator=gen)
    opt.step()
    return opt, gen


def _state(opt):
    return {g["name"]: (g["params"][0].detach().clone(), opt.state[g["params"][0]]["exp_avg"].clone(),
                        opt.state[g["params"][0]]["exp_avg_sq"].clone()) for g in opt.param_groups}


SURGERY_P, SURGERY_N = 257, 19


def surgery_inputs():
    """-> (densify: Adam, its state before, the rows to append), (prune: Adam, its state before, keep mask)."""
    opt, gen = _adam_with_state(SURGERY_P, 5)
    before = _state(opt)
    ext = {g["name"]: torch.randn((SURGERY_N,) + tuple(g["params"][0].shape[1:]), generator=gen) for g in opt.param_groups}
    opt2, gen2 = _adam_with_state(SURGERY_P, 6)
    before2 = _state(opt2)
    keep = torch.rand(SURGERY_P, generator=gen2) > 0.3
    return (opt, before, ext), (opt2, before2, keep)


def surgery_outputs(cat_tensors_to_optimizer, prune_optimizer):
    """GaussianModel.cat_tensors_to_optimizer / _prune_optimizer as written, called on a bare object that only carries
    `optimizer` -> parameter, exp_avg and exp_avg_sq of every group after the call, and whether the returned tensors are
    the optimizer's parameters."""
    (opt, _, ext), (opt2, _, keep) = surgery_inputs()
    res = {}
    for tag, o, fn, arg in (("cat", opt, cat_tensors_to_optimizer, ext), ("prune", opt2, prune_optimizer, keep)):
        new = fn(SimpleNamespace(optimizer=o), arg)
        res[f"{tag}_returns_params"] = np.array(all(new[g["name"]] is g["params"][0] for g in o.param_groups))
        for k, (p, m, v) in _state(o).items():
            res[f"{tag}_{k}_param"], res[f"{tag}_{k}_exp_avg"], res[f"{tag}_{k}_exp_avg_sq"] = p.numpy(), m.numpy(), v.numpy()
    return res


def ply_model():
    """The 50-Gaussian model whose save_ply output is tests/golden/reference_save_ply.ply."""
    P = 50
    gen = torch.Generator().manual_seed(4)
    return {"_xyz": torch.randn(P, 3, generator=gen), "_features_dc": torch.randn(P, 1, 3, generator=gen),
            "_features_rest": torch.randn(P, 15, 3, generator=gen), "_opacity": torch.randn(P, 1, generator=gen),
            "_scaling": torch.randn(P, 3, generator=gen), "_rotation": torch.randn(P, 4, generator=gen)}


@pytest.fixture(scope="module")
def recorded():
    out = {}
    for path in FIXTURES:
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


@pytest.fixture()
def drop_in(monkeypatch):
    import gaussianeditor_amd

    gaussianeditor_amd.install()
    cpu_zeros_like(monkeypatch)


def test_reference_render_runs_on_the_drop_in(oracle, monkeypatch, drop_in, recorded):
    from gaussianeditor_amd import gaussian_renderer as mirror

    oracle_backend.install(monkeypatch)
    got = render_outputs(mirror.render, mirror.camera2rasterizer)
    want = {k: v for k, v in recorded.items() if k in got}
    assert set(want) == set(got)
    assert set(want["render_keys"]) == {"render", "viewspace_points", "visibility_filter", "radii", "depth_3dgs"}
    for k in got:  # the mirror returns what the reference's render() returned, bit for bit
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    case, G, mask, m = render_case()
    f = oracle_forward(oracle, case)
    g = oracle_backward(oracle, case, f, G)
    assert np.array_equal(want["render_render"], f["color"]) and np.array_equal(want["render_radii"], f["radii"])
    for getter, key in GETTERS:
        ga = want[f"render_grad_{getter}"]
        assert rel_err(ga, g[key].reshape(ga.shape)) < 1e-6, getter
    assert rel_err(want["render_grad_viewspace_points"], g["dL_dmeans2D"]) < 1e-6
    assert np.array_equal(want["override_render"], oracle_forward(oracle, case, colors_precomp=mask)["color"])
    w2, c2 = np.zeros((3000, 1), np.float32), np.zeros(3000, np.int32)
    sc, cam = case["sc"], case["cam"]
    oracle.apply_weights(sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], None, cam.world_view_transform,
                         cam.full_proj_transform, cam.camera_center, 96, 64, case["tfx"], case["tfy"], m, w2, c2)
    assert np.array_equal(want["apply_weights_cnt"].reshape(-1), c2) and np.array_equal(want["apply_weights_w"], w2)


def test_reference_point_cloud_render_equals_the_mirror(oracle, monkeypatch, drop_in, recorded):
    """`point_cloud_render`: the reference's own function on the drop-in against the mirror's, outputs and the gradient of
    the screen-space points bit for bit."""
    from gaussianeditor_amd import gaussian_renderer as mirror

    oracle_backend.install(monkeypatch)
    got = point_cloud_outputs(mirror.point_cloud_render)
    want = {k: v for k, v in recorded.items() if k in got}
    assert set(want) == set(got)
    assert set(want["pcr_keys"]) == {"render", "viewspace_points", "visibility_filter", "radii", "depth_3dgs"}
    for k in got:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert int(want["pcr_visibility_filter"].sum()) > 100 and float(want["pcr_render"].max()) > 0.5


def test_reference_optimizer_surgery_pins_the_restatements(oracle, recorded):
    """GaussianModel.cat_tensors_to_optimizer / _prune_optimizer, the reference's methods as written, against
    oracle.cpu.append_rows / compact_rows."""
    (opt, before, ext), (opt2, before2, keep) = surgery_inputs()
    assert bool(recorded["cat_returns_params"]) and bool(recorded["prune_returns_params"])
    for g in opt.param_groups:  # --- densify
        k = g["name"]
        want_p, want_m, want_v = oracle.append_rows([t.numpy() for t in before[k]], [ext[k].numpy(), None, None], SURGERY_N)
        assert recorded[f"cat_{k}_param"].shape[0] == SURGERY_P + SURGERY_N
        assert np.array_equal(recorded[f"cat_{k}_param"], want_p)
        assert np.array_equal(recorded[f"cat_{k}_exp_avg"], want_m)
        assert np.array_equal(recorded[f"cat_{k}_exp_avg_sq"], want_v)
    for g in opt2.param_groups:  # --- prune
        k = g["name"]
        want = oracle.compact_rows([t.numpy() for t in before2[k]], keep.numpy())
        assert np.array_equal(recorded[f"prune_{k}_param"], want[0])
        assert np.array_equal(recorded[f"prune_{k}_exp_avg"], want[1])
        assert np.array_equal(recorded[f"prune_{k}_exp_avg_sq"], want[2])


def test_reference_model_loads_and_saves_through_the_shims(drop_in, tmp_path):
    """GaussianModel.save_ply (scene/gaussian_model.py:396-445), the reference's own writer, wrote
    tests/golden/reference_save_ply.ply through whichever `plyfile` install() registered (compat/plyfile.py); read back
    with the same package.  (__init__ and load_ply put tensors on "cuda": the object was created bare.)"""
    gm = ply_model()
    from plyfile import PlyData  # whichever `plyfile` install() left in sys.modules

    el = PlyData.read(PLY_FIXTURE).elements[0]
    P = gm["_xyz"].shape[0]
    assert len(el["x"]) == P and np.allclose(np.asarray(el["x"]), gm["_xyz"][:, 0].numpy())
    assert np.allclose(np.asarray(el["f_rest_44"]), gm["_features_rest"].transpose(1, 2).flatten(start_dim=1)[:, 44].numpy())
    assert np.allclose(np.asarray(el["rot_3"]), gm["_rotation"][:, 3].numpy())
    # the one-command asset path (gaussianeditor_amd/scene_ply.py, bench.py --ply): what the reference's writer wrote comes
    # back, tensor for tensor, in the shapes load_ply (:455-533) produces; and a file written by scene_ply is byte-identical
    from gaussianeditor_amd import scene_ply

    back = scene_ply.load_gaussians_ply(PLY_FIXTURE)
    for k, t in (("xyz", gm["_xyz"]), ("f_dc", gm["_features_dc"]), ("f_rest", gm["_features_rest"]),
                 ("opacity", gm["_opacity"]), ("scaling", gm["_scaling"]), ("rotation", gm["_rotation"])):
        assert torch.equal(back[k], t), k
    assert back["max_sh_degree"] == 3
    mine = str(tmp_path / "pc" / "mine.ply")
    os.makedirs(os.path.dirname(mine), exist_ok=True)
    scene_ply.save_gaussians_ply(mine, gm["_xyz"], gm["_features_dc"], gm["_features_rest"], gm["_opacity"], gm["_scaling"],
                                 gm["_rotation"])
    assert open(mine, "rb").read() == open(PLY_FIXTURE, "rb").read()
