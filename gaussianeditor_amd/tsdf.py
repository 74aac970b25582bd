"""TSDF fusion of rendered depth on the GPU and the mesh of the fused surface (the mathematics is
stated at the gsr_tsdf_* entry points of include/gsr.h, the kernels are csrc/gsr_tsdf.hip).  What 2DGS, GOF and gsplat hand
to Open3D's TSDF fusion after training with the normal-consistency and distortion losses: depth maps in, a mesh out.

    vol = TSDFVolume(origin=(-1, -1, -1), voxel_size=2 / 255, dims=(256, 256, 256), trunc=4 * 2 / 255)
    pkgs = [render(cam, gaussians, pipe, bg, return_alpha=True) for cam in cameras]
    vol.integrate_renders(pkgs, cameras)                 # one launch for all views
    vertices, faces, colors = vol.extract_mesh()         # (Nv,3) f32, (Nf,3) i32, (Nv,3) f32 | None
    save_mesh_ply("scene.ply", vertices, faces, colors)

  * The volume is dense: `tsdf` (nx,ny,nz) float32, 1 when fresh, `weight` (nx,ny,nz) float32, 0 when fresh, and with
    `with_color` `color` (3,nx,ny,nz) float32.  Lattice point (i,j,k) sits at origin + voxel_size (i,j,k).  origin and
    voxel_size are rounded to float32 once, here.
  * `integrate` fuses V views, in order, in ONE launch: every lattice point is projected into every view (binary64), takes
    the depth of the nearest pixel (`depth / alpha` where alpha is given: `depth_3dgs` is alpha-weighted), and averages the
    truncated signed distance min(1, (depth - z) / trunc) with weight 1 per view (binary32).  A call with V views gives the
    bits of V calls with one view.
  * `extract_mesh` is marching tetrahedra on the same lattice (six Kuhn tetrahedra per cube): watertight by construction
    wherever the surface is surrounded by observed points, every normal towards the positive side, vertices shared through
    their lattice edge.  Two phases as the forward's num_rendered: a count with one small host read-back, then the fill.

Every tensor is allocated by torch; every result is the same bits on every run.  There is no CPU fallback and no
torch-operator fallback.  Out of scope: hashed or block-sparse volumes, marching cubes, mesh cleaning, decimation and
texturing, off-centre principal points, and gradients through any of it.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from .filter3d import CAMERA_DOUBLES, PackedCameras, camera_records
from .normals import _check, _check_devices, _ptr, _stream

__all__ = ["TSDFVolume", "extract_mesh", "save_mesh_ply", "load_mesh_ply", "BLOCK_DIMS", "CAMERAS_PER_CHUNK",
           "MESH_ROWS_PER_BLOCK", "MAX_MESH_POINTS"]

#: lattice points (x, y, z) one block of the integration owns, cameras one LDS stage holds, lattice points one block of the
#: mesh kernels scans (gsr_tsdf.hip: TS_BX / TS_BY / TS_BZ, TS_CHUNK, MT_ROWS); the tests size their cases around them
BLOCK_DIMS = (2, 4, 32)
CAMERAS_PER_CHUNK = 32
MESH_ROWS_PER_BLOCK = 1024
#: the largest lattice a mesh is extracted from: the vertex keys 7 n + kind are 31-bit
MAX_MESH_POINTS = (2 ** 31 - 1) // 7
_MAX_POINTS = 2 ** 31 - 1


def _check_dims(what: str, dims) -> Tuple[int, int, int]:
    try:
        d = tuple(int(x) for x in dims)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: dims must be three integers, got {dims!r}") from None
    if len(d) != 3 or any(x < 1 for x in d) or any(int(x) != x for x in dims):
        raise ValueError(f"{what}: dims must be three integers of at least 1, got {dims!r}")
    if d[0] * d[1] * d[2] > _MAX_POINTS:
        raise ValueError(f"{what}: dims {d} hold more than 2^31 - 1 lattice points")
    return d


def _check_origin(what: str, origin) -> Tuple[float, float, float]:
    try:
        o = tuple(float(np.float32(x)) for x in origin)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: origin must be three numbers, got {origin!r}") from None
    if len(o) != 3 or not all(math.isfinite(x) for x in o):
        raise ValueError(f"{what}: origin must be three finite numbers, got {origin!r}")
    return o


def _check_positive(what: str, name: str, v, single: bool = False) -> float:
    try:
        x = float(np.float32(v)) if single else float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be a number, got {v!r}") from None
    if not (math.isfinite(x) and x > 0.0):
        raise ValueError(f"{what}: {name} must be finite and positive, got {v!r}")
    return x


def _check_mesh_points(what: str, dims) -> None:
    if dims[0] * dims[1] * dims[2] > MAX_MESH_POINTS:
        raise ValueError(f"{what}: dims {tuple(dims)} hold more than {MAX_MESH_POINTS} lattice points (7 nx ny nz must stay "
                         "below 2^31: the vertex keys are 31-bit)")


def _is_camera(c) -> bool:
    return hasattr(c, "world_view_transform") and hasattr(c, "image_width")


class TSDFVolume:
    """A dense truncated-signed-distance volume (module docstring).  `origin`: the position of lattice point (0,0,0);
    `voxel_size`: the lattice spacing; `dims` = (nx, ny, nz) lattice points; `trunc`: the truncation distance in world units
    (a few voxels).  The tensors `tsdf`, `weight`, `color` are plain attributes: they may be read, saved, or assigned."""

    def __init__(self, origin, voxel_size, dims, trunc, with_color: bool = True, device="cuda"):
        what = "TSDFVolume"
        self.dims = _check_dims(what, dims)
        self.origin = _check_origin(what, origin)
        self.voxel_size = _check_positive(what, "voxel_size", voxel_size, single=True)
        self.trunc = _check_positive(what, "trunc", trunc)
        self.with_color = bool(with_color)
        self.device = torch.device(device)
        self.tsdf = self.weight = self.color = None
        self.reset()

    def reset(self) -> None:
        """A fresh volume: tsdf 1, weight 0, colour 0 (new tensors)."""
        self.tsdf = torch.ones(self.dims, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
        self.color = torch.zeros((3,) + self.dims, dtype=torch.float32, device=self.device) if self.with_color else None

    def _check_state(self, what: str) -> None:
        _check(what, "tsdf", self.tsdf, self.dims)
        _check(what, "weight", self.weight, self.dims)
        if self.color is not None:
            _check(what, "color", self.color, (3,) + self.dims)

    def integrate(self, depth: torch.Tensor, cameras, alpha: Optional[torch.Tensor] = None,
                  color: Optional[torch.Tensor] = None, alpha_min: float = 0.5, max_weight: float = 0.0) -> None:
        """Fuses V views, in order, in one launch.  depth (V,1,H,W) or one view (1,H,W); alpha | None the same shape: where
        given, depth is divided by it (`depth_3dgs` / `alpha` is the expected depth) and pixels with alpha < alpha_min are
        skipped; color (V,3,H,W) or (3,H,W), required exactly when the volume has colour.  All float32, contiguous, on the
        volume's device.  `cameras`: one camera, a list as `pack_cameras` accepts (its image sizes are checked against the
        depth's), or a `PackedCameras` (its image sizes are NOT checked: the W and H of the depth hold).  max_weight > 0 caps
        the weight, so that later views keep their influence; 0: no cap."""
        what = "TSDFVolume.integrate"
        self._check_state(what)
        if not isinstance(depth, torch.Tensor):
            raise TypeError(f"{what}: depth must be a tensor, got {type(depth).__name__}")
        if depth.ndimension() not in (3, 4):
            raise RuntimeError(f"{what}: depth has shape {tuple(depth.shape)}, expected (V, 1, H, W) or (1, H, W)")
        lead = () if depth.ndimension() == 3 else (int(depth.shape[0]),)
        V, H, W = (lead + (1,))[0], int(depth.shape[-2]), int(depth.shape[-1])
        _check(what, "depth", depth, lead + (1, H, W))
        if V < 1 or H < 1 or W < 1:
            raise RuntimeError(f"{what}: depth has shape {tuple(depth.shape)}, expected at least one view and one pixel")
        if V * H * W > _MAX_POINTS:
            raise RuntimeError(f"{what}: depth holds more than 2^31 - 1 pixels")
        if alpha is not None:
            _check(what, "alpha", alpha, lead + (1, H, W))
        if color is not None:
            _check(what, "color", color, lead + (3, H, W))
        if (color is None) != (self.color is None):
            raise RuntimeError(f"{what}: color must be given exactly when the volume has colour (with_color={self.color is not None}): "
                               "the colour average shares the weight")
        alpha_min = _check_positive(what, "alpha_min", alpha_min)
        try:
            max_weight = float(np.float32(max_weight))
        except (TypeError, ValueError):
            raise ValueError(f"{what}: max_weight must be a number, got {max_weight!r}") from None
        if not (math.isfinite(max_weight) and max_weight >= 0.0):
            raise ValueError(f"{what}: max_weight must be finite and not negative, got {max_weight!r}")
        if _is_camera(cameras):
            cameras = [cameras]
        rec = None
        if isinstance(cameras, PackedCameras):
            rec = cameras.records
            if (not isinstance(rec, torch.Tensor) or rec.dtype != torch.float64 or rec.ndimension() != 2
                    or rec.shape[1] != CAMERA_DOUBLES or not rec.is_contiguous()):
                raise RuntimeError(f"{what}: cameras.records must be a contiguous (V, {CAMERA_DOUBLES}) float64 tensor")
            if int(rec.shape[0]) != V:
                raise RuntimeError(f"{what}: {int(rec.shape[0])} cameras for {V} views")
        else:
            cams = list(cameras)
            if len(cams) != V:
                raise RuntimeError(f"{what}: {len(cams)} cameras for {V} views")
            host, _ = camera_records(cams, what)
            for i, c in enumerate(cams):
                if (int(c.image_width), int(c.image_height)) != (W, H):
                    raise RuntimeError(f"{what}: camera {i} has image size {int(c.image_width)} x {int(c.image_height)} (W x H), the "
                                       f"depth has {W} x {H}")
        _check_devices(what, tsdf=self.tsdf, weight=self.weight, vol_color=self.color, depth=depth, alpha=alpha, color=color,
                       **({} if rec is None else {"cameras": rec}))
        dev = self.tsdf.device
        if rec is None:
            rec = torch.from_numpy(host).to(dev).contiguous()
        nx, ny, nz = self.dims
        with torch.cuda.device(dev):
            _native.check("gsr_tsdf_integrate", _native.lib().gsr_tsdf_integrate(
                _stream(dev), nx, ny, nz, *self.origin, self.voxel_size, V, H, W, _ptr(depth.detach()),
                _ptr(None if alpha is None else alpha.detach()), _ptr(None if color is None else color.detach()), _ptr(rec),
                self.trunc, alpha_min, max_weight, _ptr(self.tsdf), _ptr(self.weight), _ptr(self.color)))

    def integrate_renders(self, render_pkgs, cameras, alpha_min: float = 0.5, max_weight: float = 0.0) -> None:
        """`integrate` from render outputs: `depth_3dgs`, `alpha` (render with return_alpha=True) and, for a volume with
        colour, `render` of every package, stacked.  One package or a list, with its camera(s)."""
        what = "TSDFVolume.integrate_renders"
        pkgs = [render_pkgs] if isinstance(render_pkgs, dict) else list(render_pkgs)
        if len(pkgs) == 0:
            raise ValueError(f"{what}: render_pkgs is empty")
        need = ("depth_3dgs", "alpha") + (("render",) if self.color is not None else ())
        for i, p in enumerate(pkgs):
            for k in need:
                if not isinstance(p, dict) or not isinstance(p.get(k), torch.Tensor):
                    raise RuntimeError(f"{what}: render package {i} has no tensor '{k}'"
                                       + (" (render with return_alpha=True)" if k == "alpha" else ""))
        stack = lambda k: torch.stack([p[k].detach().to(torch.float32) for p in pkgs]).contiguous()  # noqa: E731
        self.integrate(stack("depth_3dgs"), cameras, alpha=stack("alpha"), color=stack("render") if self.color is not None else None,
                       alpha_min=alpha_min, max_weight=max_weight)

    def extract_mesh(self):
        """(vertices (Nv,3) float32, faces (Nf,3) int32, colors (Nv,3) float32 | None) of the zero level."""
        return extract_mesh(self.tsdf, self.weight, self.origin, self.voxel_size, self.color)


def extract_mesh(tsdf: torch.Tensor, weight: torch.Tensor, origin, voxel_size,
                 color: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Marching tetrahedra on a (nx,ny,nz) lattice (module docstring): tsdf, weight (nx,ny,nz), color (3,nx,ny,nz) | None,
    float32, contiguous, on the GPU.  A point is inside where tsdf < 0 and observed where weight > 0; a tetrahedron with an
    unobserved point emits nothing.  -> (vertices (Nv,3) float32, faces (Nf,3) int32, colors (Nv,3) float32 | None); an
    empty mesh has Nv = Nf = 0.  Waits once for the stream (the two counts size the outputs)."""
    what = "extract_mesh"
    if not isinstance(tsdf, torch.Tensor):
        raise TypeError(f"{what}: tsdf must be a tensor, got {type(tsdf).__name__}")
    if tsdf.ndimension() != 3:
        raise RuntimeError(f"{what}: tsdf has shape {tuple(tsdf.shape)}, expected (nx, ny, nz)")
    dims = tuple(int(d) for d in tsdf.shape)
    if any(d < 1 for d in dims):
        raise RuntimeError(f"{what}: tsdf has shape {dims}, expected every extent at least 1")
    _check(what, "tsdf", tsdf, dims)
    _check(what, "weight", weight, dims)
    if color is not None:
        _check(what, "color", color, (3,) + dims)
    origin = _check_origin(what, origin)
    voxel_size = _check_positive(what, "voxel_size", voxel_size, single=True)
    _check_mesh_points(what, dims)
    _check_devices(what, tsdf=tsdf, weight=weight, color=color)
    dev = tsdf.device
    L = _native.lib()
    nx, ny, nz = dims
    nbytes = ctypes.c_size_t(0)
    _native.check("gsr_tsdf_mesh_workspace_size", L.gsr_tsdf_mesh_workspace_size(nx, ny, nz, ctypes.byref(nbytes)))
    work = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    counts = (ctypes.c_int64 * 2)(0, 0)
    tsdf, weight = tsdf.detach(), weight.detach()
    color = None if color is None else color.detach()
    with torch.cuda.device(dev):
        _native.check("gsr_tsdf_mesh_count", L.gsr_tsdf_mesh_count(_stream(dev), nx, ny, nz, _ptr(tsdf), _ptr(weight), _ptr(work),
                                                                  counts))
        n_v, n_f = int(counts[0]), int(counts[1])
        vertices = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((n_f, 3), dtype=torch.int32, device=dev)
        colors = None if color is None else torch.empty((n_v, 3), dtype=torch.float32, device=dev)
        if n_v > 0 or n_f > 0:
            _native.check("gsr_tsdf_mesh_emit", L.gsr_tsdf_mesh_emit(
                _stream(dev), nx, ny, nz, *origin, voxel_size, _ptr(tsdf), _ptr(weight), _ptr(color), _ptr(work), n_v, n_f,
                _ptr(vertices), _ptr(colors), _ptr(faces)))
    return vertices, faces, colors


# ---- PLY ------------------------------------------------------------------------------------------------------------------
def _mesh_arrays(what: str, vertices, faces, colors):
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)  # noqa: E731
    v, f = to_np(vertices), to_np(faces)
    if v.ndim != 2 or v.shape[1] != 3 or v.dtype != np.float32:
        raise ValueError(f"{what}: vertices must be (Nv, 3) float32, got {v.shape} {v.dtype}")
    if f.ndim != 2 or f.shape[1] != 3 or f.dtype != np.int32:
        raise ValueError(f"{what}: faces must be (Nf, 3) int32, got {f.shape} {f.dtype}")
    if f.size and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise ValueError(f"{what}: faces index vertices outside 0 .. {v.shape[0] - 1}")
    c = None
    if colors is not None:
        c = to_np(colors)
        if c.shape != v.shape or c.dtype != np.float32:
            raise ValueError(f"{what}: colors must be ({v.shape[0]}, 3) float32, got {c.shape} {c.dtype}")
    return v, f, c


def save_mesh_ply(path, vertices, faces, colors=None) -> None:
    """Writes a binary little-endian PLY: `vertex` with float x y z (and uchar red green blue: colours in [0, 1] times 255,
    rounded, clamped), `face` with the list property `vertex_indices` (uchar count, int indices) -- what Blender, MeshLab and
    Open3D read.  Tensors or numpy arrays: vertices (Nv,3) float32, faces (Nf,3) int32, colors (Nv,3) float32 | None."""
    v, f, c = _mesh_arrays("save_mesh_ply", vertices, faces, colors)
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}", "property float x", "property float y",
              "property float z"]
    vdt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if c is not None:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
        vdt += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    va = np.empty(v.shape[0], dtype=vdt)
    va["x"], va["y"], va["z"] = v[:, 0], v[:, 1], v[:, 2]
    if c is not None:
        q = np.clip(np.rint(np.nan_to_num(c.astype(np.float64)) * 255.0), 0, 255).astype(np.uint8)
        va["red"], va["green"], va["blue"] = q[:, 0], q[:, 1], q[:, 2]
    fa = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    fa["n"], fa["i"] = 3, f
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(va.tobytes())
        out.write(fa.tobytes())


def load_mesh_ply(path):
    """Reads what `save_mesh_ply` wrote -> (vertices (Nv,3) float32, faces (Nf,3) int32, colors (Nv,3) float32 | None) as
    numpy arrays; the colours are the stored bytes / 255.  Any other layout is refused."""
    what = "load_mesh_ply"
    with open(path, "rb") as src:
        data = src.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{what}: {path} is not a PLY file")
    lines = data[:end].decode("ascii").split("\n")[:-1]
    body = data[end + len(b"end_header\n"):]
    xyz = ["property float x", "property float y", "property float z"]
    rgb = ["property uchar red", "property uchar green", "property uchar blue"]
    with_color = len(lines) == 11
    want = ["ply", "format binary_little_endian 1.0", None] + xyz + (rgb if with_color else []) + [None, "property list uchar int vertex_indices"]
    if len(lines) != len(want) or any(w is not None and w != ln for w, ln in zip(want, lines)):
        raise ValueError(f"{what}: {path} does not have the layout save_mesh_ply writes")
    try:
        (ev, nv), (ef, nf) = (ln.rsplit(" ", 1) for ln in (lines[2], lines[-2]))
        nv, nf = int(nv), int(nf)
    except ValueError:
        raise ValueError(f"{what}: {path} has a malformed element line") from None
    if ev != "element vertex" or ef != "element face" or nv < 0 or nf < 0:
        raise ValueError(f"{what}: {path} does not have the layout save_mesh_ply writes")
    vdt = np.dtype([("xyz", "<f4", (3,))] + ([("rgb", "u1", (3,))] if with_color else []))
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    if len(body) != nv * vdt.itemsize + nf * fdt.itemsize:
        raise ValueError(f"{what}: {path} holds {len(body)} bytes of data, its header announces {nv * vdt.itemsize + nf * fdt.itemsize}")
    va = np.frombuffer(body, dtype=vdt, count=nv)
    fa = np.frombuffer(body, dtype=fdt, count=nf, offset=nv * vdt.itemsize)
    if nf and not (fa["n"] == 3).all():
        raise ValueError(f"{what}: {path} has a face that is not a triangle")
    colors = (va["rgb"].astype(np.float32) / np.float32(255.0)) if with_color else None
    return np.ascontiguousarray(va["xyz"]), np.ascontiguousarray(fa["i"]), colors
