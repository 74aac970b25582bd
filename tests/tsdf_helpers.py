"""What the TSDF tests share (tests/test_cpu_tsdf.py, tests/test_gpu_tsdf.py): both halves of the gsr_tsdf_* entry points
(include/gsr.h) restated in numpy, the seeded cases, and the mesh properties.

  * integrate_ref: projection and comparisons in binary64 on the binary32 inputs, the running average in binary32, one IEEE
    operation per operator in the stated order (numpy's ufuncs do not contract a product and a sum).  The product is held to
    it BIT FOR BIT, so it takes what the kernel takes from the host -- focal lengths -- from filter3d_helpers.camera_table,
    which restates the record layout itself.
  * extract_ref: marching tetrahedra as a plain loop over cubes, tetrahedra and cases; the orientation table is built here
    in integers from the edge midpoints (`flip_table`), as the kernel file builds its own at compile time.
  * mesh properties: edge manifoldness, Euler characteristic, signed volume, area.
"""
import functools
import math

import numpy as np

import filter3d_helpers as FH

F32 = np.float32
NEAR = float(F32(0.2))          # (double)0.2f, the rasterizer's near plane
BLOCK = (2, 4, 32)              # tsdf.BLOCK_DIMS (asserted by the CPU tests)
CHUNK = 32                      # tsdf.CAMERAS_PER_CHUNK (likewise)
MESH_ROWS = 1024                # tsdf.MESH_ROWS_PER_BLOCK (likewise)
IMG_W, IMG_H = 37, 23

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
KINDS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))


# ---- integration --------------------------------------------------------------------------------------------------------
def fresh(dims, with_color=True):
    """(tsdf, weight, color | None) of a fresh volume"""
    return (np.ones(dims, dtype=F32), np.zeros(dims, dtype=F32), np.zeros((3,) + tuple(dims), dtype=F32) if with_color else None)


def integrate_ref(state, origin, voxel_size, cameras, trunc, depth, alpha=None, image=None, alpha_min=0.5, max_weight=0.0):
    """state = (tsdf, weight, color | None) float32 arrays -> the new state.  depth (V,1,H,W), alpha (V,1,H,W) | None, image
    (V,3,H,W) | None float32; cameras: objects as filter3d.pack_cameras takes them."""
    tsdf, weight, color = (None if a is None else np.array(a, dtype=F32) for a in state)
    assert (image is None) == (color is None)
    nx, ny, nz = tsdf.shape
    o = [float(F32(c)) for c in origin]
    vs = float(F32(voxel_size))
    i, j, k = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nz, dtype=np.float64),
                          indexing="ij")
    x, y, z = o[0] + vs * i, o[1] + vs * j, o[2] + vs * k
    V, _, H, W = depth.shape
    cx, cy = (float(W) - 1.0) * 0.5, (float(H) - 1.0) * 0.5
    mw = F32(max_weight)
    table = FH.camera_table(cameras)
    assert len(table) == V
    for v, cam in enumerate(table):
        M = cam["M"]
        p = [((x * M[0, c] + y * M[1, c]) + z * M[2, c]) + M[3, c] for c in range(3)]
        zc = p[2]
        ok = zc > NEAR
        with np.errstate(all="ignore"):
            fu = np.floor(((p[0] / zc) * cam["fx"] + cx) + 0.5)
            fv = np.floor(((p[1] / zc) * cam["fy"] + cy) + 0.5)
            ok &= (fu >= 0.0) & (fu < float(W)) & (fv >= 0.0) & (fv < float(H))
            iu, iv = np.where(ok, fu, 0.0).astype(np.int64), np.where(ok, fv, 0.0).astype(np.int64)
            d = depth[v, 0][iv, iu]
            if alpha is not None:
                a = alpha[v, 0][iv, iu]
                ok &= ~(a.astype(np.float64) < alpha_min)
                d = d / a
            assert d.dtype == F32
            ok &= d > F32(0)
            sdf = d.astype(np.float64) - zc
            ok &= ~(sdf < -trunc)
            r = sdf / trunc
            obs = np.where(r < 1.0, r, 1.0).astype(F32)
            w1 = weight + F32(1)
            new_tsdf = (tsdf * weight + obs) / w1
            if color is not None:
                new_color = np.stack([(color[c] * weight + image[v, c][iv, iu]) / w1 for c in range(3)])
                assert new_color.dtype == F32
                color = np.where(ok[None], new_color, color)
            if mw > 0:
                w1 = np.where(w1 < mw, w1, mw)
            assert new_tsdf.dtype == F32 and w1.dtype == F32
        tsdf = np.where(ok, new_tsdf, tsdf)
        weight = np.where(ok, w1, weight)
    return tsdf, weight, color


def grid_of(dims, voxel_size=0.13):
    """(origin, voxel_size): the lattice roughly centred on the world origin, off it by an odd fraction"""
    return tuple(-0.5 * voxel_size * (n - 1) + 0.011 * (a + 1) for a, n in enumerate(dims)), voxel_size


@functools.lru_cache(maxsize=None)
def integrate_case(dims, V, with_alpha=True, with_color=True, seed=0):
    """dict(origin, voxel_size, trunc, cameras, depth, alpha | None, image | None, alpha_min): V general rolled cameras around
    the lattice -- some so close that lattice points lie behind the near plane, narrow enough that many points project
    outside the image --, depths scattered around the cameras' distances so that sdf falls on both sides of -trunc and of
    +trunc, zero depths, and alphas under, at and over alpha_min (its float32 neighbours included)."""
    rng = np.random.default_rng(9100 + 31 * V + 7 * sum(dims) + seed)
    origin, vs = grid_of(dims)
    trunc, alpha_min = 0.2, 0.5
    cams, depth = [], np.empty((V, 1, IMG_H, IMG_W), dtype=F32)
    for v in range(V):
        eye = rng.standard_normal(3)
        dist = rng.uniform(0.5, 2.5)
        eye *= dist / np.linalg.norm(eye)
        M = FH.look_at(eye, rng.uniform(-0.3, 0.3, size=3), roll_deg=rng.uniform(-40.0, 40.0))
        cams.append(FH.Cam(M, IMG_W, IMG_H, rng.uniform(0.5, 1.2), rng.uniform(0.4, 1.0)))
        depth[v, 0] = (dist + rng.uniform(-0.6, 0.6, size=(IMG_H, IMG_W))).astype(F32)
    depth[rng.uniform(size=depth.shape) < 0.08] = 0.0
    alpha = image = None
    if with_alpha:
        alpha = rng.uniform(0.3, 1.0, size=depth.shape).astype(F32)
        pick = rng.uniform(size=depth.shape)
        half = F32(alpha_min)
        alpha[pick < 0.05] = np.nextafter(half, F32(0))   # just under: skipped
        alpha[(pick >= 0.05) & (pick < 0.10)] = half      # at: taken
        alpha[(pick >= 0.10) & (pick < 0.15)] = np.nextafter(half, F32(1))
        depth = (depth * alpha).astype(F32)               # what depth_3dgs is: alpha-weighted
    if with_color:
        image = rng.uniform(0.0, 1.0, size=(V, 3, IMG_H, IMG_W)).astype(F32)
    return dict(origin=origin, voxel_size=vs, trunc=trunc, cameras=cams, depth=depth, alpha=alpha, image=image,
                alpha_min=alpha_min, dims=tuple(dims))


def edge_case():
    """One camera at the world origin looking down +z at a plane of lattice points whose projections step by a quarter pixel
    from 1.375 pixels outside the image on one side to 1.625 pixels outside on the other, in u and in v (no projection on a
    rounding boundary)."""
    W, H, f = IMG_W, IMG_H, 16.0
    cam = FH.Cam(np.eye(4), W, H, 2.0 * math.atan(W / (2.0 * f)), 2.0 * math.atan(H / (2.0 * f)))
    vs = 1.0 / 64.0
    dims = (int((W + 3) * 4 + 1), int((H + 3) * 4 + 1), 1)
    origin = (-((W - 1) / 2.0 + 1.375) / f, -((H - 1) / 2.0 + 1.375) / f, 1.0)
    depth = np.full((1, 1, H, W), 1.05, dtype=F32)
    return dict(origin=origin, voxel_size=vs, trunc=0.2, cameras=[cam], depth=depth, alpha=None, image=None, alpha_min=0.5, dims=dims)


def run_case_ref(case, max_weight=0.0, state=None, views=None):
    """the restatement on a case (all views, or the views `views`), from a fresh volume or from `state`"""
    sel = slice(None) if views is None else list(views)
    pick = lambda a: None if a is None else a[sel]  # noqa: E731
    cams = case["cameras"] if views is None else [case["cameras"][v] for v in views]
    state = fresh(case["dims"], case["image"] is not None) if state is None else state
    return integrate_ref(state, case["origin"], case["voxel_size"], cams, case["trunc"], pick(case["depth"]), pick(case["alpha"]),
                         pick(case["image"]), case["alpha_min"], max_weight)


# ---- marching tetrahedra ------------------------------------------------------------------------------------------------
def tet_path(t):
    """the four corner offsets of tetrahedron t, in path order"""
    p = PERMS[t]
    v0 = (0, 0, 0)
    v1 = tuple(int(a == p[0]) for a in range(3))
    v2 = tuple(int(a in (p[0], p[1])) for a in range(3))
    return v0, v1, v2, (1, 1, 1)


def case_triangles(case):
    """the triangles of a case before orientation: lists of three edges (p, q) of path positions"""
    ins = [p for p in range(4) if (case >> p) & 1]
    outs = [p for p in range(4) if not (case >> p) & 1]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1:
        return [[(ins[0], b) for b in outs]]
    if len(ins) == 3:
        return [[(outs[0], b) for b in ins]]
    (a, b), (c, d) = ins, outs
    q = [(a, c), (a, d), (b, d), (b, c)]
    return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]


@functools.lru_cache(maxsize=None)
def flip_table():
    """(6, 16) bool: the triangle (A,B,C) of (tetrahedron, case) is emitted as (A,C,B).  Integers only: doubled edge
    midpoints, ((B - A) x (C - A)) . (n_in sum(outside) - n_out sum(inside)); never zero, and the two triangles of a quad
    agree."""
    flip = np.zeros((6, 16), dtype=bool)
    for t in range(6):
        path = np.array(tet_path(t), dtype=np.int64)
        for case in range(1, 15):
            ins = [p for p in range(4) if (case >> p) & 1]
            outs = [p for p in range(4) if not (case >> p) & 1]
            direction = len(ins) * path[outs].sum(0) - len(outs) * path[ins].sum(0)
            signs = []
            for tri in case_triangles(case):
                A, B, C = (path[p] + path[q] for p, q in tri)
                dot = int(np.dot(np.cross(B - A, C - A), direction))
                assert dot != 0
                signs.append(dot < 0)
            assert len(set(signs)) == 1
            flip[t, case] = signs[0]
    return flip


def extract_ref(tsdf, weight, origin, voxel_size, color=None):
    """(vertices (Nv,3) float32, faces (Nf,3) int32, colors (Nv,3) float32 | None), as specified"""
    tsdf, weight = np.asarray(tsdf, dtype=F32), np.asarray(weight, dtype=F32)
    nx, ny, nz = tsdf.shape
    inside, observed = tsdf < 0, weight > 0
    flip = flip_table()
    lin = lambda p: (p[0] * ny + p[1]) * nz + p[2]  # noqa: E731
    face_keys = []
    if min(nx, ny, nz) >= 2:
        n_in = sum(inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
        for i, j, k in np.argwhere((n_in > 0) & (n_in < 8)):   # (lexicographic: the cubes in order)
            for t in range(6):
                pts = [(i + d[0], j + d[1], k + d[2]) for d in tet_path(t)]
                if not all(observed[p] for p in pts):
                    continue
                case = sum(int(inside[p]) << q for q, p in enumerate(pts))
                for tri in case_triangles(case):
                    keys = []
                    for p, q in tri:
                        p, q = min(p, q), max(p, q)
                        d = tuple(b - a for a, b in zip(pts[p], pts[q]))
                        keys.append(7 * lin(pts[p]) + KINDS.index(d))
                    if flip[t, case]:
                        keys = [keys[0], keys[2], keys[1]]
                    face_keys.append(keys)
    face_keys = np.array(face_keys, dtype=np.int64).reshape(-1, 3)
    used = np.unique(face_keys)
    faces = np.searchsorted(used, face_keys).astype(np.int32)
    n, kind = used // 7, used % 7
    lower = np.stack([n // (ny * nz), (n // nz) % ny, n % nz], axis=1)
    d = np.array(KINDS, dtype=np.int64)[kind].reshape(-1, 3)
    upper = lower + d
    f0 = tsdf[tuple(lower.T)] if len(used) else np.zeros(0, dtype=F32)
    f1 = tsdf[tuple(upper.T)] if len(used) else np.zeros(0, dtype=F32)
    t = f0 / (f0 - f1)
    o, vs = np.array(origin, dtype=F32), F32(voxel_size)
    step = np.where(d > 0, t[:, None], F32(0)).astype(F32)
    vertices = (o[None, :] + vs * (lower.astype(F32) + step)).astype(F32)
    assert t.dtype == F32 and (lower.astype(F32) + step).dtype == F32
    colors = None
    if color is not None:
        color = np.asarray(color, dtype=F32)
        c0 = np.stack([color[a][tuple(lower.T)] for a in range(3)], axis=1) if len(used) else np.zeros((0, 3), dtype=F32)
        c1 = np.stack([color[a][tuple(upper.T)] for a in range(3)], axis=1) if len(used) else np.zeros((0, 3), dtype=F32)
        colors = (c0 + t[:, None] * (c1 - c0)).astype(F32)
    return vertices.reshape(-1, 3), faces.reshape(-1, 3), colors


def sphere_field(n, radius_fraction=0.4):
    """(tsdf (n,n,n) float32 = distance to a sphere's surface in lattice units, negative inside; weight all 1; centre;
    radius): voxel_size 1, origin 0, the centre off the lattice by odd fractions"""
    centre = np.array([(n - 1) / 2.0 + 0.13, (n - 1) / 2.0 - 0.21, (n - 1) / 2.0 + 0.07])
    radius = radius_fraction * (n - 1)
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij"), axis=-1)
    return (np.linalg.norm(g - centre, axis=-1) - radius).astype(F32), np.ones((n, n, n), dtype=F32), centre, radius


def smooth_field(dims, seed=0):
    """a smooth random field with both signs, weights with a few unobserved points, colours"""
    rng = np.random.default_rng(700 + seed + sum(dims))
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing="ij"), axis=-1)
    f = sum(rng.standard_normal() * np.sin(g @ rng.uniform(0.3, 1.4, size=3) + rng.uniform(0, 6.28)) for _ in range(4))
    weight = (rng.uniform(size=dims) > 0.03).astype(F32) * F32(2)
    return (f / 3.0).astype(F32), weight, rng.uniform(size=(3,) + tuple(dims)).astype(F32)


# ---- mesh properties ----------------------------------------------------------------------------------------------------
def edge_counts(faces):
    """(largest multiplicity of a directed edge, smallest and largest number of faces at an undirected edge, edges)"""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, directed = np.unique(e, axis=0, return_counts=True)
    _, undirected = np.unique(np.sort(e, axis=1), axis=0, return_counts=True)
    return int(directed.max()), int(undirected.min()), int(undirected.max()), len(undirected)


def volume_and_area(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = (v[np.asarray(faces)[:, q]] for q in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0), float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)


def sphere_report(n, vertices, faces, centre, radius):
    """dict of the sphere properties the tests assert"""
    dmax, umin, umax, E = edge_counts(faces)
    vol, area = volume_and_area(np.asarray(vertices, dtype=np.float64) - centre, faces)
    radial = np.abs(np.linalg.norm(np.asarray(vertices, dtype=np.float64) - centre, axis=1) - radius)
    return dict(directed_max=dmax, undirected_min=umin, undirected_max=umax, euler=len(vertices) - E + len(faces),
                volume_ratio=vol / (4.0 / 3.0 * math.pi * radius ** 3), area_ratio=area / (4.0 * math.pi * radius ** 2),
                radial_max=float(radial.max()), referenced=len(np.unique(faces)) == len(vertices))
