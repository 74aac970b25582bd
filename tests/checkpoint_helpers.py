"""Checkpoints (K6) and list segments (K7) as production runs them: the scenes, and a host model of what the default table does
with them (a helper module of tests/test_cpu_checkpoints.py and tests/test_gpu_checkpoints.py).

With no knob in the environment a view whose lists are long -- on(R, W, H) -- leaves checkpoints at the positions FINE_POS of a
tile's list (gsr_capi.hip: checkpoint_table), the ck_tiles(T) <= CK_TILES_CAP tiles with the longest lists own the slots
(gsr_binning.hip: tile_worklist_kernel) and the backward's work list (gsr_blend.hip: backward_worklist_kernel<true>) cuts a
tile into ns(deep) list segments if it owns slots, is walked deeper than the first checkpoint, carries >= 5/8 of a
workgroup's fair share of the work and its largest segment holds <= 4/5 of its work.  Everything here is a statement about
the ORACLE's forward (oracle/cpu.py): R, the tile lists, n_contrib.  n_contrib is bit-exact between the oracle and K6, so
deep(tile) -- the largest n_contrib among a tile's pixels -- is K6's tile_maxc wherever that is recorded.

Scenes (all make_case(..., bg=BG) with the opacity redrawn uniformly in an interval, generator seed = the case's seed + 100):
  reach     16 x 16, 17 500 Gaussians, ONE tile: every slot of the table and the tail beyond its reach of 16 384 positions;
  ragged    13 x 11, 3 300: an image smaller than a tile, across the 256 -> 512 stride change at slots 6 / 7;
  just_on / just_off   16 x 16, 1 300 / 1 199 of the same recipe: either side of on()'s 1 200 entries per tile;
  edge(n)   reach with every entry at list position >= n made invisible (opacity 1e-3: alpha < 1/255 everywhere) and the
            entry at position n - 1 given opacity 0.5: K6 walks and checkpoints the whole list, K7's walk ends at n exactly;
  saturating  one tile whose pixels all stop (T (1 - alpha) < 1e-4) in the first half of the list: K6 leaves the walk early and
            the checkpoints behind stay unwritten;
  cap       832 x 800 = 2 600 tiles > CK_TILES_CAP, every tile walked deeper than the first checkpoint: 552 tiles own no slot;
  wide      2064 x 1040 = 8 385 tiles > 8 192 (the work-list kernel re-reads its inputs instead of holding them in
            registers), two dense translucent clusters over the first and the last tile rows, for a process under
            GSR_CK_CHUNKS=4 GSR_BWD_SEG=1 (the uniform table; the work list's path is what that scene is about).
"""
import numpy as np
import torch

from helpers import make_case, oracle_backward, oracle_forward, seed_gradient

#: the production table, restated: list positions of the 16 checkpoints.  Changing checkpoint_table means changing this line.
FINE_POS = tuple(64 * c for c in (0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 64, 80, 96, 128, 192, 256))
CK_MAX = len(FINE_POS)
CK_TILES_CAP = 2048
REGS_TILES = 8192  # above it backward_worklist_kernel re-reads the tiles' counts (in_regs is false)
KNOBS = ("GSR_CK_CHUNKS", "GSR_CK_SLOTS", "GSR_CK_DEBUG", "GSR_BWD_SEG", "GSR_BIN_LEGACY", "GSR_SORT_THREADS")
BG = (0.2, 0.5, 0.7)
EDGES = (256, 257, 1536, 1537, 2048, 2049, 16384, 16385)
ONE_TILE = ("reach", "ragged", "just_on", "just_off") + tuple(f"edge{n}" for n in EDGES) + ("saturating",)
#: one-tile scenes whose tile must be cut into exactly ns segments; not deeper than the first checkpoint; the 4/5 rule decides
CUT = ("reach", "ragged", "just_on", "edge1536", "edge1537", "edge2049", "edge16384", "edge16385", "saturating")
NEVER_CUT = ("edge256", "just_off")
EITHER = ("edge257", "edge2048")
WIDE_KNOBS = dict(GSR_CK_CHUNKS="4", GSR_BWD_SEG="1")


# ---- the host model -------------------------------------------------------------------------------------------------------
def tiles(W, H):
    return ((W + 15) // 16) * ((H + 15) // 16)


def on(R, W, H):
    """Does a view's forward leave checkpoints (no knob set)?  (pinned through gsr_scratch_sizes in tests/test_cpu_abi.py)"""
    T = tiles(W, H)
    return R >= (1200 if T <= 4096 else 2048) * T


def ns(deep, pos=FINE_POS):
    """Segments the backward's walk reaches into: one more than the checkpoints in front of its end."""
    return 1 + sum(1 for k in range(1, len(pos)) if pos[k] < int(deep))


def uniform_pos(chunks, slots=CK_MAX):
    """The table under GSR_CK_CHUNKS=chunks."""
    return tuple(64 * chunks * k for k in range(slots))


def tile_deep(f, W, H):
    """deep(tile) -> int64 (T,): the largest n_contrib among the tile's pixels."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    nc = np.zeros((gy * 16, gx * 16), np.int64)
    nc[:H, :W] = f["n_contrib"].reshape(H, W)
    return nc.reshape(gy, 16, gx, 16).max(axis=(1, 3)).reshape(-1)


def tile_lengths(f):
    r = f["ranges"].reshape(-1, 2).astype(np.int64)
    return r[:, 1] - r[:, 0]


def stop_positions(f, W, H):
    """For a ONE-tile view: per pixel the list position (1-based) of the entry at which the walk stops -- the first with
    T (1 - alpha) < 1e-4 -- or 0 where it never does; float64 on the oracle's per-Gaussian state (a model: a pixel within
    rounding of a threshold may differ from the binary32 walk, which is why callers ask for a margin)."""
    lo, hi = (int(v) for v in f["ranges"].reshape(-1, 2)[0])
    ids = f["point_list"][lo:hi].astype(np.int64)
    co, m = f["conic_opacity"][ids].astype(np.float64), f["means2D"][ids].astype(np.float64)
    py, px = np.mgrid[0:H, 0:W]
    dx, dy = m[:, 0][None, :] - px.reshape(-1, 1), m[:, 1][None, :] - py.reshape(-1, 1)
    power = -0.5 * (co[:, 0] * dx * dx + co[:, 2] * dy * dy) - co[:, 1] * dx * dy
    alpha = np.minimum(0.99, co[:, 3] * np.exp(np.minimum(power, 0.0)))
    alpha[(power > 0) | (alpha < 1.0 / 255.0)] = 0.0
    T, stop = np.ones(H * W), np.zeros(H * W, np.int64)
    for j in range(ids.shape[0]):
        t = T * (1.0 - alpha[:, j])
        hit = (alpha[:, j] > 0) & (t < 1e-4) & (stop == 0)
        stop[hit] = j + 1
        T = np.where((stop == 0), t, T)
    return stop


# ---- the scenes -----------------------------------------------------------------------------------------------------------
def _translucent(P, W, H, seed, s0, lo, hi, scale_xyz=1.0):
    case = make_case(P, W, H, seed=seed, s0=s0, scale_xyz=scale_xyz, bg=BG)
    u = torch.rand(P, 1, generator=torch.Generator().manual_seed(seed + 100))
    case["sc"]["opacity"] = (lo + (hi - lo) * u).contiguous()
    return case


_RECIPES = dict(reach=(17500, 16, 16, 1, 0.08, 0.01, 0.04), ragged=(3300, 13, 11, 1, 0.1, 0.02, 0.1),
                just_on=(1300, 16, 16, 1, 0.1, 0.02, 0.3), just_off=(1199, 16, 16, 1, 0.1, 0.02, 0.3))
CAP_P, SAT_P, SAT_FRONT, SAT_OPAQUE = 30000, 6000, 2600, 400
_scenes, _fwd, _bwd, _f64 = {}, {}, {}, {}


def _list_of_the_tile(f):
    lo, hi = (int(v) for v in f["ranges"].reshape(-1, 2)[0])
    return f["point_list"][lo:hi].astype(np.int64)


def _centre_inside(f, ids, W, H):
    m = f["means2D"][ids]
    return (m[:, 0] > -0.5) & (m[:, 0] < W - 0.5) & (m[:, 1] > -0.5) & (m[:, 1] < H - 0.5)


def _edge(O, n):
    base = scene(O, "reach")["case"]
    f = forward(O, "reach")
    ids = _list_of_the_tile(f)
    ok = np.nonzero(_centre_inside(f, ids, base["W"], base["H"]))[0]
    n = int(ok[np.abs(ok - (n - 1)).argmin()]) + 1  # (the nearest position whose Gaussian's centre lies inside the image)
    op = base["sc"]["opacity"].clone()
    op[torch.from_numpy(ids[n:])] = 1e-3
    last = int(ids[n - 1])
    op[last] = 0.5
    sc = dict(base["sc"], opacity=op.contiguous())
    # The entry can only end the walk where a pixel is still live.  In the middle of the tile every pixel has stopped by
    # position ~9 600 (T < 1e-4), and alpha = 0.5 exp(power) reaches 1/255 within 1.8 pixels of the centre only: where no pixel
    # that reach still blends at position >= n lies under the centre, the Gaussian is slid ACROSS the view onto the nearest one
    # -- along the camera's right / up axes, so its depth and with it the list order stay as they are.
    W, H = base["W"], base["H"]
    live = (f["n_contrib"].reshape(H, W) >= n)
    cx, cy = (float(v) for v in f["means2D"][last])
    if not live[int(round(cy)), int(round(cx))]:
        ys, xs = np.nonzero(live)
        j = int(((xs - cx) ** 2 + (ys - cy) ** 2).argmin())
        V = base["cam"].world_view_transform.double()
        zv = float(torch.cat([base["sc"]["xyz"][last].double(), torch.ones(1, dtype=torch.float64)]) @ V[:, 2])
        dxv, dyv = (xs[j] - cx) * zv * 2 * base["tfx"] / W, (ys[j] - cy) * zv * 2 * base["tfy"] / H
        xyz = base["sc"]["xyz"].clone()
        xyz[last] = (xyz[last].double() + dxv * V[:3, 0] + dyv * V[:3, 1]).float()
        sc["xyz"] = xyz.contiguous()
    case = dict(base, sc=sc)
    return case, n


def _saturating(O):
    """ragged's recipe on a full tile; the SAT_OPAQUE entries behind the first SAT_FRONT of the list made opaque and sixteen
    times as large: whatever is left of a pixel's transmittance ends there.  The wall stands 2 600 positions deep: on an image
    this small the forward cuts every quadrant into four items, a tile's checkpoint row then counts up to four times what
    its work estimate does, and the first segment alone looks like more than 4/5 of a tile walked less than ~1 300 deep
    (such a tile stays whole: with the wall at 320, 1 000 and 1 500 the work list held (2, 0): the front of a list, nearest the
    camera, is also where the footprints are largest and the entries evaluated most)."""
    case = _translucent(SAT_P, 16, 16, 2, 0.1, 0.02, 0.1)
    ids = _list_of_the_tile(oracle_forward(O, case))
    wall = torch.from_numpy(ids[SAT_FRONT:SAT_FRONT + SAT_OPAQUE])
    sc = dict(case["sc"])
    sc["opacity"], sc["scaling"] = sc["opacity"].clone(), sc["scaling"].clone()
    sc["opacity"][wall] = 0.99
    sc["scaling"][wall] *= 16.0
    return dict(case, sc=sc)


def _wide():
    """A sparse background (6 000 Gaussians over three times the cube) and two clusters of 1 500 small translucent ones, each
    around the background Gaussian whose centre projects nearest a tile corner of the first / the last tile rows."""
    W, H = 2064, 1040
    case = make_case(6000, W, H, seed=5, s0=0.02, scale_xyz=3.0, bg=BG)
    sc, cam = case["sc"], case["cam"]
    xyz = sc["xyz"].double()
    ph = torch.cat([xyz, torch.ones(xyz.shape[0], 1, dtype=torch.float64)], 1) @ cam.full_proj_transform.double()
    px = ((ph[:, 0] / ph[:, 3] + 1) * W - 1) / 2
    py = ((ph[:, 1] / ph[:, 3] + 1) * H - 1) / 2
    front = ph[:, 3] > 1.0
    parts = {k: [v] for k, v in sc.items() if isinstance(v, torch.Tensor) and v.dim() >= 2}
    for i, (tx, ty) in enumerate(((48.0, 16.0), (1600.0, 1024.0))):
        d = (px - tx) ** 2 + (py - ty) ** 2
        d[~front] = float("inf")
        c = sc["xyz"][int(d.argmin())]
        add = make_case(1500, 16, 16, seed=50 + i, s0=0.02)["sc"]
        g = torch.Generator().manual_seed(60 + i)
        add["xyz"] = (c[None, :] + 0.05 * add["xyz"]).contiguous()
        add["opacity"] = (0.02 + 0.06 * torch.rand(1500, 1, generator=g)).contiguous()
        for k in parts:
            parts[k].append(add[k])
    case["sc"] = dict(sc, **{k: torch.cat(v, 0).contiguous() for k, v in parts.items()})
    return case


def scene(O, name):
    """-> the f64_regimes-style record of the scene `name`: dict(name, case, D, sm, colors_precomp, cov3D_precomp, G, GD) (+ n
    for edge(n): the position the family rule settled on).  Built once per process, never modified."""
    if name not in _scenes:
        extra = {}
        if name in _RECIPES:
            P, W, H, seed, s0, lo, hi = _RECIPES[name]
            case = _translucent(P, W, H, seed, s0, lo, hi)
        elif name.startswith("edge"):
            case, extra["n"] = _edge(O, int(name[4:]))
        elif name == "saturating":
            case = _saturating(O)
        elif name == "cap":
            case = _translucent(CAP_P, 832, 800, 3, 0.12, 0.005, 0.03, scale_xyz=2.0)
        elif name == "wide":
            case = _wide()
        else:
            raise KeyError(name)
        H, W = case["H"], case["W"]
        _scenes[name] = dict(name=name, case=case, D=3, sm=1.0, colors_precomp=None, cov3D_precomp=None,
                             G=seed_gradient(H, W, 11) * (H * W), GD=None, **extra)
    return _scenes[name]


def forward(O, name):
    """The oracle's forward of the scene, computed once per process."""
    if name not in _fwd:
        _fwd[name] = oracle_forward(O, scene(O, name)["case"])
    return _fwd[name]


def backward(O, name):
    if name not in _bwd:
        r = scene(O, name)
        _bwd[name] = oracle_backward(O, r["case"], forward(O, name), r["G"])
    return _bwd[name]


def f64(O, name):
    """float64 autograd of the scene's loss on the oracle's tile lists -> (gradients, masked rows, report); once per process."""
    if name not in _f64:
        import f64_regimes as F

        r, f = scene(O, name), forward(O, name)
        want, stats, _ = F.f64_run(f, r)
        mask, report = F.masked_rows(r, f, stats)
        _f64[name] = (want, mask, report)
    return _f64[name]


def facts(O, name):
    """What the host model says of the scene -> dict(R, T, on, deep (T,), ns (T,), lengths (T,))."""
    r, f = scene(O, name), forward(O, name)
    W, H = r["case"]["W"], r["case"]["H"]
    pos = uniform_pos(int(WIDE_KNOBS["GSR_CK_CHUNKS"])) if name == "wide" else FINE_POS
    deep = tile_deep(f, W, H)
    return dict(R=int(f["num_rendered"]), T=tiles(W, H), on=on(int(f["num_rendered"]), W, H), deep=deep,
                ns=np.array([ns(d, pos) for d in deep]), lengths=tile_lengths(f))
