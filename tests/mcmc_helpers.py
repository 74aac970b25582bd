"""The 3DGS-MCMC strategy restated, for tests/test_cpu_mcmc.py, tests/test_gpu_mcmc.py and tools/bench_mcmc.py (DESIGN.md
section 21; include/gsr.h: gsr_mcmc_*):

  sample_int             classification and the draws in pure Python integers (what gsr_mcmc_sample must reproduce bit for bit);
  relocation_values_f64  the relocation values in numpy float64, in the operation order include/gsr.h states;
  noise_f64              the noise step evaluated in numpy float64 from the float32 inputs;
  noise_torch, mcmc_refine_torch  the noise step and the whole refine from torch ops only (masked assignment, torch.cat),
                         as a user without the kernels writes them."""
import bisect
import math

import numpy as np
import torch

F = np.float32
RATIO_CAP = 51
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
PS = (1, 2, 255, 256, 257, 70001)  # one lane, the block edges of the weight scan, several blocks with a ragged tail
O_MAX = 1.0 - 2.0 ** -24           # the largest opacity the relocation formula takes
OP_MAX = 1.0 - 2.0 ** -23          # the largest new opacity


# ----------------------------------------------------------------------------------------------------------------------
# classification and sampling: Python integers
# ----------------------------------------------------------------------------------------------------------------------
def weights_int(opacity, mask, min_opacity):
    """(dead [bool], alive [bool], k [int]) per row.  opacity: float32 array; the comparison is with float32(min_opacity)."""
    mo = F(min_opacity)
    dead, alive, k = [], [], []
    for j, o in enumerate(np.asarray(opacity, F)):
        m = True if mask is None else bool(mask[j])
        d = bool(m and o <= mo)       # (a NaN fails both comparisons)
        a = bool(m and o > mo)
        dead.append(d)
        alive.append(a)
        k.append(min(int(float(o) * 2 ** 23), 2 ** 23) if a else 0)  # exact: float32 times a power of two, truncated
    return dead, alive, k


def draw_int(u, total):
    """t of one draw: m = trunc(u 2^24), t = (m total) >> 24 in unbounded integers."""
    u = float(F(u))
    m = min(int(u * 2 ** 24), 2 ** 24 - 1) if u >= 0.0 else 0
    return (m * total) >> 24


def sample_int(opacity, u, min_opacity, mask=None, n_draws=None):
    """gsr_mcmc_sample: dict(dead_sel, dead_idx (the dead rows, ascending), src, count, ratio, record = (n_dead, n_alive,
    n_draws, total)).  n_draws=None: one draw per dead row (at most len(u))."""
    P, n = len(opacity), len(u)
    dead, alive, k = weights_int(opacity, mask, min_opacity)
    S, acc = [], 0
    for w in k:
        acc += w
        S.append(acc)
    total = acc
    dead_idx = [j for j in range(P) if dead[j]]
    nd = min(len(dead_idx), n) if n_draws is None else int(n_draws)
    src = [-1] * (n if n_draws is None else nd)
    count = [0] * P
    if total > 0:
        for r in range(nd):
            j = bisect.bisect_right(S, draw_int(u[r], total))  # the smallest j with S_j > t
            src[r] = j
            count[j] += 1
    ratio = [0 if s < 0 else min(count[s] + 1, RATIO_CAP) for s in src]
    return dict(dead_sel=np.array(dead, bool), dead_idx=np.array(dead_idx, np.int32), src=np.array(src, np.int32),
                count=np.array(count, np.int32), ratio=np.array(ratio, np.int32), record=(len(dead_idx), sum(alive), nd, total))


# ----------------------------------------------------------------------------------------------------------------------
# relocation values: numpy float64 in the kernel's order
# ----------------------------------------------------------------------------------------------------------------------
def relocation_f64(o, N, min_opacity):
    """(new opacity o' after the clamp, scale factor o / denom) in float64 for arrays o (activated opacities, any float
    type) and N (ratios; capped at RATIO_CAP here)."""
    o = np.minimum(np.asarray(o, np.float64), O_MAX)
    N = np.clip(np.asarray(N, np.int64), 1, RATIO_CAP)
    op = 1.0 - np.power(1.0 - o, 1.0 / N.astype(np.float64))
    root = np.sqrt(np.arange(1, RATIO_CAP + 1, dtype=np.float64))
    denom = np.zeros_like(o)
    for n in np.unique(N):
        sel = N == n
        x = op[sel]
        acc = np.zeros_like(x)
        for i in range(1, int(n) + 1):
            p = x.copy()
            for k in range(i):
                term = (float(math.comb(i - 1, k)) * p) / root[k]
                acc = acc - term if k & 1 else acc + term
                p = p * x
        denom[sel] = acc
    f = o / denom
    op = np.minimum(np.maximum(op, np.float64(F(min_opacity))), OP_MAX)
    return op, f


def relocation_values_f64(opacity, scaling_raw, src, ratio, min_opacity):
    """gsr_mcmc_relocation_values before the final rounding: (raw opacity (n,), raw scaling (n,3)) in float64; rows of a
    draw with src < 0 are zero."""
    src = np.asarray(src, np.int64)
    ok = src >= 0
    s = np.where(ok, src, 0)
    op, f = relocation_f64(np.asarray(opacity, F)[s], np.where(ok, ratio, 1), min_opacity)
    new_o = np.log(op / (1.0 - op))
    new_s = np.log(np.exp(np.asarray(scaling_raw, F)[s].astype(np.float64)) * f[:, None])
    return np.where(ok, new_o, 0.0), np.where(ok[:, None], new_s, 0.0)


# ----------------------------------------------------------------------------------------------------------------------
# the noise step
# ----------------------------------------------------------------------------------------------------------------------
def _rotation_np(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.zeros((q.shape[0], 3, 3), q.dtype)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def noise_f64(xyz, scaling_raw, rotation_raw, opacity_raw, noise, scaler, mask=None, k=100.0, x0=0.995):
    """The new xyz in float64 from the float32 inputs (rows outside the mask: the old xyz)."""
    d = lambda a: np.asarray(a, F).astype(np.float64)  # noqa: E731
    x, sr, rot, orw, nz = d(xyz), d(scaling_raw), d(rotation_raw), d(opacity_raw).reshape(-1), d(noise)
    with np.errstate(all="ignore"):
        o = 1.0 / (1.0 + np.exp(-orw))
        s = np.exp(sr)
        q = rot / np.sqrt((rot * rot).sum(axis=1, keepdims=True))
        R = _rotation_np(q)
        sigma = np.einsum("nac,nc,nbc->nab", R, s * s, R)
        g = 1.0 / (1.0 + np.exp(k * (o - (1.0 - x0))))
        out = x + np.einsum("nab,nb->na", sigma, nz * g[:, None] * scaler)
    if mask is not None:
        out[~np.asarray(mask, bool)] = x[~np.asarray(mask, bool)]
    return out


def build_rotation_torch(r):
    q = r / torch.norm(r, dim=1, keepdim=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), dim=1).reshape(-1, 3, 3)


def noise_torch(xyz, scaling_raw, rotation_raw, opacity_raw, noise, scaler, mask=None, k=100.0, x0=0.995):
    """3DGS-MCMC's inject_noise_to_position with torch ops, in place on xyz."""
    opac = torch.sigmoid(opacity_raw).reshape(-1)
    scales = torch.exp(scaling_raw)
    R = build_rotation_torch(rotation_raw)
    M = R * scales[:, None, :]
    covars = torch.bmm(M, M.transpose(1, 2))
    gate = 1.0 / (1.0 + torch.exp(-k * ((1.0 - opac) - x0)))
    delta = torch.bmm(covars, (noise * gate[:, None] * scaler)[:, :, None]).squeeze(-1)
    xyz.add_(delta if mask is None else delta * mask[:, None])  # (no boolean indexing: that would synchronise)


# ----------------------------------------------------------------------------------------------------------------------
# the whole refine from torch ops
# ----------------------------------------------------------------------------------------------------------------------
def sample_torch(opacity, u, min_opacity, mask, n_draws):
    """(dead rows (int64, ascending), src (n_draws,) int64 | None when nothing can be drawn, ratio) with torch ops: nonzero,
    cumsum, searchsorted, bincount.  n_draws=None: one draw per dead row."""
    m = torch.ones_like(opacity, dtype=torch.bool) if mask is None else mask
    dead = m & (opacity <= min_opacity)
    alive = m & (opacity > min_opacity)
    dead_idx = dead.nonzero().reshape(-1)
    n = int(dead_idx.numel()) if n_draws is None else n_draws
    k = torch.where(alive, (opacity * float(2 ** 23)).to(torch.int64).clamp(max=2 ** 23), torch.zeros((), dtype=torch.int64, device=opacity.device))
    S = torch.cumsum(k, 0)
    total = int(S[-1])
    if total == 0 or n == 0:
        return dead_idx, None, None
    mm = (u[:n] * float(2 ** 24)).to(torch.int64).clamp(max=2 ** 24 - 1)
    t = mm * (total >> 24) + ((mm * (total & (2 ** 24 - 1))) >> 24)  # (m total) >> 24 without leaving 64 bits
    src = torch.searchsorted(S, t, right=True)
    count = torch.bincount(src, minlength=opacity.numel())
    return dead_idx, src, (count[src] + 1).clamp(max=RATIO_CAP)


_COEF = {}


def _coef(dev):
    """(51,51) float64: row i-1, column k = C(i-1,k) (-1)^k / sqrt(k+1)."""
    if dev not in _COEF:
        c = [[(math.comb(i, k) * (-1) ** k / math.sqrt(k + 1)) if k <= i else 0.0 for k in range(RATIO_CAP)] for i in range(RATIO_CAP)]
        _COEF[dev] = torch.tensor(c, dtype=torch.float64, device=dev)
    return _COEF[dev]


def relocation_values_torch(opacity, scaling_raw, src, ratio, min_opacity):
    """(new raw opacity (n,1), new raw scaling (n,3)) float32, the double sum as one matrix product in float64."""
    o = opacity[src].double().clamp(max=O_MAX)
    N = ratio.clamp(1, RATIO_CAP)
    op = 1.0 - torch.pow(1.0 - o, 1.0 / N.double())
    pw = op[:, None] ** torch.arange(1, RATIO_CAP + 1, device=o.device, dtype=torch.float64)[None, :]
    inner = torch.cumsum(pw @ _coef(o.device).T, dim=1)            # [:, i-1] = the sum over rows 1..i
    denom = inner.gather(1, (N.long() - 1)[:, None]).squeeze(1)
    f = o / denom
    op = op.clamp(float(F(min_opacity)), OP_MAX)
    new_o = torch.log(op / (1.0 - op)).float()[:, None]
    new_s = torch.log(torch.exp(scaling_raw[src].double()) * f[:, None]).float()
    return new_o, new_s


def mcmc_refine_torch(par, moments, extra, *, cap_max, min_opacity=0.005, grow=1.05, mask=None, generation_num=None,
                      generator=None, copy=True):
    """mcmc_refine on {name: tensor} `par`, {name: (exp_avg, exp_avg_sq)} `moments` and the bookkeeping `extra`, from torch ops
    only.  Returns the new (par, moments, extra, (P, n_dead, n_relocated, n_added), touched) where touched = dict(dead, src of
    the relocation, src of the growth) as int64 tensors (empty where nothing happened).  No input tensor is written to
    (copy=False: the relocation writes `par` and `moments` in place, as the native route does -- tools/bench_mcmc.py)."""
    if copy:
        par = {k: v.clone() for k, v in par.items()}
        moments = {k: (a.clone(), b.clone()) for k, (a, b) in moments.items()}
    else:
        par, moments = dict(par), dict(moments)
    extra = dict(extra)
    if mask is None:
        mask = extra.get("mask")
    dev = par["xyz"].device
    P = par["xyz"].shape[0]
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    touched = dict(dead=none, src_relocate=none, src_grow=none)
    n_dead = n_rel = n_add = 0
    if P > 0:
        opacity = torch.sigmoid(par["opacity"]).reshape(-1)
        u = torch.rand(P, dtype=torch.float32, device=dev, generator=generator)
        dead_idx, src, ratio = sample_torch(opacity, u, min_opacity, mask, None)
        n_dead = int(dead_idx.numel())
        if src is not None:
            n_rel = n_dead
            new_o, new_s = relocation_values_torch(opacity, par["scaling"], src, ratio, min_opacity)
            for k in NAMES:
                par[k][dead_idx] = par[k][src]
            for k, v in (("opacity", new_o), ("scaling", new_s)):
                par[k][dead_idx] = v
                par[k][src] = v
            for k in NAMES:
                moments[k][0][src] = 0
                moments[k][1][src] = 0
            touched.update(dead=dead_idx, src_relocate=src)
    n_new = max(0, min(cap_max, int(grow * P)) - P)
    if n_new > 0 and P > 0:
        opacity = torch.sigmoid(par["opacity"]).reshape(-1)
        u = torch.rand(n_new, dtype=torch.float32, device=dev, generator=generator)
        _, src, ratio = sample_torch(opacity, u, min_opacity, mask, n_new)
        if src is not None:
            n_add = n_new
            new_o, new_s = relocation_values_torch(opacity, par["scaling"], src, ratio, min_opacity)
            par["opacity"][src] = new_o
            par["scaling"][src] = new_s
            for k in NAMES:
                par[k] = torch.cat((par[k], par[k][src]))
                a, b = moments[k]
                z = torch.zeros((n_new,) + tuple(a.shape[1:]), dtype=a.dtype, device=dev)
                moments[k] = (torch.cat((a, z)), torch.cat((b, z)))
            for key, t in list(extra.items()):
                if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[0] != P:
                    continue
                if key == "mask":
                    extra[key] = torch.cat((t, t[src]))
                elif key == "generation":
                    extra[key] = torch.cat((t, torch.full((n_new,), generation_num or 0, dtype=t.dtype, device=dev)))
                else:
                    extra[key] = torch.cat((t, torch.zeros((n_new,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)))
            touched.update(src_grow=src)
    return par, moments, extra, (P, n_dead, n_rel, n_add), touched


# ----------------------------------------------------------------------------------------------------------------------
# the second size regimes (tests/test_cpu_size_regimes.py, tests/test_gpu_size_regimes.py)
# ----------------------------------------------------------------------------------------------------------------------
N_LARGE_DRAWS = 30000
P_REFINE, DEAD_EVERY, MASK_FRACTION = 300000, 7, 0.6   # the end-to-end refine: every 7th row dead, 60 % of the rows masked in
GROW_REFINE = 1.1                                      # 30 000 appended rows: the growth's copies stride too
F_REST_WORDS = 45                                      # a (P, 15, 3) float32 row
P_VALUE, N_VALUE = 400000, 350001                      # a relocation whose 3-word VALUE rows (scaling) stride: 3 n > 1 048 576


def relocate_case_large(P=P_VALUE, n=N_VALUE, seed=0):
    """A relocation of n dead rows out of P on three narrow groups: ({xyz (P,3), opacity (P,1), scaling (P,3)}, dead (n,) int64
    ascending, src (n,) int64 among the other rows, new_opacity (n,1), new_scaling (n,3)); the new values are a function of
    the source row, as relocation_values makes them, so the draws of one source agree."""
    g = torch.Generator().manual_seed(8200 + seed)
    par = dict(xyz=torch.randn(P, 3, generator=g), opacity=torch.randn(P, 1, generator=g), scaling=torch.randn(P, 3, generator=g))
    perm = torch.randperm(P, generator=g)
    dead, alive = perm[:n].sort().values, perm[n:]
    src = alive[torch.randint(0, int(alive.numel()), (n,), generator=g)]
    table_o, table_s = torch.randn(P, 1, generator=g), torch.randn(P, 3, generator=g)
    return par, dead, src, table_o[src], table_s[src]


def large_sample_case(P, seed=0, min_opacity=0.005):
    """(opacity (P,) f32, mask (P,) bool, u (N_LARGE_DRAWS,) f32): about 5 % of the rows dead, spread over every block, the
    last row and the rows on both sides of 1024 * 1024 among them; u holds both of its ends."""
    rng = np.random.default_rng(8000 + seed)
    opacity = rng.random(P).astype(F)
    opacity[opacity <= F(min_opacity)] = F(0.5)
    opacity[rng.random(P) < 0.05] = F(0.001)
    mask = rng.random(P) < 0.9
    edge = 1024 * 1024
    for r in (3, edge - 1, edge, P - 1):
        opacity[r], mask[r] = F(0.001), True
    opacity[4], mask[4] = np.nextafter(F(min_opacity), F(1)), True
    opacity[P - 2], mask[P - 2] = F(1.0), True  # the last alive row: the largest u must find it
    u = np.minimum(rng.random(N_LARGE_DRAWS).astype(F), F(1 - 2.0 ** -24))
    u[0], u[1] = F(0), F(1 - 2.0 ** -24)
    return opacity, mask, u


def refine_mask_large(P=P_REFINE):
    """The edit mask of the end-to-end refine at scale (CPU generator: the CPU test counts the dead rows inside it)."""
    return torch.rand(P, generator=torch.Generator().manual_seed(8100)) < MASK_FRACTION
