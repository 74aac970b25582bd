"""The densification policy restated twice, for tests/test_cpu_densify_policy.py and tests/test_gpu_densify_policy.py:

  *_np     numpy float32, every operation a single binary32 operation in the order include/gsr.h states for the
           gsr_densify_* entry points (what the kernels must reproduce bit for bit);
  *_torch  the reference's own lines with torch ops (gaussiansplatting/scene/gaussian_model.py:673-815,
           threestudio/systems/GassuianEditor.py:251-281, utils/general_utils.py:78-99), on whatever device the inputs live.

Plus the input cases both test files share."""
import numpy as np
import torch

from oracle.cpu import _quantile_f32

F = np.float32
PS = (1, 2, 255, 256, 257, 70001)  # one lane, the block edges, several blocks with a ragged tail
MAX_GRAD = 0.0002                  # the reference's densify_grad_threshold
PERCENT_DENSE = 0.01
PERCENTS = (0.01, 0.5, 1.0)


def _extent_rounding_up():
    """An extent whose percent_dense * extent rounds UP to binary32: a row with max(scaling) == float32(product) is then above
    the double product, so comparing in double instead of binary32 would flip it."""
    for k in range(1, 200):
        e = 1.0 + k / 16.0
        if float(F(PERCENT_DENSE * e)) > PERCENT_DENSE * e:
            return e
    raise AssertionError("no extent found")


EXTENT = _extent_rounding_up()
T_DENSE = F(PERCENT_DENSE * EXTENT)
assert float(T_DENSE) > PERCENT_DENSE * EXTENT and float(F(MAX_GRAD)) != MAX_GRAD


# ----------------------------------------------------------------------------------------------------------------------
# statistics
# ----------------------------------------------------------------------------------------------------------------------
def stats_np(accum, denom, max_radii, grads, radii):
    """gsr_densify_stats on numpy arrays: returns the three updated arrays (inputs untouched)."""
    accum, denom, max_radii = accum.copy(), denom.copy(), max_radii.copy()
    r = radii[0].copy()
    for x in radii[1:]:
        r = np.maximum(r, x)
    vis = r > 0
    gx = np.zeros(accum.shape[0], F)
    gy = np.zeros(accum.shape[0], F)
    with np.errstate(all="ignore"):
        for g in grads:
            gx = (gx + g[:, 0]).astype(F)
            gy = (gy + g[:, 1]).astype(F)
        norm = np.sqrt(((gx * gx).astype(F) + (gy * gy).astype(F)).astype(F)).astype(F)
        accum[vis] = (accum[vis] + norm[vis]).astype(F)
        denom[vis] = (denom[vis] + F(1)).astype(F)
        max_radii[vis] = np.maximum(max_radii[vis], r[vis].astype(F))
    return accum, denom, max_radii, norm


def stats_torch(accum, denom, max_radii, grads, radii):
    """on_before_optimizer_step, GassuianEditor.py:251-281 with gaussian_model.py:811-815 (in place; accum / denom (P,1))."""
    g = torch.zeros_like(grads[0])
    r = None
    for v, x in zip(grads, radii):
        g = g + v
        r = x if r is None else torch.max(r, x)
    vis = r > 0
    max_radii[vis] = torch.max(max_radii[vis], r[vis].float())
    accum[vis] += torch.norm(g[vis, :2], dim=-1, keepdim=True)
    denom[vis] += 1


# ----------------------------------------------------------------------------------------------------------------------
# selection
# ----------------------------------------------------------------------------------------------------------------------
def select_np(accum, denom, mask, scaling, max_grad, max_densify_percent, percent_dense, extent):
    """gsr_densify_select: (clone_sel, split_sel, nonzero, n_clone, n_split, threshold)."""
    P = accum.shape[0]
    with np.errstate(all="ignore"):
        g = (accum.astype(F) / denom.astype(F)).astype(F)
    g[np.isnan(g)] = F(0)
    g[~mask.astype(bool)] = F(0)
    nnz = int(np.count_nonzero(g))
    thr = F(0)
    if max_densify_percent < 1:
        vp = float(nnz) * max_densify_percent / float(P)
        with np.errstate(all="ignore"):
            thr = _quantile_f32(g, 1.0 - vp)
        g[g < thr] = F(0)
    t_dense = F(percent_dense * extent)
    smax = np.maximum(np.maximum(scaling[:, 0], scaling[:, 1]), scaling[:, 2])
    hot = g >= F(max_grad)
    clone = hot & (smax <= t_dense)
    split = hot & (smax > t_dense)
    return clone, split, nnz, int(clone.sum()), int(split.sum()), thr


def select_torch(accum, denom, mask, scaling, max_grad, max_densify_percent, percent_dense, extent):
    """densify_and_prune :771-777, densify_and_clone :732-739, densify_and_split :676-683 (accum / denom (P,1), mask bool,
    scaling = get_scaling): (clone_sel, split_sel over the ORIGINAL rows, nonzero, n_clone, n_split, threshold | None)."""
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    grads[~mask] = 0.0
    nnz = len(grads.nonzero())
    thr = None
    if max_densify_percent < 1:
        valid_percent = nnz * max_densify_percent / grads.shape[0]
        thr = torch.quantile(grads, 1 - valid_percent)
        grads[grads < thr] = 0.0
    clone = torch.where(torch.norm(grads, dim=-1) >= max_grad, True, False)
    clone = torch.logical_and(clone, torch.max(scaling, dim=1).values <= percent_dense * extent)
    scaling2 = torch.cat((scaling, scaling[clone]))  # densification_postfix appended the clones
    padded = torch.zeros((scaling2.shape[0],), device=accum.device)
    padded[: grads.shape[0]] = grads.squeeze()
    split = torch.where(padded >= max_grad, True, False)
    split = torch.logical_and(split, torch.max(scaling2, dim=1).values > percent_dense * extent)
    P = grads.shape[0]
    assert not bool(split[P:].any())  # the clones' padded gradient is 0
    return clone, split[:P], nnz, int(clone.sum()), int(split.sum()), thr


def select_case(P, kind, seed=0):
    """Inputs of one selection: accum, denom (P) f32, mask (P) bool, scaling (P,3) f32 -- numpy."""
    rng = np.random.default_rng(1000 * seed + P)
    accum = np.zeros(P, F)
    denom = rng.integers(1, 6, P).astype(F)
    mask = rng.random(P) < 0.9
    mg = F(MAX_GRAD)
    idx = np.arange(P)
    if kind == "sparse":  # > 90 % exact zeros (6 % random + 2 % boundary rows); 0/0 rows; rows at and one ulp below max_grad
        nz = rng.random(P) < 0.06
        accum[nz] = (rng.random(int(nz.sum())) * 2e-3).astype(F)
        z = rng.random(P) < 0.05
        denom[z] = 0
        accum[z & (idx % 2 == 0)] = 0  # 0 / 0 -> NaN -> 0; the others x / 0 -> +inf
        at = (idx % 101 == 3)
        accum[at], denom[at] = mg, 1
        below = (idx % 101 == 7)
        accum[below], denom[below] = np.nextafter(mg, F(0)), 1
    elif kind == "zeros":
        pass
    elif kind == "unmasked":
        accum[:] = (rng.random(P) * 2e-3).astype(F)
        mask[:] = False
    elif kind == "one":
        accum[P // 2], denom[P // 2], mask[P // 2] = F(1e-3), 1, True
    elif kind == "lowbyte":  # values that differ only in their lowest byte: every radix pass but the last sees one bin
        bits = (np.uint32(0x3a000000) + rng.integers(0, 256, P).astype(np.uint32)).astype(np.uint32)
        accum[:] = bits.view(F)
        denom[:] = 1
        mask[:] = True
    elif kind == "extremes":  # a denormal, a +inf ratio, 0 / 0
        nz = rng.random(P) < 0.05
        accum[nz] = (rng.random(int(nz.sum())) * 2e-3).astype(F)
        accum[0], denom[0], mask[0] = F(1e-42), 1, True
        if P > 1:
            accum[P - 1], denom[P - 1], mask[P - 1] = 1, 0, True
        if P > 2:
            accum[1], denom[1], mask[1] = 0, 0, True
    else:
        raise ValueError(kind)
    scaling = (float(T_DENSE) * np.exp(rng.uniform(-1.5, 1.5, (P, 3)))).astype(F)
    edge = (idx % 5 == 1)  # max(scaling) exactly at the boundary: cloned, not split
    scaling[edge] = np.minimum(scaling[edge], T_DENSE)
    scaling[edge, idx[edge] % 3] = T_DENSE
    return accum, denom, mask, scaling


KINDS = ("sparse", "zeros", "unmasked", "one", "lowbyte", "extremes")


def same_value(a, b):
    a, b = float(a), float(b)
    return a == b or (a != a and b != b)


# ----------------------------------------------------------------------------------------------------------------------
# split positions
# ----------------------------------------------------------------------------------------------------------------------
def split_np(xyz, scaling, rotation, sel, noise, N, dtype=F):
    """gsr_densify_split_xyz with every operation rounded to `dtype` (float32: the kernel's bits; float64 from the same
    float32 inputs: the yardstick of the error bound).  Returns (new_xyz, sum of |sample| per child, the parents' xyz)."""
    T = dtype
    idx = np.nonzero(sel)[0]
    n = idx.shape[0]
    par = np.tile(idx, N)
    s = (noise.astype(T) * scaling[par].astype(T)).astype(T)
    r = rotation[par].astype(T)
    with np.errstate(all="ignore"):
        nrm = np.sqrt((((r[:, 0] * r[:, 0]).astype(T) + (r[:, 1] * r[:, 1]).astype(T)).astype(T) + (r[:, 2] * r[:, 2]).astype(T)).astype(T)
                      + (r[:, 3] * r[:, 3]).astype(T)).astype(T)
        q = (r / nrm[:, None]).astype(T)
    a, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = T(1), T(2)
    m = lambda u, v: (u * v).astype(T)  # noqa: E731
    R = np.zeros((N * n, 3, 3), T)
    R[:, 0, 0] = one - two * (m(y, y) + m(z, z)).astype(T)
    R[:, 0, 1] = two * (m(x, y) - m(a, z)).astype(T)
    R[:, 0, 2] = two * (m(x, z) + m(a, y)).astype(T)
    R[:, 1, 0] = two * (m(x, y) + m(a, z)).astype(T)
    R[:, 1, 1] = one - two * (m(x, x) + m(z, z)).astype(T)
    R[:, 1, 2] = two * (m(y, z) - m(a, x)).astype(T)
    R[:, 2, 0] = two * (m(x, z) - m(a, y)).astype(T)
    R[:, 2, 1] = two * (m(y, z) + m(a, x)).astype(T)
    R[:, 2, 2] = one - two * (m(x, x) + m(y, y)).astype(T)
    p = xyz[par].astype(T)
    out = np.zeros((N * n, 3), T)
    for i in range(3):
        out[:, i] = (((m(R[:, i, 0], s[:, 0]) + m(R[:, i, 1], s[:, 1])).astype(T) + m(R[:, i, 2], s[:, 2])).astype(T) + p[:, i]).astype(T)
    return out, np.abs(s.astype(np.float64)).sum(axis=1), p.astype(np.float64)


def split_bound(sample_l1, parent_xyz):
    """32 * 2^-24 * ||sample||_1 + 2 * 2^-24 * |xyz_i| per component."""
    u = 2.0 ** -24
    return 32 * u * sample_l1[:, None] + 2 * u * np.abs(parent_xyz)


def build_rotation_torch(r):  # general_utils.py:78-99
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device, dtype=r.dtype)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
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


def split_torch(xyz, scaling, rotation, sel, noise, N):
    """densify_and_split :685-691, the draw replaced by noise * std (torch.normal(0, std) = randn * std)."""
    stds = scaling[sel].repeat(N, 1)
    samples = noise * stds
    rots = build_rotation_torch(rotation[sel]).repeat(N, 1, 1)
    return torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + xyz[sel].repeat(N, 1)


# ----------------------------------------------------------------------------------------------------------------------
# prune
# ----------------------------------------------------------------------------------------------------------------------
def keep_np(opacity, scaling, mask, min_opacity, max_screen_size, extent, max_radii=None, drop=None):
    prune = opacity < F(min_opacity)
    if max_radii is not None:
        prune = prune | (max_radii > F(max_screen_size))
    prune = prune | (scaling.max(axis=1) > F(0.1 * extent))
    prune = prune & mask.astype(bool)
    keep = ~prune
    if drop is not None:
        keep = keep & ~drop.astype(bool)
    return keep


def keep_torch(opacity, scaling, mask, min_opacity, max_screen_size, extent, max_radii=None, drop=None):
    """:787-794 (opacity (P,1) = get_opacity), then the split parents' removal."""
    prune_mask = (opacity < min_opacity).squeeze(-1)
    if max_radii is not None:
        prune_mask = torch.logical_or(prune_mask, max_radii > max_screen_size)
    prune_mask = torch.logical_or(prune_mask, scaling.max(dim=1).values > 0.1 * extent)
    prune_mask = torch.logical_and(prune_mask, mask)
    keep = ~prune_mask
    if drop is not None:
        keep = keep & ~drop
    return keep


# ----------------------------------------------------------------------------------------------------------------------
# the whole of densify_and_prune on plain tensors (the lines tests/test_gpu_edit_loop.py:206-255 use)
# ----------------------------------------------------------------------------------------------------------------------
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def densify_and_prune_torch(par, moments, extra, noise_fn, *, max_grad, max_densify_percent, min_opacity, extent,
                            max_screen_size, percent_dense, N=2, generation_num=0, with_bound=True,
                            screen_prune="reference"):
    """gaussian_model.py:768-797 with its two postfixes and two prunes, on {name: tensor} `par`, {name: (exp_avg,
    exp_avg_sq)} `moments` and the bookkeeping `extra`.  noise_fn(n) -> (n,3) standard-normal numbers.  Returns the new
    (par, moments, extra, (before, n_clone, n_split, n_pruned)); extra["xyz_bound"] (rows,3) float64 is split_bound for the
    rows that are split children and 0 for all others, extra["xyz64"] the float64 evaluation of the children's positions
    from the same float32 inputs (other rows: their xyz) (with_bound=False: neither is computed -- tools/
    bench_densify_policy.py times this function).  screen_prune="accumulated" tests the max_radii2D gathered since the last
    densification (new rows: 0) instead of the zeros densification_postfix left.  No input tensor is written to."""
    par, moments = dict(par), dict(moments)
    mask, gen = extra["mask"], extra["generation"]
    dev = mask.device
    side = dict(radii=extra["max_radii2D"].reshape(-1))  # carried through every cat (zeros unless given) and prune
    if with_bound:
        side.update(bound=torch.zeros(par["xyz"].shape, dtype=torch.float64, device=dev), xyz64=par["xyz"].double())

    def cat(ext):  # cat_tensors_to_optimizer :609-641 + densification_postfix :643-671
        for k in NAMES:
            a, b = moments[k]
            moments[k] = (torch.cat((a, torch.zeros_like(ext[k])), dim=0), torch.cat((b, torch.zeros_like(ext[k])), dim=0))
            par[k] = torch.cat((par[k], ext[k]), dim=0)
        n = ext["xyz"].shape[0]
        for k, v in side.items():
            new = ext[k] if k in ext else (ext["xyz"].double() if k == "xyz64" else torch.zeros((n,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev))
            side[k] = torch.cat((v, new))

    def prune(remove):  # prune_points :593-607
        keep = ~remove
        for k in NAMES:
            par[k] = par[k][keep]
            moments[k] = (moments[k][0][keep], moments[k][1][keep])
        for k in side:
            side[k] = side[k][keep]
        return keep

    before = par["xyz"].shape[0]
    grads = extra["xyz_gradient_accum"] / extra["denom"]
    grads[grads.isnan()] = 0.0
    grads[~mask] = 0.0
    if max_densify_percent < 1:
        valid_percent = len(grads.nonzero()) * max_densify_percent / grads.shape[0]
        threshold = torch.quantile(grads, 1 - valid_percent)
        grads[grads < threshold] = 0.0
    # densify_and_clone
    sel = (torch.norm(grads, dim=-1) >= max_grad) & (torch.exp(par["scaling"]).max(dim=1).values <= percent_dense * extent)
    n_clone = int(sel.sum())
    cat({k: par[k][sel] for k in NAMES})
    assert len(torch.nonzero(mask[sel] == 0)) == 0, "nontarget area should not be densified"  # :756-758
    mask = torch.cat([mask, mask[sel]], dim=0)
    gen = torch.cat([gen, torch.full((n_clone,), generation_num, dtype=torch.int64, device=dev)])
    # densify_and_split
    n_init = par["xyz"].shape[0]
    padded = torch.zeros((n_init,), device=dev)
    padded[: grads.shape[0]] = grads.squeeze()
    get_scaling = torch.exp(par["scaling"])
    sel = (padded >= max_grad) & (get_scaling.max(dim=1).values > percent_dense * extent)
    n_split = int(sel.sum())
    stds = get_scaling[sel].repeat(N, 1)
    noise = noise_fn(stds.size(0))
    samples = noise * stds
    rots = build_rotation_torch(par["rotation"][sel]).repeat(N, 1, 1)
    ext = dict(xyz=torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + par["xyz"][sel].repeat(N, 1),
               scaling=torch.log(get_scaling[sel].repeat(N, 1) / (0.8 * N)), rotation=par["rotation"][sel].repeat(N, 1),
               f_dc=par["f_dc"][sel].repeat(N, 1, 1), f_rest=par["f_rest"][sel].repeat(N, 1, 1),
               opacity=par["opacity"][sel].repeat(N, 1))
    u = 2.0 ** -24
    if with_bound:
        ext["bound"] = 32 * u * samples.double().abs().sum(dim=1, keepdim=True) + 2 * u * par["xyz"][sel].repeat(N, 1).double().abs()
        rots64 = build_rotation_torch(par["rotation"][sel].double()).repeat(N, 1, 1)
        ext["xyz64"] = torch.bmm(rots64, (noise.double() * stds.double()).unsqueeze(-1)).squeeze(-1) + par["xyz"][sel].repeat(N, 1).double()
    cat(ext)
    mask = torch.cat([mask] + [mask[sel]] * N, dim=0)
    gen = torch.cat([gen] + [torch.full((n_split,), generation_num, dtype=torch.int64, device=dev)] * N)
    keep = prune(torch.cat((sel, torch.zeros(N * n_split, device=dev, dtype=torch.bool))))
    mask, gen = mask[keep], gen[keep]
    # prune; densification_postfix has reset max_radii2D to zeros
    P2 = par["xyz"].shape[0]
    prune_mask = (torch.sigmoid(par["opacity"]) < min_opacity).squeeze(-1)
    if max_screen_size:
        big_vs = (side["radii"] if screen_prune == "accumulated" else torch.zeros((P2,), device=dev)) > max_screen_size
        big_ws = torch.exp(par["scaling"]).max(dim=1).values > 0.1 * extent
        prune_mask = torch.logical_or(torch.logical_or(prune_mask, big_vs), big_ws)
    prune_mask = torch.logical_and(prune_mask, mask)
    n_pruned = int(prune_mask.sum())
    keep = prune(prune_mask)
    mask, gen = mask[keep], gen[keep]
    final = par["xyz"].shape[0]
    new_extra = dict(xyz_gradient_accum=torch.zeros((final, 1), device=dev), denom=torch.zeros((final, 1), device=dev),
                     max_radii2D=torch.zeros((final,), device=dev), mask=mask, generation=gen, xyz_bound=side.get("bound"), xyz64=side.get("xyz64"))
    return par, moments, new_extra, (before, n_clone, n_split, n_pruned)


# ----------------------------------------------------------------------------------------------------------------------
# the second size regimes of the row-surgery and policy kernels (tests/test_cpu_size_regimes.py checks that every size
# below lies where it claims, tests/test_gpu_size_regimes.py runs the kernels there)
# ----------------------------------------------------------------------------------------------------------------------
SCAN_EDGE = 1024 * 1024             # rows one trip of compact_scan_kernel covers: 1024 blocks of 1024 rows
PC = SCAN_EDGE + 1024 + 1           # 1026 row blocks: the scan's second trip holds two, the last with one row
PD = 1024 * 256 + 257               # 1026 blocks of 256 rows: the densify kernels' grid stride, ragged
P_APPEND, N_APPEND = 400001, 12345  # (P + n) * 180 bytes > 4096 blocks * 256 threads * 64 bytes
P_COUNTS = 1025                     # the tensor-count cases: two row blocks, the second with one row
TENSOR_COUNTS = (33, 65)            # two and three Python chunks of 32 tensors
ROW_WIDTHS = (1, 3, 4, 12, 16, 20, 180, 2, 8)  # bytes per row, cycled over the tensors of a count case


def kernel_constants():
    """The thresholds the size-regime tests rely on, parsed out of the sources' text: every `constexpr int NAME = value`
    of the .hip / .h files (names resolved through one another), the step of compact_scan_kernel's carry loop, the grid
    caps of append_rows_kernel and mcmc_scatter_kernel with append's bytes per block, and the Python chunk of densify.py."""
    import os
    import re

    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussianeditor_amd")

    def text(*parts):
        with open(os.path.join(pkg, *parts)) as f:
            return f.read()

    src = {n: text("csrc", *n.split("/")) for n in ("gsr_kernels.h", "gsr_common.h", "gsr_compact.hip", "gsr_densify.hip",
                                                    "gsr_mcmc.hip", "loss/gsr_loss.hip")}
    raw = {}
    for body in src.values():
        for line in re.findall(r"^\s*constexpr\s+int\s+([^;]*);", body, flags=re.M):
            for part in line.split(","):
                m = re.fullmatch(r"\s*(\w+)\s*=\s*(\w+)\s*", part)
                if m:
                    raw[m.group(1)] = m.group(2)

    def value(name):
        v = raw[name]
        return int(v) if v.isdigit() else value(v)

    out = {k: value(k) for k in ("VIEW_MSG_ROWS", "CMP_ROWS", "CMP_MAX_TENSORS", "CMP_TENSORS_PER_BLOCK", "SPLIT_ROWS", "DNS_BLOCK",
                                 "DNS_MAX_BLOCKS", "MC_BLOCK", "MC_MAX_TENSORS", "LT_W", "LT_H", "LTHREADS")}

    def one(pattern, body, what):
        found = set(re.findall(pattern, body))
        assert len(found) == 1, (what, found)
        return found.pop()

    out["SCAN_CHUNK"] = int(one(r"base < nb; base \+= (\d+)\)", src["gsr_compact.hip"], "compact_scan_kernel's step"))
    a, b = one(r"\(most \+ (\d+)ull \* (\d+)ull - 1\)", src["gsr_compact.hip"], "append_rows_kernel's bytes per block")
    out["APPEND_BLOCK_BYTES"] = int(a) * int(b)
    a, b = one(r"want > (\d+) \? (\d+) : want", src["gsr_compact.hip"], "append_rows_kernel's grid cap")
    assert a == b
    out["APPEND_MAX_BLOCKS"] = int(a)
    a, b = one(r"want > (\d+) \? (\d+) : want", src["gsr_mcmc.hip"], "mcmc_scatter_kernel's grid cap")
    assert a == b
    out["MC_SCATTER_MAX_BLOCKS"] = int(a)
    out["PY_CHUNK"] = int(one(r"range\(0, len\(srcs\), (\d+)\)", text("densify.py"), "densify.py's chunk of tensors"))
    return out


def compact_tensors(P, seed=0):
    """The tensors of test_compact_rows_equals_boolean_indexing (its copy of the mask replaced by a random bool tensor) and
    three further narrow ones -- 2-, 4- and 20-byte rows -- so that compact_apply_kernel runs two blockIdx.y groups of 8."""
    g = torch.Generator().manual_seed(7000 + seed)
    return [torch.randn(P, 3, generator=g), torch.randn(P, 15, 3, generator=g), torch.randn(P, 1, generator=g),
            torch.randn(P, 4, generator=g), torch.arange(P, dtype=torch.int64), torch.rand(P, generator=g) < 0.5,
            torch.randn(P, generator=g), torch.randint(0, 255, (P, 3), generator=g, dtype=torch.uint8),
            torch.randint(-30000, 30000, (P,), generator=g, dtype=torch.int16), torch.randint(0, 2 ** 31 - 1, (P,), generator=g, dtype=torch.int32),
            torch.randn(P, 5, generator=g)]


def compact_masks(P, seed=0):
    """name -> (P,) bool keep mask: a random half (with the rows on both sides of SCAN_EDGE and the last one); only the rows
    from SCAN_EDGE on (carry 0: the output comes from the scan's second trip alone); every row below SCAN_EDGE and a random
    half of the tail with the last row (carry SCAN_EDGE); the very last row alone.  P > SCAN_EDGE."""
    assert P > SCAN_EDGE
    g = torch.Generator().manual_seed(7100 + seed)
    rows = torch.arange(P)
    half = torch.rand(P, generator=g) < 0.5
    head = (rows < SCAN_EDGE) | half
    head[P - 1] = True
    last = torch.zeros(P, dtype=torch.bool)
    last[P - 1] = True
    rnd = torch.rand(P, generator=g) < 0.5
    rnd[[SCAN_EDGE - 1, SCAN_EDGE, P - 1]] = True  # (cut to SCAN_EDGE + 1 rows its last block of one row has its survivor)
    return {"random": rnd, "tail_only": rows >= SCAN_EDGE, "head_kept": head, "last_row": last}


def split_case_large(P, n_random=300, N=2, seed=0):
    """test_split_positions' inputs at P rows: (xyz, scaling, rotation, sel, noise) numpy; the selection holds rows 0,
    SCAN_EDGE - 1, SCAN_EDGE and P - 1 and n_random random ones."""
    rng = np.random.default_rng(7200 + seed)
    xyz = (rng.standard_normal((P, 3)) * 3).astype(F)
    scaling = np.exp(rng.uniform(-6, -1, (P, 3))).astype(F)
    rot = rng.standard_normal((P, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(0.1), np.log(10), (P, 1)))).astype(F)
    sel = np.zeros(P, bool)
    sel[rng.choice(P, n_random, replace=False)] = True
    sel[[0, SCAN_EDGE - 1, SCAN_EDGE, P - 1]] = True
    noise = rng.standard_normal((N * int(sel.sum()), 3)).astype(F)
    return xyz, scaling, rot, sel, noise


def message_case_large(P, seed=0):
    """Synthetic dense gradients of one view for the view-message plan: ([means3D (P,3), scales (P,3), rotations (P,4),
    means2D (P,3), opacities (P,1)], rgb (P,3), touched (P,) bool) as torch tensors.  About 1 % of the rows are touched, the
    last row of every one of the last three blocks among them; a touched row is non-zero in tensor (row % 6) and in a random
    half of the others, so that no single tensor gives the mask away."""
    g = torch.Generator().manual_seed(7300 + seed)
    touched = torch.rand(P, generator=g) < 0.01
    touched[[0, SCAN_EDGE - 1, SCAN_EDGE, SCAN_EDGE + 1023, P - 1]] = True
    rows = torch.arange(P)
    out = []
    for i, k in enumerate((3, 3, 4, 3, 1, 3)):
        on = touched & ((rows % 6 == i) | (torch.rand(P, generator=g) < 0.5))
        v = torch.randn(P, k, generator=g)
        v[v == 0] = 1.0
        out.append(torch.where(on[:, None], v, torch.zeros(())))  # (+0 elsewhere: v * False would leave -0)
    return out[:5], out[5], touched


def count_case(count, P=P_COUNTS, seed=0):
    """`count` uint8 tensors of P rows whose widths cycle through ROW_WIDTHS, with their n-row extensions (every third
    None: zero rows) -> (tensors, extensions, n)."""
    g = torch.Generator().manual_seed(7400 + count + seed)
    n = 77
    ts = [torch.randint(0, 256, (P, ROW_WIDTHS[i % len(ROW_WIDTHS)]), generator=g, dtype=torch.uint8) for i in range(count)]
    ex = [None if i % 3 == 2 else torch.randint(0, 256, (n, t.shape[1]), generator=g, dtype=torch.uint8) for i, t in enumerate(ts)]
    return ts, ex, n
