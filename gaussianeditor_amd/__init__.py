"""MI355X-native differentiable 3D-Gaussian-splatting rasterizer: a drop-in for the
`diff_gaussian_rasterization` extension used by buaacyw/GaussianEditor.

    import gaussianeditor_amd; gaussianeditor_amd.install()
    # from here on `import diff_gaussian_rasterization` resolves to the HIP implementation
"""
import sys as _sys

__version__ = "0.1.0"


def install() -> None:
    """Register the drop-in under the reference's module name so that unmodified reference
    code (gaussian_renderer/__init__.py:14-17, scene/gaussian_model.py:32) imports it."""
    from . import diff_gaussian_rasterization as _dgr

    _sys.modules["diff_gaussian_rasterization"] = _dgr
    _sys.modules["diff_gaussian_rasterization._C"] = _dgr._C
    # the other two hard imports of scene/gaussian_model.py (:24, :26)
    from . import simple_knn as _knn

    _sys.modules["simple_knn"] = _knn
    _sys.modules["simple_knn._C"] = _knn._C
    try:  # a real `plyfile` installation wins
        import plyfile as _ply  # noqa: F401
    except ImportError:
        from .compat import plyfile as _ply

        _sys.modules["plyfile"] = _ply


def __getattr__(name: str):
    # contribution statistics / pick buffer (contrib.py), resolved on first use: importing the package loads no torch code
    if name in ("ContributionStats", "trace_view"):
        from . import contrib

        return getattr(contrib, name)
    # similarity transforms of Gaussians (transform.py), likewise
    if name in ("transform_rows", "transform_gaussians"):
        from . import transform

        return getattr(transform, name)
    # surface normals (normals.py), likewise
    if name in ("gaussian_normals", "depth_to_normals", "normal_consistency_loss", "camera_intrinsics"):
        from . import normals

        return getattr(normals, name)
    # Mip-Splatting's 3D filter (filter3d.py), likewise
    if name in ("pack_cameras", "compute_3d_filter", "apply_3d_filter", "bake_3d_filter"):
        from . import filter3d

        return getattr(filter3d, name)
    # TSDF fusion and mesh extraction (tsdf.py), likewise
    if name in ("TSDFVolume", "extract_mesh", "save_mesh_ply", "load_mesh_ply"):
        from . import tsdf

        return getattr(tsdf, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def set_tile_bounds(mode: str) -> None:
    """Opt-in binning rule: the default of the GSR_FLAG_TILE_BOUNDS_ALPHA flag (include/gsr.h) for renders started
    from now on (a render's backward always reuses the flags of its forward; `options.override` is per thread).

    "reference" (default): every Gaussian is binned into the reference's square of side 2 ceil(3 sigma_max); the
    internal state (num_rendered, instance lists, n_contrib) equals the reference's bit for bit.
    "alpha": only into the tiles its alpha >= 1/255 level set can reach.  Images, depths, radii, traced weights and
    gradients are unchanged (every dropped instance would have been skipped at each pixel); fewer instances are
    sorted and walked."""
    from . import options

    if mode not in ("reference", "alpha"):
        raise ValueError('tile bounds: "reference" or "alpha"')
    f = options.default_flags() & ~options.FLAG_TILE_BOUNDS_ALPHA  # the default only: never a thread's override()
    options.set_default_flags(f | (options.FLAG_TILE_BOUNDS_ALPHA if mode == "alpha" else 0))


def get_tile_bounds() -> str:
    from . import options

    return "alpha" if options.default_flags() & options.FLAG_TILE_BOUNDS_ALPHA else "reference"


def set_fast_exp(on: bool) -> None:
    """Opt-in: the default of GSR_FLAG_FAST_EXP (include/gsr.h) -- exp() of the blend loops on the hardware's
    v_exp_f32 instead of the exactly specified polynomial.  Results stay within the 1e-5 parity bar; n_contrib /
    final_T are then no longer bit-identical to the CPU oracle."""
    from . import options

    f = options.default_flags() & ~options.FLAG_FAST_EXP
    options.set_default_flags(f | (options.FLAG_FAST_EXP if on else 0))


def get_fast_exp() -> bool:
    from . import options

    return bool(options.default_flags() & options.FLAG_FAST_EXP)


def set_depth_grad(on: bool) -> None:
    """Opt-in: the default of GSR_FLAG_DEPTH_GRAD (include/gsr.h) -- a loss on the rendered depth image (the third output
    of the rasterizer, `render_pkg["depth_3dgs"]`) reaches means3D, scales, rotations, opacities and colours.  Off
    (default): the depth image carries no gradient, exactly as in the reference.  Like every flag it is read once by a
    render's forward and reused by that render's backward."""
    from . import options

    f = options.default_flags() & ~options.FLAG_DEPTH_GRAD
    options.set_default_flags(f | (options.FLAG_DEPTH_GRAD if on else 0))


def get_depth_grad() -> bool:
    from . import options

    return bool(options.default_flags() & options.FLAG_DEPTH_GRAD)


def set_abs_grad(on: bool) -> None:
    """Opt-in: the default of GSR_FLAG_ABS_GRAD (include/gsr.h) -- the backward of a render also leaves the ABSOLUTE
    screen-space gradient on the `means2D` tensor the rasterizer was given (`render()`'s `viewspace_points`), as
    `means2D.absgrad`: (P,3) float32, per Gaussian the sums over pixels of the absolute values of the per-pixel terms of
    `means2D.grad[:, :2]`, z = 0 -- the densification statistic of AbsGS (gsplat's `absgrad`), which does not cancel for a
    large splat that straddles an edge.  A new tensor per backward, assigned, never accumulated.  Off (default): the
    attribute is neither set nor cleared.  Images and every other gradient are the same either way."""
    from . import options

    f = options.default_flags() & ~options.FLAG_ABS_GRAD
    options.set_default_flags(f | (options.FLAG_ABS_GRAD if on else 0))


def get_abs_grad() -> bool:
    from . import options

    return bool(options.default_flags() & options.FLAG_ABS_GRAD)


def set_alpha_output(on: bool) -> None:
    """Opt-in: the default of FLAG_ALPHA_OUT (options.py; a bit of the binding, the library has none) -- `render()` also
    returns the alpha image, `out["alpha"]`: (1,H,W) float32, per pixel the accumulated opacity A = 1 - prod (1 - alpha_i)
    over the Gaussians the pixel blended, i.e. 1 - the final transmittance.  It carries a gradient (a mask / silhouette loss
    reaches means3D, scales, rotations and opacities), and `depth_3dgs / alpha.clamp_min(eps)` is the normalised depth.
    `render(..., return_alpha=True)` and `GaussianRasterizer.forward(..., return_alpha=True)` ask for it per call whatever
    the flag says.  Off (default): the dict has no such key and nothing else changes."""
    from . import options

    f = options.default_flags() & ~options.FLAG_ALPHA_OUT
    options.set_default_flags(f | (options.FLAG_ALPHA_OUT if on else 0))


def get_alpha_output() -> bool:
    from . import options

    return bool(options.default_flags() & options.FLAG_ALPHA_OUT)


def set_pose_grad(on: bool) -> None:
    """Opt-in: the default of FLAG_POSE_GRAD (options.py; a bit of the binding, the library has none) -- the camera becomes
    a differentiable input.  A render whose `viewmatrix`, `projmatrix` or `campos` (`world_view_transform`,
    `full_proj_transform`, `camera_center` of the camera `render()` is given) requires a gradient returns, from its
    backward, the raw partial derivative with respect to each of the three, and autograd carries them on through whatever
    torch code built the tensors from a pose (`gaussianeditor_amd.pose.camera_tensors`).  Gaussians may be frozen: a
    pose-only optimisation works.  Off (default), or with a camera that requires no gradient: every render is the call it
    always was, and a camera that does require one silently gets none, as in the reference."""
    from . import options

    f = options.default_flags() & ~options.FLAG_POSE_GRAD
    options.set_default_flags(f | (options.FLAG_POSE_GRAD if on else 0))


def get_pose_grad() -> bool:
    from . import options

    return bool(options.default_flags() & options.FLAG_POSE_GRAD)


def set_antialiasing(on: bool) -> None:
    """Opt-in: the default of GSR_FLAG_ANTIALIAS (include/gsr.h) -- the opacity-compensated 2D filter of antialiased
    3DGS rasterizers.  Every Gaussian is blended with opacity * h, h = sqrt(max(2.5e-5, det(S) / det(S + 0.3 I))) of its
    undilated screen-space covariance S, so a sub-pixel Gaussian keeps its integrated weight instead of spreading its full
    opacity over the 0.3 px^2 dilation.  Turn it on for a scene trained with such a rasterizer.  Off (default): the
    reference's image.  Read once by a render's forward and reused by that render's backward."""
    from . import options

    f = options.default_flags() & ~options.FLAG_ANTIALIAS
    options.set_default_flags(f | (options.FLAG_ANTIALIAS if on else 0))


def get_antialiasing() -> bool:
    from . import options

    return bool(options.default_flags() & options.FLAG_ANTIALIAS)


def set_view_reuse(on: bool) -> None:
    """View reuse (default on; `GSR_VIEW_REUSE=0` in the environment turns it off): a colour-override render of the view
    the rasterizer rendered last -- the reference's second `render(..., override_color=...)` of every training view and
    GUI frame -- runs the blend kernel alone on that render's state, after PROVING that camera, positions, scales,
    rotations and opacities are the first render's (diff_gaussian_rasterization/_reuse.py).  Off: every render runs in full."""
    from .diff_gaussian_rasterization import _reuse

    _reuse.set_view_reuse(on)


def get_view_reuse() -> bool:
    from .diff_gaussian_rasterization import _reuse

    return _reuse.view_reuse()
