"""Drop-in replacement for the reference's `diff_gaussian_rasterization` Python package
(DGR/diff_gaussian_rasterization/__init__.py, 364 lines): same public names, same call
signatures, same return arities, same exceptions -- backed by the gfx950 HIP library
instead of the CUDA extension.

Public surface (reference line numbers):
    GaussianRasterizationSettings   :228-240   NamedTuple of 12 fields
    GaussianRasterizer              :243-364   nn.Module with forward / markVisible / apply_weights
    rasterize_gaussians             :26-47
    _RasterizeGaussians             :50-225    autograd.Function

To let unmodified GaussianEditor code `import diff_gaussian_rasterization`, call
`gaussianeditor_amd.install()` once.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C, _reuse
from .. import options as _options

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "_RasterizeGaussians"]


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _snapshot(args):
    """CPU deep copy of a native call's arguments (reference: cpu_deep_copy_tuple, :18-23)."""
    return tuple(a.cpu().clone() if isinstance(a, torch.Tensor) else a for a in args)


def _call_native(fn, args, debug: bool, dump_path: str, message: str):
    """Invoke a `_C` entry point; in debug mode dump the inputs on failure, as the
    reference does (:88-107 forward, :180-200 backward)."""
    if not debug:
        return fn(*args)
    saved = _snapshot(args)  # before anything can corrupt them
    try:
        return fn(*args)
    except Exception:
        torch.save(saved, dump_path)
        print(message)
        raise


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, aux_colors=None, return_alpha=False, viewmatrix=None, projmatrix=None, campos=None,
                features=None, distortion=None):
        # (distortion: None, or the (near, far) pair of a render with `return_distortion` -- (0.0, 0.0): the linear depth --,
        #  whose (1,H,W) depth-distortion image is returned behind everything else; passed by such a render only)
        # (features: (P,C) per-Gaussian features, composited into a differentiable (C,H,W) image that is returned last --
        #  passed by a render with `features=` only; every other render passes the argument tuple it always passed)
        # (viewmatrix, projmatrix, campos: rs.viewmatrix / rs.projmatrix / rs.campos once more, as inputs autograd can see --
        #  passed under FLAG_POSE_GRAD only, and only when one of them requires a gradient: _pose_inputs)
        rs = raster_settings
        # behaviour flags (include/gsr.h: GSR_FLAG_*) are fixed per render: read once here, reused by the backward
        flags = _options.current_flags()
        # a render no input of which requires a gradient (the viewer, torch.no_grad()) will never see a backward: the
        # preprocessing then leaves out what only the backward reads (GSR_FLAG_FORWARD_ONLY)
        fwd_flags = flags if any(ctx.needs_input_grad) else flags | _options.FLAG_FORWARD_ONLY
        run = lambda fn: (lambda *a: fn(*a, flags=fwd_flags))  # noqa: E731
        # argument order of _C.rasterize_gaussians (rasterize_points.h:17-36)
        args = (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh,
                rs.sh_degree, rs.campos, rs.prefiltered, rs.debug)
        num_rendered, color, depth, radii, geomBuffer, binningBuffer, imgBuffer = _call_native(
            run(_C.rasterize_gaussians), args, rs.debug, "snapshot_fw.dump",
            "\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
        ctx.raster_settings = rs
        ctx.gsr_flags = flags
        ctx.gsr_pose = viewmatrix is not None
        ctx.num_rendered = num_rendered
        if flags & _options.FLAG_ABS_GRAD:
            ctx.gsr_means2D = means2D  # the caller's screen-space tensor: the backward assigns its `.absgrad`
        # view reuse (_reuse.py): a following colour-override render of this view runs the blend kernel on this state
        _reuse.remember(rs, flags, means3D, scales, rotations, opacities, cov3Ds_precomp, num_rendered, geomBuffer,
                        binningBuffer, imgBuffer, radii, depth)
        ctx.gsr_features = features is not None
        dist_out = dist_moments = None
        if distortion is not None:
            # extension: the distortion image, one forward kernel on the state K6 just left; the per-pixel moments for the
            # backward only where there will be one
            dist_out, dist_moments = _call_native(
                run(_C.rasterize_distortion), (int(means3D.shape[0]), num_rendered, geomBuffer, binningBuffer, imgBuffer,
                                               rs.image_height, rs.image_width, None if distortion == (0.0, 0.0) else distortion,
                                               any(ctx.needs_input_grad), rs.debug), rs.debug, "snapshot_fw.dump",
                "\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
        ctx.gsr_distortion_slot = distortion is not None  # (the image is an output, the (near, far) pair input 15)
        ctx.gsr_distortion = distortion if dist_moments is not None else None
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer,
                              binningBuffer, imgBuffer, *((features,) if features is not None else ()),
                              *((dist_moments,) if dist_moments is not None else ()))
        ctx.mark_non_differentiable(radii)
        # radii / depth never carry a gradient: do not let autograd fill zero tensors for them on every backward
        ctx.set_materialize_grads(False)
        # extension: the alpha image 1 - final_T out of the image state K6 just left, a differentiable last output
        ctx.gsr_alpha = return_alpha
        alpha = (_C.alpha_image(imgBuffer, rs.image_height, rs.image_width),) if return_alpha else ()
        if features is not None:
            # extension: the feature image, one forward kernel on the state K6 just left; differentiable, the last output
            alpha = alpha + (_call_native(
                run(_C.rasterize_features), (features.detach(), num_rendered, geomBuffer, binningBuffer, imgBuffer,
                                             rs.image_height, rs.image_width, rs.debug), rs.debug, "snapshot_fw.dump",
                "\nAn error occured in forward. Please forward snapshot_fw.dump for debugging."),)
        if dist_out is not None:
            alpha = alpha + (dist_out,)
        if aux_colors is None:
            return (color, radii, depth) + alpha
        # extension: a second, gradient-free image of the same view with other colours (K6 only)
        aux = _call_native(run(_C.rasterize_gaussians_aux),
                           (rs.bg, aux_colors.detach(), num_rendered, geomBuffer, binningBuffer, imgBuffer, rs.image_height,
                            rs.image_width, rs.debug), rs.debug, "snapshot_fw.dump",
                           "\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
        ctx.mark_non_differentiable(radii, aux)
        return (color, radii, depth, aux) + alpha

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_depth, *grad_rest):  # (grad_rest: of aux, alpha, features, distortion)
        # grad_radii is ignored exactly as in the reference (:137, :155-177); so is grad_depth -- depth is a forward-only
        # output -- unless this render ran with FLAG_DEPTH_GRAD (gaussianeditor_amd.set_depth_grad)
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer,
         imgBuffer) = ctx.saved_tensors[:10]
        dist = None
        has_dist_out = ctx.gsr_distortion_slot  # (its image is the last output)
        if has_dist_out:
            if ctx.gsr_distortion is not None and grad_rest[-1] is not None:
                dist = (ctx.saved_tensors[-1], grad_rest[-1], ctx.gsr_distortion)
            grad_rest = grad_rest[:-1]
        feats = None
        if ctx.gsr_features:  # the feature image is the last output, the alpha image the one in front of it
            feats = (ctx.saved_tensors[10], grad_rest[-1])
            grad_rest = grad_rest[:-1]
        return _backward(ctx, (means3D, sh, colors_precomp, scales, rotations, cov3Ds_precomp),
                         (ctx.num_rendered, radii, geomBuffer, binningBuffer, imgBuffer),
                         (grad_out_color, grad_depth, grad_rest[-1] if ctx.gsr_alpha else None), dump=True, features=feats,
                         **({"distortion": dist, "distortion_slot": True} if has_dist_out else {}),
                         grad_allocator=getattr(ctx, "gsr_grad_allocator", None))


def _backward(ctx, inputs, state, grads, dump=False, features=None, distortion=None, distortion_slot=False, **route_kw):
    """The backward of both autograd functions: _C.rasterize_gaussians_backward on `inputs` (means3D, sh, colors_precomp, scales,
    rotations, cov3Ds_precomp) and the `state` their forward left (num_rendered, radii, geomBuffer, binningBuffer, imgBuffer),
    with `grads`, the gradients of the colour, depth and alpha outputs -> one gradient slot per forward() input (:213-225).
    The extension keywords are passed only where there is something to pass -- a depth gradient of a render that ran with
    FLAG_DEPTH_GRAD (depth is a forward-only output otherwise), the tensor for the absolute screen-space gradient under
    FLAG_ABS_GRAD (a new (P,3) one per backward, assigned to `means2D.absgrad`), a gradient of an alpha image that was
    returned AND used, `features` = (the features, the gradient of their image) of a render with `features=` whose feature
    image was used (one more gradient slot then), `distortion` = (the moments, the gradient of the image, its (near, far)) of
    a render with `return_distortion` whose distortion image was used (`distortion_slot`: the render had that input, one
    more gradient slot behind the features'); `route_kw` likewise -- so that every other backward is the
    reference's call, to any `_C` backend."""
    rs, flags = ctx.raster_settings, ctx.gsr_flags
    means3D, sh, colors_precomp, scales, rotations, cov3Ds_precomp = inputs
    num_rendered, radii, geomBuffer, binningBuffer, imgBuffer = state
    grad_out_color, grad_depth, grad_alpha = grads
    kw = dict(route_kw, flags=flags)
    pose = None
    if getattr(ctx, "gsr_pose", False):  # the camera tensors were inputs of this render (FLAG_POSE_GRAD)
        pose = kw["pose_grad_out"] = torch.empty((35,), dtype=torch.float32, device=means3D.device)
    if (flags & _options.FLAG_DEPTH_GRAD) and grad_depth is not None:
        kw["dL_dout_depth"] = grad_depth
    abs_grad = None
    if flags & _options.FLAG_ABS_GRAD:
        abs_grad = kw["abs_grad_out"] = torch.empty((means3D.shape[0], 3), dtype=torch.float32, device=means3D.device)
    if grad_alpha is not None:
        kw["dL_dout_alpha"] = grad_alpha
    grad_features = None
    if features is not None and features[1] is not None:
        grad_features = torch.zeros_like(features[0], memory_format=torch.contiguous_format)  # (added into: zeroed here)
        kw.update(features=features[0], dL_dout_features=features[1], feature_grad_out=grad_features)
    if distortion is not None:
        kw.update(distortion_moments=distortion[0], dL_dout_distortion=distortion[1])
        if distortion[2] != (0.0, 0.0):
            kw["distortion_near_far"] = distortion[2]
    if grad_out_color is None:  # only the depth, alpha, feature and / or distortion output was used downstream
        grad_out_color = torch.zeros((3, rs.image_height, rs.image_width), dtype=torch.float32, device=means3D.device)
    # argument order of _C.rasterize_gaussians_backward (rasterize_points.h:38-60)
    args = (rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
            rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, sh, rs.sh_degree, rs.campos,
            geomBuffer, num_rendered, binningBuffer, imgBuffer, rs.debug)
    (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
     grad_rotations) = _call_native(
         lambda *a: _C.rasterize_gaussians_backward(*a, **kw), args, rs.debug and dump, "snapshot_bw.dump",
         "\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
    if abs_grad is not None:
        ctx.gsr_means2D.absgrad = abs_grad
    out = (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_scales, grad_rotations,
           grad_cov3Ds_precomp, None, None, None)
    tail = () if features is None and not distortion_slot else (grad_features,)  # (input 14; the camera tensors keep 11 .. 13)
    if distortion_slot:
        tail = tail + (None,)  # (input 15: the (near, far) pair)
    if pose is None:
        return out + ((None, None, None) + tail if tail else ())
    # three more slots, in the layout of the tensors themselves; None for one that does not require a gradient
    need = ctx.needs_input_grad[11:14]
    parts = ((pose[:16], rs.viewmatrix), (pose[16:32], rs.projmatrix), (pose[32:], rs.campos))
    return out + tuple(g.reshape(t.shape) if n else None for (g, t), n in zip(parts, need)) + tail


class _ReusedRender(torch.autograd.Function):
    """A colour-override render served from the state of the preceding full render of the same view (_reuse.py): the
    blend kernel alone.  Same outputs as `_RasterizeGaussians`; differentiable like it -- a backward through this image
    (nobody in GaussianEditor asks for one) first runs the full forward that was skipped, then the ordinary backward."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                entry, return_alpha=False):
        rs = raster_settings
        flags = _options.current_flags()
        color = _call_native(lambda *a: _C.rasterize_gaussians_aux(*a, flags=flags),
                             (rs.bg, colors_precomp.detach(), entry.R, entry.geom, entry.binning, entry.img, rs.image_height,
                              rs.image_width, rs.debug), rs.debug, "snapshot_fw.dump",
                             "\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
        radii, depth = entry.radii.clone(), entry.depth.clone()
        ctx.raster_settings = rs
        ctx.gsr_flags = flags
        if flags & _options.FLAG_ABS_GRAD:
            ctx.gsr_means2D = means2D
        ctx.save_for_backward(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        ctx.gsr_alpha = bool(return_alpha)
        if return_alpha:  # the remembered state holds the full render's final_T: no K6 of this render's own wrote it
            return color, radii, depth, _C.alpha_image(entry.img, rs.image_height, rs.image_width)
        return color, radii, depth

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_depth, grad_alpha=None):
        rs, flags = ctx.raster_settings, ctx.gsr_flags
        means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp = ctx.saved_tensors
        fwd = _C.rasterize_gaussians(rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier,
                                     cov3Ds_precomp, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height,
                                     rs.image_width, sh, rs.sh_degree, rs.campos, rs.prefiltered, rs.debug, flags=flags)
        return _backward(ctx, (means3D, sh, colors_precomp, scales, rotations, cov3Ds_precomp), (fwd[0], *fwd[3:]),
                         (grad_out_color, grad_depth, grad_alpha if ctx.gsr_alpha else None))


def _pose_inputs(rs):
    """The camera tensors as trailing inputs of `_RasterizeGaussians.apply` -- under FLAG_POSE_GRAD
    (gaussianeditor_amd.set_pose_grad) and only when one of them requires a gradient; () otherwise, so that every other
    render is the call it always was.  (Inside a NamedTuple autograd does not see them: a camera built from a learnable
    pose renders correctly and gets no gradient.)"""
    if not (_options.current_flags() & _options.FLAG_POSE_GRAD):
        return ()
    cams = (rs.viewmatrix, rs.projmatrix, rs.campos)
    if not any(isinstance(t, torch.Tensor) and t.requires_grad for t in cams):
        return ()
    return cams


def _rasterize_with_features(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                             raster_settings, aux_colors, return_alpha, features, distortion=None):
    """A render with `features=` and / or `return_distortion`: always in full (never served by view reuse; it may be
    remembered), the features a trailing input autograd sees, behind the camera tensors' slots, the distortion image's
    (near, far) behind them -- passed only where that image is asked for."""
    pose = _pose_inputs(raster_settings) or (None, None, None)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                     raster_settings, aux_colors, bool(return_alpha), *pose, features,
                                     *(() if distortion is None else (distortion,)))


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, return_alpha=False):
    # (return_alpha: the alpha image as an additional last value; the extra arguments only then, so that a call without it
    #  is the call it always was)
    with_alpha = (True,) if return_alpha else ()
    pose = _pose_inputs(raster_settings)
    if pose:  # (a render whose camera takes a gradient is never served from a remembered state: it runs in full)
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                         cov3Ds_precomp, raster_settings, None, bool(return_alpha), *pose)
    if colors_precomp.numel() != 0 and sh.numel() == 0 and means3D.is_cuda:
        # a colour-override render: is it the view the rasterizer rendered last (the reference's second render() of every
        # training view / GUI frame)?  Then the blend kernel alone, on that render's state (_reuse.py)
        entry = _reuse.lookup(raster_settings, _options.current_flags(), means3D, scales, rotations, opacities, cov3Ds_precomp)
        if entry is not None:
            return _ReusedRender.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                       raster_settings, entry, *with_alpha)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, *((None, True) if return_alpha else ()))


def rasterize_gaussians_with_aux(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                 raster_settings, aux_colors, return_alpha=False):
    """rasterize_gaussians plus a second image blended with `aux_colors` (P,3): (color, radii, depth, aux_color), with
    `return_alpha` (color, radii, depth, aux_color, alpha)."""
    pose = _pose_inputs(raster_settings)
    if pose:
        return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                         cov3Ds_precomp, raster_settings, aux_colors, bool(return_alpha), *pose)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, aux_colors, *((True,) if return_alpha else ()))


def distortion_asked(return_distortion) -> bool:
    """`return_distortion` of GaussianRasterizer.forward / render(): False / None -- no; True or a (near, far) pair -- yes."""
    return return_distortion is not False and return_distortion is not None


def _absent(like: torch.Tensor) -> torch.Tensor:
    """The reference encodes "not provided" as an empty float32 tensor on "cuda" (:285-295);
    we put it on the device of `means3D`, which is the same thing for every valid call."""
    return torch.empty(0, dtype=torch.float32, device=like.device)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        """Boolean mask of the points in front of the camera's near plane (:248-256)."""
        with torch.no_grad():
            rs = self.raster_settings
            return _C.mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, aux_colors=None, return_alpha=False, features=None, return_normals=False,
                return_distortion=False):
        """Reference signature (:258-309) plus five extensions.  With `aux_colors` (P,3) a second image of the same
        view, blended with those colours instead, is returned as a fourth value (forward only, no gradient).  It is
        what a second call with colors_precomp=aux_colors would render, at the cost of the blend kernel alone.
        With `return_alpha=True` the alpha image (1,H,W) -- accumulated opacity, 1 - the final transmittance -- is an
        additional LAST value, (color, radii, depth, alpha) or (color, radii, depth, aux, alpha), differentiable like the
        colour.  With `features` (P,C) float32, 1 <= C <= 256, the feature image (C,H,W) -- those per-Gaussian features
        composited with the view's alpha on background 0, every 16 channels in one walk of the tile lists -- is appended
        as the LAST value: (color, radii, depth[, aux][, alpha], feature_image).  It is differentiable with respect to
        `features`, means3D, means2D, opacities and scales / rotations / cov3D_precomp, not with respect to shs /
        colors_precomp.  With `return_normals=True` the normal image (3,H,W) -- the camera-space normal of every Gaussian
        (gaussianeditor_amd.normals.gaussian_normals of this view), composited like a feature -- is appended behind all of
        them: (color, radii, depth[, aux][, alpha][, feature_image], normals), with a gradient to the rotations and the
        geometry.  It rides the feature route (three more channels behind the caller's, so C <= 253 then) and needs
        scales / rotations, not cov3D_precomp.  With `return_distortion=True`, or `return_distortion=(near, far)` with finite
        0 < near < far, the depth-distortion image (1,H,W) -- per pixel 1/2 sum_{i != j} w_i w_j (m_i - m_j)^2 over the
        entries the colour image blends, m the view-space depth or 2DGS's mapped depth far (z - near) / ((far - near) z);
        the regulariser of Mip-NeRF 360 / 2DGS, accumulated in depths shifted by the pixel's first blended one -- is appended
        as the LAST value, behind all of the others, with a gradient to means3D, means2D, opacities and scales / rotations /
        cov3D_precomp.  `means2D.absgrad` (FLAG_ABS_GRAD) is what it is without the distortion image, as with features.  The
        arity depends on these five arguments alone, never on process state."""
        if (shs is None) == (colors_precomp is None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")  # sic, :271-276
        has_sr = scales is not None or rotations is not None
        if ((scales is None or rotations is None) and cov3D_precomp is None) or (has_sr and cov3D_precomp is not None):
            raise Exception(
                "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")  # :278-283
        shs = _absent(means3D) if shs is None else shs
        colors_precomp = _absent(means3D) if colors_precomp is None else colors_precomp
        scales = _absent(means3D) if scales is None else scales
        rotations = _absent(means3D) if rotations is None else rotations
        cov3D_precomp = _absent(means3D) if cov3D_precomp is None else cov3D_precomp
        distortion = None
        if distortion_asked(return_distortion):
            distortion = _C.check_near_far(None if return_distortion is True else return_distortion, "return_distortion")
        if return_normals:
            return self._forward_with_normals(means3D, means2D, opacities, shs, colors_precomp, scales, rotations,
                                              cov3D_precomp, aux_colors, return_alpha, features, return_distortion)
        if features is not None:
            if not isinstance(features, torch.Tensor) or features.dtype != torch.float32:
                raise RuntimeError("diff_gaussian_rasterization: `features` must be a float32 tensor, got "
                                   f"{getattr(features, 'dtype', type(features).__name__)}")
            if features.dim() != 2 or features.shape[0] != means3D.shape[0] or not 1 <= features.shape[1] <= 256:
                raise RuntimeError(f"diff_gaussian_rasterization: `features` must be a ({means3D.shape[0]}, C) tensor with "
                                   f"1 <= C <= 256, got {tuple(features.shape)}")
            if features.device != means3D.device:
                raise RuntimeError(f"diff_gaussian_rasterization: `features` is on {features.device} but `means3D` is on "
                                   f"{means3D.device}")
            return _rasterize_with_features(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                            cov3D_precomp, self.raster_settings, aux_colors, return_alpha, features,
                                            distortion)
        if distortion is not None:
            return _rasterize_with_features(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                            cov3D_precomp, self.raster_settings, aux_colors, return_alpha, None, distortion)
        if aux_colors is not None:
            return rasterize_gaussians_with_aux(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                                cov3D_precomp, self.raster_settings, aux_colors, return_alpha)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   self.raster_settings, return_alpha)

    def _forward_with_normals(self, means3D, means2D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp,
                              aux_colors, return_alpha, features, return_distortion=False):
        """forward(..., return_normals=True): the Gaussian normals of this view as the last three feature channels, split
        off again.  Absent arguments arrive as empty tensors."""
        from .. import normals as _normals

        if cov3D_precomp.numel() != 0:
            raise RuntimeError("diff_gaussian_rasterization: `return_normals` needs scales and rotations; a precomputed 3D "
                               "covariance has no axes to take a normal from")
        C = 0
        if features is not None:
            if not isinstance(features, torch.Tensor) or features.dim() != 2:
                raise RuntimeError("diff_gaussian_rasterization: `features` must be a (P, C) float32 tensor")
            C = int(features.shape[1])
            if C + 3 > 256:
                raise RuntimeError(f"diff_gaussian_rasterization: `return_normals` takes three of the 256 feature channels: "
                                   f"`features` may have at most 253 with it, got {C}")
        nrm = _normals.gaussian_normals(rotations.contiguous(), scales.contiguous(), means3D.contiguous(),
                                        self.raster_settings.viewmatrix.contiguous())
        feats = nrm if features is None else torch.cat([features, nrm], dim=1)
        outs = self.forward(means3D, means2D, opacities, shs=shs if shs.numel() else None,
                            colors_precomp=colors_precomp if colors_precomp.numel() else None, scales=scales,
                            rotations=rotations, aux_colors=aux_colors, return_alpha=return_alpha, features=feats,
                            **({"return_distortion": return_distortion} if distortion_asked(return_distortion) else {}))
        tail = ()
        if distortion_asked(return_distortion):  # (the distortion image is the last value, the normals in front of it)
            outs, tail = outs[:-1], outs[-1:]
        if features is None:
            return outs + tail
        return outs[:-1] + (outs[-1][:C], outs[-1][C:]) + tail

    def apply_weights(self, means3D, means2D, opacities, shs=None, weights=None, scales=None, rotations=None,
                      cov3Ds_precomp=None, cnt=None, image_weights=None):
        """Semantic tracing (:311-364): every pixel adds its `image_weights` value(s) to
        `weights[i]` and C to `cnt[i]` for every Gaussian i it would blend.  In place; returns None."""
        assert weights is not None
        assert cnt is not None
        assert image_weights is not None
        rs = self.raster_settings
        shs = _absent(means3D) if shs is None else shs
        scales = _absent(means3D) if scales is None else scales
        rotations = _absent(means3D) if rotations is None else rotations
        cov3Ds_precomp = _absent(means3D) if cov3Ds_precomp is None else cov3Ds_precomp
        # argument order of _C.apply_weights (rasterize_points.h:66-77)
        _C.apply_weights(rs.bg, means3D, weights, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                         rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, shs,
                         rs.sh_degree, rs.campos, rs.prefiltered, image_weights, cnt, rs.debug)

    @torch.no_grad()
    def trace_contributions(self, means3D, opacities, scales=None, rotations=None, cov3Ds_precomp=None, stats=None,
                            image_weights=None, return_pixels=False):
        """Extension (no reference counterpart): the contribution-weighted sibling of apply_weights.  Every pixel adds, for
        every Gaussian i it would blend, its blending weight alpha T to `stats[i]` -- an int64 (P, 3 + C) table, accumulated
        in place in integers (_C.trace_contributions_state states the columns) -- and, with `image_weights` (C,H,W), C <= 3,
        the weight times the pixel's mask value per channel.  With `return_pixels` -> (top_id (H,W) int32, top_weight (H,W)
        float32): the Gaussian under every pixel, by largest weight; else None.  Not differentiable."""
        assert stats is not None
        rs = self.raster_settings
        scales = _absent(means3D) if scales is None else scales
        rotations = _absent(means3D) if rotations is None else rotations
        cov3Ds_precomp = _absent(means3D) if cov3Ds_precomp is None else cov3Ds_precomp
        return _C.trace_contributions(rs.bg, means3D, stats, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                                      rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width,
                                      _absent(means3D), rs.sh_degree, rs.campos, rs.prefiltered, image_weights=image_weights,
                                      return_pixels=return_pixels, debug=rs.debug)
