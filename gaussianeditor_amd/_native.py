"""ctypes binding of libgsr_hip.so (the C ABI of include/gsr.h).

There is NO fallback: if the library is missing or fails to load, importing the
rasterizer raises.  ctypes releases the GIL for the duration of every native call
(the reference's pybind functions hold it, ext.cpp:16-19).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_float, c_int, c_int64, c_size_t, c_uint, c_void_p, POINTER

_HERE = os.path.dirname(os.path.abspath(__file__))
#: GSR_LIBRARY_PATH (development only: A/B timing of differently built libraries, tools/ab_variants.py) replaces the
#: in-tree library; it must export the same ABI and is loaded under the same "no fallback" rule.
LIB_PATH = os.environ.get("GSR_LIBRARY_PATH") or os.path.join(_HERE, "libgsr_hip.so")
GSR_ABI_VERSION = 6

_P = c_void_p
#: floats per row of the blend backward's accumulator table and its columns (include/gsr.h: GSR_ACC_*)
ACC_ROW, ACC_MEAN2D, ACC_OPACITY, ACC_CONIC, ACC_COLOR, ACC_DEPTH, ACC_ABS2D = 16, 0, 3, 4, 8, 11, 12


class AdamTensor(ctypes.Structure):
    """gsr_adam_tensor (include/gsr.h)."""
    _fields_ = [("param", _P), ("grad", _P), ("exp_avg", _P), ("exp_avg_sq", _P), ("anchor", _P), ("numel", c_int64),
                ("row_len", ctypes.c_int32), ("masked", ctypes.c_int32), ("lr", ctypes.c_double), ("anchor_scale", c_float)]


class DenseGrads(ctypes.Structure):
    """gsr_dense_grads (include/gsr.h)."""
    _fields_ = [("means3D", _P), ("scales", _P), ("rotations", _P), ("means2D", _P), ("opacities", _P), ("sh", _P)]


class AppendTensor(ctypes.Structure):
    """gsr_append_tensor (include/gsr.h)."""
    _fields_ = [("src", _P), ("ext", _P), ("dst", _P), ("row_bytes", c_int64)]


class CompactTensor(ctypes.Structure):
    """gsr_compact_tensor (include/gsr.h)."""
    _fields_ = [("src", _P), ("dst", _P), ("row_bytes", c_int64)]


class DensifyResult(ctypes.Structure):
    """gsr_densify_result (include/gsr.h)."""
    _fields_ = [("nonzero", c_int64), ("n_clone", c_int64), ("n_split", c_int64), ("threshold", c_float)]


class McmcRecord(ctypes.Structure):
    """gsr_mcmc_record (include/gsr.h)."""
    _fields_ = [("n_dead", c_int64), ("n_alive", c_int64), ("n_draws", c_int64), ("total", ctypes.c_uint64)]


class McmcTensor(ctypes.Structure):
    """gsr_mcmc_tensor (include/gsr.h)."""
    _fields_ = [("base", _P), ("dst", _P), ("values", _P), ("row_bytes", c_int64), ("role", ctypes.c_int32)]


#: roles of a gsr_mcmc_tensor (include/gsr.h: GSR_MCMC_*)
MCMC_COPY, MCMC_VALUE, MCMC_ZERO = 0, 1, 2

#: every symbol include/gsr.h declares, with (restype, argtypes)
SIGNATURES = {
    "gsr_abi_version": (c_int, []),
    "gsr_status_string": (ctypes.c_char_p, [c_int]),
    "gsr_last_hip_error": (c_int, []),
    "gsr_scratch_sizes": (c_int, [c_int, c_int64, c_int64, c_int, c_int, POINTER(c_size_t)]),
    "gsr_sort_key_bits": (c_int, [c_int, c_int]),
    "gsr_preprocess": (c_int, [_P, c_int, c_int, c_int, _P, _P, c_float, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int,
                               c_float, c_float, c_int, c_int, c_uint, _P, _P, POINTER(c_int64)]),
    "gsr_preprocess_begin": (c_int, [_P, c_int, c_int, c_int, _P, _P, c_float, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int,
                                     c_float, c_float, c_int, c_int, c_uint, _P, _P, POINTER(_P)]),
    "gsr_preprocess_end": (c_int, [_P, c_int, c_int, c_int, _P, _P, POINTER(c_int64)]),
    "gsr_arrays_equal": (c_int, [_P, c_int, POINTER(_P), POINTER(_P), POINTER(c_size_t), POINTER(c_int)]),
    "gsr_bin": (c_int, [_P, c_int, c_int64, c_int64, c_int, c_int, _P, _P, _P]),
    "gsr_blend_forward": (c_int, [_P, c_int, c_int64, c_int, c_int, _P, _P, _P, _P, _P, _P, c_uint]),
    "gsr_blend_forward_aux": (c_int, [_P, c_int, c_int64, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_uint]),
    "gsr_backward": (c_int, [_P, c_int, c_int, c_int, c_int64, c_int, c_int, _P, _P, _P, _P, _P, c_float, _P, _P, _P,
                             _P, _P, c_float, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_uint]),
    # (stream, P, R, W, H, bg, geom, binning, image, dL_dpix, acc, touched, flags)
    "gsr_blend_backward": (c_int, [_P, c_int, c_int64, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_uint]),
    # depth gradients (GSR_FLAG_DEPTH_GRAD): gsr_blend_backward / gsr_backward with dL_ddepth (1,H,W) behind dL_dpix
    "gsr_blend_backward_depth": (c_int, [_P, c_int, c_int64, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, c_uint]),
    "gsr_backward_depth": (c_int, [_P, c_int, c_int, c_int, c_int64, c_int, c_int, _P, _P, _P, _P, _P, c_float, _P, _P, _P,
                                   _P, _P, c_float, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                   c_uint]),
    # absolute screen-space gradients (GSR_FLAG_ABS_GRAD), between the two halves: (stream, P, acc, touched, absgrad (P,3))
    "gsr_abs_grad_take": (c_int, [_P, c_int, _P, _P, _P]),
    # the camera gradient, between the two halves: (P, bytes); (stream, P, D, M, W, H, means3D, scales, scale_modifier,
    # rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii, geom, acc, workspace, pose_grad[35], flags)
    "gsr_pose_workspace_size": (c_int, [c_int, POINTER(c_size_t)]),
    "gsr_pose_backward": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, c_float, _P, _P, _P, _P, _P, c_float, c_float,
                                  _P, _P, _P, _P, _P, c_uint]),
    # alpha image: (stream, W, H, image, out_alpha (1,H,W)); its backward: gsr_blend_backward with dL_ddepth | NULL and
    # dL_dalpha (1,H,W) behind dL_dpix
    "gsr_alpha_image": (c_int, [_P, c_int, c_int, _P, _P]),
    "gsr_blend_backward_alpha": (c_int, [_P, c_int, c_int64, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_uint]),
    # feature image: (stream, P, R, W, H, C, geom, binning, image, features (P,C), out (C,H,W), flags); its backward:
    # (stream, P, R, W, H, C, geom, binning, image, features, dL_dfeature_image (C,H,W), acc, dL_dfeatures (P,C), flags)
    "gsr_blend_forward_features": (c_int, [_P, c_int, c_int64, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_uint]),
    "gsr_blend_backward_features": (c_int, [_P, c_int, c_int64, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_uint]),
    # distortion image: (stream, P, R, W, H, geom, binning, image, near, far, out (H,W), moments (H,W,4) | NULL, flags); its
    # backward: (stream, P, R, W, H, geom, binning, image, near, far, moments, dL_ddistortion (H,W), acc, flags)
    "gsr_blend_forward_distortion": (c_int, [_P, c_int, c_int64, c_int, c_int, _P, _P, _P, c_float, c_float, _P, _P, c_uint]),
    "gsr_blend_backward_distortion": (c_int, [_P, c_int, c_int64, c_int, c_int, _P, _P, _P, c_float, c_float, _P, _P, _P,
                                              c_uint]),
    # (... radii, geom, acc, dL_dmeans2D, dL_dopacity, dL_dcolors, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drots, flags)
    "gsr_preprocess_backward": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_float, _P, _P, _P, _P, _P,
                                        c_float, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_uint]),
    # (... radii, geom, acc, dL_dmeans2D, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_drgb, dL_dscales, dL_drots)
    "gsr_preprocess_backward_rgb": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_float, _P, _P, _P, _P, _P,
                                            c_float, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_uint]),
    # (... radii, geom, acc, dL_dmeans2D, dL_dopacity, dL_dcolors, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_drgb, dL_dscales, dL_drots, row_state)
    "gsr_preprocess_backward_rows": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_float, _P, _P, _P, _P, _P,
                                            c_float, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    # (... the same, then flags: 0 | GSR_FLAG_ANTIALIAS)
    "gsr_preprocess_backward_rows_flags": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_float, _P, _P, _P, _P,
                                                  _P, c_float, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                  c_uint]),
    "gsr_sh_grad_compose": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "gsr_view_message_words": (c_int, [c_int64, c_int64, POINTER(c_int64)]),
    "gsr_view_message_plan": (c_int, [_P, c_int64, POINTER(DenseGrads), _P, _P, _P, POINTER(c_int64)]),
    "gsr_view_message_plan_blend": (c_int, [_P, c_int64, _P, _P]),
    "gsr_view_message_pack": (c_int, [_P, c_int64, POINTER(DenseGrads), _P, _P, _P, _P, c_int64, _P]),
    "gsr_view_messages_accumulate": (c_int, [_P, c_int64, c_int, c_int, c_int, _P, c_int64, c_int64, _P, POINTER(DenseGrads)]),
    "gsr_view_messages_accumulate_rows": (c_int, [_P, c_int64, c_int, c_int, c_int, _P, c_int64, c_int64, _P, POINTER(DenseGrads), _P]),
    "gsr_knn_workspace_size": (c_int, [c_int, POINTER(c_size_t)]),
    "gsr_knn_mean_dist2": (c_int, [_P, c_int, _P, _P, _P]),
    "gsr_near_workspace_size": (c_int, [c_int, POINTER(c_size_t)]),
    "gsr_near_points": (c_int, [_P, c_int, _P, c_int, _P, c_float, _P, _P, _P]),
    "gsr_compact_workspace_size": (c_int, [c_int64, POINTER(c_size_t)]),
    "gsr_compact_plan": (c_int, [_P, c_int64, _P, _P, POINTER(c_int64)]),
    "gsr_compact_apply": (c_int, [_P, c_int64, _P, _P, c_int, POINTER(CompactTensor)]),
    "gsr_append_rows": (c_int, [_P, c_int64, c_int64, c_int, POINTER(AppendTensor)]),
    # the densification policy (gaussianeditor_amd/densify.py): (stream, P, V, grads[V], radii[V], accum, denom, max_radii2D);
    # (stream, P, accum, denom, mask, scaling, max_grad, max_densify_percent, percent_dense, extent, workspace, clone_sel,
    #  split_sel, result); (workspace, P, &clone_plan, &split_plan);
    # (stream, P, xyz, scaling, rotation, split_sel, split_plan, n_split, N, noise, new_xyz);
    # (stream, P, opacity, scaling, max_radii2D | NULL, mask, drop | NULL, min_opacity, max_screen_size, extent, keep)
    "gsr_densify_stats": (c_int, [_P, c_int64, c_int, POINTER(_P), POINTER(_P), _P, _P, _P]),
    "gsr_densify_workspace_size": (c_int, [c_int64, POINTER(c_size_t)]),
    "gsr_densify_select": (c_int, [_P, c_int64, _P, _P, _P, _P, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_double, _P, _P, _P, POINTER(DensifyResult)]),
    "gsr_densify_plans": (c_int, [_P, c_int64, POINTER(_P), POINTER(_P)]),
    "gsr_densify_split_xyz": (c_int, [_P, c_int64, _P, _P, _P, _P, _P, c_int64, c_int, _P, _P]),
    "gsr_densify_keep": (c_int, [_P, c_int64, _P, _P, _P, _P, _P, ctypes.c_double, ctypes.c_double, ctypes.c_double, _P]),
    # the 3DGS-MCMC strategy (gaussianeditor_amd/mcmc.py): (stream, P, xyz, scaling_raw, rotation_raw, opacity_raw, noise,
    # mask | NULL, k, x0, scaler); (P, bytes); (stream, P, n, opacity, mask | NULL, min_opacity, u, draws_from_dead, workspace,
    # dead_sel, dead_idx, src, count, ratio, record); (stream, P, n, src, ratio, opacity, scaling_raw, min_opacity,
    # new_opacity_raw, new_scaling_raw); (stream, P, n, src, dst_idx | NULL, dst_rows, num_tensors, tensors)
    "gsr_mcmc_noise": (c_int, [_P, c_int64, _P, _P, _P, _P, _P, _P, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    "gsr_mcmc_workspace_size": (c_int, [c_int64, POINTER(c_size_t)]),
    "gsr_mcmc_sample": (c_int, [_P, c_int64, c_int64, _P, _P, ctypes.c_double, _P, c_int, _P, _P, _P, _P, _P, _P,
                                POINTER(McmcRecord)]),
    "gsr_mcmc_relocation_values": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, ctypes.c_double, _P, _P]),
    "gsr_mcmc_scatter": (c_int, [_P, c_int64, c_int64, _P, _P, c_int64, c_int, POINTER(McmcTensor)]),
    # similarity transforms (gaussianeditor_amd/transform.py): (rot[9], out[83]), host only; (stream, P, rest, xyz | NULL,
    # rotation | NULL, scaling | NULL, sh_rest | NULL, mask | NULL, rot[9], trans[3], scale, scale_eps)
    "gsr_sh_rotation": (c_int, [POINTER(ctypes.c_double), POINTER(ctypes.c_double)]),
    "gsr_transform_rows": (c_int, [_P, c_int64, c_int, _P, _P, _P, _P, _P, POINTER(ctypes.c_double), POINTER(ctypes.c_double),
                                   ctypes.c_double, ctypes.c_double]),
    # surface normals (gaussianeditor_amd/normals.py): (stream, P, rotations, scales, means3D, viewmatrix, out);
    # (stream, P, rotations, scales, means3D, viewmatrix, dL_dout, dL_drotations);
    # (stream, H, W, fx, fy, cx, cy, alpha_min, depth, alpha | NULL, out);
    # (stream, H, W, fx, fy, cx, cy, alpha_min, depth, alpha | NULL, dL_dout, dL_ddepth | NULL, dL_dalpha | NULL); (H, W, bytes);
    # (stream, H, W, fx, fy, cx, cy, alpha_min, normals, depth, alpha, workspace, out_loss);
    # (stream, H, W, fx, fy, cx, cy, alpha_min, normals, depth, alpha, dL_dloss, dL_dnormals | NULL, dL_ddepth | NULL, dL_dalpha | NULL)
    "gsr_gaussian_normals_forward": (c_int, [_P, c_int64] + [_P] * 5),
    "gsr_gaussian_normals_backward": (c_int, [_P, c_int64] + [_P] * 6),
    "gsr_depth_normals_forward": (c_int, [_P, c_int, c_int] + [ctypes.c_double] * 5 + [_P] * 3),
    "gsr_depth_normals_backward": (c_int, [_P, c_int, c_int] + [ctypes.c_double] * 5 + [_P] * 5),
    "gsr_normal_loss_workspace_size": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "gsr_normal_loss_forward": (c_int, [_P, c_int, c_int] + [ctypes.c_double] * 5 + [_P] * 5),
    "gsr_normal_loss_backward": (c_int, [_P, c_int, c_int] + [ctypes.c_double] * 5 + [_P] * 7),
    # Mip-Splatting's 3D filter (gaussianeditor_amd/filter3d.py): (P, bytes);
    # (stream, P, V, means3D, cameras (V,20) f64, f_max, coef, workspace, filter_3D (P,1), valid (P) u8);
    # (stream, P, from_raw, scales, opacity, filter_3D, scales_eff, opacity_eff);
    # (stream, P, from_raw, scales, opacity, filter_3D, dL_dscales_eff | NULL, dL_dopacity_eff | NULL, dL_dscales | NULL, dL_dopacity | NULL)
    "gsr_filter3d_workspace_size": (c_int, [c_int64, POINTER(c_size_t)]),
    "gsr_filter3d_sweep": (c_int, [_P, c_int64, c_int, _P, _P, ctypes.c_double, ctypes.c_double, _P, _P, _P]),
    "gsr_filter3d_apply_forward": (c_int, [_P, c_int64, c_int] + [_P] * 5),
    "gsr_filter3d_apply_backward": (c_int, [_P, c_int64, c_int] + [_P] * 7),
    # TSDF fusion and mesh extraction (gaussianeditor_amd/tsdf.py): (stream, nx, ny, nz, origin x y z, voxel_size, V, H, W,
    # depth (V,1,H,W), alpha | NULL, color (V,3,H,W) | NULL, cameras (V,20) f64, trunc, alpha_min, max_weight, tsdf, weight,
    # vol_color (3,nx,ny,nz) | NULL); (nx, ny, nz, bytes); (stream, nx, ny, nz, tsdf, weight, workspace, counts_host[2]);
    # (stream, nx, ny, nz, origin x y z, voxel_size, tsdf, weight, vol_color | NULL, workspace, n_vertices, n_faces,
    #  vertices (Nv,3), colors (Nv,3) | NULL, faces (Nf,3) i32)
    "gsr_tsdf_integrate": (c_int, [_P, c_int, c_int, c_int] + [c_float] * 4 + [c_int] * 3 + [_P] * 4
                           + [ctypes.c_double, ctypes.c_double, c_float] + [_P] * 3),
    "gsr_tsdf_mesh_workspace_size": (c_int, [c_int, c_int, c_int, POINTER(c_size_t)]),
    "gsr_tsdf_mesh_count": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, POINTER(c_int64)]),
    "gsr_tsdf_mesh_emit": (c_int, [_P, c_int, c_int, c_int] + [c_float] * 4 + [_P] * 4 + [c_int64, c_int64] + [_P] * 3),
    "gsr_adam_step": (c_int, [_P, c_int, POINTER(AdamTensor), c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _P,
                            _P]),
    "gsr_adam_step_rows": (c_int, [_P, c_int, POINTER(AdamTensor), c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _P,
                            _P, _P]),
    "gsr_mark_visible": (c_int, [_P, c_int, _P, _P, _P, _P]),
    "gsr_trace_weights": (c_int, [_P, c_int, c_int64, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, c_uint]),
    "gsr_trace_contributions": (c_int, [_P, c_int, c_int64, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_uint]),
    "gsr_debug_export_geom": (c_int, [_P, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "gsr_debug_cov3d": (c_int, [_P, c_int, _P, c_float, _P, _P]),
    "gsr_debug_export_binning": (c_int, [_P, c_int, c_int64, c_int, c_int, _P, _P, _P, _P]),
    "gsr_debug_blend_backward_profile": (c_int, [_P, c_int, c_int64, c_int, c_int, _P, _P, _P, _P, _P, _P, _P,
                                                 c_int64, POINTER(c_int64)]),
    "gsr_debug_blend_forward_profile": (c_int, [_P, c_int, c_int64, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_int64,
                                                POINTER(c_int64)]),
    "gsr_debug_export_image": (c_int, [_P, c_int, c_int, _P, _P, _P, _P]),
    # which K7 ran, on what work (host-side bookkeeping): (counts[32]), index FAST | SEG << 1 | DEPTH << 2 | ABS << 3 |
    # ALPHA << 4; (stream, W, H, image, counts[2] = {items, list-segment items} of the latest backward's work list)
    "gsr_debug_blend_backward_launches": (c_int, [POINTER(ctypes.c_uint64)]),
    "gsr_debug_blend_backward_items": (c_int, [_P, c_int, c_int, _P, POINTER(c_int64)]),
    # which radix scatter ran (host-side bookkeeping): (counts[24]), index layout at the declaration in include/gsr.h
    "gsr_debug_sort_launches": (c_int, [POINTER(ctypes.c_uint64)]),
    # which chunk kernel of the grouped binning ran (host-side bookkeeping): (counts[16]), index log2(NB) | SCATTER << 2 |
    # (stage of 2048 entries) << 3
    "gsr_debug_group_launches": (c_int, [POINTER(ctypes.c_uint64)]),
    # the fused L1 + SSIM loss (gaussianeditor_amd/losses.py): (planes, H, W, bytes);
    # (stream, planes, H, W, img, gt, w_l1, w_ssim, c, maps | NULL, workspace, out3);
    # (stream, planes, H, W, img, gt, maps, w_l1, w_ssim, dL_dloss, dL_dimg)
    "gsr_loss_workspace_size": (c_int, [c_int, c_int, c_int, POINTER(c_size_t)]),
    "gsr_photometric_loss_forward": (c_int, [_P, c_int, c_int, c_int, _P, _P, c_float, c_float, c_float, _P, _P, _P]),
    "gsr_photometric_loss_backward": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, c_float, c_float, _P, _P]),
    # the bilateral-grid slice and its TV regulariser (gaussianeditor_amd/bilagrid.py): (B, H, W, GX, GY, GZ, bytes);
    # (stream, B, H, W, N, GX, GY, GZ, grids, idx, img, out);
    # (stream, B, H, W, N, GX, GY, GZ, grids, idx, img, dL_dout, workspace, dL_dimg | NULL, dL_dgrids | NULL);
    # (N, GX, GY, GZ, bytes); (stream, N, GX, GY, GZ, grids, workspace, out1); (stream, N, GX, GY, GZ, grids, dL_dtv, dL_dgrids)
    "gsr_bilagrid_workspace_size": (c_int, [c_int] * 6 + [POINTER(c_size_t)]),
    "gsr_bilagrid_slice_forward": (c_int, [_P] + [c_int] * 7 + [_P] * 4),
    "gsr_bilagrid_slice_backward": (c_int, [_P] + [c_int] * 7 + [_P] * 7),
    "gsr_bilagrid_tv_workspace_size": (c_int, [c_int] * 4 + [POINTER(c_size_t)]),
    "gsr_bilagrid_tv_forward": (c_int, [_P] + [c_int] * 4 + [_P] * 3),
    "gsr_bilagrid_tv_backward": (c_int, [_P] + [c_int] * 4 + [_P] * 3),
}

_lib = None


class GsrError(RuntimeError):
    """A native call returned a non-zero gsr_status."""

    def __init__(self, fn: str, status: int, message: str, hip_error: int = 0):
        self.status = status
        self.hip_error = hip_error
        extra = f" (hipError_t {hip_error})" if hip_error else ""
        super().__init__(f"{fn} failed: {message} [status {status}]{extra}")


def lib() -> ctypes.CDLL:
    """Load (once) and type the native library.  Raises if it is absent: build it with
    `python -c 'import __graft_entry__ as g; g.build()'` or `make -C gaussianeditor_amd/csrc`."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: the HIP extension is not built. There is no CPU or PyTorch fallback; "
                "run `make -C gaussianeditor_amd/csrc` (hipcc --offload-arch=gfx950).")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        if L.gsr_abi_version() != GSR_ABI_VERSION:
            raise ImportError(f"{LIB_PATH}: ABI version {L.gsr_abi_version()} != expected {GSR_ABI_VERSION}")
        _lib = L
    return _lib


def check(fn: str, status: int) -> None:
    if status != 0:
        L = lib()
        msg = L.gsr_status_string(status).decode()
        raise GsrError(fn, status, msg, L.gsr_last_hip_error() if status == -4 else 0)


def scratch_sizes(P: int, R: int, W: int, H: int, G: int = 0):
    """(geometry, binning, image) scratch bytes; R, G = the two counts gsr_preprocess returns (0, 0 before they are known)."""
    sizes = (c_size_t * 3)()
    check("gsr_scratch_sizes", lib().gsr_scratch_sizes(P, R, G, W, H, sizes))
    return int(sizes[0]), int(sizes[1]), int(sizes[2])
