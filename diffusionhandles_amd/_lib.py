"""ctypes binding of libdiffhandles_hip.so (the C ABI declared in include/diffhandles_hip.h).

There is no CPU fallback: if the shared library is missing, or no HIP device is visible
when a compute entry point is called, the caller gets a RuntimeError.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DIFFHANDLES_LIB: another build of the same library (A/B timing of two builds on one box); never a different backend
LIB_PATH = os.environ.get("DIFFHANDLES_LIB") or os.path.join(_HERE, "libdiffhandles_hip.so")
_LIB = None

c_p = ctypes.c_void_p
c_i = ctypes.c_int
c_f = ctypes.c_float
c_d = ctypes.c_double
c_sz = ctypes.c_size_t
c_l = ctypes.c_long


class UNetConfig(ctypes.Structure):
    _fields_ = [("in_channels", c_i), ("out_channels", c_i), ("n_levels", c_i),
                ("block_out_channels", c_i * 4), ("layers_per_block", c_i), ("heads", c_i * 4),
                ("cross_attention_dim", c_i), ("norm_groups", c_i), ("sample_size", c_i),
                ("text_len", c_i), ("max_batch", c_i), ("dtype", c_i), ("max_diff_batch", c_i)]


class VAEConfig(ctypes.Structure):
    _fields_ = [("latent_channels", c_i), ("out_channels", c_i), ("block_out_channels", c_i * 4),
                ("layers_per_block", c_i), ("norm_groups", c_i), ("latent_size", c_i), ("dtype", c_i)]


class TextConfig(ctypes.Structure):
    _fields_ = [("hidden", c_i), ("heads", c_i), ("layers", c_i), ("intermediate", c_i), ("max_tokens", c_i),
                ("max_batch", c_i), ("eps", c_f), ("dtype", c_i)]


class EnergyItem(ctypes.Structure):
    """dh_energy_item: one item of dh_energy_fwd_bwd_planned_batch"""
    _fields_ = [("cur", c_p), ("orig", c_p), ("plan", c_p), ("plan_bytes", c_sz), ("bg_orig", c_p), ("bg_trans", c_p),
                ("loss_out", c_p), ("grad", c_p), ("n_pairs", c_i), ("n_bg_orig", c_i), ("n_bg_trans", c_i),
                ("fg_w", c_f), ("bg_w", c_f), ("grad_scale", c_f)]


class EnergyDonorItem(ctypes.Structure):
    """dh_energy_donor_item: one item of dh_energy_fwd_bwd_planned_donor_batch"""
    _fields_ = [("item", EnergyItem), ("donor", c_p), ("donor_objects", ctypes.c_uint32)]


class ReprojectArgs(ctypes.Structure):
    """dh_reproject_args: the one argument record of dh_reproject / dh_reproject_workspace (zero means off); field for field
    the header's struct.  A new record has struct_bytes set."""
    _i32, _u8p, _i32p = ctypes.c_int32, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
    _fields_ = [("struct_bytes", ctypes.c_uint32),
                ("res", _i32), ("n_fg", _i32), ("n_objects", _i32), ("n_edits", _i32), ("n_instances", _i32), ("n_bones", _i32),
                ("corr_capacity", _i32),
                ("footprints", _i32), ("n_donor_objects", _i32), ("infill_border", _i32), ("view_surfaces", _i32),
                ("max_ratio", c_f), ("surface_max_ratio", c_f), ("inv_fx", c_f), ("inv_fy", c_f), ("fx", c_d), ("fy", c_d),
                # device inputs
                ("depth", c_p), ("bg_depth", c_p), ("fg_pix", c_p), ("grid_x", c_p), ("grid_y", c_p), ("bounds", c_p),
                ("donor_depth", c_p), ("bg_valid", c_p), ("bone_w", c_p),
                # host inputs
                ("obj_start", _i32p), ("inst_obj", _i32p), ("xforms_host", ctypes.POINTER(c_d)), ("views", ctypes.POINTER(c_d)),
                ("has_view", _u8p),
                # device outputs
                ("zmap", c_p), ("raw_mask", c_p), ("clean_mask", c_p), ("disparity", c_p), ("vis", c_p), ("target_xy", c_p),
                ("corr", c_p), ("corr_inst", c_p), ("counts", c_p), ("bg_corr", c_p), ("bg_counts", c_p),
                ("workspace", c_p), ("workspace_bytes", c_sz), ("stream", c_p)]

    def __init__(self, **fields):
        super().__init__(struct_bytes=ctypes.sizeof(ReprojectArgs), **fields)


class LockItem(ctypes.Structure):
    """dh_lock_item: one edit of dh_ddim_cfg_step_locked"""
    _fields_ = [("keep", c_p), ("ref", c_p)]


class GemmPlanQuery(ctypes.Structure):
    """dh_gemm_plan_query: one GEMM launch described without pointers (dh_dbg_gemm_plan)"""
    _fields_ = [("M", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32), ("conv", ctypes.c_int32), ("hw", ctypes.c_int32),
                ("stride", ctypes.c_int32), ("up", ctypes.c_int32), ("lda", ctypes.c_int64), ("ldc", ctypes.c_int64),
                ("partial_elems", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("gn_HW", ctypes.c_int32), ("gn_G", ctypes.c_int32),
                ("glub_f", ctypes.c_int32), ("xa_Nq", ctypes.c_int32), ("xa_Nk", ctypes.c_int32), ("xa_H", ctypes.c_int32)]


class AttnPlanQuery(ctypes.Structure):
    """dh_attn_plan_query: one attention launch described without pointers (dh_dbg_attn_plan)"""
    _fields_ = [("kind", ctypes.c_int32), ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("Nq", ctypes.c_int32), ("Nk", ctypes.c_int32),
                ("causal", ctypes.c_int32), ("scratch_elems", ctypes.c_uint64), ("force_ks", ctypes.c_int32), ("force_qw", ctypes.c_int32),
                ("force_dkv_ks", ctypes.c_int32), ("force_dkv_qw", ctypes.c_int32), ("cus", ctypes.c_int32)]


# name -> (restype, argtypes); mirrors include/diffhandles_hip.h one to one
SIGNATURES = {
    "dh_last_error": (ctypes.c_char_p, []),
    # host-only query of the GEMM dispatch (declared in the header; tests/test_gemm_plan.py)
    "dh_dbg_gemm_plan": (c_i, [ctypes.POINTER(GemmPlanQuery), ctypes.POINTER(ctypes.c_int32), c_i]),
    # host-only query of the attention dispatch, and what the last launch of a kind passed (tests/test_attn_plan.py)
    "dh_dbg_attn_plan": (c_i, [ctypes.POINTER(AttnPlanQuery), ctypes.POINTER(ctypes.c_int32), c_i]),
    "dh_dbg_attn_last_launch": (c_i, [c_i, ctypes.POINTER(ctypes.c_int32), c_i]),
    # (dtype, x, ldx, gamma, beta, y, stats, dy, add, dx, rows, C, eps, stream): dh_dbg_layernorm with a row pitch for x
    "dh_dbg_layernorm_ld": (c_i, [c_i, c_p, c_l, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_f, c_p]),
    "dh_version": (c_i, []),
    "dh_device_count": (c_i, []),
    "dh_reproject_workspace_bytes": (c_i, [c_i, c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_fg_pixel_list": (c_i, [c_p, c_i, c_p, c_p, c_p, c_sz, c_p]),
    "dh_reproject_edits": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_f, c_f, c_d, c_d, c_i,
                                 ctypes.POINTER(c_d), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "dh_reproject_objects_workspace_bytes": (c_i, [c_i, c_i, c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_reproject_object_edits": (c_i, [c_p, c_p, c_p, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_i, c_p, c_p, c_f, c_f, c_d, c_d,
                                        c_i, ctypes.POINTER(c_d), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "dh_reproject_similarity_edits": (c_i, [c_p, c_p, c_p, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_i, c_p, c_p, c_f, c_f, c_d,
                                            c_d, c_i, ctypes.POINTER(c_d), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                            c_p]),
    "dh_reproject_footprints_workspace_bytes": (c_i, [c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_reproject_footprint_edits": (c_i, [c_p, c_p, c_p, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_i, c_p, c_p, c_f, c_f, c_d,
                                           c_d, c_i, ctypes.POINTER(c_d), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                           c_p, c_i, c_f, c_i]),
    "dh_reproject_instances_workspace_bytes": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_reproject_instance_edits": (c_i, [c_p, c_p, c_p, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_i, c_p, c_p, c_f, c_f, c_d,
                                          c_d, c_i, ctypes.POINTER(c_d), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                          c_p, c_i, c_f, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_p]),
    "dh_reproject_donor_workspace_bytes": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_reproject_donor_edits": (c_i, [c_p, c_p, c_p, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_i, c_p, c_p, c_f, c_f, c_d,
                                       c_d, c_i, ctypes.POINTER(c_d), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                       c_p, c_i, c_f, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_p, c_p, c_i]),
    "dh_reproject_camera_workspace_bytes": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_reproject_camera_edits": (c_i, [c_p, c_p, c_p, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_i, c_p, c_p, c_f, c_f, c_d,
                                        c_d, c_i, ctypes.POINTER(c_d), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                        c_p, c_i, c_f, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_p, c_p, c_i,
                                        ctypes.POINTER(c_d), ctypes.POINTER(ctypes.c_uint8), c_p, c_p, c_p]),
    "dh_reproject_camera_background": (c_i, [c_p, c_i, c_p, c_p, c_f, c_f, c_d, c_d, c_p, c_p, c_p, c_p, c_p, c_sz, c_p,
                                             ctypes.POINTER(c_d), c_p, c_p, c_p]),
    "dh_reproject_border_edits": (c_i, [c_p, c_p, c_p, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_i, c_p, c_p, c_f, c_f, c_d,
                                        c_d, c_i, ctypes.POINTER(c_d), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                        c_p, c_i, c_f, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_p, c_p, c_i,
                                        ctypes.POINTER(c_d), ctypes.POINTER(ctypes.c_uint8), c_p, c_p, c_p, c_i]),
    "dh_reproject_border_background": (c_i, [c_p, c_i, c_p, c_p, c_f, c_f, c_d, c_d, c_p, c_p, c_p, c_p, c_p, c_sz, c_p,
                                             ctypes.POINTER(c_d), c_p, c_p, c_p, c_i]),
    "dh_reproject_surface_ws_bytes": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_reproject_surface_background_ws_bytes": (c_i, [c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_reproject_surface_edits": (c_i, [c_p, c_p, c_p, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_i, c_p, c_p, c_f, c_f, c_d,
                                         c_d, c_i, ctypes.POINTER(c_d), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                         c_p, c_i, c_f, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_p, c_p, c_i,
                                         ctypes.POINTER(c_d), ctypes.POINTER(ctypes.c_uint8), c_p, c_p, c_p, c_i, c_i, c_f]),
    "dh_reproject_surface_background": (c_i, [c_p, c_i, c_p, c_p, c_f, c_f, c_d, c_d, c_p, c_p, c_p, c_p, c_p, c_sz, c_p,
                                              ctypes.POINTER(c_d), c_p, c_p, c_p, c_i, c_i, c_f]),
    "dh_reproject_bend_ws_bytes": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_reproject_bend_edits": (c_i, [c_p, c_p, c_p, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_i, c_p, c_p, c_f, c_f, c_d,
                                      c_d, c_i, ctypes.POINTER(c_d), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                      c_p, c_i, c_f, c_i, c_i, ctypes.POINTER(ctypes.c_int32), c_p, c_p, c_i,
                                      ctypes.POINTER(c_d), ctypes.POINTER(ctypes.c_uint8), c_p, c_p, c_p, c_i, c_i, c_f, c_i, c_p]),
    # the call and its query; every dh_reproject_* row above is this record filled by the library (csrc/reproject_compat.cpp)
    "dh_reproject": (c_i, [ctypes.POINTER(ReprojectArgs)]),
    "dh_reproject_workspace": (c_i, [ctypes.POINTER(ReprojectArgs), ctypes.POINTER(c_sz)]),
    "dh_reproject_background_workspace_bytes": (c_i, [c_i, ctypes.POINTER(c_sz)]),
    "dh_reproject_background": (c_i, [c_p, c_i, c_p, c_p, c_f, c_f, c_d, c_d, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "dh_unproject": (c_i, [c_p, c_i, c_p, c_p, c_f, c_f, c_p, c_p]),
    "dh_masked_centroid": (c_i, [c_p, c_p, c_i, c_i, c_p, c_p, c_f, c_f, c_p, c_p]),
    "dh_laplacian_blend_workspace_bytes": (c_i, [c_i, ctypes.POINTER(c_sz)]),
    "dh_laplacian_blend": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_sz, c_p]),
    "dh_laplacian_blend_border": (c_i, [c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_sz, c_p, c_i]),
    "dh_cells_workspace_bytes": (c_i, [c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_cells_from_correspondences": (c_i, [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "dh_cells_from_correspondences_vacated": (c_i, [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p, c_p]),
    "dh_cells_from_correspondences_donor": (c_i, [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p, c_p, c_p]),
    "dh_cells_from_correspondences_rows": (c_i, [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p, c_p, c_p]),
    "dh_energy_workspace_bytes": (c_i, [c_i, c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_energy_fwd_bwd": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_i,
                                c_f, c_f, c_i, c_i, c_i, c_f, c_p, c_p, c_i, c_p, c_sz, c_p]),
    "dh_mesh_workspace_bytes": (c_i, [c_i, ctypes.POINTER(c_sz)]),
    "dh_mesh_reproject": (c_i, [c_p, c_p, c_p, c_i, c_p, c_p, c_f, c_f, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_p, c_p,
                                c_sz, c_p]),
    "dh_energy_plan_bytes": (c_i, [c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_energy_plan_build": (c_i, [c_p, c_i, c_p, c_i, c_i, c_p, c_sz, c_p]),
    "dh_energy_planned_workspace_bytes": (c_i, [c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_energy_fwd_bwd_planned": (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_sz, c_i, c_p, c_i, c_p, c_i, c_f, c_f, c_f,
                                        c_p, c_p, c_i, c_p, c_sz, c_p]),
    "dh_energy_planned_batch_workspace_bytes": (c_i, [c_i, c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_energy_fwd_bwd_planned_batch": (c_i, [ctypes.POINTER(EnergyItem), c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "dh_energy_plan_objects_bytes": (c_i, [c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_energy_plan_build_objects": (c_i, [c_p, c_p, c_i, c_p, c_i, c_i, c_i, ctypes.POINTER(c_f), ctypes.POINTER(ctypes.c_int32),
                                           c_p, c_sz, c_p]),
    "dh_energy_fwd_bwd_planned_objects": (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_sz, c_i, c_p, c_i, c_p, c_i, c_f, c_f, c_f,
                                                c_p, c_p, c_i, c_p, c_sz, c_p]),
    "dh_energy_planned_objects_batch_workspace_bytes": (c_i, [c_i, c_i, c_i, ctypes.POINTER(c_sz)]),
    "dh_energy_fwd_bwd_planned_objects_batch": (c_i, [ctypes.POINTER(EnergyItem), c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "dh_energy_fwd_bwd_planned_mixed_batch": (c_i, [ctypes.POINTER(EnergyItem), ctypes.POINTER(ctypes.c_uint8), c_i, c_i, c_i, c_i, c_i,
                                              c_p, c_sz, c_p]),
    "dh_energy_fwd_bwd_planned_donor": (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_sz, c_i, c_p, c_i, c_p, c_i, c_f, c_f, c_f,
                                              c_p, c_p, c_i, c_p, c_sz, c_p, c_p, ctypes.c_uint32]),
    "dh_energy_fwd_bwd_planned_donor_batch": (c_i, [ctypes.POINTER(EnergyDonorItem), c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p]),
    "dh_unet_create": (c_i, [ctypes.POINTER(UNetConfig), ctypes.POINTER(c_p)]),
    "dh_unet_create_shared": (c_i, [c_p, c_i, c_p, ctypes.POINTER(c_p)]),
    "dh_unet_destroy": (None, [c_p]),
    "dh_unet_num_params": (c_i, [c_p]),
    "dh_unet_param_info": (c_i, [c_p, c_i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_i),
                                 ctypes.POINTER(ctypes.c_int64)]),
    "dh_unet_load_param": (c_i, [c_p, c_i, c_p, c_p]),
    "dh_unet_weight_bytes": (c_sz, [c_p]),
    "dh_unet_workspace_bytes": (c_sz, [c_p]),
    "dh_unet_forward": (c_i, [c_p, c_p, c_f, c_p, c_i, c_i, c_p, ctypes.POINTER(c_p), c_p]),
    "dh_unet_backward": (c_i, [c_p, ctypes.POINTER(c_p), c_p, c_p, c_p, c_p]),
    "dh_unet_set_text_key": (c_i, [c_p, ctypes.c_ulonglong]),
    "dh_unet_stats": (c_i, [c_p, ctypes.POINTER(c_d), ctypes.POINTER(c_d), ctypes.POINTER(ctypes.c_int64)]),
    "dh_vae_decoder_create": (c_i, [c_p, ctypes.POINTER(c_p)]),
    "dh_vae_decoder_destroy": (None, [c_p]),
    "dh_vae_decoder_num_params": (c_i, [c_p]),
    "dh_vae_decoder_param_info": (c_i, [c_p, c_i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_i),
                                        ctypes.POINTER(ctypes.c_int64)]),
    "dh_vae_decoder_load_param": (c_i, [c_p, c_i, c_p, c_p]),
    "dh_vae_decoder_bytes": (c_sz, [c_p]),
    "dh_vae_decoder_decode": (c_i, [c_p, c_p, c_i, c_p, c_p]),
    "dh_vae_encoder_create": (c_i, [c_p, ctypes.POINTER(c_p)]),
    "dh_vae_encoder_encode": (c_i, [c_p, c_p, c_i, c_p, c_p]),
    "dh_text_encoder_create": (c_i, [c_p, ctypes.POINTER(c_p)]),
    "dh_text_encoder_destroy": (None, [c_p]),
    "dh_text_encoder_num_params": (c_i, [c_p]),
    "dh_text_encoder_param_info": (c_i, [c_p, c_i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_i),
                                         ctypes.POINTER(ctypes.c_int64)]),
    "dh_text_encoder_load_param": (c_i, [c_p, c_i, c_p, c_p]),
    "dh_text_encoder_bytes": (c_sz, [c_p]),
    "dh_text_encoder_encode": (c_i, [c_p, c_p, c_i, c_i, c_p, c_p]),
    "dh_gemm_profile_begin": (c_i, []),
    "dh_gemm_profile_end": (c_i, [ctypes.POINTER(c_d), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_d)]),
    "dh_gemm_profile_bytes": (c_i, [ctypes.POINTER(c_d)]),
    "dh_ddim_cfg_step": (c_i, [c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_i, c_p]),
    "dh_latent_update": (c_i, [c_p, c_p, c_p, c_f, c_f, c_i, c_p]),
    "dh_adam_step": (c_i, [c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_f, c_i, c_i, c_p]),
    "dh_mse_fwd_bwd": (c_i, [c_p, c_p, c_i, c_p, c_p, c_p]),
    "dh_latent_update_strided": (c_i, [c_p, c_p, c_p, c_i, c_i, c_f, c_f, c_i, c_p]),
    "dh_pack_sample": (c_i, [c_p, c_p, c_i, c_i, c_p, c_i, c_i, c_i, c_i, c_p]),
    "dh_unet_io_ptr": (c_i, [c_p, c_i, c_i, ctypes.POINTER(c_p), ctypes.POINTER(c_sz)]),
    "dh_mse_cotangent": (c_i, [c_p, c_p, c_i, c_f, c_f, c_p, c_p, c_p, c_p]),
    "dh_adam_step_scaled": (c_i, [c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_f, c_i, c_i, c_p]),
    "dh_mse_cotangent_batch": (c_i, [c_p, c_p, c_i, c_i, c_f, c_f, c_d, c_p, c_p, c_p, c_p, c_p, c_p]),
    "dh_adam_step_scaled_batch": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_p]),
    "dh_latent_update_guarded": (c_i, [c_p, c_p, c_p, c_i, c_i, c_f, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_p]),
    "dh_ddim_cfg_step_flagged": (c_i, [c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_i, c_i, c_p, c_i, c_i, c_p]),
    "dh_ddim_cfg_step_locked": (c_i, [c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_i, c_i, c_i, ctypes.POINTER(LockItem), c_i, c_p, c_i, c_i,
                                      c_p]),
    "dh_keep_map": (c_i, [c_p, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_sz, c_p]),
}

# test hooks (csrc/debug_api.cpp): single-kernel entry points used only by tests/
DEBUG_SIGNATURES = {
    "dh_dbg_gemm": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_i,
                          c_p, c_l, c_p, c_l, c_i, c_p, c_sz, c_p]),
    "dh_dbg_gemm_groupnorm": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_sz, c_i, c_i, c_p, c_p, c_f, c_i,
                                    c_p, c_p, c_p, ctypes.POINTER(c_i), c_p]),
    # (dtype, A, lda, W, M, N, K, mode, Hin, Win, Cin, C, partial, partial_elems, HW, G, x, gamma, beta, stats, silu, dx, scratch, have_out, stream)
    "dh_dbg_gemm_groupnorm_bwd": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_sz, c_i, c_i, c_p, c_p, c_p, c_p, c_i,
                                        c_p, c_p, ctypes.POINTER(c_i), c_p]),
    # the same two with a residual R (row pitch ldr; NULL, or C itself)
    # (dtype, A, lda, W, M, N, K, mode, Hin, Win, Cin, bias, R, ldr, C, partial, partial_elems, HW, G, gamma, beta, eps, silu, Y, stats,
    #  scratch, have_out, stream)
    "dh_dbg_gemm_groupnorm_res": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_l, c_p, c_p, c_sz, c_i, c_i, c_p, c_p,
                                    c_f, c_i, c_p, c_p, c_p, ctypes.POINTER(c_i), c_p]),
    # (dtype, A, lda, W, M, N, K, mode, Hin, Win, Cin, R, ldr, C, partial, partial_elems, HW, G, x, gamma, beta, stats, silu, dx, scratch,
    #  have_out, stream)
    "dh_dbg_gemm_groupnorm_bwd_res": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_l, c_p, c_p, c_sz, c_i, c_i, c_p, c_p, c_p,
                                        c_p, c_i, c_p, c_p, ctypes.POINTER(c_i), c_p]),
    # ... and with the whole convolution geometry (and the forward's per-image vector)
    # (dtype, A, lda, W, M, N, K, mode, Hin, Win, Cin, Hout, Wout, stride, up, bias, rowvec, rowvec_ld, rows_per_batch, R, ldr, C, partial,
    #  partial_elems, HW, G, gamma, beta, eps, silu, Y, stats, scratch, have_out, stream)
    "dh_dbg_gemm_groupnorm_geo": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_p, c_l,
                                        c_p, c_p, c_sz, c_i, c_i, c_p, c_p, c_f, c_i, c_p, c_p, c_p, ctypes.POINTER(c_i), c_p]),
    # (dtype, A, lda, W, M, N, K, mode, Hin, Win, Cin, Hout, Wout, stride, up, R, ldr, C, partial, partial_elems, HW, G, x, gamma, beta,
    #  stats, silu, dx, scratch, have_out, stream)
    "dh_dbg_gemm_groupnorm_bwd_geo": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_l, c_p, c_p, c_sz,
                                            c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p, ctypes.POINTER(c_i), c_p]),
    # (dtype, A, lda, W, M, N, K, ln_s, ln_t, ln_stats, ln_eps, C, y, stream)
    "dh_dbg_gemm_lnfold_glu": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_f, c_p, c_p, c_p]),
    # (dtype, A, lda, W, M, N, K, x, ldx, gamma, stats, add, dy, dx, partial, partial_elems, done_out, stream)
    "dh_dbg_gemm_layernorm_bwd": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_p, c_l, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                        ctypes.POINTER(c_i), c_p]),
    # (dtype, a, Ca, b, Cb, out, B, HW, G, gamma, beta, eps, silu, Y, stats, scratch, stream)
    "dh_dbg_concat_groupnorm": (c_i, [c_i, c_p, c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_f, c_i, c_p, c_p, c_p, c_p]),
    "dh_dbg_gemm_last_tile": (c_i, [ctypes.POINTER(c_i)]),
    "dh_dbg_unet_concat_ops": (c_i, [ctypes.POINTER(UNetConfig), ctypes.POINTER(c_i), c_i, ctypes.POINTER(c_i)]),
    "dh_dbg_gemm_lnfold": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_f, c_p, c_l, c_p]),
    "dh_dbg_gemm_glu": (c_i, [c_i, c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "dh_dbg_gemm_glub_split": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_i, c_p, c_l, c_i, c_p, c_p, ctypes.POINTER(c_i), c_p]),
    "dh_dbg_unet_ff_fold": (c_i, [c_p, c_i, ctypes.POINTER(c_i), ctypes.POINTER(c_i), c_p, c_p, c_p]),
    "dh_dbg_gemm_family": (c_i, [c_i]),
    "dh_dbg_gemm_stage": (c_i, [c_i]),
    "dh_dbg_gemm_xattn": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_l, c_p, c_p, c_i, c_i, c_i,
                                ctypes.POINTER(c_i), c_p]),
    "dh_dbg_gemm_xattn_dq": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_l, c_p, c_p, c_p, c_i, c_i, ctypes.POINTER(c_i), c_p]),
    "dh_dbg_gemm_xattn_carried": (c_i, [ctypes.POINTER(c_i), ctypes.POINTER(ctypes.c_longlong)]),
    "dh_dbg_gemm_pp_variant": (c_i, [c_i, c_p]),
    "dh_dbg_gemm_pp_ablate": (c_i, [c_i]),
    "dh_dbg_gemm_pp_persist": (c_i, [c_i]),
    "dh_dbg_gemm_pp_glu": (c_i, [c_i]),
    "dh_dbg_gemm_pp_plan": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i, c_sz, ctypes.POINTER(c_i), ctypes.POINTER(c_i), ctypes.POINTER(c_i)]),
    "dh_dbg_touch_tiled": (c_i, [c_sz, c_p]),
    "dh_dbg_groupnorm": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_i, c_i, c_p]),
    "dh_dbg_layernorm": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_f, c_p]),
    "dh_dbg_geglu": (c_i, [c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_p]),
    "dh_dbg_attention": (c_i, [c_i, c_p, c_l, c_p, c_p, c_l, c_p, c_l, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "dh_dbg_attention_bwd_pair": (c_i, [c_i, c_p, c_l, c_p, c_p, c_l, c_p, c_l, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p]),
    "dh_dbg_pool2x2": (c_i, [c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "dh_dbg_ellipse_offsets": (c_i, [c_i, ctypes.POINTER(ctypes.c_int32), c_i, ctypes.POINTER(c_i)]),
    "dh_dbg_lane_ops": (c_i, [c_p, c_p, c_p, c_p]),
    "dh_dbg_cg_limits": (c_i, [ctypes.POINTER(c_i)]),
    "dh_dbg_cg_max_iter": (c_i, [c_i]),
    "dh_dbg_footprint_tier": (c_i, [c_i]),
    # arena hooks (host only): the gap every workspace take leaves behind it, and the log of takes (base, offset, bytes)
    "dh_dbg_arena_gap": (c_i, [c_i]),
    "dh_dbg_arena_log": (c_i, [c_i]),
    "dh_dbg_arena_log_read": (c_i, [ctypes.POINTER(ctypes.c_int64), c_i, ctypes.POINTER(c_i)]),
    # (record, out, cap, n): the members of a dh_reproject_args as the library reads them (tests/test_reproject_record.py)
    "dh_dbg_reproject_args": (c_i, [ctypes.POINTER(ReprojectArgs), ctypes.POINTER(ctypes.c_int64), c_i, ctypes.POINTER(c_i)]),
    # hooks of the kernels only the engines launch (tests/test_engine_kernels_gpu.py)
    # dh_dbg_gemm's arguments with `pad` behind `up`
    "dh_dbg_gemm_pad": (c_i, [c_i, c_p, c_l, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_i,
                              c_p, c_l, c_p, c_l, c_i, c_p, c_sz, c_p]),
    # (dtype, q, ldq, k, v, ldk, o, ldo, lse, B, H, Nq, Nk, stream)
    "dh_dbg_attention_causal": (c_i, [c_i, c_p, c_l, c_p, c_p, c_l, c_p, c_l, c_p, c_i, c_i, c_i, c_i, c_p]),
    # (dtype, qkv, ld, N, C, out, tiled, scores, partial, partial_elems, stream)
    "dh_dbg_vae_attention": (c_i, [c_i, c_p, c_l, c_i, c_i, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "dh_dbg_softmax_rows": (c_i, [c_i, c_p, c_i, c_i, c_p]),
    # (dtype, bwd, x, x_is_f32, w, bias, y, y_is_f32, accumulate, B, H, W, Cin, Cout, stream)
    "dh_dbg_conv_small": (c_i, [c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    # dh_dbg_groupnorm's arguments, then (out0, out1, split_c, stream)
    "dh_dbg_groupnorm_split": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_i, c_i, c_p, c_p, c_i, c_p]),
    "dh_dbg_gelu": (c_i, [c_i, c_p, c_p, c_sz, c_p]),
    "dh_dbg_copy_cols": (c_i, [c_i, c_p, c_l, c_p, c_l, c_i, c_i, c_i, c_p]),
    # (dtype, src, lds, dstA, ldA, colsA, accA, dstB, ldB, colsB, accB, rows, stream)
    "dh_dbg_split_cols": (c_i, [c_i, c_p, c_l, c_p, c_l, c_i, c_i, c_p, c_l, c_i, c_i, c_i, c_p]),
    # (dtype, to_f32, src, dst, n, accumulate, stream)
    "dh_dbg_convert": (c_i, [c_i, c_i, c_p, c_p, c_sz, c_i, c_p]),
    "dh_dbg_timestep": (c_i, [c_i, c_p, c_i, c_i, c_p, c_p]),
}


def lib():
    """Load the shared library once; raise loudly if it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"native HIP library not found at {LIB_PATH}; build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)")
        handle = ctypes.CDLL(LIB_PATH)
        missing = []
        for name, (res, args) in list(SIGNATURES.items()) + list(DEBUG_SIGNATURES.items()):
            try:
                fn = getattr(handle, name)
            except AttributeError:
                missing.append(name)      # calling it later raises AttributeError (tests/test_abi.py checks none are missing)
                continue
            fn.restype = res
            fn.argtypes = args
        handle.dh_missing_symbols = missing
        # measurement switches of the GEMM dispatch, for same-box A/Bs of whole programs (bench.py, the harnesses): set before any
        # hipGraph is captured, i.e. here.  Never set in production; unknown to libraries that predate a switch.
        for env, fn in (("DH_GEMM_FAMILY", "dh_dbg_gemm_family"), ("DH_PP_GLU", "dh_dbg_gemm_pp_glu"),
                        ("DH_PP_PERSIST", "dh_dbg_gemm_pp_persist"), ("DH_GEMM_STAGE", "dh_dbg_gemm_stage")):
            if os.environ.get(env) and fn not in missing:
                getattr(handle, fn)(int(os.environ[env]))
        _LIB = handle
    return _LIB


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib().dh_last_error().decode()}")


def require_gpu(t=None):
    if not torch.cuda.is_available():
        raise RuntimeError("diffusionhandles_amd needs a HIP device (MI355X); there is no CPU fallback")
    if t is not None and not t.is_cuda:
        raise RuntimeError("expected a device tensor")


def ptr(t):
    return c_p(t.data_ptr()) if t is not None else c_p(0)


def stream_ptr():
    return c_p(torch.cuda.current_stream().cuda_stream)


DTYPE_CODE = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}
CODE_DTYPE = {v: k for k, v in DTYPE_CODE.items()}
