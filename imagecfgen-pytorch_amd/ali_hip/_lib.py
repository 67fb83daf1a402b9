"""ctypes binding of libali_hip.so (C ABI declared in include/ali_hip.h).

The library is the product: if it cannot be loaded every GPU entry point raises
``AliHipUnavailable`` -- there is no CPU or eager-PyTorch fallback for CUDA tensors.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libali_hip.so")


class AliHipUnavailable(RuntimeError):
    pass


class AliConvGeom(Structure):
    _fields_ = [(n, c_int32) for n in ("B", "H", "W", "C", "P", "Q", "K", "R", "S", "stride", "pad")]


class AliEpilogue(Structure):
    _fields_ = [("bias", c_void_p), ("act", c_int32), ("slope", c_float), ("mask", c_void_p), ("mask_ld", c_int32),
                ("dact_y", c_void_p), ("dact", c_int32), ("dslope", c_float),
                # fused BatchNorm reductions (include/ali_hip.h)
                ("bn_part", c_void_p), ("bn_mode", c_int32), ("bn_groups", c_int32), ("bn_stat_mask", c_void_p),
                ("bn_mask_ld", c_int32), ("bn_x", c_void_p), ("bn_mean", c_void_p), ("bn_invstd", c_void_p),
                ("bn_mask_in", c_void_p), ("bn_mask_pre", c_void_p), ("mfma_f16", c_int32),
                ("in16", c_void_p), ("w16", c_void_p), ("out16", c_void_p),
                ("tile_order", c_void_p), ("tile_order_n", c_int32), ("in_ld", c_int32), ("out_ld", c_int32),
                ("in_ch_live", c_int32), ("bn_slots", c_int32), ("dact_y16", c_void_p)]


class AliConvPlan(Structure):
    _fields_ = [(n, c_int32) for n in ("route", "bm", "bn", "mode", "f16", "uni", "threads", "ntile_m", "ntile_n",
                                       "tile_rows", "pixel_major", "splitk", "kt_per_split", "tail_split", "tail_u0",
                                       "lin1d", "xcd_chunk", "ordered", "grid_x", "grid_y", "grid_z", "job_variant",
                                       "empty")]


class AliWgradFold(Structure):
    _fields_ = [("ws", c_void_p), ("dst", c_void_p), ("dbws", c_void_p), ("db", c_void_p),
                ("slab", c_int64), ("s_dc", c_int64), ("s_gc", c_int64), ("s_tap", c_int64),
                ("S", c_int32), ("Mtot", c_int32), ("Cg", c_int32), ("Cd", c_int32), ("Cg_log", c_int32),
                ("Cd_log", c_int32), ("T", c_int32), ("reserved", c_int32), ("ws_used", c_uint64)]


class AliWgradJob(Structure):
    _fields_ = [("opaque", c_uint64 * 40)]


class AliCfSegment(Structure):
    _fields_ = [("kind", c_int32), ("width", c_int32), ("src_off", c_int32), ("dst_off", c_int32), ("table", c_int32),
                ("attr_off", c_int32)]


class AliGemmJob(Structure):
    _fields_ = [("opaque", c_uint64 * 112)]


class AliCatPlan(Structure):
    _fields_ = [(n, c_int32) for n in ("grid", "threads", "tile_rows", "tiles", "tiles_per_block", "grid2", "threads2",
                                       "lds_bytes")] + [("ws_bytes", c_uint64)]


class AliCatMapArgs(Structure):
    _fields_ = [("country", c_void_p), ("country_ld", c_int64), ("country_cf", c_void_p), ("country_cf_ld", c_int64),
                ("native_rows", c_void_p), ("native_ld", c_int64), ("y", c_void_p * 2), ("v", c_void_p * 2),
                ("node", c_int32), ("cf_mask", c_int32), ("out", c_void_p * 2), ("status", c_void_p),
                ("logits_out", c_void_p), ("g_out", c_void_p), ("noise_out", c_void_p)]


ACT_NONE, ACT_LEAKY, ACT_TANH = 0, 1, 2

# name -> (restype, argtypes); every symbol include/ali_hip.h declares
SIGNATURES = {
    "ali_conv_workspace_bytes": (c_size_t, [POINTER(AliConvGeom), c_int32]),
    "ali_conv_mtiles": (c_int32, [POINTER(AliConvGeom), c_int32, c_int32, POINTER(c_int32), POINTER(c_int32)]),
    "ali_conv_writes_out16": (c_int32, [POINTER(AliConvGeom), c_int32]),
    "ali_conv_uses_f16": (c_int32, [POINTER(AliConvGeom), c_int32, POINTER(AliEpilogue)]),
    "ali_conv_tile_order": (c_int32, [POINTER(AliConvGeom), c_int32, c_int32, c_void_p, c_int32]),
    "ali_conv_plan": (c_int32, [POINTER(AliConvGeom), c_int32, POINTER(AliEpilogue), c_size_t, c_int32, c_int32,
                                POINTER(AliConvPlan)]),
    "ali_conv_fwd": (c_int32, [POINTER(AliConvGeom), c_void_p, c_void_p, c_void_p, POINTER(AliEpilogue), c_void_p,
                               c_size_t, c_void_p]),
    "ali_conv_bwd_data": (c_int32, [POINTER(AliConvGeom), c_void_p, c_void_p, c_void_p, POINTER(AliEpilogue),
                                    c_void_p, c_size_t, c_void_p]),
    "ali_conv_bwd_weight": (c_int32, [POINTER(AliConvGeom), c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int64,
                                      c_int64, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32,
                                      POINTER(AliWgradFold), POINTER(AliWgradJob), c_int32, c_void_p, c_size_t, c_void_p]),
    "ali_conv_fwd_job": (c_int32, [POINTER(AliConvGeom), c_void_p, c_void_p, c_void_p, POINTER(AliEpilogue), c_void_p,
                                   c_size_t, POINTER(AliGemmJob), c_void_p]),
    "ali_conv_bwd_data_job": (c_int32, [POINTER(AliConvGeom), c_void_p, c_void_p, c_void_p, POINTER(AliEpilogue),
                                        c_void_p, c_size_t, POINTER(AliGemmJob), c_void_p]),
    "ali_gemm_launch_multi": (c_int32, [c_int32, POINTER(AliGemmJob), c_void_p]),
    "ali_wgrad_deferrable": (c_int32, [POINTER(AliConvGeom), c_int32]),
    "ali_wgrad_launch_multi": (c_int32, [c_int32, POINTER(AliWgradJob), c_void_p]),
    "ali_wgrad_fold_multi": (c_int32, [c_int32, POINTER(AliWgradFold), c_void_p]),
    "ali_wgrad_pixtab": (c_int32, [POINTER(AliConvGeom), c_void_p, c_void_p]),
    "ali_pack_weights": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int64, c_int64, c_int64,
                                   c_void_p]),
    "ali_pack_weights_multi": (c_int32, [c_int32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                                         POINTER(c_int32), POINTER(c_int64), c_void_p]),
    "ali_act_bwd": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_float, c_void_p]),
    "ali_colsum": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_rowmask_mul": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "ali_dropout_mask": (c_int32, [c_uint64, c_uint64, c_void_p, c_float, c_void_p, c_int64, c_void_p]),
    "ali_dropout_mask_multi": (c_int32, [c_uint64, c_void_p, POINTER(c_int64), POINTER(c_float), POINTER(c_int32),
                                         POINTER(c_int32), c_int32, c_void_p, c_void_p]),
    "ali_normal_fill": (c_int32, [c_uint64, c_void_p, c_uint64, c_void_p, c_int64, c_void_p]),
    "ali_batch_gather": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int32,
                                   c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ali_bn_stats": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_float, c_float, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64,
                               c_void_p, c_size_t, c_void_p]),
    "ali_bn_apply": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                               c_int32, c_int64, c_void_p]),
    "ali_bn_bwd": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                             c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_bn_stats_from_partials": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                             c_void_p]),
    "ali_bn_bwd_from_partials": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p,
                                           c_void_p, c_void_p]),
    "ali_ew_plan": (c_int32, [c_int32, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    "ali_bce_logits": (c_int32, [c_void_p, c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "ali_softmax_xent": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_vae_latent_fwd": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_uint64, c_void_p, c_uint64,
                                    c_int32, c_int32, c_int32, c_float, POINTER(c_void_p), POINTER(c_int32),
                                    POINTER(c_int32), POINTER(c_void_p), c_int32, c_void_p, c_int32, c_int32, c_int32,
                                    c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_vae_loglik": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_void_p, c_float, c_float,
                                c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_vae_latent_bwd": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                    c_float, c_float, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "ali_row_dist": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p, c_size_t,
                              c_void_p]),
    "ali_cf_hinge": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int32, c_int32, c_void_p, c_void_p,
                              c_void_p]),
    "ali_cf_join": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p, c_void_p]),
    "ali_cf_input_fwd": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, POINTER(AliCfSegment), c_int32,
                                  POINTER(c_void_p), c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                  c_void_p]),
    "ali_cf_input_step": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, POINTER(AliCfSegment), c_int32,
                                   POINTER(c_void_p), c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                   c_void_p, c_double, c_double, c_double, c_double, c_void_p, c_void_p]),
    "ali_cf_select": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    "ali_eg_input": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint64,
                              POINTER(AliCfSegment), c_int32, POINTER(c_void_p), c_int32] + [c_int32] * 8
                     + [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ali_eg_seed": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_double, c_void_p, c_void_p, c_void_p]),
    "ali_eg_reduce": (c_int32, [c_void_p, c_int32, c_void_p, POINTER(AliCfSegment), c_int32, POINTER(c_void_p), c_int32]
                      + [c_int32] * 6 + [c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_ct_attack": (c_int32, [c_void_p] + [c_int32] * 5 + [c_void_p, c_void_p, c_double, c_void_p, c_int32, c_void_p,
                                                             c_void_p, c_void_p, c_void_p]),
    "ali_ct_book": (c_int32, [c_void_p] * 5 + [c_int32, c_int32, c_int64] + [c_void_p] * 10),
    "ali_ct_cem_update": (c_int32, [c_void_p, c_int32] + [c_void_p] * 7 + [c_int32, c_double, c_double, c_double, c_int32,
                                                                          c_int64] + [c_void_p] * 5),
    "ali_ct_ce_update": (c_int32, [c_void_p, c_int32] + [c_void_p] * 8 + [c_int32] + [c_double] * 6
                         + [c_int32, c_int64, c_void_p, c_void_p, c_void_p]),
    "ali_ct_pp_attack": (c_int32, [c_void_p] + [c_int32] * 5 + [c_void_p, c_void_p, c_double, c_void_p, c_int32,
                                                                c_void_p, c_void_p, c_void_p, c_void_p]),
    "ali_ct_pp_update": (c_int32, [c_void_p, c_int32] + [c_void_p] * 3 + [c_float] + [c_void_p] * 2
                         + [c_int32, c_double, c_double, c_double, c_int32, c_int64] + [c_void_p] * 5),
    "ali_bce_logits_pair": (c_int32, [c_void_p, c_int32, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "ali_gp_mix": (c_int32, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_int32, c_int64, c_void_p,
                            c_void_p, c_void_p]),
    "ali_gp_penalty": (c_int32, [c_void_p, c_int32, c_int64, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_wgan_critic": (c_int32, [c_void_p, c_void_p, c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ali_flow_stats": (c_int32, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_float, c_void_p, c_size_t, c_void_p]),
    "ali_flow_nll": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_flow_map": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32,
                              c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ali_gumbel_posterior": (c_int32, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_int32, c_int32,
                                      c_void_p, c_void_p, c_void_p]),
    "ali_cat_plan": (c_int32, [c_int64, c_int32, c_int32, c_int32, c_int32, POINTER(AliCatPlan)]),
    "ali_cat_theta_size": (c_int32, [c_int32, c_int32, c_int32, c_int32]),
    "ali_cat_nll": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_int64,
                              c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_float, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_cat_map": (c_int32, [c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int64, POINTER(AliCatMapArgs),
                              c_uint64, c_void_p, c_uint64, c_void_p]),
    "ali_mse": (c_int32, [c_void_p, c_void_p, c_int64, c_float, c_int32, c_void_p, c_void_p, c_void_p, c_size_t,
                          c_void_p]),
    "ali_cf_recon": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                               c_void_p, c_void_p]),
    "ali_oracle_scores": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                    c_void_p]),
    "ali_group_moments": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ali_manifold_err": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_size_t,
                                   c_void_p]),
    "ali_morpho_binarise": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_float,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_morpho_edt": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_morpho_thin": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_uint64, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_morpho_measure": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ali_morpho_reshape": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                     c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                     c_void_p]),
    "ali_morpho_shear_reduce": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                          c_void_p]),
    "ali_morpho_set_intensity": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                           c_void_p]),
    "ali_morpho_locate": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                    c_int32, c_int32, c_uint64, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p]),
    "ali_morpho_local": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_double, c_double, c_double, c_double, c_int32, c_int32, c_int32,
                                   c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ali_morpho_bounds": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_double,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_morpho_width": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_size_t, c_void_p]),
    "ali_morpho_affine_reduce": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_size_t, c_void_p]),
    "ali_attr_pack": (c_int32, [POINTER(c_void_p), POINTER(c_int32), POINTER(c_int32), c_int32, POINTER(c_void_p), c_int32,
                                c_int32, c_void_p, c_void_p, c_void_p]),
    "ali_g_input": (c_int32, [c_void_p, c_int32, POINTER(c_void_p), POINTER(c_int32), POINTER(c_int32), POINTER(c_void_p),
                              c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "ali_g_input_table_grad": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p,
                                         c_void_p]),
    "ali_adam": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                           c_int32, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "ali_add_i64_multi": (c_int32, [c_int32, POINTER(c_void_p), POINTER(c_int64), c_void_p]),
    "ali_assemble_planes": (c_int32, [c_void_p, c_void_p, POINTER(c_void_p), c_int32, c_void_p, c_int32, c_void_p,
                                      c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "ali_spect_post": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "ali_plane_table_grad": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32,
                                       c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "ali_col2im": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p] + [c_int32] * 12 + [c_float, c_void_p]),
    "ali_tconv_scatter_ok": (c_int32, [c_int32] * 5),
    "ali_tconv_scatter_wgrad_ws": (c_int64, [c_int32] * 7),
    "ali_tconv_scatter_wgrad": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64] + [c_int32] * 10
                                + [c_void_p, c_size_t, c_void_p]),
    "ali_tconv_scatter": (c_int32, [c_void_p] * 4 + [c_int32] * 13 + [c_float, c_void_p]),
    "ali_tconv_scatter_plan": (c_int32, [c_int32] * 13 + [POINTER(c_int64)]),
    "ali_tconv1_fwd": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int32] * 9 + [c_float, c_void_p, c_int32,
                                                                                            c_void_p]),
    "ali_tconv1_dgrad": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_float, c_void_p] + [c_int32] * 7
                         + [c_void_p]),
    "ali_tconv1_wgrad": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_int64, c_int64]
                         + [c_int32] * 7 + [c_void_p, c_size_t, c_void_p]),
    "ali_tconv1_route": (c_int32, [c_int32] * 9 + [c_size_t]),
    "ali_ssim_fwd": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_float, c_float,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ali_ssim_bwd": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32,
                               c_void_p, c_int32, c_void_p, c_void_p]),
    "ali_gl_init": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_float, c_float, c_void_p,
                              c_void_p, c_int32, c_uint64, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p]),
    "ali_gl_ola": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int64, c_int32,
                             c_void_p, c_int32, c_void_p, c_void_p]),
    "ali_gl_phase": (c_int32, [c_void_p, c_void_p, c_void_p, c_float, c_int64, c_int32, c_void_p, c_void_p]),
    "ali_gl_check": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int64]),
    "ali_last_error": (c_char_p, []),
    "ali_head_fwd": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "ali_head_wgrad": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "ali_head_bwd": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_float, c_void_p, c_int32, c_void_p, c_void_p,
                               c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    "ali_copy_multi": (c_int32, [c_int32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int64), c_void_p]),
    "ali_version": (c_int32, []),
    "ali_reload_tuning": (None, []),
}

_lib = None
_load_error = None


def load():
    """Load libali_hip.so (no GPU needed just to load and resolve symbols)."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        _load_error = f"{LIB_PATH} not found: build it with `python __graft_entry__.py build` (hipcc, gfx950)"
        raise AliHipUnavailable(_load_error)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        _load_error = f"cannot load {LIB_PATH}: {e}"
        raise AliHipUnavailable(_load_error)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and the header drifted apart
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().ali_last_error()
        raise RuntimeError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
