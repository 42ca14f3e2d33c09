"""ctypes binding of `libirx.so` (the C ABI declared in include/irx.h).

The product path has no CPU or eager-PyTorch fallback: if the library is missing, or a call
fails, an `IrxError` is raised with the native error message.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("IRX_LIB", _PKG / "libirx.so"))

IRX_F32, IRX_BF16, IRX_F16 = 0, 1, 2
IRX_MODEL_UNET, IRX_MODEL_VAE, IRX_MODEL_CLIP = 0, 1, 2
IRX_MODEL_LPIPS = 3       # LPIPS(alex), the reference's src/metrics.py:97-111
IRX_MODEL_FID = 4         # InceptionV3 pooled features, the reference's src/metrics.py:70-80
IRX_MODEL_SRVGG = 5       # Real-ESRGAN's SRVGGNetCompact, the reference's src/inference.py:335-336, :579-591
IRX_MODEL_SAFETY = 6      # StableDiffusionSafetyChecker, run_safety_checker inside src/inference.py:486, :566, :664
IRX_MODEL_RRDB = 7        # Real-ESRGAN's RRDBNet (RealESRGAN_x4plus.pth), the reference's src/inference.py:335-346, :579-591
IRX_LAYOUT_VEC, IRX_LAYOUT_MAT, IRX_LAYOUT_CONV, IRX_LAYOUT_EMB = 0, 1, 2, 3
IRX_LAYOUT_MAT_GEGLU64, IRX_LAYOUT_VEC_GEGLU64 = 4, 5
IRX_LAYOUT_VEC_LN_U, IRX_LAYOUT_VEC_LN_V = 6, 7
IRX_LAYOUT_MAT_CHAIN, IRX_LAYOUT_VEC_CHAIN = 8, 9
IRX_LAYOUT_CONV_UP2 = 10
IRX_RCCL_ID_BYTES = 128   # include/irx.h (sizeof(ncclUniqueId))
IRX_RESAMPLE_LANCZOS, IRX_RESAMPLE_BICUBIC, IRX_RESAMPLE_MAX_KSIZE = 0, 1, 97


class IrxError(RuntimeError):
    pass


class ModelConfig(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int), ("out_channels", C.c_int), ("latent_channels", C.c_int),
        ("n_blocks", C.c_int), ("block_out_channels", C.c_int * 8), ("layers_per_block", C.c_int),
        ("heads", C.c_int), ("cross_attention_dim", C.c_int), ("norm_groups", C.c_int), ("norm_eps", C.c_float),
        ("flip_sin_to_cos", C.c_int), ("freq_shift", C.c_float),
        ("down_attn", C.c_int * 8), ("up_attn", C.c_int * 8),
        ("vocab_size", C.c_int), ("hidden_size", C.c_int), ("intermediate_size", C.c_int),
        ("num_layers", C.c_int), ("max_positions", C.c_int), ("layer_norm_eps", C.c_float),
        ("quick_gelu", C.c_int),
        ("image_size", C.c_int), ("patch_size", C.c_int), ("projection_dim", C.c_int),
        ("n_special", C.c_int), ("n_concepts", C.c_int),
    ]


class JpegInfo(C.Structure):
    """irx_jpeg_info (include/irx.h): what irx_jpeg_parse reads out of a file."""
    _fields_ = [("H", C.c_int), ("W", C.c_int), ("ncomp", C.c_int),
                ("qsel", C.c_int * 3), ("dcsel", C.c_int * 3), ("acsel", C.c_int * 3),
                ("qt", (C.c_uint16 * 64) * 2),
                ("dc_bits", (C.c_uint8 * 16) * 2), ("dc_vals", (C.c_uint8 * 16) * 2),
                ("ac_bits", (C.c_uint8 * 16) * 2), ("ac_vals", (C.c_uint8 * 256) * 2),
                ("dc_count", C.c_int * 2), ("ac_count", C.c_int * 2),
                ("scan_off", C.c_long), ("scan_len", C.c_long)]


class ParamInfo(C.Structure):
    _fields_ = [("name", C.c_char_p), ("layout", C.c_int), ("dtype", C.c_int), ("ndim", C.c_int),
                ("shape", C.c_int64 * 4), ("offset", C.c_size_t), ("bytes", C.c_size_t),
                ("row_scale", C.c_float), ("scale_rows", C.c_int64), ("aux", C.c_char_p)]


class StepParams(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("batch", C.c_int), ("h", C.c_int), ("w", C.c_int),
        ("eps", C.c_void_p), ("cfg", C.c_int), ("guidance", C.c_float),
        ("hist_store", C.c_void_p), ("hist", C.c_void_p * 4), ("hw", C.c_float * 5),
        ("e_div", C.c_float), ("e_mul", C.c_float),
        ("mode", C.c_int), ("c0", C.c_float), ("c1", C.c_float), ("c2", C.c_float), ("c3", C.c_float),
        ("x_src", C.c_void_p), ("cur_store", C.c_void_p), ("x_out", C.c_void_p),
        ("unet_in", C.c_void_p), ("cin_pad", C.c_int), ("inpaint", C.c_int), ("mask", C.c_void_p),
        ("masked", C.c_void_p),
    ]


class UnetOpts(C.Structure):
    _fields_ = [("cfg_share", C.c_int), ("time_proj", C.c_void_p)]


vp, i32, f32, sz, i64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_long
u64 = C.c_ulonglong
# name: (restype, argtypes); every status-returning function is checked
_SIGS = {
    "irx_last_error": (C.c_char_p, []),
    "irx_version": (i32, []),
    "irx_set_option": (i32, [C.c_char_p, i32]),
    "irx_get_option": (i32, [C.c_char_p, C.POINTER(i32)]),
    "irx_option_name": (C.c_char_p, [i32]),
    "irx_profile_begin": (i32, []),
    "irx_graph_begin": (i32, [vp]),
    "irx_graph_end": (i32, [vp, C.POINTER(vp)]),
    "irx_graph_launch": (i32, [vp, vp]),
    "irx_graph_destroy": (i32, [vp]),
    "irx_profile_end": (i32, [C.POINTER(i32)]),
    "irx_profile_get": (i32, [i32, C.POINTER(C.c_char_p), C.POINTER(C.c_long), C.POINTER(C.c_double),
                              C.POINTER(C.c_double)]),
    "irx_model_create": (i32, [i32, C.POINTER(ModelConfig), i32, C.POINTER(vp)]),
    "irx_model_destroy": (i32, [vp]),
    "irx_model_num_params": (i32, [vp, C.POINTER(i32)]),
    "irx_model_param_info": (i32, [vp, i32, C.POINTER(ParamInfo)]),
    "irx_model_blob_bytes": (i32, [vp, C.POINTER(sz)]),
    "irx_model_bind": (i32, [vp, vp, sz]),
    "irx_unet_workspace_bytes": (i32, [vp, i32, i32, i32, C.POINTER(sz)]),
    "irx_unet_context_bytes": (i32, [vp, i32, i32, C.POINTER(sz)]),
    "irx_unet_prepare_context": (i32, [vp, vp, vp, i32, i32, vp, vp, sz]),
    "irx_unet_forward": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, i32, vp, vp, sz]),
    "irx_unet_input_channels": (i32, [vp, C.POINTER(i32)]),
    "irx_unet_workspace_bytes_ex": (i32, [vp, i32, i32, i32, vp, C.POINTER(sz)]),
    "irx_unet_forward_ex": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, i32, vp, vp, vp, sz]),
    "irx_unet_time_table_bytes": (i32, [vp, i32, C.POINTER(sz), C.POINTER(sz)]),
    "irx_unet_time_table": (i32, [vp, vp, vp, i32, vp, vp, sz]),
    "irx_op_gemm_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32, i32]),
    "irx_op_gemm_res_rows": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp, i32]),
    "irx_vae_encode_workspace_bytes": (i32, [vp, i32, i32, i32, C.POINTER(sz)]),
    "irx_vae_encode": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, sz]),
    "irx_vae_decode_workspace_bytes": (i32, [vp, i32, i32, i32, C.POINTER(sz)]),
    "irx_vae_decode": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, sz]),
    "irx_clip_workspace_bytes": (i32, [vp, i32, i32, C.POINTER(sz)]),
    "irx_clip_encode": (i32, [vp, vp, vp, i32, i32, vp, vp, sz]),
    "irx_sched_step": (i32, [vp, C.POINTER(StepParams)]),
    "irx_pack_unet_input": (i32, [vp, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
    "irx_latent_sample": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, i32, f32, f32, f32, vp]),
    "irx_latents_to_vae": (i32, [vp, i32, vp, i32, i32, i32, f32, vp]),
    "irx_image_to_tensor": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, vp]),
    "irx_tensor_to_image": (i32, [vp, i32, vp, i32, i32, i32, i32, vp, vp]),
    "irx_degrade_noise": (i32, [vp, vp, i64, f32, vp, u64, vp]),
    "irx_degrade_blur_down": (i32, [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp]),
    "irx_degrade_gray": (i32, [vp, vp, i64, i32, i32, vp]),
    "irx_degrade_strokes": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
    "irx_degrade_motion_blur": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp]),
    "irx_degrade_jpeg_ws_bytes": (i64, [i32, i32, i32]),
    "irx_degrade_jpeg": (i32, [vp, vp, i32, i32, i32, vp, i32, vp, vp]),
    # PIL.Image.save on a .jpg name (scripts/generate_predictions.py:83-84)
    "irx_jpeg_encode_ws_bytes": (i64, [i32, i32, i32]),
    "irx_jpeg_encode_bound": (i64, [i32, i32]),
    "irx_jpeg_encode": (i32, [vp, vp, i32, i32, i32, vp, i32, vp, vp, i64, vp]),
    "irx_jpeg_header": (i32, [i32, i32, vp, vp, i32]),
    "irx_jpeg_parse": (i32, [vp, i64, vp]),
    "irx_jpeg_decode_ws_bytes": (i64, [vp, i32, i32]),
    "irx_jpeg_decode": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
    "irx_nlm_weights": (i32, [f32, i32, i32, i32, C.POINTER(i32), i32, C.POINTER(i32)]),
    "irx_nlmeans_u8": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32]),
    "irx_bilateral_tables": (i32, [i32, C.c_double, C.c_double, i32, vp, vp, vp, i32, C.POINTER(i32),
                                   C.POINTER(i32)]),
    "irx_bilateral_u8": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, vp]),
    "irx_lab_convert_u8": (i32, [vp, vp, vp, i64, i32]),
    "irx_auto_mask_u8": (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
    "irx_colorize_lab_u8": (i32, [vp, vp, i64, vp, vp, vp]),
    "irx_median_blur_u8": (i32, [vp, vp, vp, i32, i32, i32, i32, i32]),
    "irx_resample_coeffs": (i32, [i32, i32, i32, vp, vp, i32, C.POINTER(i32)]),
    "irx_resample_u8": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, i32, i32, vp]),
    "irx_metrics_ws_bytes": (i64, [i32, i32, i32, i32]),
    "irx_metrics_pair_u8": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "irx_resize_linear_u8": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, vp]),
    # LPIPS(alex): MetricsCalculator.calculate_lpips, src/metrics.py:97-111
    "irx_lpips_workspace_bytes": (i32, [vp, i32, i32, i32, C.POINTER(sz)]),
    "irx_lpips_u8": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, sz]),
    "irx_op_lpips_input": (i32, [vp, vp, vp, i32, i32, i32, vp, vp]),
    "irx_op_lpips_relu_pool": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    # FID features: MetricsCalculator.get_inception_features, src/metrics.py:150-165
    "irx_fid_workspace_bytes": (i32, [vp, i32, i32, i32, C.POINTER(sz)]),
    "irx_fid_features": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, sz]),
    "irx_op_fid_input": (i32, [vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp]),
    "irx_op_fid_bn_relu": (i32, [vp, vp, C.c_long, i32, vp, vp, vp, i32, i32]),
    "irx_op_fid_avgpool3": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "irx_op_fid_maxpool3s2": (i32, [vp, vp, i32, i32, i32, i32, vp, i32, i32]),
    "irx_op_fid_gap": (i32, [vp, vp, i32, i32, i32, vp]),
    # Real-ESRGAN (SRVGGNetCompact): RestorationPipeline._sr_realesrgan, src/inference.py:579-591
    "irx_srvgg_workspace_bytes": (i32, [vp, i32, i32, i32, C.POINTER(sz)]),
    "irx_srvgg_u8": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, sz]),
    "irx_op_srvgg_conv": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "irx_op_srvgg_tail": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "irx_op_srvgg_prelu": (i32, [vp, i32, vp, i64, i32, vp, vp]),
    # Real-ESRGAN (RRDBNet, RealESRGAN_x4plus.pth): src/inference.py:335-346, :579-591
    "irx_rrdb_workspace_bytes": (i32, [vp, i32, i32, i32, C.POINTER(sz)]),
    "irx_rrdb_u8": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, sz]),
    "irx_op_rrdb_conv": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, vp, i32, i32, vp, i32, vp, i32]),
    # SD safety checker: run_safety_checker inside the img2img calls, src/inference.py:486, :566, :664
    "irx_safety_workspace_bytes": (i32, [vp, i32, C.POINTER(sz)]),
    "irx_safety_check_u8": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, sz]),
    "irx_safety_embed_u8": (i32, [vp, vp, vp, i32, vp, vp, vp, sz]),
    "irx_safety_blank_u8": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "irx_op_safety_patches": (i32, [vp, i32, vp, i32, i32, i32, i32, vp, vp]),
    "irx_op_safety_tokens": (i32, [vp, i32, vp, vp, vp, i32, i32, i32, vp]),
    "irx_op_safety_head": (i32, [vp, vp, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp]),
    "irx_op_conv2d": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32,
                            i32, i32, i32, vp, i64, vp, vp, i32, i32]),
    "irx_op_gemm": (i32, [vp, i32, i32, i32, i32, vp, i64, vp, i64, vp, i64, vp, f32, i32, vp, i64, i32, i32, i64,
                          i64, i64, i64]),
    "irx_op_group_norm": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, i32, vp, vp]),
    "irx_rccl_available": (i32, []),
    "irx_rccl_unique_id": (i32, [C.c_char_p]),
    "irx_rccl_comm_init": (i32, [C.c_char_p, i32, i32, C.POINTER(vp)]),
    "irx_rccl_comm_init_timeout": (i32, [C.c_char_p, i32, i32, i32, C.POINTER(vp)]),
    "irx_rccl_comm_destroy": (i32, [vp]),
    "irx_rccl_broadcast": (i32, [vp, vp, sz, i32, vp]),
    "irx_weights_bcast": (i32, [vp, vp, i32, vp]),
    "irx_op_group_norm_ws_bytes": (sz, [i32, i32, i32]),
    "irx_op_gn_conv3_ws_bytes": (sz, [i32, i32, i32, i32]),
    "irx_op_gn_conv3": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp, vp, i32, vp, vp, i32, vp, i64,
                              vp, vp, vp, vp]),
    "irx_op_gn_conv_narrow": (i32, [vp, i32, vp, i32, i32, i32, i32, i32, f32, vp, vp, i32, vp, vp, i32, vp, i32, i32,
                                    vp]),
    "irx_op_gn_proj_ws_bytes": (sz, [i32, i32, i32, i32, i32]),
    "irx_op_gn_proj": (i32, [vp, i32, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, i32, vp, vp, C.POINTER(i32),
                             C.POINTER(i32)]),
    "irx_op_layer_norm": (i32, [vp, i32, vp, i32, i32, f32, vp, vp, vp]),
    "irx_op_attention": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, i64, i64, vp, i64, i64, vp, i64, i64, vp,
                               i64, i64, f32, i32]),
    "irx_op_attention_hm": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, f32]),
    "irx_op_attention_ex": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, i64, i64, i64, vp, i64, i64, i64, vp, i64, i64,
                                  i64, vp, i64, i64, i64, f32, i32, i32]),
    "irx_op_geglu": (i32, [vp, i32, vp, i32, i32, vp]),
    "irx_op_gemm_geglu": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "irx_op_gemm_ln_out": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, f32]),
    "irx_op_gemm_ln_fold": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp]),
    "irx_op_gemm_ln_out_w": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, i32, i32, f32]),
    "irx_op_gemm_ln_fold_w": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "irx_op_conv2d_gn_parts": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32,
                                     i32, i32, i32, i32, vp, i64, vp, vp, i32, i32, vp, vp, C.POINTER(i32),
                                     C.POINTER(i32), C.POINTER(i32), C.POINTER(sz)]),
    "irx_op_gemm_gn_parts": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, C.POINTER(i32),
                                   C.POINTER(i32), C.POINTER(sz)]),
    "irx_op_upsample_conv_gn_parts": (i32, [vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, C.POINTER(i32),
                                            C.POINTER(i32), C.POINTER(sz)]),
    "irx_op_group_norm_parts": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, i32, vp, vp, i32, vp, i32,
                                      vp]),
    "irx_op_group_norm_parts_ab": (i32, [vp, i32, i32, i32, i32, f32, vp, vp, vp, i32, vp, vp]),
    "irx_op_softmax_rows": (i32, [vp, i32, vp, i64, i32, i32, vp, i64]),
    "irx_op_transpose2d": (i32, [vp, i32, vp, i64, i32, i32, vp, i64, i32, i64, i64]),
    "irx_op_timestep_embed": (i32, [vp, i32, vp, i32, i32, i32, f32, vp]),
    "irx_op_embed_tokens": (i32, [vp, i32, vp, i32, i32, vp, vp, i32, vp]),
}

EXPORTED = tuple(_SIGS)

# plan queries for tests and scripts: exported by the library, not declared in include/irx.h (so not in EXPORTED)
_DEBUG_SIGS = {
    "irx_debug_gemm_tile": (i32, [i32, i32, i32, i32, i32, i32, C.POINTER(i32)]),
    "irx_debug_conv_plan": (i32, [i32] * 17 + [C.POINTER(i32)]),
}
_SIGS.update(_DEBUG_SIGS)

_lib = None


def load(path: Path | str | None = None, force: bool = False):
    """Load libirx.so once; raises IrxError (never falls back) if it is missing.  `force` re-resolves
    `path` even when a library is already loaded (the loaded one stays in use if that fails)."""
    global _lib
    if _lib is not None and not force:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise IrxError(f"native library not built: {p} (run `python -m image_restoration_and_enhancement_amd.build`)")
    lib = C.CDLL(str(p))
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def call(name: str, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if name == "irx_jpeg_header":                   # returns a length; negative: refused
        if rc < 0:
            raise IrxError(f"{name}: {lib.irx_last_error().decode(errors='replace')}")
        return rc
    if _SIGS[name][0] is i32 and name not in ("irx_version", "irx_rccl_available") and rc != 0:
        raise IrxError(f"{name}: {lib.irx_last_error().decode(errors='replace')}")
    return rc


def get_option(name: str) -> int:
    v = C.c_int()
    call("irx_get_option", name.encode(), C.byref(v))
    return v.value


def options() -> dict:
    """Every runtime option and its current value."""
    lib = load()
    out, i = {}, 0
    while True:
        n = lib.irx_option_name(i)
        if not n:
            return out
        out[n.decode()] = get_option(n.decode())
        i += 1


class option:
    """Context manager: set runtime options (irx_set_option) for a block, restoring the previous values after."""

    def __init__(self, **opts):
        self.opts = opts
        self.saved = {}

    def __enter__(self):
        for k, v in self.opts.items():
            self.saved[k] = get_option(k)
            call("irx_set_option", k.encode(), int(v))
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            call("irx_set_option", k.encode(), v)
        return False


def profile_begin() -> None:
    call("irx_profile_begin")


def profile_end() -> list:
    """[(kernel name, launches, total ms, total algorithmic flops)] since profile_begin()."""
    n = C.c_int()
    call("irx_profile_end", C.byref(n))
    out = []
    for i in range(n.value):
        name, cnt, ms, fl = C.c_char_p(), C.c_long(), C.c_double(), C.c_double()
        call("irx_profile_get", i, C.byref(name), C.byref(cnt), C.byref(ms), C.byref(fl))
        out.append((name.value.decode(), int(cnt.value), float(ms.value), float(fl.value)))
    return out


def ptr(t) -> int | None:
    """Raw device pointer of a torch tensor (None for None)."""
    return None if t is None else t.data_ptr()
