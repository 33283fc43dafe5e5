"""ctypes binding of libpclip.so (include/pclip.h).  There is no fallback: if the library is missing
or a call fails, a loud exception is raised — the product path never routes through a CPU or
PyTorch-eager substitute."""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpclip.so")

OP_SQDIST, OP_CLASSIFY, OP_ADAPTER_FC, OP_LOGITS, OP_COSINE_CE, OP_COSINE_CE_BACKWARD, OP_TIP_BACKWARD = 1, 2, 3, 4, 5, 6, 7
OP_COSINE_SIGMOID, OP_COSINE_SIGMOID_BACKWARD = 8, 9
OP_COSINE_KD, OP_COSINE_KD_BACKWARD = 10, 11          # sized with D = max(D, Dt)
KD_NORMALIZE_A, KD_NORMALIZE_B, KD_NORMALIZE_TA, KD_NORMALIZE_TB = 0x1, 0x2, 0x4, 0x8          # flags of pclip_cosine_kd_f16 / pclip_cosine_kd_backward_f16
FREG_L1, FREG_COS, FREG_CHUNK = 0, 1, 1024          # modes of pclip_feature_reg_f16 / pclip_feature_reg_backward_f16; rows per chunk of the loss's second stage
LOGITS_NORMALIZE_A, LOGITS_NORMALIZE_B = 0x1, 0x2          # flags of pclip_cosine_logits_f16
SIG_NORMALIZE_A, SIG_NORMALIZE_B, SIG_IDS_I64 = 0x1, 0x2, 0x8          # flags of pclip_cosine_sigmoid_f16 / pclip_cosine_sigmoid_backward_f16
CE_NORMALIZE_A, CE_NORMALIZE_B, CE_SYMMETRIC, CE_LABELS_I64 = 0x1, 0x2, 0x4, 0x8          # flags of pclip_cosine_ce_f16 / pclip_cosine_ce_backward_f16
# routing flags of pclip_classify_ex_f16 / pclip_classify_route_ex (include/pclip.h)
CLASSIFY_NO_SMALL, CLASSIFY_NO_MID, CLASSIFY_FORCE_MID, CLASSIFY_NO_PANELS, CLASSIFY_FORCE_PANELS = 0x1, 0x2, 0x4, 0x8, 0x10
CLASSIFY_PANEL_TWO_PASS, CLASSIFY_PANEL_FORCE_SECOND, CLASSIFY_PANEL_EXACT = 0x20, 0x40, 0x80
TIP_MAX_ALPHAS, TIP_MAX_CLASSES, TIP_MAX_D = 32, 4096, 2048                                # envelope of pclip_tip_logits_f16 / pclip_tip_grid_f16
# pclip_tower_grad_sumsq / pclip_tower_optim_finish / pclip_tower_adamw: chunk length, table row / state block sizes, row flags
TOWER_CHUNK, TOWER_ROW_BYTES, TOWER_STATE_BYTES = 4096, 64, 64
TOWER_PARAM_F16, TOWER_GRAD_F16, TOWER_ALIGNED, TOWER_DECAY = 0x1, 0x2, 0x4, 0x8
# pclip_gemm_route_f16: cfg values beside 0 .. 4, ints per launch of the report, and the report's kernel families (PCLIP_ROUTE_*)
ROUTE_AUTO, ROUTE_GENERIC, ROUTE_RING, ROUTE_FIELDS = -1, 5, 6, 5
ROUTE_RAN = {0: "cfg0", 1: "cfg1", 2: "cfg2", 3: "cfg3", 4: "cfg4", 10: "four_wave", 11: "ring", 12: "generic"}
EMBED_BWD_CHUNK = 128                                      # PCLIP_EMBED_BWD_CHUNK: sorted rows per chunk of pclip_text_embed_backward's segmented reduction
PROMPT_CTX_SLICE = 16                                      # PCLIP_PROMPT_CTX_SLICE: classes per slice of pclip_prompt_ctx_grad_f32's first stage
VPT_SLICE, VPT_MAX_L = 16, 288                             # PCLIP_VPT_SLICE: images per slice of pclip_vpt_grad_f32's first stage; PCLIP_VPT_MAX_L: L0 + P at most
COUPLE_MAX_P, COUPLE_SLICE = 16, 32                        # PCLIP_COUPLE_MAX_P: rows per depth of the coupling function; PCLIP_COUPLE_SLICE: rows of Wc per slice of dX
COCOOP_MAX_B = 16                                          # PCLIP_COCOOP_MAX_B: images per call of the meta-net and the conditional assembly


class PclipError(RuntimeError):
    pass


_lib = None

# name -> argtypes (restype is int unless listed in _RESTYPES); mirrors include/pclip.h one to one
_P = c_void_p
_SIGS = {
    "pclip_abi_version": [],
    "pclip_last_error": [],
    "pclip_device_cus": [],
    "pclip_gemm_kernel_launches": [],
    "pclip_l2norm_rows_f16": [_P, _P, c_int, c_int, _P, _P],
    "pclip_row_sqnorm_f16": [_P, c_int, c_int, _P, _P],
    "pclip_proto_build_f16": [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P],
    "pclip_bank_reduce_f16": [_P, c_int, c_int, c_int, _P, _P, _P],
    "pclip_transpose_f16": [_P, c_int, c_int, _P, _P],
    "pclip_partial_sums_f16": [_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P],
    "pclip_proto_finalize": [_P, _P, c_int, c_int, c_int, _P, _P, _P, _P],
    "pclip_sqdist_f16": [_P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_int, _P, c_size_t, _P],
    "pclip_sqdist_f32": [_P, _P, _P, c_int, c_int, c_int, _P, _P, c_int, _P],
    "pclip_fuse_probs": [_P, _P, c_int, c_int, c_int, c_float, c_float, c_float, _P, _P, _P, _P, c_int, _P],
    "pclip_classify_f16": [_P, _P, _P, c_int, c_int, c_int, _P, _P, _P, c_float, c_float, c_float, _P, _P, _P,
                           _P, c_int, _P, c_size_t, _P],
    "pclip_classify_ex_f16": [_P, _P, _P, c_int, c_int, c_int, _P, _P, _P, c_float, c_float, c_float, _P, _P, _P,
                              _P, c_int, c_int, _P, c_size_t, _P],
    "pclip_classify_panel_stats": [_P, c_int],
    "pclip_classify_panel_dump_f16": [_P, _P, _P, c_int, c_int, c_int, _P, c_int, _P, c_size_t, _P],
    "pclip_gemm_timing": [_P, c_int],
    "pclip_gemm_timing_count": [],
    "pclip_classify_route": [c_int, c_int, c_int, c_float, c_float, c_float, c_int, c_int, c_int, c_int, c_size_t],
    "pclip_classify_route_ex": [c_int, c_int, c_int, c_float, c_float, c_float, c_int, c_int, c_int, c_int, c_int, c_size_t],
    "pclip_cosine_logits_f16": [_P, c_int, c_int, _P, c_int, c_int, c_int, c_float, c_int, _P, c_int, _P, _P, _P, c_int, _P, c_size_t, _P],
    "pclip_cosine_ce_f16": [_P, c_int, c_int, _P, c_int, c_int, c_int, c_float, c_int, _P, _P, _P, _P, _P, _P, c_size_t, _P],
    "pclip_cosine_ce_backward_f16": [_P, c_int, c_int, _P, c_int, c_int, c_int, c_float, c_int, _P, _P, _P, c_float, c_int, _P, _P, _P, c_size_t, _P],
    "pclip_cosine_ce_grouped_f16": [_P, c_int, c_size_t, c_int, _P, c_int, c_size_t, c_int, c_int, c_int, c_float, c_int, _P, _P, _P, _P, _P, c_size_t, _P],
    "pclip_cosine_ce_grouped_backward_f16": [_P, c_int, c_size_t, c_int, _P, c_int, c_size_t, c_int, c_int, c_int, c_float, c_int, _P, _P, c_float, c_int, _P, _P,
                                             _P, c_size_t, _P],
    "pclip_cosine_ce_grouped_workspace": [c_int, c_int, c_int, c_int, c_int],
    "pclip_cosine_kd_f16": [_P, c_int, c_int, _P, c_int, c_int, c_int, c_float, _P, c_int, _P, c_int, c_int, c_float, c_int, _P, _P, _P, _P, _P, c_size_t, _P],
    "pclip_cosine_kd_backward_f16": [_P, c_int, c_int, _P, c_int, c_int, c_int, c_float, _P, c_int, _P, c_int, c_int, c_float, c_int, _P, _P, c_float, c_int, _P, _P,
                                     _P, c_size_t, _P],
    "pclip_feature_reg_f16": [_P, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t, _P],
    "pclip_feature_reg_backward_f16": [_P, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_float, _P, _P],
    "pclip_feature_reg_workspace": [c_int],
    "pclip_cosine_sigmoid_f16": [_P, c_int, c_int, _P, c_int, c_int, c_int, c_float, c_float, c_int, _P, _P, _P, _P, _P, c_size_t, _P],
    "pclip_cosine_sigmoid_backward_f16": [_P, c_int, c_int, _P, c_int, c_int, c_int, c_float, c_float, c_int, _P, _P, c_float, c_int, _P, _P, _P, _P, c_size_t, _P],
    "pclip_tip_logits_f16": [_P, c_int, c_int, _P, c_int, c_int, _P, _P, c_int, c_int, c_int, c_float, c_float, c_float, _P, c_int, _P, _P, _P],
    "pclip_tip_grid_f16": [_P, c_int, c_int, _P, c_int, c_int, _P, _P, c_int, c_int, c_int, c_float, _P, c_int, _P, c_int, _P, _P, _P],
    "pclip_tip_keys_backward_f16": [_P, c_int, c_int, _P, c_int, c_int, _P, c_int, c_int, c_float, c_float, _P, _P, _P, c_size_t, _P],
    "pclip_hp_sweep": [_P, _P, _P, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, _P, _P],
    "pclip_adapter_fc_f16": [_P, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, c_float, c_float, c_int, _P, _P, _P,
                             c_size_t, _P],
    "pclip_layernorm_blend_f16": [_P, _P, _P, c_float, _P, c_float, c_float, c_int, _P, _P, c_int, c_int, _P],
    "pclip_adapter_conv_f16": [_P, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P],
    "pclip_adapter_conv_w_f16": [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P],
    "pclip_gemm_f16": [_P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, _P, _P],
    "pclip_gemm4w_f16": [_P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, _P, _P],
    "pclip_gemm4w_var_f16": [_P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, _P],
    "pclip_gemm_route_f16": [_P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                             _P, c_int, _P],
    "pclip_gemm4w_stamp_buffer": [_P],
    "pclip_gemm4w_config": [c_int],
    "pclip_gemm_splitk_workspace": [c_int, c_int, c_int],
    "pclip_gemm_splitk_f16": [_P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, c_int, _P, c_size_t, _P],
    "pclip_gemm_bn_f16": [_P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, c_int, _P],
    "pclip_gemm_bn_res_f16": [_P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P],
    "pclip_conv3x3_bn_f16": [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, c_int, _P, _P],
    "pclip_conv3x3_strip_applies": [c_int, c_int, c_int, c_int, c_int],
    "pclip_conv3x3_strip_config": [c_int],
    "pclip_conv3x3_pool_applies": [c_int, c_int, c_int, c_int],
    "pclip_conv3x3_bn_pool_f16": [_P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P],
    "pclip_stem_conv_applies": [c_int, c_int],
    "pclip_stem_conv_bn_f16": [_P, c_int, c_int, c_int, _P, c_int, _P, _P, c_int, _P, _P],
    "pclip_layernorm_f16": [_P, c_int, _P, _P, c_float, _P, c_int, c_int, _P],
    "pclip_add_layernorm_f16": [_P, _P, c_int, _P, _P, _P, c_float, _P, c_int, c_int, _P],
    "pclip_attention_f16": [_P, _P, c_int, c_int, c_int, c_int, c_int, _P],
    "pclip_attention_q_f16": [_P, c_int, c_long, _P, c_int, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P],
    "pclip_attention_long_q_f16": [_P, c_int, c_long, _P, c_int, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P],
    "pclip_attention_config": [c_int, c_int],
    "pclip_im2col_patches_f16": [_P, c_int, c_int, c_int, _P, c_int, _P],
    "pclip_im2col_patches_f32": [_P, c_int, c_int, c_int, _P, c_int, _P],
    "pclip_vit_assemble_tokens_f16": [_P, _P, _P, c_int, c_int, c_int, _P, _P],
    "pclip_vit_embed_ln_f16": [_P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, c_float, _P, _P, _P],
    "pclip_text_embed_f16": [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P],
    "pclip_gather_eot_f16": [_P, _P, c_int, c_int, c_int, _P, _P],
    "pclip_im2col3x3_f16": [_P, c_long, c_long, c_long, c_long, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P],
    "pclip_bn_act_f16": [_P, _P, _P, _P, c_int, _P, c_size_t, c_int, _P],
    "pclip_avgpool_nhwc_f16": [_P, c_int, c_int, c_int, c_int, c_int, _P, _P],
    "pclip_attnpool_tokens_f16": [_P, _P, c_int, c_int, c_int, _P, _P],
    "pclip_cast_f32_f16": [_P, _P, c_size_t, _P],
    "pclip_cast_f16_f32": [_P, _P, c_size_t, _P],
    "pclip_gemm_f32": [_P, c_int, c_long, c_long, _P, c_int, c_long, c_long, _P, c_int, c_int, c_int, c_int, c_float, c_float, _P, c_size_t, _P],
    "pclip_colsum_f32": [_P, c_int, c_int, c_int, c_float, _P, c_int, _P, c_size_t, _P],
    "pclip_adapter_conv_backward_f16": [_P, _P, c_int, c_int, c_int] + [_P] * 8 + [_P] * 9 + [_P],
    "pclip_adapter_conv_backward_partials": [c_int, c_int, c_int],
    "pclip_adapter_conv_w_backward_f16": [_P, _P, c_int, c_int, c_int, c_int] + [_P] * 8 + [_P] * 9 + [_P],
    "pclip_adapter_conv_w_backward_partials": [c_int, c_int, c_int, c_int],
    "pclip_addscaled_rows_f32": [_P, c_int, _P, c_int, _P, c_float, c_int, c_int, _P],
    "pclip_nll_grad": [_P, _P, _P, c_int, c_int, c_int, c_int, c_float, c_float, c_float, _P, _P, _P, _P, _P, _P, _P],
    "pclip_nll_rows": [_P, c_int, _P, c_int, c_int, _P, _P, _P, _P],
    "pclip_fuse_probs_backward": [_P, _P, _P, c_int, c_int, c_int, c_int, c_float, c_float, c_float, _P, _P, _P, _P],
    "pclip_nll_mean_backward": [_P, c_int, _P, c_int, c_int, _P, _P, c_int, _P],
    "pclip_softmax_ce_rows": [_P, c_int, c_int, c_int, c_float, _P, c_int, _P, _P],
    "pclip_l2norm_rows_f32": [_P, _P, c_int, c_int, c_float, _P],
    "pclip_l2norm_rows_backward_f32": [_P, _P, _P, c_int, c_int, c_float, c_int, _P],
    "pclip_proto_backward_f16": [_P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P],
    "pclip_layernorm_backward_f16": [_P, c_int, _P, _P, c_int, c_int, c_int, c_float, c_float, _P, c_int, _P, c_int, _P],
    "pclip_attention_backward_f16": [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P],
    "pclip_quick_gelu_backward_f16": [_P, _P, _P, c_size_t, _P],
    "pclip_colsum_f16": [_P, c_int, c_int, c_int, _P, c_int, _P],
    "pclip_layernorm_backward_g32_f16": [_P, c_int, _P, _P, c_int, _P, c_int, c_int, c_int, c_float, _P, c_int, _P, c_int, _P],
    "pclip_prompt_embed_f16": [_P, c_int, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P],
    "pclip_prompt_ctx_grad_f32": [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, c_int, _P],
    "pclip_vpt_append_f16": [_P, _P, c_int, c_int, c_int, c_int, _P, _P],
    "pclip_vpt_replace_f16": [_P, _P, c_int, c_int, c_int, c_int, _P],
    "pclip_vpt_grad_f32": [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, c_int, _P],
    "pclip_rows_replace_f16": [_P, _P, c_int, c_int, c_int, c_int, c_int, _P],
    "pclip_rows_grad_f32": [_P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, c_int, _P],
    "pclip_couple_fwd_f32": [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P],
    "pclip_couple_bwd_f32": [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_int, _P],
    "pclip_metanet_fwd_f32": [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P],
    "pclip_metanet_bwd_f32": [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P],
    "pclip_prompt_embed_cond_f16": [_P, c_int, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P],
    "pclip_prompt_cond_grad_f32": [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_int, _P],
    "pclip_text_embed_backward": [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P],
    "pclip_vit_embed_backward_f16": [_P, c_int, c_int, c_int, _P, _P, _P],
    "pclip_adamw_f16": [_P, _P, _P, _P, c_size_t, c_double, c_double, c_double, c_double, c_double, c_int, _P],
    "pclip_tower_grad_sumsq": [_P, c_int, c_int, _P, _P],
    "pclip_tower_optim_finish": [_P, c_int, _P, c_float, c_double, c_double, c_float, c_float, c_int, c_int, _P],
    "pclip_tower_adamw": [_P, _P, c_int, c_int, _P, c_double, c_double, c_double, _P],
    "pclip_preprocess_u8": [_P, _P, c_int, c_int, c_int, c_float, c_float, c_float, c_float, c_float, c_float, _P, c_int, _P, _P],
    "pclip_workspace_bytes": [c_int, c_int, c_int, c_int],
}
_RESTYPES = {"pclip_last_error": c_char_p, "pclip_workspace_bytes": c_size_t, "pclip_gemm_splitk_workspace": c_size_t, "pclip_cosine_ce_grouped_workspace": c_size_t, "pclip_feature_reg_workspace": c_size_t, "pclip_gemm_kernel_launches": c_long}
EXPORTED_SYMBOLS = tuple(_SIGS)


def load():
    """Load libpclip.so once; raise PclipError loudly if it is not built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PclipError(
            f"{LIB_PATH} is missing: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C proto-clip_amd/csrc`). There is no CPU/eager fallback for this path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in _SIGS.items():
        fn = getattr(lib, name)     # AttributeError if a declared symbol is not exported
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, c_int)
    if lib.pclip_abi_version() != 1:
        raise PclipError(f"libpclip ABI version {lib.pclip_abi_version()} != 1")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().pclip_last_error()
        raise PclipError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else c_void_p(t.data_ptr())


def stream():
    """The current stream of the CURRENT device; `require_cuda` has checked that the operands live there."""
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda(*tensors):
    """Operands must be device tensors, all on one GPU, and that GPU must be the current device: the kernels are launched on the
    current device's stream (one process per GPU is the deployment model; a bank on another GPU would otherwise be a silent peer
    access or a fault).  `with torch.cuda.device(x.device):` around the call is the way to drive a second GPU from one process."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise PclipError("libpclip operates on device tensors only (got a CPU tensor); there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise PclipError(f"operands on different GPUs ({dev} and {t.device}): move them to one device")
    if dev is not None and dev.index != torch.cuda.current_device():
        raise PclipError(f"operands live on {dev} but the current device is cuda:{torch.cuda.current_device()}: call "
                         f"torch.cuda.set_device({dev.index}) or wrap the call in `with torch.cuda.device({dev.index}):`")


def workspace_bytes(op: int, Q: int, N: int, D: int) -> int:
    return int(load().pclip_workspace_bytes(op, Q, N, D))
