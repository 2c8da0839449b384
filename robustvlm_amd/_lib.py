"""ctypes binding of librvlm.so (the C ABI declared in include/rvlm.h).

The library is hand-written HIP for gfx950, built in-tree by ``robustvlm_amd/csrc/Makefile``
(``__graft_entry__.build()``).  There is NO fallback: if the shared object is missing or a call
fails, this module raises - the product path never routes through a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RVLM_LIB_PATH: development knob for A/B runs of two builds on one box (scripts/trip_ab.sh); never a fallback
LIB_PATH = os.path.abspath(os.environ["RVLM_LIB_PATH"]) if os.environ.get("RVLM_LIB_PATH") else os.path.join(_HERE, "librvlm.so")

RVLM_OK, RVLM_ERR_ARG, RVLM_ERR_HIP, RVLM_ERR_STATE, RVLM_ERR_UNSUPPORTED = 0, 1, 2, 3, 4
PREC_F32, PREC_BF16, PREC_F32X3 = 0, 1, 2
ACT_QUICK_GELU, ACT_GELU = 0, 1
LOSS_L2, LOSS_CE, LOSS_DLR, LOSS_DLR_TARGETED, LOSS_LOGIT_DIFF = 0, 1, 2, 3, 4
RED_MEAN, RED_NONE = 0, 1
FLAG_INPUT_RANGE, FLAG_NAN_GRAD, FLAG_NAN_DELTA, FLAG_ADV_RANGE = 1, 2, 4, 8
FLAG_TOKEN_RANGE, FLAG_EOT_ACTIVE = 16, 32
FLAG_FAB_NONFINITE = 64
FLAG_TOKENS_NONFINITE = 128
FLAG_SQUARE_NONFINITE = 256
TOKENS_ALL, TOKENS_PATCH = 0, 1

c_f32p = C.c_void_p   # device pointers travel as integers (tensor.data_ptr())
c_stream = C.c_void_p


class VitConfigC(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("patch", C.c_int32), ("width", C.c_int32),
                ("layers", C.c_int32), ("heads", C.c_int32), ("out_dim", C.c_int32),
                ("act", C.c_int32), ("precision", C.c_int32), ("max_batch", C.c_int32),
                ("mean", C.c_float * 3), ("std", C.c_float * 3), ("trainable", C.c_int32)]


BLOCK_FIELDS = ["ln_1_weight", "ln_1_bias", "attn_in_proj_weight", "attn_in_proj_bias",
                "attn_out_proj_weight", "attn_out_proj_bias", "ln_2_weight", "ln_2_bias",
                "mlp_c_fc_weight", "mlp_c_fc_bias", "mlp_c_proj_weight", "mlp_c_proj_bias"]
# C field -> open_clip state_dict suffix under transformer.resblocks.{i}.
BLOCK_KEYS = {"ln_1_weight": "ln_1.weight", "ln_1_bias": "ln_1.bias",
              "attn_in_proj_weight": "attn.in_proj_weight", "attn_in_proj_bias": "attn.in_proj_bias",
              "attn_out_proj_weight": "attn.out_proj.weight", "attn_out_proj_bias": "attn.out_proj.bias",
              "ln_2_weight": "ln_2.weight", "ln_2_bias": "ln_2.bias",
              "mlp_c_fc_weight": "mlp.c_fc.weight", "mlp_c_fc_bias": "mlp.c_fc.bias",
              "mlp_c_proj_weight": "mlp.c_proj.weight", "mlp_c_proj_bias": "mlp.c_proj.bias"}


class BlockWeightsC(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in BLOCK_FIELDS]


TOP_FIELDS = ["class_embedding", "positional_embedding", "proj", "conv1_weight", "ln_pre_weight",
              "ln_pre_bias", "ln_post_weight", "ln_post_bias"]
TOP_KEYS = {"class_embedding": "class_embedding", "positional_embedding": "positional_embedding",
            "proj": "proj", "conv1_weight": "conv1.weight", "ln_pre_weight": "ln_pre.weight",
            "ln_pre_bias": "ln_pre.bias", "ln_post_weight": "ln_post.weight",
            "ln_post_bias": "ln_post.bias"}


class VitWeightsC(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in TOP_FIELDS] + [("blocks_host", C.POINTER(BlockWeightsC))]


class TextConfigC(C.Structure):
    _fields_ = [("vocab", C.c_int32), ("context", C.c_int32), ("width", C.c_int32), ("layers", C.c_int32),
                ("heads", C.c_int32), ("out_dim", C.c_int32), ("act", C.c_int32), ("precision", C.c_int32),
                ("max_batch", C.c_int32)]


TEXT_TOP_FIELDS = ["token_embedding", "positional_embedding", "ln_final_weight", "ln_final_bias", "text_projection"]
TEXT_TOP_KEYS = {"token_embedding": "token_embedding.weight", "positional_embedding": "positional_embedding",
                 "ln_final_weight": "ln_final.weight", "ln_final_bias": "ln_final.bias",
                 "text_projection": "text_projection"}


class TextWeightsC(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in TEXT_TOP_FIELDS] + [("blocks_host", C.POINTER(BlockWeightsC))]


class LossSpecC(C.Structure):
    _fields_ = [("loss_kind", C.c_int32), ("reduction", C.c_int32), ("output_normalize", C.c_int32),
                ("n_classes", C.c_int32), ("logit_scale", C.c_float), ("ref", C.c_void_p),
                ("targets", C.c_void_p), ("y_target", C.c_void_p)]


class ProfileEntryC(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("total_ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double), ("launches", C.c_int64)]


class RvlmError(RuntimeError):
    pass


_lib = None

_SIGS = {
    # name: (restype, argtypes)
    "rvlm_version": (C.c_int, []),
    "rvlm_last_error": (C.c_char_p, []),
    "rvlm_vit_create": (C.c_int, [C.POINTER(VitConfigC), C.POINTER(VitWeightsC), c_stream,
                                  C.POINTER(C.c_void_p)]),
    "rvlm_vit_destroy": (C.c_int, [C.c_void_p]),
    "rvlm_vit_load_weights": (C.c_int, [C.c_void_p, C.POINTER(VitWeightsC), c_stream]),
    "rvlm_vit_workspace_bytes": (C.c_size_t, [C.c_void_p]),
    "rvlm_vit_forward": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, c_f32p,
                                   c_stream]),
    "rvlm_vit_backward_input": (C.c_int, [C.c_void_p, c_f32p, C.c_int, c_f32p, c_stream]),
    "rvlm_vit_backward_params": (C.c_int, [C.c_void_p, c_f32p, C.c_int, C.POINTER(VitWeightsC), C.c_int, c_stream]),
    "rvlm_vit_backward_params_stages": (C.c_int, [C.c_void_p, c_f32p, C.c_int, C.POINTER(VitWeightsC), C.c_int, C.c_int,
                                                  C.c_int, c_stream]),
    "rvlm_vit_fwd_inputgrad": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.POINTER(LossSpecC), c_f32p, c_f32p,
                                         c_f32p, c_f32p, c_stream]),
    "rvlm_ce_logits": (C.c_int, [c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, C.c_void_p,
                                 c_stream]),
    "rvlm_head_logits": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, c_f32p, c_stream]),
    "rvlm_head_logits_bwd": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, c_f32p, c_stream]),
    "rvlm_cosine_rows": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, c_f32p, c_f32p, c_stream]),
    "rvlm_l2_normalize_rows": (C.c_int, [c_f32p, C.c_int, C.c_int, c_f32p, c_f32p, c_stream]),
    "rvlm_adamw_step": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_size_t, C.c_double, C.c_double, C.c_double,
                                  C.c_double, C.c_double, C.c_int, C.c_float, c_stream]),
    "rvlm_loss_grad": (C.c_int, [C.c_int, C.c_int, c_f32p, c_f32p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                 C.c_int, C.c_float, c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p,
                                 c_stream]),
    "rvlm_argmax_eq": (C.c_int, [c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_stream]),
    "rvlm_check_image_range": (C.c_int, [c_f32p, C.c_size_t, C.c_void_p, c_stream]),
    "rvlm_pgd_linf_update": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_size_t, C.c_float,
                                       C.c_float, C.c_float, C.c_int, c_f32p, C.c_void_p, c_stream]),
    "rvlm_project_perturbation": (C.c_int, [c_f32p, C.c_size_t, C.c_int, C.c_int, C.c_float, c_f32p, c_stream]),
    "rvlm_normalize_grad": (C.c_int, [c_f32p, C.c_size_t, C.c_int, C.c_int, c_f32p, c_stream]),
    "rvlm_pgd_l2_update": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_size_t, C.c_int, C.c_float, C.c_float,
                                     C.c_float, C.c_int, c_f32p, C.c_void_p, c_stream]),
    "rvlm_pgd_run_norm": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.POINTER(LossSpecC), C.c_int, C.c_float,
                                    C.c_int, C.c_float, C.c_float, C.c_int, c_f32p, c_f32p, C.c_void_p, c_stream]),
    "rvlm_apgd_linf_step": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_float, C.c_float,
                                      C.c_size_t, C.c_int, c_stream]),
    "rvlm_apgd_l2_step": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_float, C.c_float, C.c_size_t, C.c_int,
                                    c_stream]),
    "rvlm_apgd_run_norm": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.POINTER(LossSpecC), C.c_int, C.c_float,
                                     C.c_int, C.c_float, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, C.c_void_p, c_stream]),
    "rvlm_apgd_controller": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p,
                                       C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, c_stream]),
    "rvlm_apgd_controller_rho": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, c_f32p,
                                           C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, c_stream]),
    "rvlm_vit_set_apgd_rho": (C.c_int, [C.c_void_p, C.c_double]),
    "rvlm_apgd_select": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_int, c_stream]),
    "rvlm_linf_random_start": (C.c_int, [c_f32p, c_f32p, C.c_float, C.c_size_t, C.c_int, c_f32p,
                                         c_stream]),
    "rvlm_l2_random_start": (C.c_int, [c_f32p, c_f32p, C.c_float, C.c_size_t, C.c_int, c_f32p, c_stream]),
    "rvlm_pgd_run": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.POINTER(LossSpecC), C.c_float,
                               C.c_int, C.c_float, C.c_float, C.c_int, c_f32p, c_f32p, C.c_void_p,
                               c_stream]),
    "rvlm_pgd_run_mixed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_f32p, c_f32p, C.c_int, C.POINTER(LossSpecC), C.c_int,
                                     C.c_float, C.c_int, C.c_float, C.c_float, C.c_int, c_f32p, c_f32p, C.c_void_p,
                                     c_stream]),
    "rvlm_pgd_run_mixed_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_f32p, c_f32p, C.c_int, C.POINTER(LossSpecC), C.c_int,
                                         C.c_float, C.c_int, C.c_float, C.c_float, C.c_int, c_f32p, c_f32p, C.c_void_p,
                                         c_stream]),
    "rvlm_vit_backward_input_from": (C.c_int, [C.c_void_p, C.c_void_p, c_f32p, C.c_int, c_f32p, c_stream]),
    "rvlm_vit_set_flash_inference": (C.c_int, [C.c_void_p, C.c_int]),
    "rvlm_vit_forward_for": (C.c_int, [C.c_void_p, C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, c_f32p, c_stream]),
    "rvlm_apgd_run": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.POINTER(LossSpecC), C.c_float,
                                C.c_int, C.c_float, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p,
                                C.c_void_p, c_stream]),
    "rvlm_preproc_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rvlm_preproc_destroy": (C.c_int, [C.c_void_p]),
    "rvlm_preproc_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, c_f32p, c_stream]),
    "rvlm_preproc_run_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                         c_f32p, c_stream]),
    "rvlm_vit_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "rvlm_vit_get_profile": (C.c_int, [C.c_void_p, C.POINTER(ProfileEntryC), C.POINTER(C.c_int)]),
    "rvlm_vit_reset_profile": (C.c_int, [C.c_void_p]),
    "rvlm_square_linf_propose": (C.c_int, [c_f32p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_float, c_f32p, c_f32p, c_stream]),
    "rvlm_square_accept": (C.c_int, [c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_int, C.c_size_t, c_stream]),
    # kernel-level test surface (include/rvlm_kernels.h)
    "rvlm_k_gemm_bf16_nt": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, c_f32p, C.c_void_p, C.c_long,
                                      C.c_void_p, C.c_void_p, c_f32p, C.c_int, c_stream]),
    "rvlm_k_gemm_f32": (C.c_int, [c_f32p, C.c_long, C.c_long, c_f32p, C.c_long, C.c_long, c_f32p,
                                  C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_float, c_f32p,
                                  c_stream]),
    "rvlm_k_gemm_f32_ex": (C.c_int, [c_f32p, C.c_long, C.c_long, C.c_long, c_f32p, C.c_long, C.c_long, C.c_long, c_f32p,
                                     C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, c_f32p,
                                     C.c_int, c_f32p, c_f32p, c_f32p, c_stream]),
    "rvlm_k_gemm_f32_set_valu": (C.c_int, [C.c_int]),
    "rvlm_k_softmax_rows": (C.c_int, [c_f32p, c_f32p, C.c_long, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "rvlm_k_attn_fwd_f32_flash": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rvlm_k_attn_bwd_f32_flash": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rvlm_k_attn_fwd_bf16": (C.c_int, [C.c_void_p, C.c_void_p, c_f32p, C.c_int, C.c_int, C.c_int,
                                       c_stream]),
    "rvlm_k_attn_bwd_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_f32p, c_f32p,
                                       C.c_void_p, C.c_int, C.c_int, C.c_int, c_stream]),
    "rvlm_k_attn_set_use_tr": (C.c_int, [C.c_int]),
    "rvlm_k_gemm_set_variant": (C.c_int, [C.c_int]),
    "rvlm_k_gemm_last_kernels": (C.c_int, []),
    "rvlm_k_gemm_set_trace": (C.c_int, [C.c_void_p]),
    "rvlm_k_probe_operand_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, c_stream]),
    "rvlm_k_attn_occupancy": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "rvlm_k_layernorm_fwd_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int,
                                           C.c_int, c_stream]),
    "rvlm_k_layernorm_bwd_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int,
                                           C.c_int, C.c_int, c_stream]),
    "rvlm_k_layernorm_bwd_bf16": (C.c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p]),
    "rvlm_k_probe_tr16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_stream]),
    "rvlm_k_wgrad_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "rvlm_k_wgrad_set_transposed": (None, [C.c_int]),
    "rvlm_k_wgrad_bf16": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, c_f32p,
                                    C.c_long, C.c_int, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
}

_SIGS.update({
    # data-parallel trainer without torch.distributed: RCCL behind the C ABI (include/rvlm.h, csrc/comm.hip)
    "rvlm_comm_unique_id": (C.c_int, [C.c_void_p]),
    "rvlm_comm_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rvlm_comm_destroy": (C.c_int, [C.c_void_p]),
    "rvlm_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rvlm_allreduce_grads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, c_stream]),
})
COMM_ID_BYTES, DTYPE_F32, DTYPE_BF16 = 128, 0, 1
_SIGS.update({
    # text tower (csrc/text_engine.hip): forward-only handle + the kernel-level hooks of its own kernels
    "rvlm_text_create": (C.c_int, [C.POINTER(TextConfigC), C.POINTER(TextWeightsC), c_stream, C.POINTER(C.c_void_p)]),
    "rvlm_text_destroy": (C.c_int, [C.c_void_p]),
    "rvlm_text_workspace_bytes": (C.c_size_t, [C.c_void_p]),
    "rvlm_text_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_f32p, C.c_void_p, c_stream]),
    "rvlm_k_attn_causal_fwd_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_stream]),
    "rvlm_k_attn_causal_fwd_f32": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_stream]),
    "rvlm_k_text_embed": (C.c_int, [C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, c_stream]),
})
_SIGS.update({
    # FAB / FAB-T, L-inf (csrc/fab_kernels.hip)
    "rvlm_fab_projection_linf": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int, C.c_size_t, c_f32p, c_f32p, C.c_void_p, c_stream]),
    "rvlm_fab_linf_step": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_size_t, C.c_float, C.c_float, c_f32p,
                                     C.c_void_p, c_stream]),
    "rvlm_fab_track_best": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_float, C.c_int, C.c_size_t, c_stream]),
    "rvlm_fab_jacobian_argmin": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, c_f32p, c_f32p,
                                           c_f32p, c_stream]),
})
_SIGS.update({
    # the encoder's non-GEMM kernels (include/rvlm_kernels.h, tests/test_gpu_kernel_rows.py)
    "rvlm_k_layernorm_form": (C.c_int, [C.c_int]),
    "rvlm_k_layernorm_fwd_bf16": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, c_stream]),
    "rvlm_k_x3_split_rows": (C.c_int, [c_f32p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int, c_stream]),
    "rvlm_k_x3_act": (C.c_int, [c_f32p, C.c_long, c_f32p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_void_p, C.c_long, c_stream]),
    "rvlm_k_x3_export_bf16": (C.c_int, [c_f32p, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, c_stream]),
    "rvlm_k_x3_layernorm_fwd": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, c_stream]),
    "rvlm_k_x3_prepare_weight": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, c_stream]),
    "rvlm_k_attn_cls_fwd_bf16": (C.c_int, [C.c_void_p, C.c_void_p, c_f32p, C.c_int, C.c_int, C.c_int, c_stream]),
    "rvlm_k_attn_cls_bwd_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_stream]),
    "rvlm_k_embed_lnpre_fwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int,
                                         C.c_int, c_stream]),
    "rvlm_k_embed_lnpre_bwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.c_int, c_stream]),
    "rvlm_k_im2col_normalize": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                          C.c_void_p, C.c_long, C.c_int, C.c_int, c_stream]),
    "rvlm_k_col2im_grad": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), c_f32p,
                                     c_stream]),
    "rvlm_k_l2_normalize_bwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, c_stream]),
})
_SIGS.update({
    # bicubic resize inside the model (csrc/resize_kernels.hip; RVLM_HAS_INPUT_RESIZE)
    "rvlm_vit_set_input_size": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rvlm_resize_bicubic": (C.c_int, [c_f32p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    "rvlm_resize_bicubic_adjoint": (C.c_int, [c_f32p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_stream]),
    "rvlm_resize_taps": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "rvlm_k_resize_im2col_normalize": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                                 C.POINTER(C.c_float), C.c_void_p, C.c_long, C.c_int, C.c_int, c_stream]),
    "rvlm_k_col2im_resize_grad": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(C.c_float), c_f32p, c_stream]),
})
_SIGS.update({
    # token-level outputs and their input gradient (csrc/token_kernels.hip, csrc/engine_forward.hip / engine_backward.hip / engine_attacks.hip; RVLM_HAS_TOKENS)
    "rvlm_vit_forward_tokens": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_stream]),
    "rvlm_vit_backward_input_tokens": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, c_f32p, c_stream]),
    "rvlm_tokens_l2_loss_grad": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_void_p, C.c_long,
                                           c_f32p, c_f32p, c_f32p, C.c_void_p, c_stream]),
    "rvlm_vit_tokens_fwd_inputgrad": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int,
                                                c_f32p, c_f32p, c_f32p, c_f32p, c_stream]),
    "rvlm_pgd_run_tokens": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, C.c_int,
                                      C.c_float, C.c_int, C.c_float, C.c_float, C.c_int, c_f32p, c_f32p, C.c_void_p, c_stream]),
    # ---- VLM-side attacks (RVLM_HAS_VLM_ATTACKS) ----
    "rvlm_mask_grad": (C.c_int, [c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, c_f32p, C.c_void_p, c_stream]),
    "rvlm_pgd_masked_update": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_float,
                                         C.c_float, C.c_float, C.c_int, C.c_int, c_f32p, C.c_void_p, c_stream]),
    "rvlm_apgd_masked_step": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, c_f32p, C.c_float, C.c_float, C.c_int, C.c_int,
                                        C.c_size_t, C.c_int, C.c_void_p, c_stream]),
    "rvlm_apgd_masked_bookkeeping": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                               c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_size_t, c_stream]),
    "rvlm_k_tokens_seed": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_stream]),
})
_SIGS.update({
    # the training step's kernels (csrc/train_kernels.hip; include/rvlm_kernels.h, tests/test_gpu_train_kernels.py)
    "rvlm_k_reduce_chunks": (C.c_int, [C.c_int]),
    "rvlm_k_colsum_form": (C.c_int, [C.c_int, C.c_int, C.c_long, C.c_size_t]),
    "rvlm_k_colsum": (C.c_int, [C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, c_f32p, C.c_int, c_f32p, C.c_size_t, c_stream]),
    "rvlm_k_ln_param_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_long, c_f32p, C.c_long, c_f32p, c_f32p, C.c_int, C.c_int, c_f32p,
                                       c_f32p, C.c_int, c_f32p, C.c_size_t, c_stream]),
    "rvlm_k_pos_cls_grad": (C.c_int, [c_f32p, C.c_long, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, C.c_int, c_stream]),
    "rvlm_k_gather_patch_rows": (C.c_int, [c_f32p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int, c_stream]),
    "rvlm_k_transpose_pad": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int, c_stream]),
})
_SIGS.update({
    # Square Attack, L2: one query in one launch (csrc/attack_kernels.hip; RVLM_HAS_SQUARE_L2)
    "rvlm_square_l2_propose": (C.c_int, [c_f32p, c_f32p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_float, c_f32p, c_f32p, c_f32p, C.c_void_p, c_stream]),
})
_SIGS.update({
    # torch.optim.SGD with momentum on flat fp32 buffers (csrc/train_kernels.hip; RVLM_HAS_SGD)
    "rvlm_sgd_step": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_size_t, C.c_double, C.c_double, C.c_double, C.c_int, C.c_float,
                                c_stream]),
})
_SIGS.update({
    # weight gradients through the token door (csrc/engine_backward.hip, csrc/token_kernels.hip; RVLM_HAS_TOKEN_TRAINING)
    "rvlm_vit_backward_params_tokens": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.POINTER(VitWeightsC), C.c_int, c_stream]),
    "rvlm_vit_backward_params_tokens_stages": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.POINTER(VitWeightsC), C.c_int,
                                                         C.c_int, C.c_int, c_stream]),
    "rvlm_tokens_cosine": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, c_stream]),
})
_SIGS.update({
    # apgd() on the per-image token loss as one device loop (csrc/engine_attacks.hip; RVLM_HAS_TOKEN_APGD)
    "rvlm_apgd_run_tokens": (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, C.c_float,
                                       C.c_int, C.c_float, C.c_float, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p, c_stream]),
})
EXPORTED_SYMBOLS = tuple(_SIGS)


def load():
    """Load librvlm.so (raises if it has not been built - no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RvlmError(
                f"{LIB_PATH} not found: build the HIP library first "
                f"(python -c 'import __graft_entry__ as g; g.build()' or make -C robustvlm_amd/csrc)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc: int, what: str = ""):
    """Map an rvlm_status to the Python exception the reference would raise."""
    if rc == RVLM_OK:
        return
    msg = load().rvlm_last_error().decode(errors="replace")
    full = f"{what}: {msg}" if what else msg
    if rc == RVLM_ERR_ARG:
        raise ValueError(full)
    if rc == RVLM_ERR_UNSUPPORTED:
        raise NotImplementedError(full)
    raise RvlmError(f"[rvlm status {rc}] {full}")


def ptr(t):
    """Device pointer of a tensor (or None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream
