"""ctypes binding of libdgvit_hip.so (C ABI: include/dgvit_hip.h).

There is no CPU or PyTorch fallback: if the shared library is missing or a call fails, a
``DgvitError`` is raised.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_longlong, c_ulonglong, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdgvit_hip.so")
DIAG_LIB_PATH = os.path.join(_HERE, "libdgvit_hip_diag.so")   # same sources built with -DDGVIT_DIAG: knobs and experiments (tools/, A/B tests)


class DgvitError(RuntimeError):
    pass


class dgvit_config(Structure):
    _fields_ = [("image_h", c_int), ("image_w", c_int), ("patch_h", c_int), ("patch_w", c_int), ("dim", c_int),
                ("depth", c_int), ("heads", c_int), ("dim_head", c_int), ("mlp_dim", c_int), ("pool_mean", c_int), ("flags", c_int)]


FLAG_DENSE_LAST_BLOCK = 1    # include/dgvit_hip.h: DGVIT_FLAG_*
FLAG_WGRAD_OVERLAP = 2
FLAG_LONG_SEQUENCE = 4      # K / V-tiled attention for N > 288 tokens (fp32 and bf16 encoders)
MAPS_GOAL = 0               # include/dgvit_hip.h: DGVIT_MAPS_* (the rows of an attention-maps call)
MAPS_ALL = 1


class dgvit_mlp_desc(Structure):
    _fields_ = [("batch", c_int), ("nseg", c_int), ("kx", c_int * 3), ("ldx", c_int * 3), ("n1", c_int), ("n2", c_int), ("n3", c_int),
                ("towers", c_int), ("heads3", c_int)]


class dgvit_grad_events(Structure):
    """include/dgvit_hip.h: events recorded by dgvit_got_backward[_bf16]_ev where a group of gradients is final"""
    _fields_ = [("n_layers", c_int), ("layer", POINTER(c_void_p)), ("head", c_void_p)]


SMALL_FIELDS = 5            # include/dgvit_hip.h: DGVIT_SMALL_FIELDS


class dgvit_small_fields(Structure):
    """include/dgvit_hip.h: the five small fields of dgvit_ring_store_small, passed by value"""
    _fields_ = [("src", c_void_p * SMALL_FIELDS), ("ring", c_void_p * SMALL_FIELDS), ("src_ld", c_longlong * SMALL_FIELDS),
                ("cols", c_int * SMALL_FIELDS), ("ring_ld", c_int * SMALL_FIELDS)]


class dgvit_ring_view(Structure):
    """include/dgvit_hip.h: the ring as dgvit_ring_export reads it, passed by value"""
    _fields_ = [("obs", c_void_p), ("next_obs", c_void_p), ("next_row", c_void_p), ("small", c_void_p * SMALL_FIELDS), ("flags", c_void_p),
                ("leaves", c_void_p), ("frame_ld", c_longlong), ("next_rows", c_longlong), ("small_cols", c_int * SMALL_FIELDS),
                ("small_ld", c_int * SMALL_FIELDS), ("frame_u8", c_int)]


GRAD_NORM_PARTIALS = 512  # include/dgvit_hip.h: DGVIT_GRAD_NORM_PARTIALS (doubles of scratch for dgvit_grad_sqnorm_partials)
NUM_GLOBAL_PARAMS = 4
PARAMS_PER_LAYER = 11
ABI_VERSION = 7

_P, _I, _LL, _F, _ULL, _D = c_void_p, c_int, c_longlong, c_float, c_ulonglong, ctypes.c_double
_CFG = POINTER(dgvit_config)
_TABLE = POINTER(c_void_p)

# name -> (restype, argtypes); every symbol include/dgvit_hip.h declares
SIGNATURES = {
    "dgvit_abi_version": (_I, []),
    "dgvit_config_size": (_I, []),
    "dgvit_last_error": (c_char_p, []),
    "dgvit_device_count": (_I, []),
    "dgvit_got_workspace_floats": (_LL, [_CFG, _I, _I]),
    "dgvit_got_backward_scratch_floats": (_LL, [_CFG, _I]),
    "dgvit_got_forward": (_I, [_CFG, _TABLE, _P, _P, _P, _P, _LL, _I, _I, _F, _ULL, _P, _P]),
    "dgvit_got_backward": (_I, [_CFG, _TABLE, _TABLE, _P, _P, _P, _LL, _P, _LL, _I, _F, _ULL, _P, _P]),
    "dgvit_got_backward_ev": (_I, [_CFG, _TABLE, _TABLE, _P, _P, _P, _LL, _P, _LL, _I, _F, _ULL, _P, _P, POINTER(dgvit_grad_events)]),
    "dgvit_got_forward_v2": (_I, [_CFG, _TABLE, _P, _P, _P, _P, _LL, _I, _I, _F, _F, _ULL, _P, _P]),
    "dgvit_got_backward_v2": (_I, [_CFG, _TABLE, _TABLE, _P, _P, _P, _LL, _P, _LL, _I, _F, _F, _ULL, _P, _P]),
    "dgvit_got_backward_v2_ev": (_I, [_CFG, _TABLE, _TABLE, _P, _P, _P, _LL, _P, _LL, _I, _F, _F, _ULL, _P, _P, POINTER(dgvit_grad_events)]),
    "dgvit_got_backward_v3": (_I, [_CFG, _TABLE, _TABLE, _P, _P, _P, _P, _LL, _P, _LL, _I, _F, _F, _ULL, _P, _P]),
    "dgvit_got_backward_v3_ev": (_I, [_CFG, _TABLE, _TABLE, _P, _P, _P, _P, _LL, _P, _LL, _I, _F, _F, _ULL, _P, _P, POINTER(dgvit_grad_events)]),
    "dgvit_event_create": (_I, [POINTER(c_void_p)]),
    "dgvit_event_destroy": (_I, [_P]),
    "dgvit_stream_wait_event": (_I, [_P, _P]),
    "dgvit_linear_forward": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "dgvit_linear_backward_scratch_floats": (_LL, [_I, _I, _I]),
    "dgvit_linear_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _LL, _I, _I, _I, _I, _P]),
    "dgvit_mlp_head_forward": (_I, [POINTER(dgvit_mlp_desc), _TABLE, _TABLE, _P, _P, _P, _P]),
    "dgvit_mlp_head_backward_scratch_floats": (_LL, [POINTER(dgvit_mlp_desc)]),
    "dgvit_mlp_head_backward": (_I, [POINTER(dgvit_mlp_desc), _TABLE, _TABLE, _P, _P, _TABLE, _TABLE, _TABLE, _P, _LL, _P]),
    # the same head with shared input pieces (include/dgvit_hip.h: Shared input pieces); share is const int[nseg]
    "dgvit_mlp_head_forward_shared": (_I, [POINTER(dgvit_mlp_desc), POINTER(c_int), _TABLE, _TABLE, _P, _P, _P, _P]),
    "dgvit_mlp_head_backward_shared_scratch_floats": (_LL, [POINTER(dgvit_mlp_desc), POINTER(c_int)]),
    "dgvit_mlp_head_backward_shared": (_I, [POINTER(dgvit_mlp_desc), POINTER(c_int), _TABLE, _TABLE, _P, _P, _TABLE, _TABLE, _TABLE, _P, _LL, _P]),
    "dgvit_tanh_gaussian_forward": (_I, [_P, _P, _P, _P, _P, _I, _F, _F, _P, _P, _P, _I, _I, _P]),
    "dgvit_tanh_gaussian_backward": (_I, [_P, _P, _P, _P, _I, _F, _F, _P, _P, _P, _P, _P, _I, _I, _P]),
    "dgvit_tanh_gaussian_log_prob": (_I, [_P, _P, _P, _P, _P, _I, _F, _F, _P, _I, _I, _P]),
    "dgvit_tanh_gaussian_log_prob_backward": (_I, [_P, _P, _P, _P, _P, _I, _F, _F, _P, _P, _P, _I, _I, _P]),
    "dgvit_gemm_scratch_floats": (_LL, [_I, _I, _I, _I]),
    "dgvit_gemm": (_I, [_I, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _I, _P, _I, _P, _I, _P, _LL, _P]),
    "dgvit_layernorm_forward": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "dgvit_layernorm_backward_scratch_floats": (_LL, [_I, _I]),
    "dgvit_layernorm_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _LL, _I, _I, _P]),
    "dgvit_rmsnorm_forward": (_I, [_P, _LL, _P, _P, _I, _I, _P]),
    "dgvit_rmsnorm_backward_scratch_floats": (_LL, [_I, _I]),
    "dgvit_rmsnorm_backward": (_I, [_P, _P, _LL, _P, _P, _LL, _P, _P, _LL, _I, _I, _P]),
    "dgvit_attention_forward": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "dgvit_attention_backward": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "dgvit_attention_forward_tiled": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dgvit_attention_backward_tiled_scratch_floats": (_LL, [_I, _I, _I]),
    "dgvit_attention_backward_tiled": (_I, [_P, _P, _P, _P, _P, _P, _LL, _I, _I, _I, _I, _I, _P]),
    "dgvit_goal_attention_scratch_floats": (_LL, [_I, _I, _I]),
    "dgvit_got_last_block_folds": (_I, [_CFG, _I, _F, _I]),
    "dgvit_goal_attention_forward": (_I, [_P, _P, _P, _LL, _P, _LL, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dgvit_goal_attention_backward": (_I, [_P, _P, _P, _LL, _P, _LL, _P, _P, _P, _P, _LL, _P, _P, _P, _LL, _I, _I, _I, _I, _I, _P]),
    "dgvit_patchify": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "dgvit_dropout": (_I, [_P, _LL, _ULL, _F, _P]),
    "dgvit_cnn_workspace_floats": (_LL, [_I, _I, _I]),
    "dgvit_cnn_forward_scratch_floats": (_LL, [_I, _I, _I]),
    "dgvit_cnn_backward_scratch_floats": (_LL, [_I, _I, _I]),
    "dgvit_cnn_forward": (_I, [_P, _TABLE, _P, _P, _LL, _P, _LL, _I, _I, _I, _P]),
    "dgvit_cnn_backward": (_I, [_P, _TABLE, _TABLE, _P, _P, _LL, _P, _LL, _I, _I, _I, _P]),
    "dgvit_cnn_backward_v2": (_I, [_P, _TABLE, _TABLE, _P, _P, _P, _LL, _P, _LL, _I, _I, _I, _P]),
    "dgvit_cnn_workspace_floats_v2": (_LL, [_I, _I, _I, _I]),
    "dgvit_cnn_forward_scratch_floats_v2": (_LL, [_I, _I, _I, _I]),
    "dgvit_cnn_backward_scratch_floats_v2": (_LL, [_I, _I, _I, _I]),
    "dgvit_cnn_forward_v2": (_I, [_P, _TABLE, _P, _P, _LL, _P, _LL, _I, _I, _I, _I, _P]),
    "dgvit_cnn_backward_v3": (_I, [_P, _TABLE, _TABLE, _P, _P, _P, _LL, _P, _LL, _I, _I, _I, _I, _P]),
    "dgvit_gather_rows": (_I, [_P, _P, _P, _LL, _LL, _LL, _P]),
    "dgvit_gather_shift_frames": (_I, [_P, _P, _P, _P, _LL, _I, _I, _LL, _LL, _I, _I, _ULL, _P, _P]),
    "dgvit_quantize_rows_u8": (_I, [_P, _LL, _P, _LL, _LL, _LL, _LL, _LL, _P]),
    "dgvit_gather_rows_u8": (_I, [_P, _P, _P, _LL, _LL, _LL, _LL, _LL, _P]),
    "dgvit_gather_shift_frames_u8": (_I, [_P, _P, _P, _P, _LL, _I, _I, _LL, _LL, _LL, _I, _I, _ULL, _P, _P]),
    "dgvit_ring_mark": (_I, [_P, _LL, _LL, _LL, _P]),
    "dgvit_nstep_walk": (_I, [_P, _LL, _P, _LL, _P, _P, _LL, _P, _LL, _LL, _I, _D, _P, _P, _P, _P, _P, _P, _P]),
    # the ring of E parallel environments (include/dgvit_hip.h: The ring of E parallel environments)
    "dgvit_ring_store_frames": (_I, [_P, _I, _LL, _P, _I, _LL, _P, _P, _I, _LL, _LL, _LL, _LL, _LL, _P]),
    "dgvit_ring_store_small": (_I, [dgvit_small_fields, _P, _P, _I, _LL, _LL, _LL, _P]),
    "dgvit_nstep_walk_strided": (_I, [_P, _LL, _P, _LL, _P, _P, _LL, _P, _LL, _LL, _LL, _I, _D, _P, _P, _P, _P, _P, _P, _P]),
    # the ring that stores each frame once (include/dgvit_hip.h: The ring that stores each frame once)
    "dgvit_ring_plan_next": (_I, [_P, _P, _P, _P, _LL, _P, _LL, _LL, _LL, _LL, _LL, _P]),
    "dgvit_ring_store_frames_shared": (_I, [_P, _I, _LL, _P, _I, _LL, _P, _P, _I, _LL, _LL, _LL, _LL, _LL, _LL, _LL, _P]),
    "dgvit_ring_next_rows": (_I, [_P, _P, _P, _LL, _LL, _P]),
    # frame stacks at sample time and on the acting side (include/dgvit_hip.h: Frame stacks)
    "dgvit_ring_stack_rows": (_I, [_P, _P, _P, _P, _LL, _P, _P, _P, _LL, _LL, _LL, _I, _I, _LL, _P]),
    "dgvit_gather_stack_frames": (_I, [_P, _P, _P, _P, _LL, _LL, _I, _I, _LL, _LL, _LL, _LL, _P]),
    "dgvit_gather_shift_stack_frames": (_I, [_P, _P, _P, _P, _P, _LL, _I, _I, _I, _I, _LL, _LL, _LL, _LL, _I, _I, _ULL, _P, _P]),
    "dgvit_frame_stack_push": (_I, [_P, _P, _LL, _P, _I, _LL, _LL, _I, _P]),
    # the ring as a file (include/dgvit_hip.h: The ring as a file)
    "dgvit_ring_export": (_I, [dgvit_ring_view, _P, _LL, _LL, _LL, _LL, _LL, _LL, _P]),
    "dgvit_per_set_leaves": (_I, [_P, _LL, _LL, _LL, _P, _P]),
    "dgvit_per_tree_floats": (_LL, [_LL]),
    "dgvit_per_init": (_I, [_P, _LL, _P]),
    "dgvit_per_set_range": (_I, [_P, _LL, _LL, _LL, _P]),
    "dgvit_per_update": (_I, [_P, _LL, _LL, _P, _P, _LL, _F, _F, _P]),
    "dgvit_per_sample": (_I, [_P, _LL, _P, _LL, _I, _F, _P, _P, _P]),
    "dgvit_depth_preprocess_scratch_floats": (_LL, [_I, _I, _I]),
    "dgvit_depth_to_state": (_I, [_P, _P, _F, _ULL, _P, _P, _LL, _I, _I, _I, _I, _I, _P]),
    "dgvit_depth_normalize_u8": (_I, [_P, _P, _P, _LL, _I, _I, _I, _P]),
    "dgvit_noise_clip": (_I, [_P, _P, _P, _LL, _F, _ULL, _P]),
    "dgvit_gaussian_blur": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dgvit_resize_bilinear": (_I, [_P, _P, _I, _I, _I, _I, _I, _F, _P]),
    "dgvit_adam_step": (_I, [_P, _P, _P, _P, _LL, _F, _F, _F, _F, _F, _LL, _P, _P]),
    "dgvit_soft_update": (_I, [_P, _P, _LL, _F, _P]),
    "dgvit_grad_sqnorm_partials": (_I, [_P, _LL, _P, _I, _P]),
    "dgvit_grad_clip_coef": (_I, [_P, _F, _P, _P]),
    "dgvit_adam_step_scaled": (_I, [_P, _P, _P, _P, _LL, _F, _F, _F, _F, _F, _LL, _P, _P, _P]),
    "dgvit_adam_step_groups": (_I, [_P, _P, _P, _P, _LL, _P, _P, _I, _P, _I, _P, _F, _F, _F, _I, _LL, _LL, _P, _I, _LL, _LL, _F, _P, _P]),
    "dgvit_scale_by_device_scalar": (_I, [_P, _LL, _P, _P]),
    # the SAC loss head (include/dgvit_hip.h: The SAC loss head)
    "dgvit_sac_critic_loss": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _I, _I, _P]),
    "dgvit_sac_critic_loss_v2": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _I, _I, _P]),
    "dgvit_sac_actor_loss": (_I, [_P, _P, _P, _P, _F, _I, _F, _P, _P, _P, _I, _I, _P]),
    "dgvit_sac_scale_grads": (_I, [_P, _P, _LL, _P, _P]),
    "dgvit_sac_bc_loss": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P]),
    "dgvit_sac_cql_penalty": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _F, _F, _F, _I, _P, _P, _P, _I, _I, _I, _P]),
    "dgvit_got_bf16_weight_elems": (_LL, [_CFG]),
    "dgvit_got_pack_weights_bf16": (_I, [_CFG, _TABLE, _P, _LL, _I, _P]),
    "dgvit_got_bf16_workspace_bytes": (_LL, [_CFG, _I, _I]),
    "dgvit_got_forward_bf16": (_I, [_CFG, _TABLE, _P, _P, _P, _P, _P, _LL, _I, _I, _F, _ULL, _P, _P]),
    "dgvit_got_bf16_backward_scratch_bytes": (_LL, [_CFG, _I]),
    "dgvit_got_backward_bf16": (_I, [_CFG, _TABLE, _P, _TABLE, _P, _P, _P, _P, _LL, _P, _LL, _I, _F, _ULL, _P, _P]),
    "dgvit_got_backward_bf16_ev": (_I, [_CFG, _TABLE, _P, _TABLE, _P, _P, _P, _P, _LL, _P, _LL, _I, _F, _ULL, _P, _P, POINTER(dgvit_grad_events)]),
    "dgvit_got_backward_bf16_v2": (_I, [_CFG, _TABLE, _P, _TABLE, _P, _P, _P, _P, _P, _LL, _P, _LL, _I, _F, _ULL, _P, _P]),
    "dgvit_got_backward_bf16_v2_ev": (_I, [_CFG, _TABLE, _P, _TABLE, _P, _P, _P, _P, _P, _LL, _P, _LL, _I, _F, _ULL, _P, _P,
                                           POINTER(dgvit_grad_events)]),
    "dgvit_wgrad_bf16_scratch_floats": (_LL, [_I, _I, _I]),
    "dgvit_wgrad_bf16": (_I, [_P, _P, _P, _P, _P, _LL, _I, _I, _I, _P]),
    "dgvit_cast_f32_bf16": (_I, [_P, _P, _LL, _P]),
    "dgvit_gemm_bf16": (_I, [_I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _I, _P, _I, _P, _I, _P]),
    "dgvit_layernorm_forward_bf16": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "dgvit_attention_forward_bf16": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    # attention maps (include/dgvit_hip.h: Attention maps)
    "dgvit_got_forward_maps": (_I, [_CFG, _TABLE, _P, _P, _P, _P, _I, _P, _LL, _I, _F, _F, _ULL, _P, _P]),
    "dgvit_got_forward_maps_bf16": (_I, [_CFG, _TABLE, _P, _P, _P, _P, _P, _I, _P, _LL, _I, _F, _ULL, _P, _P]),
    "dgvit_attention_probs": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dgvit_attention_probs_bf16": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dgvit_attention_backward_bf16": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "dgvit_attention_forward_bf16_tiled": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dgvit_attention_backward_bf16_tiled": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    # transformer-internal dropout in the bf16 configuration (layer_keep after dropout_keep; the ops take keep, seed, seed_dev, layer)
    "dgvit_got_forward_bf16_v2": (_I, [_CFG, _TABLE, _P, _P, _P, _P, _P, _LL, _I, _I, _F, _F, _ULL, _P, _P]),
    "dgvit_got_forward_maps_bf16_v2": (_I, [_CFG, _TABLE, _P, _P, _P, _P, _P, _I, _P, _LL, _I, _F, _F, _ULL, _P, _P]),
    "dgvit_got_backward_bf16_v3": (_I, [_CFG, _TABLE, _P, _TABLE, _P, _P, _P, _P, _P, _LL, _P, _LL, _I, _F, _F, _ULL, _P, _P]),
    "dgvit_got_backward_bf16_v3_ev": (_I, [_CFG, _TABLE, _P, _TABLE, _P, _P, _P, _P, _P, _LL, _P, _LL, _I, _F, _F, _ULL, _P, _P,
                                           POINTER(dgvit_grad_events)]),
    "dgvit_attention_forward_bf16_tiled_drop": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _F, _ULL, _P, _I, _P]),
    "dgvit_attention_backward_bf16_tiled_drop": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _ULL, _P, _I, _P]),
    "dgvit_drop_rows_bf16": (_I, [_P, _LL, _P, _LL, _LL, _I, _I, _F, _ULL, _P, _I, _I, _P]),
    "dgvit_profile_start": (_I, [_I]),
    "dgvit_profile_stop": (_I, [POINTER(ctypes.c_double), POINTER(ctypes.c_double), POINTER(c_longlong)]),
    "dgvit_profile_sampling": (_I, [_I]),
    "dgvit_profile_totals": (_I, [POINTER(ctypes.c_double), POINTER(c_longlong)]),
}
# the additional entry points of libdgvit_hip_diag.so (include/dgvit_hip_diag.h)
DIAG_SIGNATURES = {
    "dgvit_set_gemm_tile": (None, [_I]),
    "dgvit_set_grouped_reduce": (None, [_I]),
    "dgvit_set_gemm_split": (None, [_I]),
    "dgvit_set_gemm_lds_pad": (None, [_I]),
    "dgvit_set_ln_fusion": (None, [_I]),
    "dgvit_set_conv_gather": (None, [_I]),
    "dgvit_set_gemm_diagnostics": (None, [_I]),
    "dgvit_set_gemm_persistent": (None, [_I, _I]),
    "dgvit_gemm_persistent_launches": (ctypes.c_longlong, []),
    "dgvit_set_gemm_stamps": (None, [_P, _I]),
    "dgvit_set_small_batch_path": (None, [_I, _I]),
    "dgvit_set_block_path": (None, [_I, _I]),
    "dgvit_set_block_stamps": (None, [_P]),
    "dgvit_set_block_stamp_layer": (None, [_I]),
    "dgvit_set_gelu_grad_store": (None, [_I]),
    "dgvit_set_block_fuse": (None, [_I]),
    "dgvit_set_gemm_bf16_tile": (None, [_I]),
    "dgvit_set_gemm_bf16_group_m": (None, [_I]),
    "dgvit_set_gemm_bf16_l2_budget_kb": (None, [_I]),
    "dgvit_set_attention_bwd_single_pass": (None, [_I]),
    "dgvit_set_attention_single_query": (None, [_I]),
    "dgvit_set_last_block_fold": (None, [_I]),
    "dgvit_set_attention_bf16_long": (None, [_I]),
    "dgvit_set_attention_bf16_tiled_waves": (None, [_I]),
    "dgvit_set_gemm_wgrad_slice_major": (None, [_I]),
    "dgvit_attention_forward_queries": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dgvit_attention_backward_queries": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dgvit_attention_forward_bf16_queries": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dgvit_attention_forward_drop": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _F, _ULL, _P, _I, _P]),
    "dgvit_attention_backward_drop": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _ULL, _P, _I, _P]),
    "dgvit_attention_forward_tiled_drop": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _F, _ULL, _P, _I, _P]),
    "dgvit_attention_backward_tiled_drop": (_I, [_P, _P, _P, _P, _P, _P, _LL, _I, _I, _I, _I, _I, _F, _ULL, _P, _I, _P]),
    "dgvit_set_gemm_bf16_mfma16": (None, [_I]),
    "dgvit_set_gemm_bf16_stamps": (None, [_P]),
    # the row kernels with row_step / nullable outputs / the queued reduction (include/dgvit_hip_diag.h)
    "dgvit_diag_layernorm_forward": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "dgvit_diag_layernorm_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _LL, _I, _I, _I, _I, _P]),
    "dgvit_diag_layernorm_forward_bf16": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "dgvit_diag_layernorm_backward_bf16": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _LL, _I, _I, _I, _P]),
    "dgvit_diag_residual_add_bf16": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "dgvit_diag_transpose_cast_f32_bf16": (_I, [_P, _P, _I, _I, _P]),
    "dgvit_diag_colsum_scratch_floats": (_LL, [_I, _I]),
    "dgvit_diag_colsum": (_I, [_P, _LL, _P, _P, _LL, _I, _I, _I, _P]),
}
PROFILE_KINDS = 4

_lib = None        # the library the package's calls go through (the product library unless diagnostic() is active)
_product = None
_diag = None


def _open(path, signatures):
    if not os.path.exists(path):
        raise DgvitError(f"{path} not found: build it with `python {os.path.join(_HERE, 'build.py')}` "
                         "(hipcc --offload-arch=gfx950). There is no fallback path.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in signatures.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise DgvitError(f"{path} does not export {name}; rebuild it") from e
        fn.restype, fn.argtypes = res, args
    if lib.dgvit_abi_version() != ABI_VERSION:
        raise DgvitError(f"ABI mismatch: library {lib.dgvit_abi_version()} != binding {ABI_VERSION}")
    if lib.dgvit_config_size() != ctypes.sizeof(dgvit_config):
        raise DgvitError(f"dgvit_config is {ctypes.sizeof(dgvit_config)} bytes in the binding, {lib.dgvit_config_size()} in the library")
    return lib


def load():
    """The library every call of the package goes through: libdgvit_hip.so (loaded and typed once; DgvitError if it is missing or
    stale), or the diagnostic build while a ``diagnostic()`` block is active."""
    global _lib, _product
    if _lib is not None:
        return _lib
    if _product is None:
        _product = _open(LIB_PATH, SIGNATURES)
    _lib = _product
    return _lib


class diagnostic:
    """``with diagnostic() as lib:`` routes the package through libdgvit_hip_diag.so (the -DDGVIT_DIAG build with the A/B knobs
    and experiments of include/dgvit_hip_diag.h) and yields it; the product library is back on exit.  Not thread-safe; for
    tools/ and the A/B equality tests, never for the product path."""

    def __enter__(self):
        global _lib, _diag
        load()
        if _diag is None:
            _diag = _open(DIAG_LIB_PATH, {**SIGNATURES, **DIAG_SIGNATURES})
        self._prev = _lib
        _lib = _diag
        return _diag

    def __exit__(self, *exc):
        global _lib
        _lib = self._prev
        return False


def check(rc, what):
    if rc != 0:
        msg = load().dgvit_last_error()
        raise DgvitError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")
