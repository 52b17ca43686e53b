"""ctypes binding of libbvc_hip.so (C ABI declared in include/bvc.h).

There is no CPU fallback: if the shared library is missing or a call fails, an exception is raised.
"""
import ctypes
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# BVC_LIB_PATH: another build of the same library (tools/: A/B of two builds on one box); the default is the in-tree build
LIB_PATH = os.environ.get("BVC_LIB_PATH") or os.path.join(_HERE, "libbvc_hip.so")

c_void_p, c_int, c_int64, c_float, c_char_p = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_char_p
c_double = ctypes.c_double


class BvcError(RuntimeError):
    pass


class VideoMAEConfigC(ctypes.Structure):
    _fields_ = [(n, c_int) for n in (
        "image_size", "patch_size", "num_channels", "num_frames", "tubelet_size",
        "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size",
        "decoder_hidden_size", "decoder_num_hidden_layers", "decoder_num_attention_heads",
        "decoder_intermediate_size")] + [("layer_norm_eps", c_float), ("decoder_norm_eps", c_float),
                                         ("norm_pix_loss", c_int)]


class VitConfigC(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("image_size", "patch_size", "num_channels", "num_frames", "tubelet_size", "embed_dim",
                                     "depth", "num_heads", "mlp_hidden")] + [("eps", c_float)]


class PredictorConfigC(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("seq_len", "embed_dim", "pred_dim", "depth", "num_heads", "mlp_hidden")] + [("eps", c_float)]


class PixelFormatC(ctypes.Structure):
    _fields_ = [("dtype", c_int), ("mean", c_float * 4), ("std", c_float * 4)]


def pixel_format(pixel_values, mean, std, channels):
    """None for f32 input (already normalised); a PixelFormatC for uint8 frames to be normalised on the GPU."""
    import torch
    if pixel_values.dtype != torch.uint8:
        return None
    def per_channel(v):
        v = list(v) if hasattr(v, "__len__") else [float(v)] * channels
        if len(v) != channels or channels > 4:
            raise ValueError("pixel mean / std need one value per channel (at most 4 channels)")
        return v + [0.0] * (4 - channels)
    f = PixelFormatC()
    f.dtype = 1
    f.mean = (c_float * 4)(*per_channel(mean))
    f.std = (c_float * 4)(*[x if i < channels else 1.0 for i, x in enumerate(per_channel(std))])
    return f


OPT_MAX_GROUPS = 8     # BVC_OPT_MAX_GROUPS (include/bvc.h)
OPT_TABLE_MAX_GROUPS = 1024     # BVC_OPT_TABLE_MAX_GROUPS: the device-table entry points (bvc_op_sgd_step_table / bvc_op_adam_step_table)


class SgdGroupsC(ctypes.Structure):
    _fields_ = [("ngroups", c_int)] + [(n, c_float * OPT_MAX_GROUPS) for n in ("lr", "momentum", "dampening", "weight_decay")] + \
               [(n, c_int * OPT_MAX_GROUPS) for n in ("nesterov", "first_step", "maximize")]


class AdamGroupsC(ctypes.Structure):
    _fields_ = [("ngroups", c_int)] + [(n, ctypes.c_double * OPT_MAX_GROUPS) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")] + \
               [(n, c_int * OPT_MAX_GROUPS) for n in ("decoupled", "maximize")]


class NormItemC(ctypes.Structure):
    """bvc_norm_item (include/bvc.h): one work item of the gradient-norm pass"""
    _fields_ = [("start", c_int64), ("length", ctypes.c_int32), ("segment", ctypes.c_int32)]


class GemmDesc(ctypes.Structure):
    _fields_ = [
        ("A", c_void_p), ("B", c_void_p),
        ("M", c_int), ("N", c_int), ("K", c_int), ("lda", c_int), ("ldb", c_int),
        ("a_bytes", ctypes.c_uint32), ("b_bytes", ctypes.c_uint32),
        ("alpha", c_float), ("alpha_dev", c_void_p),
        ("epi", c_int), ("split_k", c_int),
        ("C", c_void_p), ("ldc", c_int), ("seg_rows", c_int), ("C2", c_void_p),
        ("bias", c_void_p), ("resid", c_void_p), ("aux", c_void_p), ("ldaux", c_int), ("seg_stride", c_int),
        ("rowtok", c_void_p), ("pos", c_void_p), ("labels", c_void_p), ("partial", c_void_p),
        ("rin", c_int), ("rout", c_int),
        ("rowsum", c_void_p),
        ("ln_gamma", c_void_p), ("ln_beta", c_void_p), ("ln_mean", c_void_p), ("ln_rstd", c_void_p), ("ln_eps", c_float), ("seg_off", c_int),
        ("ln_x", c_void_p), ("ln_part", c_void_p), ("ln_dgamma", c_void_p), ("ln_dbeta", c_void_p),
    ]


class BranchDropC(ctypes.Structure):
    """bvc_branch_drop (include/bvc.h): the gate on the two residual branches of every layer of a context"""
    _fields_ = [("hidden_p", c_float), ("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64), ("path_scale", c_void_p),
                ("rows_per_sample", c_int)]


def branch_drop(hidden_p, seed, offset, path_scale, rows_per_sample):
    """A BranchDropC; path_scale = a contiguous f32 device tensor [layers][2][samples] or None."""
    d = BranchDropC()
    d.hidden_p = float(hidden_p)
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    d.offset = int(offset) & 0xFFFFFFFFFFFFFFFF
    d.path_scale = path_scale.data_ptr() if path_scale is not None else None
    d.rows_per_sample = int(rows_per_sample)
    return d


class IntrospectC(ctypes.Structure):
    """bvc_introspect (include/bvc.h): where a classification context delivers its per-layer outputs; either pointer may be null"""
    _fields_ = [("hidden_states", c_void_p), ("attentions", c_void_p)]


def introspect(hidden_states, attentions):
    """An IntrospectC over two contiguous f32 device tensors ([L + 1][B][N][D], [L][B][H][N][N]), either None; None when both are."""
    if hidden_states is None and attentions is None:
        return None
    o = IntrospectC()
    o.hidden_states = hidden_states.data_ptr() if hidden_states is not None else None
    o.attentions = attentions.data_ptr() if attentions is not None else None
    return o


BUCKET_FN = ctypes.CFUNCTYPE(None, c_int64, c_int64, c_void_p)

# every symbol include/bvc.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "bvc_last_error": (c_char_p, []),
    "bvc_version": (c_char_p, []),
    "bvc_set_option": (c_int, [c_char_p, c_int]),
    "bvc_get_option": (c_int, [c_char_p]),
    "bvc_deterministic_workspace_bytes": (c_int64, []),
    "bvc_deterministic_workspace_release": (c_int, []),
    "bvc_videomae_param_count": (c_int, [ctypes.POINTER(VideoMAEConfigC)]),
    "bvc_videomae_param_numel": (c_int64, [ctypes.POINTER(VideoMAEConfigC)]),
    "bvc_videomae_param_info": (c_int, [ctypes.POINTER(VideoMAEConfigC), c_int, ctypes.c_char_p, c_int,
                                        ctypes.POINTER(c_int64), ctypes.POINTER(c_int64), ctypes.POINTER(c_int),
                                        ctypes.POINTER(c_int64)]),
    "bvc_videomae_create": (c_int, [ctypes.POINTER(VideoMAEConfigC), c_int, c_int, ctypes.POINTER(c_void_p)]),
    "bvc_videomae_create_dual": (c_int, [ctypes.POINTER(VideoMAEConfigC), c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "bvc_videomae_destroy": (None, [c_void_p]),
    "bvc_videomae_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bvc_videomae_forward_px": (c_int, [c_void_p, c_void_p, ctypes.POINTER(PixelFormatC), c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "bvc_videomae_forward_dual": (c_int, [c_void_p, c_void_p, ctypes.POINTER(PixelFormatC), c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    "bvc_videomae_backward": (c_int, [c_void_p, c_void_p, c_void_p, BUCKET_FN, c_void_p, c_void_p]),
    "bvc_videomae_tap": (c_int, [c_void_p, c_char_p, c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    "bvc_videomae_encoder_param_numel": (c_int64, [ctypes.POINTER(VideoMAEConfigC)]),
    "bvc_videomae_encoder_create": (c_int, [ctypes.POINTER(VideoMAEConfigC), c_int, ctypes.POINTER(c_void_p)]),
    "bvc_videomae_encoder_destroy": (None, [c_void_p]),
    "bvc_videomae_encode": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "bvc_videomae_encode_px": (c_int, [c_void_p, c_void_p, ctypes.POINTER(PixelFormatC), c_int, c_void_p, c_void_p, c_void_p, c_float,
                                       c_void_p, c_void_p, c_void_p]),
    "bvc_videomae_encode_ex": (c_int, [c_void_p, c_void_p, ctypes.POINTER(PixelFormatC), c_int, c_void_p, c_void_p, c_void_p, c_float,
                                       c_void_p, c_void_p, ctypes.POINTER(IntrospectC), c_void_p]),
    "bvc_videomae_cls_introspect": (c_int, [c_void_p, ctypes.POINTER(IntrospectC), c_void_p]),
    "bvc_videomae_encoder_fc_norm_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bvc_videomae_cls_create": (c_int, [ctypes.POINTER(VideoMAEConfigC), c_int, ctypes.POINTER(c_void_p)]),
    "bvc_videomae_cls_destroy": (None, [c_void_p]),
    "bvc_videomae_cls_forward_px": (c_int, [c_void_p, c_void_p, ctypes.POINTER(PixelFormatC), c_int, c_void_p, c_void_p, c_void_p,
                                            c_float, c_void_p, c_void_p, c_void_p]),
    "bvc_videomae_cls_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, BUCKET_FN, c_void_p, c_void_p]),
    "bvc_videomae_cls_shadow": (c_int, [c_void_p, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64)]),
    "bvc_vit_param_count":(c_int, [ctypes.POINTER(VitConfigC)]),
    "bvc_vit_param_numel": (c_int64, [ctypes.POINTER(VitConfigC)]),
    "bvc_vit_param_info": (c_int, [ctypes.POINTER(VitConfigC), c_int, ctypes.c_char_p, c_int, ctypes.POINTER(c_int64),
                                   ctypes.POINTER(c_int64), ctypes.POINTER(c_int), ctypes.POINTER(c_int64)]),
    "bvc_vit_create": (c_int, [ctypes.POINTER(VitConfigC), c_int, ctypes.POINTER(c_void_p)]),
    "bvc_vit_destroy": (None, [c_void_p]),
    "bvc_vit_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "bvc_vit_forward_px": (c_int, [c_void_p, c_void_p, ctypes.POINTER(PixelFormatC), c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "bvc_vit_backward": (c_int, [c_void_p, c_void_p, c_void_p, BUCKET_FN, c_void_p, c_void_p]),
    "bvc_predictor_param_count": (c_int, [ctypes.POINTER(PredictorConfigC)]),
    "bvc_predictor_param_numel": (c_int64, [ctypes.POINTER(PredictorConfigC)]),
    "bvc_predictor_param_info": (c_int, [ctypes.POINTER(PredictorConfigC), c_int, ctypes.c_char_p, c_int, ctypes.POINTER(c_int64),
                                         ctypes.POINTER(c_int64), ctypes.POINTER(c_int), ctypes.POINTER(c_int64)]),
    "bvc_predictor_create": (c_int, [ctypes.POINTER(PredictorConfigC), c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "bvc_predictor_destroy": (None, [c_void_p]),
    "bvc_predictor_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "bvc_predictor_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bvc_predictor_backward_cb": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, BUCKET_FN, c_void_p, c_void_p]),
    "bvc_op_target_select": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "bvc_op_smooth_l1_workspace": (c_int, [c_int64]),
    "bvc_op_smooth_l1_fwd": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "bvc_op_smooth_l1_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "bvc_op_ema": (c_int, [c_void_p, c_void_p, c_int64, c_float, c_void_p]),
    "bvc_op_token_mean": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "bvc_op_token_mean_bwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "bvc_op_gemm": (c_int, [ctypes.POINTER(GemmDesc), c_int, c_int, c_int, c_int, c_void_p]),
    "bvc_op_gemm_num_tiles": (c_int, [ctypes.POINTER(GemmDesc), c_int]),
    "bvc_op_gemm_kernel": (c_int, [ctypes.POINTER(GemmDesc), c_int, c_int, c_int, c_int, ctypes.c_char_p, c_int]),
    "bvc_op_gemm_plan_dw": (c_int, [ctypes.POINTER(GemmDesc), c_int]),
    "bvc_op_gemm_gate": (c_int, [ctypes.POINTER(GemmDesc), ctypes.POINTER(BranchDropC), c_int, c_int, c_int, c_void_p]),
    "bvc_op_gemm_gate_kernel": (c_int, [ctypes.POINTER(GemmDesc), c_int, ctypes.c_char_p, c_int]),
    "bvc_op_layernorm_bwd_gate": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_int, c_int, ctypes.POINTER(BranchDropC), c_int, c_int, c_void_p]),
    "bvc_op_dropout_mask": (c_int, [ctypes.c_uint64, ctypes.c_uint64, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "bvc_dropout_mask_host": (c_int, [ctypes.c_uint64, ctypes.c_uint64, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "bvc_op_clip_transform_workspace": (c_int64, [c_int, c_int, c_int]),
    "bvc_op_clip_transform": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "bvc_clip_transform_host": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "bvc_aug_blur_weights": (c_int, [c_float, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    "bvc_op_clip_post_workspace": (c_int64, [c_int, c_int, c_int]),
    "bvc_op_clip_post": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "bvc_clip_post_host": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "bvc_frame_randaug_bytes": (c_int, []),
    "bvc_op_clip_randaug_workspace": (c_int64, [c_int, c_int, c_int]),
    "bvc_op_clip_randaug": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "bvc_clip_randaug_host": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "bvc_jpeg_info_bytes": (c_int, []),
    "bvc_jpeg_parse": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int]),
    "bvc_jpeg_decode_host": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "bvc_op_jpeg_decode_workspace": (c_int64, [c_void_p, c_int]),
    # (blob, blob_bytes, infos host / dev, n, segs host / dev, nseg, out_offsets host / dev, out, out_bytes, status, workspace, workspace_bytes, lanes, stages, stream)
    "bvc_op_jpeg_decode": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                   c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "bvc_jpeg_split_chunk": (c_int, [c_int, c_int]),
    # (data, n, info, seg, split, chunk, out_rgb, info_out)
    "bvc_jpeg_decode_host_split": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "bvc_op_jpeg_decode_split_workspace": (c_int64, [c_void_p, c_int]),
    # bvc_op_jpeg_decode's arguments up to stages, then (split, chunk, info_out, stream)
    "bvc_op_jpeg_decode_split": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                         c_int64, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "bvc_videomae_cls_set_drop": (c_int, [c_void_p, ctypes.POINTER(BranchDropC), c_int, c_void_p]),
    "bvc_videomae_encoder_set_drop": (c_int, [c_void_p, ctypes.POINTER(BranchDropC), c_int, c_void_p]),
    "bvc_videomae_cls_set_mix": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "bvc_videomae_encoder_set_mix": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "bvc_videomae_cls_set_erase": (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.c_uint64, ctypes.c_uint64, c_void_p]),
    "bvc_videomae_encoder_set_erase": (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.c_uint64, ctypes.c_uint64, c_void_p]),
    "bvc_op_erase_noise": (c_int, [ctypes.c_uint64, ctypes.c_uint64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "bvc_vit_set_drop": (c_int, [c_void_p, ctypes.POINTER(BranchDropC), c_int, c_void_p]),
    "bvc_predictor_set_drop": (c_int, [c_void_p, ctypes.POINTER(BranchDropC), c_int, c_void_p]),
    "bvc_op_attention_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "bvc_op_attention_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "bvc_op_attention_bwd_part": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "bvc_op_attention_width": (c_int, [c_int]),
    "bvc_op_attention_fwd_scaled": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, ctypes.c_float, c_void_p]),
    "bvc_op_attention_bwd_scaled": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                            ctypes.c_float, c_void_p]),
    "bvc_op_attention_probs": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, ctypes.c_float, c_void_p]),
    "bvc_op_topk_workspace": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "bvc_op_topk_splits": (c_int, [c_int, c_int, c_int, c_int]),
    "bvc_op_topk": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                            c_void_p, c_void_p, c_void_p, c_void_p]),
    "bvc_op_attn_pool_splits": (c_int, [c_int, c_int, c_int, c_int]),
    "bvc_op_attn_pool_workspace": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "bvc_op_attn_pool_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "bvc_op_attn_pool_bwd": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                     c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "bvc_op_ntxent_splits": (c_int, [c_int, c_int]),
    "bvc_op_ntxent_block_rows": (c_int, [c_int, c_int]),
    "bvc_op_ntxent_workspace": (c_int64, [c_int, c_int, c_int, c_int]),
    "bvc_op_ntxent_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_float, c_float, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    "bvc_op_ntxent_bwd": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                  c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
    "bvc_op_proto_ce_splits": (c_int, [c_int, c_int, c_int]),
    "bvc_op_proto_ce_block": (c_int, [c_int, c_int, c_int]),
    "bvc_op_proto_ce_workspace": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "bvc_op_proto_ce_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_int, c_int,
                                    c_float, c_float, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bvc_op_proto_ce_bwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_int, c_int,
                                    c_float, c_float, c_float, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64,
                                    c_void_p, c_void_p]),
    "bvc_op_xcorr_block_cols": (c_int, [c_int, c_int, c_int]),
    "bvc_op_xcorr_workspace": (c_int64, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "bvc_op_xcorr_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_float,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bvc_op_xcorr_bwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_float,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p,
                                 c_int64, c_void_p, c_void_p]),
    "bvc_op_colstats": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "bvc_op_linear_pass_workspace": (c_int64, [c_int, c_int, c_int, c_int]),
    "bvc_op_linear_pass_splits": (c_int, [c_int, c_int, c_int]),
    "bvc_op_linear_pass_tile_rows": (c_int, [c_int]),
    "bvc_op_linear_pass": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                   c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bvc_op_layernorm_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int, c_int, c_float, c_void_p]),
    "bvc_op_layernorm_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "bvc_op_layernorm_bwd_workspace": (c_int64, [c_int, c_int]),
    "bvc_op_colsum_bf16": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "bvc_op_dec_first_selected": (c_int, [c_int, c_int]),
    "bvc_op_dec_slot": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "bvc_op_first_reduce": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bvc_op_colsum_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "bvc_op_cast_bf16": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "bvc_op_row_normalize": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p]),
    "bvc_op_row_normalize_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "bvc_op_nce_finalize": (c_int, [c_void_p, c_int, c_float, c_int64, c_void_p, c_void_p, c_void_p]),
    "bvc_op_sgd_step": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_int, c_int, c_int,
                                c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "bvc_videomae_shadow": (c_int, [c_void_p, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64)]),
    "bvc_vit_shadow": (c_int, [c_void_p, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64)]),
    "bvc_predictor_shadow": (c_int, [c_void_p, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64)]),
    "bvc_op_adam_prepare": (c_int, [c_void_p, c_double, c_double, c_double, c_void_p, c_void_p]),
    "bvc_op_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_double, c_double, c_double,
                                 c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "bvc_op_row_ln_selected": (c_int, [c_int, c_int, c_int, c_int]),
    "bvc_op_sgd_step_segments": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                         c_int, c_void_p, c_void_p]),
    "bvc_op_adam_step_segments": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "bvc_op_sgd_step_table": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 7 +
                                      [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "bvc_op_adam_step_table": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 7 +
                                       [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    # (params, grads, state arrays, n, seg_start, seg_group, blk_seg, nseg, items, nitems, seg_first_item, ngroups, 7 hyper-parameter
    #  arrays, [state,] group_table, item_partial, seg_stats, grad_scale, found_inf, write_unscaled_grads, bf16_shadow, stream)
    "bvc_op_lars_step_table": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p,
                                       c_int] + [c_void_p] * 7 + [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "bvc_op_lamb_step_table": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64,
                                       c_void_p, c_int] + [c_void_p] * 7 +
                                      [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "bvc_op_nonfinite_check": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "bvc_op_grad_norm_item_cap": (c_int, []),
    "bvc_op_grad_norm_chain": (c_int, []),
    "bvc_grad_norm_items_host": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, ctypes.POINTER(c_int64)]),
    "bvc_op_grad_sqnorm_items": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "bvc_op_clip_finalize": (c_int, [c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "bvc_op_scale_by_dev": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "bvc_op_mask_index": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bvc_op_dual_mask_index": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bvc_op_gather_patches": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "bvc_op_gather_patches_mix": (c_int, [c_void_p, ctypes.POINTER(PixelFormatC), c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                          c_int, c_int, c_int, c_int, c_void_p]),
    "bvc_op_gather_patches_aug": (c_int, [c_void_p, ctypes.POINTER(PixelFormatC), c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_uint64,
                                          ctypes.c_uint64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "bvc_op_pixel_labels": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "bvc_comm_unique_id": (c_int, [c_void_p]),
    "bvc_comm_init": (c_int, [c_int, c_int, c_void_p, ctypes.POINTER(c_void_p)]),
    "bvc_comm_destroy": (c_int, [c_void_p]),
    "bvc_comm_stream": (c_void_p, [c_void_p]),
    "bvc_comm_rank": (c_int, [c_void_p]),
    "bvc_comm_world": (c_int, [c_void_p]),
    "bvc_comm_library": (c_char_p, []),
    "bvc_allreduce_bucket": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "bvc_comm_wait": (c_int, [c_void_p, c_void_p]),
    "bvc_allgather": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "bvc_allreduce": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "bvc_broadcast": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
}

_lib = None

# Deterministic mode (include/bvc.h, option "deterministic").  The effective mode is bvc.use_deterministic_algorithms(...) OR
# torch.are_deterministic_algorithms_enabled(), read at every library call (lib() below) and pushed to the library when it changes.
_det_flag = False
_det_pushed = False      # what this module last pushed (the library's own default is 0)


def use_deterministic_algorithms(mode):
    """Turn the library's deterministic mode on or off for this process (torch.use_deterministic_algorithms' counterpart).  While it,
    or torch's own flag, is on, every forward and backward of the library gives the same bits on every run for the same inputs,
    parameters, batch, device and build."""
    global _det_flag
    _det_flag = bool(mode)
    lib()


def are_deterministic_algorithms_enabled():
    """The flag use_deterministic_algorithms set (torch's flag is ORed in at each library call, not reported here)."""
    return _det_flag


def _sync_deterministic(L):
    global _det_pushed
    torch = sys.modules.get("torch")
    want = _det_flag or (torch is not None and torch.are_deterministic_algorithms_enabled())
    if want != _det_pushed:
        rc = L.bvc_set_option(b"deterministic", 1 if want else 0)
        if rc != 0:
            raise BvcError(f"bvc_set_option(deterministic) failed with status {rc}")
        _det_pushed = want


def lib():
    """Load libbvc_hip.so once; raise loudly if it has not been built (no fallback path exists).  Every call into the library goes
    through here, which is where the effective deterministic mode is brought up to date."""
    global _lib
    if _lib is not None:
        _sync_deterministic(_lib)
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BvcError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)   # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = L
    _sync_deterministic(_lib)
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().bvc_last_error()
        raise BvcError(f"{what} failed with status {rc}: {msg.decode() if msg else ''}")


def set_option(name, value):
    """bvc_set_option (include/bvc.h): "gemm8" -1 / 0 / 1, "dw_overlap" 0 / 1, "row_ln" -1 / 0 / 1, "head_pad" 0 / 1, "dec_tail" 0 / 1, "dec_first" -1 / 0 / 1, "deterministic" 0 / 1 (what
    bvc.use_deterministic_algorithms and torch.use_deterministic_algorithms switch; the library's raw flag - the next library call
    after either of those changes resets it to their OR).  Returns the previous value."""
    old = lib().bvc_get_option(name.encode())
    check(lib().bvc_set_option(name.encode(), int(value)), "bvc_set_option")
    return old


def current_stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
