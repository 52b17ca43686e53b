"""VideoMAE pre-training model object with the interface the reference's entry point uses.

Reference seam (pretraining/generative/pretrain_videomae.py):
  :43-64   get_config / get_model  -> transformers.VideoMAEConfig / VideoMAEForPreTraining
  :66-70   load_state_dict(ckpt['model_state_dict'])        (transformers key names)
  :170-176 model.config.image_size / patch_size / num_frames / tubelet_size
  :178-181 .to(rank), DDP(model), .parameters(), .train(), .eval()
  :301-302 outputs = xmodel(inputs, bool_masked_pos=m); outputs.loss
  :312     scaler.scale(loss).backward()
The arithmetic (HF:531-671) runs in libbvc_hip.so; this file only owns parameters, the flat
parameter / gradient buffers and the autograd bridge.
"""
from __future__ import annotations

import ctypes
import warnings
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from . import _lib
from .dropgate import BranchGate
from .flat import FlatParamModule, query_layout


class VideoMAEConfig:
    """The fields of transformers.VideoMAEConfig that the path reads; unknown kwargs are kept as attributes.

    ``hidden_dropout_prob`` (transformers' field: dropout on the two branch outputs of every encoder layer, HF:270-274, 316-320) and
    the extension ``drop_path_rate`` (stochastic depth, rates ``linspace(0, rate, depth)`` as the published fine-tuning recipes use
    it) take effect in ``VideoMAEForVideoClassification`` in train mode.  ``attention_probs_dropout_prob`` must stay 0.0: dropout on
    the attention probabilities is not implemented, and a config that asks for it is refused instead of training another model.

    ``output_hidden_states`` / ``output_attentions`` (default False) are the defaults of the keywords of the same name of
    ``VideoMAEForVideoClassification.forward``."""

    def __init__(self, image_size=224, patch_size=16, num_channels=3, num_frames=16, tubelet_size=2,
                 hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                 hidden_act="gelu", layer_norm_eps=1e-12, initializer_range=0.02, qkv_bias=True,
                 use_mean_pooling=True, decoder_num_attention_heads=6, decoder_hidden_size=384,
                 decoder_num_hidden_layers=4, decoder_intermediate_size=1536, norm_pix_loss=True,
                 hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0,
                 output_hidden_states=False, output_attentions=False, **kwargs):
        # transformers' PretrainedConfig fields: what VideoMAEForVideoClassification.forward returns when the call leaves them None
        self.output_hidden_states, self.output_attentions = bool(output_hidden_states), bool(output_attentions)
        if attention_probs_dropout_prob:
            raise ValueError(f"attention_probs_dropout_prob={attention_probs_dropout_prob}: dropout on the attention probabilities is not "
                             "implemented (only 0.0)")
        for name, v in (("hidden_dropout_prob", hidden_dropout_prob), ("drop_path_rate", drop_path_rate)):
            if not 0.0 <= float(v) < 1.0:
                raise ValueError(f"{name}={v} must lie in [0, 1)")
        self.hidden_dropout_prob, self.attention_probs_dropout_prob = float(hidden_dropout_prob), float(attention_probs_dropout_prob)
        self.drop_path_rate = float(drop_path_rate)
        if hidden_act != "gelu":
            raise ValueError("only hidden_act='gelu' (exact erf GELU) is implemented")
        if not qkv_bias:
            raise ValueError("qkv_bias=False is not implemented")
        self.image_size, self.patch_size, self.num_channels = image_size, patch_size, num_channels
        self.num_frames, self.tubelet_size = num_frames, tubelet_size
        self.hidden_size, self.num_hidden_layers = hidden_size, num_hidden_layers
        self.num_attention_heads, self.intermediate_size = num_attention_heads, intermediate_size
        self.hidden_act, self.layer_norm_eps, self.initializer_range = hidden_act, layer_norm_eps, initializer_range
        self.qkv_bias, self.use_mean_pooling = qkv_bias, use_mean_pooling
        self.decoder_num_attention_heads, self.decoder_hidden_size = decoder_num_attention_heads, decoder_hidden_size
        self.decoder_num_hidden_layers, self.decoder_intermediate_size = decoder_num_hidden_layers, decoder_intermediate_size
        self.norm_pix_loss = norm_pix_loss
        self.decoder_norm_eps = 1e-5   # nn.LayerNorm default used by decoder.norm (HF:484)
        for k, v in kwargs.items():
            setattr(self, k, v)

    @property
    def seq_length(self):
        g = self.image_size // self.patch_size
        return (self.num_frames // self.tubelet_size) * g * g

    def to_c(self) -> _lib.VideoMAEConfigC:
        return _lib.VideoMAEConfigC(
            self.image_size, self.patch_size, self.num_channels, self.num_frames, self.tubelet_size,
            self.hidden_size, self.num_hidden_layers, self.num_attention_heads, self.intermediate_size,
            self.decoder_hidden_size, self.decoder_num_hidden_layers, self.decoder_num_attention_heads,
            self.decoder_intermediate_size, float(self.layer_norm_eps), float(self.decoder_norm_eps),
            int(bool(self.norm_pix_loss)))


@dataclass
class VideoMAEForPreTrainingOutput:
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    hidden_states: Optional[tuple] = None
    attentions: Optional[tuple] = None


def param_layout(config: VideoMAEConfig):
    """[(state-dict key, offset, shape)] in flat-buffer order, as libbvc_hip.so defines it."""
    L = _lib.lib()
    return query_layout(L.bvc_videomae_param_count, L.bvc_videomae_param_numel, L.bvc_videomae_param_info, config.to_c())


class _CountCheck:
    """Set entries per clip of a [B, L] bool mask.  One host sync on the first call per mask shape; afterwards the cached count is
    VERIFIED asynchronously: every call leaves `count(row 0) != cached`, `rows differ` (and the caller's own `bad` condition) as a
    flag in a pinned word that the next call reads (a ratio change at the same shape - a validation phase, a curriculum stage -
    raises on the following step instead of training on NaN losses that GradScaler silently skips)."""

    def __init__(self, changed, unequal):
        self.changed, self.unequal = changed, unequal
        self.cache, self.pending, self.flag = {}, None, None

    def __deepcopy__(self, memo):
        return _CountCheck(self.changed, self.unequal)

    def count(self, mask, strict, bad=None, bad_message=None):
        """`bad`: a 0-dim bool tensor on the mask's device, a further condition under which the masks must not be used."""
        key = tuple(mask.shape)
        if self.pending is not None:
            ev, flag, pkey = self.pending
            ev.synchronize()                    # the previous step's check: long done, no stall
            self.pending = None
            if int(flag[0]) != 0:
                self.cache.pop(pkey, None)
                raise ValueError(self.changed)
        if strict or key not in self.cache:
            counts = mask.sum(dim=1)
            n = int(counts[0])       # one host sync, first call per shape only
            if not bool((counts == n).all()):
                raise ValueError(self.unequal)
            if bad is not None and bool(bad):
                raise ValueError(bad_message)
            self.cache[key] = n
            return n
        n = self.cache[key]
        if self.flag is None:
            self.flag = torch.zeros(1, dtype=torch.int32).pin_memory()
        wrong = (mask.sum(dim=1) != n).any()
        if bad is not None:
            wrong = wrong | bad
        self.flag.copy_(wrong.to(torch.int32).reshape(1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(mask.device))
        self.pending = (ev, self.flag, key)
        return n


class _Step(torch.autograd.Function):
    """loss = step(pixels, mask[, decode mask]); backward fills the flat gradient buffer and hands out views as .grad."""

    @staticmethod
    def forward(ctx, anchor, model, pixels, mask, decode, want_logits):
        ctx.model = model
        loss, logits = model._run_forward(pixels, mask, decode, want_logits)
        ctx.stamp = model._stamp_forward()
        ctx.mark_non_differentiable(logits) if logits is not None else None
        return loss, logits

    @staticmethod
    def backward(ctx, grad_loss, _grad_logits):
        ctx.model._check_generation(ctx.stamp)
        ctx.model._run_backward(grad_loss)
        return None, None, None, None, None, None


class VideoMAEForPreTraining(FlatParamModule):
    _shadow_fn = "bvc_videomae_shadow"
    """Drop-in for transformers.VideoMAEForPreTraining on the pre-training path (same state-dict keys)."""

    def __init__(self, config: VideoMAEConfig):
        super().__init__()
        for field in ("hidden_dropout_prob", "drop_path_rate", "attention_probs_dropout_prob"):
            if getattr(config, field, 0.0):
                raise ValueError(f"{field}={getattr(config, field)}: dropout / stochastic depth in pre-training is not implemented "
                                 "(VideoMAEForVideoClassification applies hidden_dropout_prob and drop_path_rate)")
        self.config = config
        layout, numel = param_layout(config)
        std = config.initializer_range

        def init(name, shape):
            # transformers' _init_weights: normal(0, initializer_range) for Linear/Conv3d weights, zero biases,
            # LayerNorm weight 1 / bias 0; mask_token is created as zeros (HF:515)
            if len(shape) >= 2 and name != "mask_token":
                return torch.empty(shape).normal_(0.0, std)
            if name.endswith("layernorm_before.weight") or name.endswith("layernorm_after.weight") or name == "decoder.norm.weight":
                return torch.ones(shape)
            return torch.zeros(shape)

        self._init_flat(layout, numel, init)
        self._ctx = None
        self._ctx_key = None
        self.strict_mask_check = False
        self._mask_count = _CountCheck(
            "bool_masked_pos: the number of masked patches per clip changed (or differs between clips) "
            "without a new model object; every clip must mask the same number of patches",
            "every clip must have the same number of masked patches")
        self._decode_count = _CountCheck(
            "bool_decode_pos: the number of decoded patches per clip changed (or differs between clips, or a decoded patch was not "
            "masked) without a new model object; every clip must decode the same number of its masked patches",
            "every clip must have the same number of decoded patches")
        # uint8 pixel_values are normalised on the GPU as (u / 255 - mean) / std, the loader's ToTensor + Normalize
        # (homeview.py:221-230 uses 0.5 / 0.25 for every channel); f32 pixel_values are taken as already normalised
        self.pixel_mean, self.pixel_std = 0.5, 0.25

    # ---- library context
    def _get_ctx(self, batch, nmask, ndec=None):
        """ndec: decoded masked tokens per clip (None: all nmask of them, the context bvc_videomae_create makes)."""
        key = (batch, nmask, self._flat.device.index, nmask if ndec is None else ndec)
        if self._ctx is not None and self._ctx_key[1:] == key[1:] and self._ctx_key[0] >= batch:
            return self._ctx
        self._free_ctx()
        h = ctypes.c_void_p()
        cc = self.config.to_c()
        if ndec is None:
            _lib.check(_lib.lib().bvc_videomae_create(ctypes.byref(cc), batch, nmask, ctypes.byref(h)), "bvc_videomae_create")
        else:
            _lib.check(_lib.lib().bvc_videomae_create_dual(ctypes.byref(cc), batch, nmask, ndec, ctypes.byref(h)), "bvc_videomae_create_dual")
        self._ctx, self._ctx_key = h, key
        return h

    def _free_ctx(self):
        if self._ctx is not None:
            _lib.lib().bvc_videomae_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self._free_ctx()
        except Exception:
            pass

    # ---- step
    def _num_masked(self, mask):
        """Masked tokens per clip (_CountCheck: cached per mask shape, verified asynchronously; strict_mask_check verifies on the spot)."""
        return self._mask_count.count(mask, self.strict_mask_check)

    def _num_decoded(self, decode, mask):
        """Decoded tokens per clip, checked as the mask's count is, together with the subset condition: a decoded token that the
        encoder sees would leak its target into the loss (the library makes the loss NaN; here it raises - on the spot under
        strict_mask_check or on the first call per shape, otherwise on the following step)."""
        return self._decode_count.count(decode, self.strict_mask_check, bad=(decode & ~mask).any(),
                                        bad_message="bool_decode_pos must be a subset of bool_masked_pos: a decoded patch is visible to the encoder")

    def _run_forward(self, pixels, mask, decode, want_logits):
        cfg = self.config
        fmt = _lib.pixel_format(pixels, self.pixel_mean, self.pixel_std, cfg.num_channels)
        B = pixels.shape[0]
        nmask = self._num_masked(mask)
        ndec = self._num_decoded(decode, mask) if decode is not None else None
        h = self._get_ctx(B, nmask, ndec)
        loss = torch.empty((), dtype=torch.float32, device=pixels.device)
        logits = None
        if want_logits:
            pd = cfg.num_channels * cfg.tubelet_size * cfg.patch_size ** 2
            logits = torch.empty((B, nmask if ndec is None else ndec, pd), dtype=torch.float32, device=pixels.device)
        self._shadow_vouch(h)
        pf = ctypes.byref(fmt) if fmt is not None else None
        lg = logits.data_ptr() if logits is not None else None
        if decode is None:
            _lib.check(_lib.lib().bvc_videomae_forward_px(h, pixels.data_ptr(), pf, mask.data_ptr(), B, self._flat.data_ptr(), loss.data_ptr(), lg,
                                                          _lib.current_stream_ptr()), "bvc_videomae_forward")
        else:
            _lib.check(_lib.lib().bvc_videomae_forward_dual(h, pixels.data_ptr(), pf, mask.data_ptr(), decode.data_ptr(), B, self._flat.data_ptr(),
                                                            loss.data_ptr(), lg, _lib.current_stream_ptr()), "bvc_videomae_forward_dual")
        self._shadow_established(h)
        self._live = (pixels, mask, decode)   # keep the borrowed inputs alive until backward
        return loss, logits

    def _run_backward(self, grad_loss):
        target, accumulate = self._grad_target()
        g = grad_loss.detach().to(dtype=torch.float32).contiguous()
        cb = self._bucket_callback(accumulate)
        self._library_backward("bvc_videomae_backward",
                               _lib.lib().bvc_videomae_backward(self._ctx, g.data_ptr(), target.data_ptr(), cb, None, _lib.current_stream_ptr()))
        self._publish_grads(target, accumulate)
        self._live = None

    def forward(self, pixel_values, bool_masked_pos=None, bool_decode_pos=None, output_logits=False, **kwargs):
        """``bool_decode_pos`` ([B, L] bool, optional): the masked tokens the decoder reconstructs (VideoMAE V2's decoder masking,
        Wang et al., CVPR 2023, section 3.2).  True = the token gets a mask-token row in the decoder and is a loss target; it must be a
        subset of ``bool_masked_pos`` with the same count ``ndec`` in every clip.  The decoder then runs on ``nvis + ndec`` tokens, the
        loss is the mean over the decoded tokens and ``logits`` is ``[B, ndec, patch_dim]`` in ascending token order.  ``None``: every
        masked token, the step transformers' VideoMAEForPreTraining computes."""
        for name in ("output_hidden_states", "output_attentions"):
            if kwargs.get(name):
                raise NotImplementedError(f"VideoMAEForPreTraining.forward({name}=True) is not implemented: read single activations of the "
                                          "last forward with tap('embed' / 'enc<i>' / 'x_full' / 'dec<i>'); per-layer outputs exist on "
                                          "VideoMAEForVideoClassification")
        if bool_masked_pos is None:
            raise ValueError("One must provided a boolean mask ")
        if not pixel_values.is_cuda:
            raise _lib.BvcError("VideoMAEForPreTraining runs on a GPU only (libbvc_hip.so has no CPU path)")
        cfg = self.config
        B, T, C, H, W = pixel_values.shape
        if C != cfg.num_channels:
            raise ValueError("Make sure that the channel dimension of the pixel values match with the one set in the configuration.")
        if H != cfg.image_size or W != cfg.image_size or T != cfg.num_frames:
            raise ValueError(f"Input size ({T}x{H}*{W}) doesn't match model ({cfg.num_frames}x{cfg.image_size}*{cfg.image_size}).")
        if tuple(bool_masked_pos.shape) != (B, cfg.seq_length):
            raise ValueError(f"bool_masked_pos must have shape {(B, cfg.seq_length)}")
        self._ensure_flat(pixel_values.device)
        pixels = pixel_values.detach()
        pixels = (pixels if pixels.dtype == torch.uint8 else pixels.to(dtype=torch.float32)).contiguous()
        mask = bool_masked_pos.to(device=pixels.device, dtype=torch.bool).contiguous()
        decode = None
        if bool_decode_pos is not None:
            if tuple(bool_decode_pos.shape) != (B, cfg.seq_length):
                raise ValueError(f"bool_decode_pos must have shape {(B, cfg.seq_length)}")
            decode = bool_decode_pos.to(device=pixels.device, dtype=torch.bool).contiguous()
        anchor = self._param(self._names[0])
        if torch.is_grad_enabled() and anchor.requires_grad:
            loss, logits = _Step.apply(anchor, self, pixels, mask, decode, output_logits)
        else:
            loss, logits = self._run_forward(pixels, mask, decode, output_logits)
            self._stamp_forward()     # a pending backward of an earlier forward must not run on these activations
        return VideoMAEForPreTrainingOutput(loss=loss, logits=logits)

    # ---- parity probes
    def tap(self, name):
        """f32 copy of a saved activation of the last forward ('embed', 'enc<i>', 'x_full', 'dec<i>', 'labels').  With a decode mask
        'x_full' / 'dec<i>' hold nvis + ndec rows per clip and 'labels' ndec."""
        cfg = self.config
        cap = max(self._ctx_key[0] * cfg.seq_length * max(cfg.hidden_size, cfg.decoder_hidden_size),
                  self._ctx_key[0] * self._ctx_key[1] * cfg.num_channels * cfg.tubelet_size * cfg.patch_size ** 2)
        buf = torch.empty(cap, dtype=torch.float32, device=self._flat.device)
        n = ctypes.c_int64()
        _lib.check(_lib.lib().bvc_videomae_tap(self._ctx, name.encode(), buf.data_ptr(), cap, ctypes.byref(n),
                                               _lib.current_stream_ptr()), "bvc_videomae_tap")
        return buf[: n.value]


@dataclass
class ImageClassifierOutput:
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    hidden_states: Optional[tuple] = None
    attentions: Optional[tuple] = None
    last_hidden_state: Optional[torch.Tensor] = None


def classification_path(training, grad_enabled, encoder_trainable):
    """Which library context a VideoMAEForVideoClassification forward runs: "train" (the fine-tuning context, the encoder receives
    gradients) only in train mode with grad mode on and some ``videomae.*`` parameter requiring grad; otherwise "encode" (the
    inference context: forward only through the encoder, fc_norm and the classifier still under autograd when grad mode is on)."""
    return "train" if (training and grad_enabled and encoder_trainable) else "encode"


def infer_problem_type(num_labels, labels):
    """transformers' ForSequenceClassificationLoss rule when config.problem_type is None."""
    if num_labels == 1:
        return "regression"
    if num_labels > 1 and labels.dtype in (torch.long, torch.int):
        return "single_label_classification"
    return "multi_label_classification"


def soft_target_cross_entropy(logits, target):
    """mean over b of -sum_k target[b, k] * log_softmax(logits)[b, k]: cross-entropy against soft targets [B, K] (rows summing to 1),
    as Mixup / CutMix with label smoothing produce them."""
    if target.shape != logits.shape:
        raise ValueError(f"soft targets {tuple(target.shape)} must have the logits' shape {tuple(logits.shape)}")
    return torch.sum(-target.to(device=logits.device, dtype=logits.dtype) * nn.functional.log_softmax(logits, dim=-1), dim=-1).mean()


def classification_loss(config, logits, labels):
    """transformers 5.15.0 VideoMAEForVideoClassification.forward -> loss_utils.ForSequenceClassificationLoss: infers
    config.problem_type when it is None and writes it back, then MSE (regression) / cross-entropy with ignore_index -100 /
    BCEWithLogits on the [B, num_labels] logits.  One extension, never inferred: ``config.problem_type ==
    "soft_label_classification"`` is ``soft_target_cross_entropy`` on [B, num_labels] float labels (the targets ``bvc.Mixup`` makes)."""
    num_labels = int(getattr(config, "num_labels", 2))
    if getattr(config, "problem_type", None) is None:
        config.problem_type = infer_problem_type(num_labels, labels)
    labels = labels.to(logits.device)
    if config.problem_type == "regression":
        if num_labels == 1:
            return nn.functional.mse_loss(logits.squeeze(), labels.squeeze())
        return nn.functional.mse_loss(logits, labels)
    if config.problem_type == "single_label_classification":
        return nn.functional.cross_entropy(logits.view(-1, num_labels), labels.view(-1), ignore_index=-100)
    if config.problem_type == "multi_label_classification":
        return nn.functional.binary_cross_entropy_with_logits(logits, labels)
    if config.problem_type == "soft_label_classification":
        return soft_target_cross_entropy(logits, labels)
    raise ValueError(f"problem_type {config.problem_type!r} unknown")


def attentions_nbytes(config, batch):
    """Bytes of ``output_attentions`` for ``batch`` clips: L * B * H * N * N f32 (base size: 1.42 GB per clip)."""
    n = config.seq_length
    return int(config.num_hidden_layers) * int(batch) * int(config.num_attention_heads) * n * n * 4


def hidden_states_nbytes(config, batch):
    """Bytes of ``output_hidden_states`` for ``batch`` clips: (L + 1) * B * N * D f32 (base size: 62.6 MB per clip)."""
    return (int(config.num_hidden_layers) + 1) * int(batch) * config.seq_length * int(config.hidden_size) * 4


def free_device_memory(device):
    """Bytes an allocation on ``device`` can still get: what the driver reports free plus what torch's allocator holds unused."""
    free, _total = torch.cuda.mem_get_info(device)
    return int(free) + int(torch.cuda.memory_reserved(device)) - int(torch.cuda.memory_allocated(device))


def alloc_introspection(config, batch, device, want_hidden, want_attentions):
    """(hidden_states f32 [L + 1, B, N, D] or None, attentions f32 [L, B, H, N, N] or None): one allocation each.  The attention maps
    are large (``attentions_nbytes``), so their size is checked against the free device memory before anything is allocated."""
    hs = att = None
    L, N = int(config.num_hidden_layers), config.seq_length
    if want_attentions:
        need, free = attentions_nbytes(config, batch), free_device_memory(device)
        if need > free:
            raise ValueError(f"output_attentions needs {need} bytes ({need / 2 ** 30:.2f} GiB = layers {L} x clips {batch} x heads "
                             f"{config.num_attention_heads} x {N} x {N} tokens x 4) but {free} bytes of device memory are free: pass "
                             "fewer clips per call")
        att = torch.empty((L, batch, int(config.num_attention_heads), N, N), dtype=torch.float32, device=device)
    if want_hidden:
        hs = torch.empty((L + 1, batch, N, int(config.hidden_size)), dtype=torch.float32, device=device)
    return hs, att


def _mark_detached(ctx, *tensors):
    live = [t for t in tensors if t is not None]
    if live:
        ctx.mark_non_differentiable(*live)


class _TrainCtx:
    """The fine-tuning context of one model.  Owned: destroyed with its holder, and a deepcopy starts without one."""

    def __init__(self):
        self.h, self.key = None, None

    def free(self):
        if self.h is not None:
            _lib.lib().bvc_videomae_cls_destroy(self.h)
            self.h, self.key = None, None

    def __deepcopy__(self, memo):
        return _TrainCtx()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _ClsTrain(torch.autograd.Function):
    """pooled = fc_norm(mean over tokens(encoder(pixels))) on the fine-tuning context; backward fills the encoder's flat gradient
    buffer (views as .grad) and returns fc_norm's gradients to autograd."""

    @staticmethod
    def forward(ctx, anchor, fc_w, fc_b, model, pixels, want_tokens, want_hidden=False, want_attentions=False, mix=None, erase=None):
        ctx.model = model
        pooled, tokens, hs, att = model._run_train_forward(pixels, fc_w, fc_b, want_tokens, want_hidden, want_attentions, mix, erase)
        ctx.stamp = model._stamp_forward()
        _mark_detached(ctx, tokens, hs, att)
        return pooled, tokens, hs, att

    @staticmethod
    def backward(ctx, dpooled, _dtokens, _dhs, _datt):
        ctx.model._check_generation(ctx.stamp)
        dw, db = ctx.model._run_train_backward(dpooled)
        return None, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None, None, None, None, None, None, None, None


class _FcNormProbe(torch.autograd.Function):
    """The inference context's encode (today's call, the same bits) with fc_norm under autograd: the linear-probe case."""

    @staticmethod
    def forward(ctx, fc_w, fc_b, model, pixels, want_tokens, want_hidden=False, want_attentions=False, mix=None, erase=None):
        ctx.model = model
        pooled, tokens, hs, att = model._run_encode(pixels, fc_w, fc_b, want_tokens, want_hidden, want_attentions, mix, erase)
        ctx.stamp = model._stamp_forward()
        ctx.save_for_backward(fc_w)
        _mark_detached(ctx, tokens, hs, att)
        return pooled, tokens, hs, att

    @staticmethod
    def backward(ctx, dpooled, _dtokens, _dhs, _datt):
        ctx.model._check_generation(ctx.stamp)
        (fc_w,) = ctx.saved_tensors
        m = ctx.model
        g = dpooled.detach().to(dtype=torch.float32).contiguous()
        w = fc_w.detach().to(dtype=torch.float32).contiguous()
        dw, db = torch.empty_like(w), torch.empty_like(w)
        _lib.check(_lib.lib().bvc_videomae_encoder_fc_norm_backward(m._ctx, g.data_ptr(), w.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                                                    _lib.current_stream_ptr()), "bvc_videomae_encoder_fc_norm_backward")
        return dw if ctx.needs_input_grad[0] else None, db if ctx.needs_input_grad[1] else None, None, None, None, None, None, None, None


class VideoMAEForVideoClassification(FlatParamModule):
    """Drop-in for transformers.VideoMAEForVideoClassification: the embedding benchmark's inference
    (benchmarks/compute_embeddings_videomae.py:78-96,253-264), a linear probe and full fine-tuning.

    Same sub-module tree / state-dict keys as transformers: ``videomae.embeddings.*``, ``videomae.encoder.*`` (so ``adapt_videomae``'s
    ``target.videomae.embeddings.load_state_dict(source.videomae.embeddings.state_dict())`` works against a pre-training model),
    ``fc_norm.*`` and, for ``num_labels > 0``, ``classifier.*``.  ``forward(pixel_values, labels=None).logits`` = classifier(fc_norm(mean
    over all tokens of the encoder output)); the reference uses ``num_labels=0`` (classifier = Identity), i.e. the logits ARE the
    embedding.  ``labels`` adds transformers' loss (``classification_loss``).

    The encoder (a flat module: its parameters and gradients are views of one buffer each) runs in the library; fc_norm and the
    classifier are ordinary torch modules.  Which context runs (``classification_path``): in train mode with grad mode on and a trainable
    encoder parameter, the fine-tuning context, whose every layer keeps its activations for the backward (about 36 x hidden bytes per
    token and layer: 0.52 GB per clip at base size); otherwise the inference context, forward only through the encoder, with fc_norm's
    gradient from the library's LayerNorm backward when fc_norm is trainable.  Both give the same logits bit for bit.

    ``config.hidden_dropout_prob`` and ``config.drop_path_rate`` gate the two residual branches of every encoder layer whenever the
    module is in train mode - on either context, with or without grad mode, as ``nn.Dropout`` follows ``training`` alone - with draws
    from torch's generator of the device (``torch.manual_seed`` reproduces them; both contexts draw alike, so the two paths still agree
    bit for bit under one seed).  ``drop_path_scale`` / ``dropout_state`` report what the last gated forward used.
    """

    _shadow_fn = "bvc_videomae_cls_shadow"

    def __init__(self, config: VideoMAEConfig):
        super().__init__()
        if not getattr(config, "use_mean_pooling", True):
            raise ValueError("only use_mean_pooling=True (the reference's setting) is implemented")
        if getattr(config, "attention_probs_dropout_prob", 0.0):
            raise ValueError(f"attention_probs_dropout_prob={config.attention_probs_dropout_prob}: dropout on the attention "
                             "probabilities is not implemented (only 0.0)")
        self.config = config
        # the gate on every layer's two residual branches, applied whenever self.training is set (dropgate.py)
        self._gate = BranchGate(config.num_hidden_layers, getattr(config, "drop_path_rate", 0.0), getattr(config, "hidden_dropout_prob", 0.0))
        self.num_labels = int(getattr(config, "num_labels", 2))
        full, _ = param_layout(config)
        cc = config.to_c()
        numel = int(_lib.lib().bvc_videomae_encoder_param_numel(ctypes.byref(cc)))
        layout = [e for e in full if e[0].startswith("videomae.")]
        assert sum(int(torch.Size(e[2]).numel()) for e in layout) == numel
        std = config.initializer_range

        def init(name, shape):
            if len(shape) >= 2:
                return torch.empty(shape).normal_(0.0, std)
            if name.endswith("layernorm_before.weight") or name.endswith("layernorm_after.weight"):
                return torch.ones(shape)
            return torch.zeros(shape)

        self._init_flat(layout, numel, init)
        self.fc_norm = nn.LayerNorm(config.hidden_size)    # as in HF: default eps 1e-5, not config.layer_norm_eps
        self.classifier = nn.Linear(config.hidden_size, self.num_labels) if self.num_labels > 0 else nn.Identity()
        if self.num_labels > 0:
            nn.init.normal_(self.classifier.weight, 0.0, std)
            nn.init.zeros_(self.classifier.bias)
        self._ctx = None
        self._ctx_key = None
        self._train = _TrainCtx()
        self._warned_eval_grad = False
        self.pixel_mean, self.pixel_std = 0.5, 0.25      # for uint8 pixel_values, as in VideoMAEForPreTraining

    # ---- library contexts: _ctx = inference (encode), _train.h = fine-tuning
    def _get_ctx(self, batch):
        key = (batch, self._flat.device.index)
        if self._ctx is not None and self._ctx_key[1] == key[1] and self._ctx_key[0] >= batch:
            return self._ctx
        self._free_ctx()
        h = ctypes.c_void_p()
        cc = self.config.to_c()
        _lib.check(_lib.lib().bvc_videomae_encoder_create(ctypes.byref(cc), batch, ctypes.byref(h)), "bvc_videomae_encoder_create")
        self._ctx, self._ctx_key = h, key
        return h

    def _get_train_ctx(self, batch):
        """Re-created when the device changes or the batch grows (VideoMAEForPreTraining._get_ctx)."""
        t = self._train
        key = (batch, self._flat.device.index)
        if t.h is not None and t.key[1] == key[1] and t.key[0] >= batch:
            return t.h
        t.free()
        h = ctypes.c_void_p()
        cc = self.config.to_c()
        _lib.check(_lib.lib().bvc_videomae_cls_create(ctypes.byref(cc), batch, ctypes.byref(h)), "bvc_videomae_cls_create")
        t.h, t.key = h, key
        return h

    def _shadow_ctx(self):
        return self._train.h

    def __deepcopy__(self, memo):
        # FlatParamModule's copy rebuilds the flat parameters only: fc_norm and the classifier are ordinary sub-modules
        import copy
        new = super().__deepcopy__(memo)
        new.fc_norm = copy.deepcopy(self.fc_norm, memo)
        new.classifier = copy.deepcopy(self.classifier, memo)
        return new

    def _free_ctx(self):
        if self._ctx is not None:
            _lib.lib().bvc_videomae_encoder_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self._free_ctx()
        except Exception:
            pass

    @property
    def drop_path_scale(self):
        """[depth, 2, clips] f32: the stochastic-depth factors of the last train-mode forward (0 = branch dropped for that clip,
        1 / (1 - rate) = kept; branch 0 = attention, 1 = MLP), or None when drop_path_rate is 0."""
        return self._gate.scale

    @property
    def dropout_state(self):
        """(seed, offset, p) of the last train-mode forward's hidden dropout: dropgate.dropout_mask(seed, offset, layer, branch,
        clips * seq_length, hidden_size, p, device) is the keep mask a branch used.  None before the first gated forward."""
        return self._gate.state

    def _arm_gate(self, set_drop, h, B, dev):
        if self.training and self._gate.enabled:
            self._gate.arm(set_drop, h, dev, B, self.config.seq_length)

    def _arm_mix(self, set_mix, h, mix, B):
        """Hand a ClipMix to the context that runs next (``set_mix`` = its bvc_*_set_mix): that forward gathers through it and disarms."""
        if mix is not None:
            _lib.check(set_mix(h, mix.table.data_ptr(), int(B), _lib.current_stream_ptr()), "set_mix")

    def _arm_erase(self, set_erase, h, erase, B):
        """Hand a ClipErase to the context that runs next (``set_erase`` = its bvc_*_set_erase), as ``_arm_mix`` does with a ClipMix."""
        if erase is not None:
            _lib.check(set_erase(h, erase.table.data_ptr(), int(B), erase.num_boxes, erase.seed, erase.offset, _lib.current_stream_ptr()),
                       "set_erase")

    def _encoder_trainable(self):
        return any(self._param(n).requires_grad for n in self._names)

    # ---- the two paths
    def _fc_norm_args(self, fc_w, fc_b, dev):
        return fc_w.detach().to(device=dev, dtype=torch.float32).contiguous(), fc_b.detach().to(device=dev, dtype=torch.float32).contiguous()

    def _run_encode(self, pixels, fc_w, fc_b, want_tokens, want_hidden=False, want_attentions=False, mix=None, erase=None):
        cfg = self.config
        B, dev = pixels.shape[0], pixels.device
        fmt = _lib.pixel_format(pixels, self.pixel_mean, self.pixel_std, cfg.num_channels)
        hs, att = alloc_introspection(cfg, B, dev, want_hidden, want_attentions)
        h = self._get_ctx(B)
        w, b = self._fc_norm_args(fc_w, fc_b, dev)
        pooled = torch.empty((B, cfg.hidden_size), dtype=torch.float32, device=dev)
        tokens = None
        if want_tokens:     # with hidden states the residual stream already ends in the caller's array: its last slot
            tokens = hs[-1] if hs is not None else torch.empty((B, cfg.seq_length, cfg.hidden_size), dtype=torch.float32, device=dev)
        self._arm_gate(_lib.lib().bvc_videomae_encoder_set_drop, h, B, dev)     # train mode on the forward-only path: the same gate
        self._arm_mix(_lib.lib().bvc_videomae_encoder_set_mix, h, mix, B)
        self._arm_erase(_lib.lib().bvc_videomae_encoder_set_erase, h, erase, B)
        args = (h, pixels.data_ptr(), ctypes.byref(fmt) if fmt is not None else None, B, self._flat.data_ptr(), w.data_ptr(), b.data_ptr(),
                float(self.fc_norm.eps), tokens.data_ptr() if tokens is not None and hs is None else None, pooled.data_ptr())
        out = _lib.introspect(hs, att)
        if out is None:
            _lib.check(_lib.lib().bvc_videomae_encode_px(*args, _lib.current_stream_ptr()), "bvc_videomae_encode")
        else:
            _lib.check(_lib.lib().bvc_videomae_encode_ex(*args, ctypes.byref(out), _lib.current_stream_ptr()), "bvc_videomae_encode_ex")
        return pooled, tokens, hs, att

    def _run_train_forward(self, pixels, fc_w, fc_b, want_tokens, want_hidden=False, want_attentions=False, mix=None, erase=None):
        cfg = self.config
        B, dev = pixels.shape[0], pixels.device
        fmt = _lib.pixel_format(pixels, self.pixel_mean, self.pixel_std, cfg.num_channels)
        hs, att = alloc_introspection(cfg, B, dev, want_hidden, want_attentions)
        h = self._get_train_ctx(B)
        w, b = self._fc_norm_args(fc_w, fc_b, dev)
        pooled = torch.empty((B, cfg.hidden_size), dtype=torch.float32, device=dev)
        tokens = torch.empty((B, cfg.seq_length, cfg.hidden_size), dtype=torch.float32, device=dev) if want_tokens else None
        self._shadow_vouch(h)
        self._arm_gate(_lib.lib().bvc_videomae_cls_set_drop, h, B, dev)
        self._arm_mix(_lib.lib().bvc_videomae_cls_set_mix, h, mix, B)
        self._arm_erase(_lib.lib().bvc_videomae_cls_set_erase, h, erase, B)
        _lib.check(_lib.lib().bvc_videomae_cls_forward_px(
            h, pixels.data_ptr(), ctypes.byref(fmt) if fmt is not None else None, B, self._flat.data_ptr(), w.data_ptr(), b.data_ptr(),
            float(self.fc_norm.eps), pooled.data_ptr(), tokens.data_ptr() if tokens is not None else None, _lib.current_stream_ptr()),
            "bvc_videomae_cls_forward")
        self._shadow_established(h)
        self._live = pixels       # keep the borrowed input alive until backward
        out = _lib.introspect(hs, att)
        if out is not None:       # what every layer kept for the backward: its input, and the qkv / lse its attention ran on
            _lib.check(_lib.lib().bvc_videomae_cls_introspect(h, ctypes.byref(out), _lib.current_stream_ptr()), "bvc_videomae_cls_introspect")
        return pooled, tokens, hs, att

    def _run_train_backward(self, dpooled):
        target, accumulate = self._grad_target()
        g = dpooled.detach().to(dtype=torch.float32).contiguous()
        dw = torch.empty(self.config.hidden_size, dtype=torch.float32, device=g.device)
        db = torch.empty_like(dw)
        cb = self._bucket_callback(accumulate)
        self._library_backward("bvc_videomae_cls_backward", _lib.lib().bvc_videomae_cls_backward(
            self._train.h, g.data_ptr(), target.data_ptr(), dw.data_ptr(), db.data_ptr(), cb, None, _lib.current_stream_ptr()))
        self._publish_grads(target, accumulate)
        self._live = None
        return dw.to(self.fc_norm.weight.dtype), db.to(self.fc_norm.bias.dtype)

    def forward(self, pixel_values=None, labels=None, output_last_hidden_state=False, output_hidden_states=None, output_attentions=None,
                mix=None, erase=None, **kwargs):
        """``output_hidden_states`` / ``output_attentions`` (None = ``config.output_hidden_states`` / ``config.output_attentions``, as in
        transformers): ``hidden_states`` is a tuple of L + 1 tensors (B, N, D) - the embedding output, then every layer's output -
        and ``attentions`` a tuple of L tensors (B, H, N, N) of softmax probabilities (row = query).  Each tuple is f32 views of one
        allocation; ``attentions`` takes ``attentions_nbytes(config, B)`` bytes and the call raises ValueError before allocating when
        that exceeds the free device memory.  Unlike transformers', both are detached (no gradient flows through them, as through
        ``last_hidden_state``).  They are those of the forward that ran: in train mode they include the drop-path / dropout gates.
        The logits are the same bits with or without them.

        ``mix`` (a ``ClipMix`` from ``bvc.Mixup``, train mode only): the clips enter the patch embedding mixed with their partners
        (Mixup / CutMix inside the patch gather, uint8 or f32 input; nothing is written back and ``pixel_values`` is untouched).
        It serves this forward alone.  Pass the soft targets that came with it as ``labels`` under
        ``config.problem_type = "soft_label_classification"``.  A table entry out of range makes the logits NaN.

        ``erase`` (a ``ClipErase`` from ``bvc.RandomErasing``, train mode only): the clips enter the patch embedding with their boxes
        erased (random erasing inside the patch gather, uint8 or f32 input; nothing is written back).  With ``mix`` as well each clip
        is erased first and the batch is mixed then.  It serves this forward alone, and a bad table entry makes the logits NaN."""
        if mix is not None and not self.training:
            raise ValueError("mix= in eval mode: evaluating on mixed clips is a mistake (call .train(), or pass mix=None)")
        if erase is not None and not self.training:
            raise ValueError("erase= in eval mode: evaluating on erased clips is a mistake (call .train(), or pass erase=None)")
        if erase is not None and pixel_values is not None and erase.batch_size != pixel_values.shape[0]:
            raise ValueError(f"erase was built for a batch of {erase.batch_size} clips, pixel_values holds {pixel_values.shape[0]}")
        if pixel_values is None or not pixel_values.is_cuda:
            raise _lib.BvcError("VideoMAEForVideoClassification runs on a GPU only (libbvc_hip.so has no CPU path)")
        cfg = self.config
        want_hs = bool(getattr(cfg, "output_hidden_states", False) if output_hidden_states is None else output_hidden_states)
        want_att = bool(getattr(cfg, "output_attentions", False) if output_attentions is None else output_attentions)
        B, T, C, H, W = pixel_values.shape
        if C != cfg.num_channels or H != cfg.image_size or W != cfg.image_size or T != cfg.num_frames:
            raise ValueError(f"Input size ({T}x{C}x{H}*{W}) doesn't match model ({cfg.num_frames}x{cfg.num_channels}x{cfg.image_size}*{cfg.image_size}).")
        dev = pixel_values.device
        if mix is not None:
            if mix.batch_size != B:
                raise ValueError(f"mix was built for a batch of {mix.batch_size} clips, pixel_values holds {B}")
            if mix.table is None or mix.table.device != dev:
                raise ValueError(f"mix has no device table on {dev}: build it with device=pixel_values.device")
        if erase is not None and (erase.table is None or erase.table.device != dev):
            raise ValueError(f"erase has no device table on {dev}: build it with device=pixel_values.device")
        self._ensure_flat(dev)
        pixels = pixel_values.detach()
        pixels = (pixels if pixels.dtype == torch.uint8 else pixels.to(dtype=torch.float32)).contiguous()
        grad = torch.is_grad_enabled()
        trainable = self._encoder_trainable()
        fc_w, fc_b = self.fc_norm.weight, self.fc_norm.bias
        if classification_path(self.training, grad, trainable) == "train":
            anchor = next(self._param(n) for n in self._names if self._param(n).requires_grad)
            pooled, tokens, hs, att = _ClsTrain.apply(anchor, fc_w, fc_b, self, pixels, output_last_hidden_state, want_hs, want_att, mix, erase)
        else:
            if grad and trainable and not self._warned_eval_grad:
                self._warned_eval_grad = True
                warnings.warn("VideoMAEForVideoClassification in eval mode: the encoder receives no gradient (call .train() to "
                              "fine-tune it); fc_norm and the classifier still do", stacklevel=2)
            if grad and (fc_w.requires_grad or fc_b.requires_grad):
                pooled, tokens, hs, att = _FcNormProbe.apply(fc_w, fc_b, self, pixels, output_last_hidden_state, want_hs, want_att, mix, erase)
            else:
                with torch.no_grad():
                    pooled, tokens, hs, att = self._run_encode(pixels, fc_w, fc_b, output_last_hidden_state, want_hs, want_att, mix, erase)
                self._stamp_forward()     # a pending backward of an earlier forward must not run on overwritten state
        logits = self.classifier(pooled)
        loss = classification_loss(cfg, logits, labels) if labels is not None else None
        return ImageClassifierOutput(loss=loss, logits=logits, last_hidden_state=tokens,
                                     hidden_states=tuple(hs.unbind(0)) if hs is not None else None,
                                     attentions=tuple(att.unbind(0)) if att is not None else None)


# The VideoMAE (v1) pre-training shapes: (hidden, layers, heads, decoder hidden, decoder heads).  All use patch 16, tubelet 2,
# decoder depth 4, MLP ratio 4 and norm_pix_loss=True; 'base' is exactly get_config's.  Heads are 64 wide except huge's 80 (1280 / 16
# in the encoder, 640 / 8 in the decoder), which the attention kernels run in place.
VIDEOMAE_ARCHS = {
    "small": (384, 12, 6, 192, 3),
    "base": (768, 12, 12, 384, 6),
    "large": (1024, 24, 16, 512, 8),
    "huge": (1280, 32, 16, 640, 8),
}


def videomae_config(architecture="base", **overrides):
    """VideoMAEConfig of one VIDEOMAE_ARCHS entry at 16 frames of 224^2; keyword overrides (num_frames, image_size, a reduced
    num_hidden_layers, ...) replace single fields.  The MLP widths follow the hidden sizes unless overridden too."""
    if architecture not in VIDEOMAE_ARCHS:
        raise ValueError(f"architecture {architecture!r} not in {sorted(VIDEOMAE_ARCHS)}")
    D, depth, heads, Dd, Hd = VIDEOMAE_ARCHS[architecture]
    kw = dict(image_size=224, patch_size=16, num_channels=3, num_frames=16, tubelet_size=2, hidden_size=D, num_hidden_layers=depth,
              num_attention_heads=heads, initializer_range=0.02, use_mean_pooling=True, decoder_num_attention_heads=Hd,
              decoder_hidden_size=Dd, decoder_num_hidden_layers=4, norm_pix_loss=True)
    kw.update(overrides)
    kw.setdefault("intermediate_size", 4 * kw["hidden_size"])
    kw.setdefault("decoder_intermediate_size", 4 * kw["decoder_hidden_size"])
    return VideoMAEConfig(**kw)


def get_config(image_size, args):
    """pretrain_videomae.py:43-58 (only architecture='base' exists in the reference; videomae_config builds the other sizes)."""
    if getattr(args, "architecture", "base") != "base":
        raise ValueError("only architecture='base' is defined by the reference")
    return VideoMAEConfig(image_size=image_size, patch_size=16, num_channels=3, num_frames=args.num_frames,
                          tubelet_size=args.tubelet_size, hidden_size=768, num_hidden_layers=12,
                          num_attention_heads=12, intermediate_size=3072, initializer_range=0.02,
                          use_mean_pooling=True, decoder_num_attention_heads=6, decoder_hidden_size=384,
                          decoder_num_hidden_layers=4, decoder_intermediate_size=1536, norm_pix_loss=True)


def get_model(image_size, args):
    """pretrain_videomae.py:61-64"""
    return VideoMAEForPreTraining(get_config(image_size, args))
