"""fp32 plain-torch reference for the gated pre-LN stacks  --  TEST INFRASTRUCTURE ONLY.

One gated layer is
    h     = x + g1 * (proj(attention(LN1(x))) + b_o)
    x_out = h + g2 * (fc2(gelu(fc1(LN2(h)))) + b_2)
with the gates g1 / g2 given as INPUTS (anything broadcastable to (B, N, D), or None for 1): stochastic depth is a per-sample
factor 0 or 1 / (1 - rate) (drop_path, pretraining/predictive/vision_transformer.py:145-153), hidden dropout an element mask
divided by 1 - p (nn.Dropout on VideoMAESelfOutput / VideoMAEOutput, modeling_videomae.py:270-274, 316-320).  `oracle/` restates the
same stacks without gates; tests/test_dropout_ref.py pins this file to it (all gates one), to transformers (hidden dropout) and to
the reference's own vision_transformer.py (drop path, tests/golden/jepa_droppath.json) before any GPU test relies on it.

`gates` everywhere: a list with one (g1, g2) pair per layer, or None.
"""
import torch
import torch.nn.functional as F

from oracle import jepa_oracle as jo
from oracle import videomae_oracle as vo


def _attention(q, k, v):
    d = q.shape[-1]
    return torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-2, -1)) * d ** -0.5, dim=-1), v)


def _gate(branch, g):
    return branch if g is None else branch * g


def videomae_layer(x, p, prefix, heads, eps, g1=None, g2=None):
    """transformers' VideoMAELayer (HF key names) with gated branches."""
    B, N, D = x.shape
    d = D // heads
    a = prefix + "attention.attention."
    h = F.layer_norm(x, (D,), p[prefix + "layernorm_before.weight"], p[prefix + "layernorm_before.bias"], eps)
    q, k, v = (F.linear(h, p[a + n + ".weight"], p[a + n + ".bias"]).view(B, N, heads, d).transpose(1, 2) for n in ("query", "key", "value"))
    ctx = _attention(q, k, v).transpose(1, 2).reshape(B, N, D)
    x = x + _gate(F.linear(ctx, p[prefix + "attention.output.dense.weight"], p[prefix + "attention.output.dense.bias"]), g1)
    h = F.layer_norm(x, (D,), p[prefix + "layernorm_after.weight"], p[prefix + "layernorm_after.bias"], eps)
    h = F.gelu(F.linear(h, p[prefix + "intermediate.dense.weight"], p[prefix + "intermediate.dense.bias"]))
    return x + _gate(F.linear(h, p[prefix + "output.dense.weight"], p[prefix + "output.dense.bias"]), g2)


def jepa_block(x, p, prefix, heads, eps, g1=None, g2=None):
    """Block of vision_transformer.py:213-231 (JEPA key names) with gated branches."""
    B, N, D = x.shape
    d = D // heads
    h = F.layer_norm(x, (D,), p[prefix + "norm1.weight"], p[prefix + "norm1.bias"], eps)
    qkv = F.linear(h, p[prefix + "attn.qkv.weight"], p[prefix + "attn.qkv.bias"]).reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    y = _attention(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(B, N, D)
    x = x + _gate(F.linear(y, p[prefix + "attn.proj.weight"], p[prefix + "attn.proj.bias"]), g1)
    h = F.layer_norm(x, (D,), p[prefix + "norm2.weight"], p[prefix + "norm2.bias"], eps)
    h = F.gelu(F.linear(h, p[prefix + "mlp.fc1.weight"], p[prefix + "mlp.fc1.bias"]))
    return x + _gate(F.linear(h, p[prefix + "mlp.fc2.weight"], p[prefix + "mlp.fc2.bias"]), g2)


def _pair(gates, i):
    return (None, None) if gates is None else gates[i]


def videomae_encode(cfg, p, pixel_values, fc_norm_w=None, fc_norm_b=None, fc_norm_eps=1e-5, gates=None):
    """vo.encode with gated encoder layers: (pooled (B, hidden), last_hidden_state (B, L, hidden))."""
    D, L = cfg.hidden_size, cfg.seq_len
    x = F.conv3d(pixel_values.permute(0, 2, 1, 3, 4), p["videomae.embeddings.patch_embeddings.projection.weight"],
                 p["videomae.embeddings.patch_embeddings.projection.bias"],
                 stride=(cfg.tubelet_size, cfg.patch_size, cfg.patch_size)).flatten(2).transpose(1, 2)
    x = x + vo.sinusoid_table(L, D)[None]
    for i in range(cfg.num_hidden_layers):
        x = videomae_layer(x, p, f"videomae.encoder.layer.{i}.", cfg.num_attention_heads, cfg.layer_norm_eps, *_pair(gates, i))
    pooled = x.mean(1)
    if fc_norm_w is not None:
        pooled = F.layer_norm(pooled, (D,), fc_norm_w, fc_norm_b, fc_norm_eps)
    return pooled, x


def cls_step(cfg, params, heads, pixel_values, loss_fn, gates=None):
    """One classification step under autograd: (loss, logits, {name: grad}) - the `_oracle` of tests/test_gpu_videomae_cls.py, gated."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in params.items() if k.startswith("videomae.")}
    p.update({k: v.detach().clone().requires_grad_(True) for k, v in heads.items()})
    pooled, _ = videomae_encode(cfg, p, pixel_values, p["fc_norm.weight"], p["fc_norm.bias"], 1e-5, gates)
    logits = F.linear(pooled, p["classifier.weight"], p["classifier.bias"])
    loss = loss_fn(logits)
    loss.backward()
    return loss.detach(), logits.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}


def jepa_encoder_forward(cfg, p, imgs, masks=None, gates=None):
    x = F.conv3d(imgs.permute(0, 2, 1, 3, 4), p["patch_embed.proj.weight"], p["patch_embed.proj.bias"],
                 stride=(cfg.tubelet_size, cfg.patch_size, cfg.patch_size)).flatten(2).transpose(1, 2)
    x = x + p["pos_embed"]
    if masks is not None:
        x = jo.apply_masks(x, masks)
    for i in range(cfg.depth):
        x = jepa_block(x, p, f"blocks.{i}.", cfg.num_heads, cfg.eps, *_pair(gates, i))
    return F.layer_norm(x, (cfg.embed_dim,), p["norm.weight"], p["norm.bias"], cfg.eps)


def jepa_predictor_forward(cfg, p, x, masks_x, masks, gates=None):
    B = len(x) // len(masks_x)
    x = F.linear(x, p["predictor_embed.weight"], p["predictor_embed.bias"])
    x = x + jo.apply_masks(p["predictor_pos_embed"].repeat(B, 1, 1), masks_x)
    n_ctx = x.shape[1]
    pos = jo.repeat_interleave_batch(jo.apply_masks(p["predictor_pos_embed"].repeat(B, 1, 1), masks), B, repeat=len(masks_x))
    pred = p["mask_token"].repeat(pos.size(0), pos.size(1), 1) + pos
    x = torch.cat([x.repeat(len(masks), 1, 1), pred], dim=1)
    for i in range(cfg.pred_depth):
        x = jepa_block(x, p, f"predictor_blocks.{i}.", cfg.num_heads, cfg.eps, *_pair(gates, i))
    x = F.layer_norm(x, (cfg.pred_dim,), p["predictor_norm.weight"], p["predictor_norm.bias"], cfg.eps)
    return F.linear(x[:, n_ctx:], p["predictor_proj.weight"], p["predictor_proj.bias"])


def jepa_step(cfg, enc_p, pred_p, tgt_p, imgs, masks_enc, masks_pred, enc_gates=None, pred_gates=None, grad_scale=1.0):
    """jo.step with gated encoder / predictor (the target encoder ungated): (loss, encoder grads, predictor grads, z, h)."""
    ep = {k: v.detach().clone().requires_grad_(k != "pos_embed") for k, v in enc_p.items()}
    pp = {k: v.detach().clone().requires_grad_(k != "predictor_pos_embed") for k, v in pred_p.items()}
    h = jo.targets(cfg, tgt_p, imgs, masks_enc, masks_pred)
    z = jepa_predictor_forward(cfg, pp, jepa_encoder_forward(cfg, ep, imgs, masks_enc, enc_gates), masks_enc, masks_pred, pred_gates)
    loss = F.smooth_l1_loss(z, h)
    (loss * grad_scale).backward()
    ge = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in ep.items()}
    gp = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in pp.items()}
    return loss.detach(), ge, gp, z.detach(), h


def make_gates(depth, samples, rows, width, scale=None, mask_fn=None, p=0.0):
    """[(g1, g2)] per layer from what a model reports: scale = drop_path_scale [depth, 2, samples] (or None), mask_fn(layer, branch)
    = the keep mask [samples * rows, width] (uint8 / bool, or None), p = the hidden dropout probability."""
    out = []
    for layer in range(depth):
        pair = []
        for branch in (0, 1):
            g = torch.ones((samples, 1, 1), dtype=torch.float32)
            if scale is not None:
                g = g * scale[layer, branch].detach().float().cpu().view(samples, 1, 1)
            if mask_fn is not None:
                g = g * mask_fn(layer, branch).cpu().view(samples, rows, width).float() / (1.0 - p)
            pair.append(g)
        out.append(tuple(pair))
    return out


def scale_exercised(scale, rates, one_sample_mlp=False):
    """Does a reported drop_path_scale hold both a zero and a nonzero entry among the layers with a nonzero rate (for a one-sample
    case: a zero in an MLP branch)?  What the GPU tests ask of the seed they run on."""
    rows = [scale[i] for i, r in enumerate(rates) if r > 0]
    if not rows:
        return False
    s = torch.stack(rows).detach().cpu()
    if one_sample_mlp:
        return bool((s[:, 1] == 0).any())
    return bool((s == 0).any() and (s != 0).any())
