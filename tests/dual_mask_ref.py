"""fp32 plain-torch reference for the VideoMAE pre-training step with a decoder subset  --  TEST INFRASTRUCTURE ONLY.

VideoMAE V2's decoder masking (Wang et al., CVPR 2023, section 3.2): the encoder sees the tokens `~mask` as always, the decoder
gets mask-token rows only for the tokens `dec` (a subset of `mask`, the same count in every clip) and the loss is the MSE on those.
Built from oracle.videomae_oracle (`_layer`, `sinusoid_table`, `pixel_labels`): `vo.forward` with `pos[dec]` for the mask-token
rows and `pixel_labels(cfg, pixels, dec)` for the targets.  tests/test_dual_mask_ref.py pins this file to `vo.step` (dec == mask:
bit for bit) and to transformers' own modules composed by hand (a strict subset) before any GPU test relies on it.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import videomae_oracle as vo


def forward(cfg, p, pixel_values, bool_masked_pos, bool_decode_pos, taps=None):
    """Returns (loss, logits [B, ndec, P], labels).  `taps` as in vo.forward; 'x_full' / 'dec<i>' have nvis + ndec rows per clip."""
    B = pixel_values.shape[0]
    D, Dd, L = cfg.hidden_size, cfg.decoder_hidden_size, cfg.seq_len
    x = F.conv3d(pixel_values.permute(0, 2, 1, 3, 4), p["videomae.embeddings.patch_embeddings.projection.weight"],
                 p["videomae.embeddings.patch_embeddings.projection.bias"],
                 stride=(cfg.tubelet_size, cfg.patch_size, cfg.patch_size))
    x = x.flatten(2).transpose(1, 2)
    x = x + vo.sinusoid_table(L, D)[None]
    x = x[~bool_masked_pos].reshape(B, -1, D)
    if taps is not None:
        taps["embed"] = x
    for i in range(cfg.num_hidden_layers):
        x = vo._layer(x, p, f"videomae.encoder.layer.{i}.", cfg.num_attention_heads, cfg.layer_norm_eps, taps, f"enc{i}")
    x = F.linear(x, p["encoder_to_decoder.weight"])
    pos = vo.sinusoid_table(L, Dd)[None].expand(B, -1, -1)
    pos_vis = pos[~bool_masked_pos].reshape(B, -1, Dd)
    pos_dec = pos[bool_decode_pos].reshape(B, -1, Dd)
    x = torch.cat([x + pos_vis, p["mask_token"] + pos_dec], dim=1)
    if taps is not None:
        taps["x_full"] = x
    for i in range(cfg.decoder_num_hidden_layers):
        x = vo._layer(x, p, f"decoder.decoder_layers.{i}.", cfg.decoder_num_attention_heads, cfg.layer_norm_eps, taps, f"dec{i}")
    n_dec = pos_dec.shape[1]
    x = x[:, -n_dec:]
    x = F.layer_norm(x, (Dd,), p["decoder.norm.weight"], p["decoder.norm.bias"], cfg.decoder_norm_eps)
    logits = F.linear(x, p["decoder.head.weight"], p["decoder.head.bias"])
    with torch.no_grad():
        labels = vo.pixel_labels(cfg, pixel_values, bool_decode_pos)
    loss = F.mse_loss(logits, labels)
    if taps is not None:
        taps["logits"] = logits
        taps["labels"] = labels
    return loss, logits, labels


def step(cfg, params, pixel_values, bool_masked_pos, bool_decode_pos, grad_scale=1.0, taps=None):
    """Forward + backward of one batch, as vo.step: (loss, grads dict multiplied by grad_scale)."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    loss, _, _ = forward(cfg, p, pixel_values, bool_masked_pos, bool_decode_pos, taps)
    (loss * grad_scale).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}
    return loss.detach(), grads


def every_second(mask):
    """[B, L] bool: every second masked token of each clip (the 1st, 3rd, ... in token order)."""
    rank = torch.cumsum(mask.to(torch.int64), dim=1) - 1
    return mask & (rank % 2 == 0)


def per_slot_subset(cfg, mask, keep, seed):
    """[B, L] bool: `keep` of every temporal slot's masked positions, a fresh seeded draw per clip and slot."""
    rng = np.random.RandomState(seed)
    slots = cfg.grid[0]
    m = mask.numpy().reshape(mask.shape[0], slots, -1)
    out = np.zeros_like(m)
    for b in range(m.shape[0]):
        for t in range(slots):
            pos = np.flatnonzero(m[b, t])
            out[b, t, rng.permutation(pos)[:keep]] = True
    return torch.from_numpy(out.reshape(mask.shape[0], -1))
