"""References for the per-layer outputs (output_hidden_states / output_attentions) and for bvc_op_attention_probs  --  TEST
INFRASTRUCTURE ONLY.  Pinned on the CPU by tests/test_introspection_ref.py; used by tests/test_gpu_attention_probs.py (the op) and
tests/test_gpu_videomae_introspect.py (the model).  Nothing here touches the library.

Two levels, each with an exact reference and a rounding model whose distance from it is the error that correct arithmetic at the
library's precision produces (the per-row bars of the GPU tests are multiples of that distance, as in tests/attention_ref.py):

  the op      probs_reference   float64 softmax(q k^T scale) of the bf16 operands, [B][H][N][N]
              probs_model       float32 exp2(s2 - lse2) with s2 = (q k^T) * (scale * log2 e) and lse2 the float32 log2-sum-exp2 of s2:
                                what the kernel evaluates, with torch's exp2 / log2 in place of v_exp_f32 / the forward's lse

  the model   encoder_states        the encoder of oracle.videomae_oracle.encode, returning every hidden state ('embed', then each
                                    layer's output) and every layer's attention probabilities, in float64 (or any dtype)
              layer_attention       one layer's probabilities from a given layer input (float64): lets a test factor the upstream
                                    error out by starting from the hidden state the GPU returned
              layer_attention_bf16  the same under the library's operand policy: LayerNorm output, weights and qkv rounded to bf16,
                                    float32 accumulation, float32 softmax
              encoder_states_bf16   the whole encoder under that policy (oracle.videomae_oracle_bf16's layer pieces), for
                                    comparisons that cannot factor the upstream error out (the committed transformers fixture)
"""
import math

import torch
import torch.nn.functional as F

from oracle import videomae_oracle as vo
from oracle import videomae_oracle_bf16 as vb
from tests import attention_ref as R

LOG2E = math.log2(math.e)


# --------------------------------------------------------------------------- the op
def probs_reference(qkv, B, N, H, HD, scale=None):
    """float64 softmax(q k^T scale) of the bf16-rounded operands, [B][H][N][N], on the device of `qkv`."""
    scale = HD ** -0.5 if scale is None else float(scale)
    q, k, _ = R._split(qkv.to(torch.bfloat16), B, N, H, HD, torch.float64)
    return torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)


def probs_model(qkv, B, N, H, HD, scale=None):
    """float32 exp2(s2 - lse2), [B][H][N][N]: the kernel's formula with its lse input at float32 precision."""
    scale = HD ** -0.5 if scale is None else float(scale)
    q, k, _ = R._split(qkv.to(torch.bfloat16), B, N, H, HD, torch.float32)
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    s2 = (q @ k.transpose(-1, -2)) * c.to(q.device)
    m = s2.amax(dim=-1, keepdim=True)
    lse2 = m + torch.log2(torch.exp2(s2 - m).sum(dim=-1, keepdim=True))
    return torch.exp2(s2 - lse2)


# --------------------------------------------------------------------------- the model
def _cast(p, dtype):
    return {k: v.to(dtype) for k, v in p.items() if k.startswith("videomae.")}


def embed(cfg, p, pixels):
    """Patch embedding + position table (hidden state 0), in the dtype of `p`."""
    dt = p["videomae.embeddings.patch_embeddings.projection.weight"].dtype
    x = F.conv3d(pixels.to(dt).permute(0, 2, 1, 3, 4), p["videomae.embeddings.patch_embeddings.projection.weight"],
                 p["videomae.embeddings.patch_embeddings.projection.bias"],
                 stride=(cfg.tubelet_size, cfg.patch_size, cfg.patch_size)).flatten(2).transpose(1, 2)
    return x + vo.sinusoid_table(cfg.seq_len, cfg.hidden_size).to(dt)[None]


def _qk(x, p, prefix, heads, eps):
    B, N, D = x.shape
    d = D // heads
    a = prefix + "attention.attention."
    h = F.layer_norm(x, (D,), p[prefix + "layernorm_before.weight"], p[prefix + "layernorm_before.bias"], eps)
    q = F.linear(h, p[a + "query.weight"], p[a + "query.bias"]).view(B, N, heads, d).transpose(1, 2)
    k = F.linear(h, p[a + "key.weight"], p[a + "key.bias"]).view(B, N, heads, d).transpose(1, 2)
    return h, q, k


def _layer(x, p, prefix, heads, eps):
    """vo._layer, returning (layer output, attention probabilities)."""
    B, N, D = x.shape
    d = D // heads
    h, q, k = _qk(x, p, prefix, heads, eps)
    a = prefix + "attention.attention."
    v = F.linear(h, p[a + "value.weight"], p[a + "value.bias"]).view(B, N, heads, d).transpose(1, 2)
    pr = torch.softmax(torch.matmul(q, k.transpose(2, 3)) * (d ** -0.5), dim=-1)
    ctx = torch.matmul(pr, v).transpose(1, 2).reshape(B, N, D)
    x = x + F.linear(ctx, p[prefix + "attention.output.dense.weight"], p[prefix + "attention.output.dense.bias"])
    h = F.layer_norm(x, (D,), p[prefix + "layernorm_after.weight"], p[prefix + "layernorm_after.bias"], eps)
    h = F.gelu(F.linear(h, p[prefix + "intermediate.dense.weight"], p[prefix + "intermediate.dense.bias"]))
    return x + F.linear(h, p[prefix + "output.dense.weight"], p[prefix + "output.dense.bias"]), pr


def encoder_states(cfg, params, pixels, dtype=torch.float64):
    """(hidden_states: L + 1 tensors [B][N][D], attentions: L tensors [B][H][N][N]) of the classification model's encoder."""
    p = _cast(params, dtype)
    x = embed(cfg, p, pixels)
    hs, att = [x], []
    for i in range(cfg.num_hidden_layers):
        x, pr = _layer(x, p, f"videomae.encoder.layer.{i}.", cfg.num_attention_heads, cfg.layer_norm_eps)
        hs.append(x)
        att.append(pr)
    return hs, att


def layer_attention(cfg, params, i, x, dtype=torch.float64):
    """Layer i's attention probabilities [B][H][N][N] from its input x [B][N][D], everything in `dtype`."""
    p = _cast(params, dtype)
    heads = cfg.num_attention_heads
    _, q, k = _qk(x.to(dtype), p, f"videomae.encoder.layer.{i}.", heads, cfg.layer_norm_eps)
    return torch.softmax(torch.matmul(q, k.transpose(2, 3)) * ((cfg.hidden_size // heads) ** -0.5), dim=-1)


def _qk_bf16(x, p, prefix, heads, eps):
    B, N, D = x.shape
    d = D // heads
    a = prefix + "attention.attention."
    h = F.layer_norm(x, (D,), p[prefix + "layernorm_before.weight"], p[prefix + "layernorm_before.bias"], eps)

    def proj(nm):      # r(LN) r(W)^T + b accumulated in float32, stored as bf16
        return vb._r(vb.linear(h, p[a + nm + ".weight"], p[a + nm + ".bias"], vb.BUILD)).view(B, N, heads, d).transpose(1, 2)
    return proj("query"), proj("key")


def layer_attention_bf16(cfg, params, i, x):
    """The rounding model of layer i's probabilities from the float32 layer input x: LayerNorm output, weights and qkv rounded to
    bf16, float32 accumulation and softmax."""
    p = _cast(params, torch.float32)
    heads = cfg.num_attention_heads
    q, k = _qk_bf16(x.float(), p, f"videomae.encoder.layer.{i}.", heads, cfg.layer_norm_eps)
    return torch.softmax(torch.matmul(q, k.transpose(2, 3)) * ((cfg.hidden_size // heads) ** -0.5), dim=-1)


def encoder_states_bf16(cfg, params, pixels):
    """encoder_states under the library's operand policy (vb.BUILD) end to end, float32 results."""
    p = _cast(params, torch.float32)
    B = pixels.shape[0]
    D, L, ts, ps = cfg.hidden_size, cfg.seq_len, cfg.tubelet_size, cfg.patch_size
    T, C, Hh, Ww = pixels.shape[1:]
    patches = pixels.float().permute(0, 2, 1, 3, 4).reshape(B, C, T // ts, ts, Hh // ps, ps, Ww // ps, ps)
    patches = patches.permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, L, C * ts * ps * ps)
    x = vb.linear(patches, p["videomae.embeddings.patch_embeddings.projection.weight"].reshape(D, -1),
                  p["videomae.embeddings.patch_embeddings.projection.bias"], vb.BUILD)
    x = x + vo.sinusoid_table(L, D)[None]
    hs, att = [x], []
    heads = cfg.num_attention_heads
    for i in range(cfg.num_hidden_layers):
        prefix = f"videomae.encoder.layer.{i}."
        q, k = _qk_bf16(x, p, prefix, heads, cfg.layer_norm_eps)
        att.append(torch.softmax(torch.matmul(q, k.transpose(2, 3)) * ((D // heads) ** -0.5), dim=-1))
        x = vb._layer(x, p, prefix, heads, cfg.layer_norm_eps, vb.BUILD, None, "")
        hs.append(x)
    return hs, att


# --------------------------------------------------------------------------- the committed transformers fixture
FIXTURE = "videomae_introspect_tiny.json"
FIXTURE_ROWS = (0, 21)      # the token rows (queries) the fixture keeps in full, of every clip (and head)


def fixture_view(hs, att):
    """What tools/make_introspection_golden.py stores of a (hidden_states, attentions) pair, as nested lists of floats:
    hidden_norm [L + 1], attention_norm [L][H], hidden_rows [L + 1][B][len(FIXTURE_ROWS)][D],
    attention_rows [L][B][H][len(FIXTURE_ROWS)][N]."""
    rows = list(FIXTURE_ROWS)
    return dict(
        hidden_norm=[float(h.double().norm()) for h in hs],
        attention_norm=[[float(a[:, j].double().norm()) for j in range(a.shape[1])] for a in att],
        hidden_rows=[h[:, rows].double().tolist() for h in hs],
        attention_rows=[a[:, :, rows].double().tolist() for a in att],
    )
