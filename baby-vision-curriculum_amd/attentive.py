"""Attentive probe: one learned query token cross-attends the frozen encoder's tokens, then a linear classifier.

The pooler is a cross-attention block (LayerNorm, q / kv / proj linears, ``H`` heads, optional norm2 + GELU MLP).  Because the query
is a parameter and not data, LayerNorm's affine, the K projection and the query fold into ``U [H][D]``, and the V projection moves
behind the softmax sum (DESIGN.md "Attentive pooling"):

    u_h   = scale * gamma o (Wk_h^T q_h)                         q = Wq t + bq
    Ph_h  = sum_j softmax_j(xh_j . u_h) xh_j                     xh_j = the standardised token row   (attentive_pool, HIP)
    out_h = Wv_h (gamma o Ph_h + beta) + bv_h

so the only work on ``[B][N][D]`` is ``attentive_pool`` (bvc_op_attn_pool_fwd / _bwd, csrc/attnpool.hip): one streaming pass over the
tokens forward and one backward, no K or V array.  Everything else is f32 torch algebra on ``[H][D]``, ``[D][D]`` and ``[B][D]``
tensors under autograd.  The state-dict names (``pooler.query_tokens``, ``pooler.cross_attention_block.xattn.kv.weight`` ..,
``linear.weight``) are this project's own definition.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

MAX_QUERIES = 16


def _token_rows(x):
    """f32 [B][N][D] with dense columns, clip stride N * row stride, a row stride that is a multiple of 4 and a 16-byte base."""
    B, N, D = x.shape
    ok = x.stride(2) == 1 and x.stride(1) >= D and x.stride(1) % 4 == 0 and x.stride(0) == N * x.stride(1) and x.data_ptr() % 16 == 0
    if not ok:
        x = x.contiguous()
        if x.data_ptr() % 16:
            x = x.clone()
    return x, x.stride(1)


def splits(B, N, D, R):
    """What ``splits=0`` resolves to for this shape (bvc_op_attn_pool_splits)."""
    L = _lib.lib()
    s = L.bvc_op_attn_pool_splits(int(B), int(N), int(D), int(R))
    if s < 0:
        raise _lib.BvcError(f"bvc_op_attn_pool_splits: {L.bvc_last_error().decode()}")
    return s


def _workspace(B, N, D, R, nsplit, device):
    L = _lib.lib()
    nbytes = L.bvc_op_attn_pool_workspace(B, N, D, R, nsplit)
    if nbytes < 0:
        raise _lib.BvcError(f"bvc_op_attn_pool_workspace: {L.bvc_last_error().decode()}")
    return torch.empty((nbytes + 15) // 16 * 4, dtype=torch.float32, device=device)


class _AttentivePool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, u, eps, nsplit):
        x, ldx = _token_rows(x)
        u = u.contiguous()
        B, N, D = x.shape
        R = u.shape[0]
        ws = _workspace(B, N, D, R, nsplit, x.device)
        pooled = torch.empty(B, R, D, dtype=torch.float32, device=x.device)
        lse = torch.empty(B, R, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().bvc_op_attn_pool_fwd(x.data_ptr(), ldx, u.data_ptr(), B, N, D, R, eps, nsplit, pooled.data_ptr(),
                                                       lse.data_ptr(), ws.data_ptr(), _lib.current_stream_ptr()), "bvc_op_attn_pool_fwd")
        ctx.save_for_backward(x, u, pooled, lse)
        ctx.eps, ctx.nsplit = eps, nsplit
        ctx.mark_non_differentiable(lse)
        return pooled, lse

    @staticmethod
    def backward(ctx, dpooled, _dlse):
        x, u, pooled, lse = ctx.saved_tensors
        x, ldx = _token_rows(x)
        B, N, D = x.shape
        R = u.shape[0]
        dpooled = dpooled.contiguous().float()
        ws = _workspace(B, N, D, R, ctx.nsplit, x.device)
        du = torch.empty(R, D, dtype=torch.float32, device=x.device)
        dx = torch.empty(B, N, D, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[0] else None     # frozen encoder: no dx
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().bvc_op_attn_pool_bwd(x.data_ptr(), ldx, u.data_ptr(), pooled.data_ptr(), lse.data_ptr(), dpooled.data_ptr(),
                                                       B, N, D, R, ctx.eps, ctx.nsplit, du.data_ptr(), None if dx is None else dx.data_ptr(), D,
                                                       ws.data_ptr(), _lib.current_stream_ptr()), "bvc_op_attn_pool_bwd")
        return dx, du, None, None


def _checked(x, u, eps, splits):
    if not (isinstance(x, torch.Tensor) and x.dim() == 3 and isinstance(u, torch.Tensor) and u.dim() == 2):
        raise ValueError("attentive_pool: x must be a tensor [B][N][D] and u a tensor [R][D]")
    if u.shape[1] != x.shape[2]:
        raise ValueError(f"attentive_pool: x has {x.shape[2]} columns, u {u.shape[1]}")
    if not (x.is_cuda and u.is_cuda):
        raise _lib.BvcError("attentive_pool: x and u must be on the GPU (there is no CPU path)")
    if x.device != u.device:
        raise ValueError("attentive_pool: x and u must be on the same device")
    if not (x.is_floating_point() and u.is_floating_point()):
        raise ValueError("attentive_pool: x and u must be floating-point tensors")
    if int(splits) < 0 or not float(eps) >= 0:
        raise ValueError("attentive_pool: splits and eps must not be negative")
    return x.float(), u.float(), float(eps), int(splits)


def attentive_pool(x, u, eps=1e-5, splits=0):
    """pooled f32 [B][R][D]: for each clip, the ``R`` (<= 16) rows of ``u`` [R][D] softmax-pool the standardised token rows of ``x``
    [B][N][D]: ``xh_j = (x_j - mean_j) / sqrt(var_j + eps)``, ``pooled_r = sum_j softmax_j(xh_j . u_r) xh_j``.  Differentiable in
    ``u`` and, only when ``x.requires_grad``, in ``x``.  ``D % 64 == 0``, ``64 <= D <= 2048``.  Runs on the current stream; the same
    bits on every run; ``splits=0`` lets the library cut the token range.  Non-CUDA tensors raise ``BvcError``."""
    x, u, eps, nsplit = _checked(x, u, eps, splits)
    return _AttentivePool.apply(x, u, eps, nsplit)[0]


def attentive_pool_lse(x, u, eps=1e-5, splits=0):
    """(pooled, lse f32 [B][R] = log sum_j exp(xh_j . u_r)); lse carries no gradient."""
    x, u, eps, nsplit = _checked(x, u, eps, splits)
    return _AttentivePool.apply(x, u, eps, nsplit)


class _CrossAttention(nn.Module):
    def __init__(self, dim, num_heads, qkv_bias):
        super().__init__()
        self.q = nn.Linear(dim, dim, bias=qkv_bias)
        self.kv = nn.Linear(dim, 2 * dim, bias=qkv_bias)      # K rows first, then V
        self.proj = nn.Linear(dim, dim)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class _CrossAttentionBlock(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, qkv_bias, complete_block, norm_eps):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=norm_eps)
        self.xattn = _CrossAttention(dim, num_heads, qkv_bias)
        if complete_block:
            self.norm2 = nn.LayerNorm(dim, eps=norm_eps)
            self.mlp = _Mlp(dim, int(dim * mlp_ratio))


class AttentivePooler(nn.Module):
    """tokens [B][N][D] -> [B][D]: ``q = t + proj(xattn(t, norm1(x)))`` with one learned query token ``t`` and ``num_heads`` heads of
    softmax scale ``(D / H) ** -0.5``; ``q = q + mlp(norm2(q))`` when ``complete_block``.  Computed in the folded form of the module
    docstring: K and V are never formed.  ``splits`` (0 = the library's choice) is passed to ``attentive_pool``."""

    def __init__(self, embed_dim, num_heads, mlp_ratio=4.0, qkv_bias=True, complete_block=True, norm_eps=1e-5, init_std=0.02):
        super().__init__()
        if embed_dim % num_heads or not 1 <= num_heads <= MAX_QUERIES:
            raise ValueError(f"AttentivePooler: {num_heads} heads (1 .. {MAX_QUERIES}) must divide embed_dim {embed_dim}")
        self.embed_dim, self.num_heads, self.complete_block, self.init_std = embed_dim, num_heads, bool(complete_block), init_std
        self.splits = 0
        self.query_tokens = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.cross_attention_block = _CrossAttentionBlock(embed_dim, num_heads, mlp_ratio, qkv_bias, complete_block, norm_eps)
        nn.init.trunc_normal_(self.query_tokens, std=init_std)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=self.init_std)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.LayerNorm):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)

    def folded_queries(self):
        """(u [H][D], the query token [D]): ``u_h = scale * gamma o (Wk_h^T q_h)``."""
        blk, D, H = self.cross_attention_block, self.embed_dim, self.num_heads
        d = D // H
        t = self.query_tokens[0, 0].float()
        q = blk.xattn.q(t).view(H, d)
        wk = blk.xattn.kv.weight[:D].float().view(H, d, D)
        u = torch.einsum("hd,hdk->hk", q, wk) * (blk.norm1.weight.float() * d ** -0.5)
        return u, t

    def forward(self, tokens):
        blk, D, H = self.cross_attention_block, self.embed_dim, self.num_heads
        d = D // H
        u, t = self.folded_queries()
        pooled = attentive_pool(tokens, u, blk.norm1.eps, self.splits)                 # [B][H][D]
        z = pooled * blk.norm1.weight.float() + blk.norm1.bias.float()
        out = torch.einsum("bhk,hdk->bhd", z, blk.xattn.kv.weight[D:].float().view(H, d, D))
        if blk.xattn.kv.bias is not None:
            out = out + blk.xattn.kv.bias[D:].float().view(H, d)
        q = t + blk.xattn.proj(out.reshape(-1, D))
        if self.complete_block:
            q = q + blk.mlp(blk.norm2(q))
        return q


class AttentiveClassifier(nn.Module):
    """tokens [B][N][D] -> logits [B][num_classes]: ``linear(pooler(tokens))``; ``pooler_kwargs`` go to ``AttentivePooler``."""

    def __init__(self, embed_dim, num_heads, num_classes, **pooler_kwargs):
        super().__init__()
        self.pooler = AttentivePooler(embed_dim, num_heads, **pooler_kwargs)
        self.linear = nn.Linear(embed_dim, num_classes)
        nn.init.trunc_normal_(self.linear.weight, std=self.pooler.init_std)
        nn.init.zeros_(self.linear.bias)

    def forward(self, tokens):
        return self.linear(self.pooler(tokens))
