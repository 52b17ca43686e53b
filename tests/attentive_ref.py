"""References for bvc.attentive (csrc/attnpool.hip), plain torch in the dtype of their inputs (the tests pass float64; the GPU tests
also run them in float32 on the device as the comparator).  tests/test_attentive_ref.py pins them on the CPU.

  core / core_backward    the op the kernel computes and the hand-written backward formulas of its design;
  core_scales             the per-row magnitudes the GPU bars are relative to, and the eps_p terms A and S;
  folded_logits           the module through the folded form (u, core, per-head Wv product);
  unfused_logits          the module written literally: LayerNorm, kv linear, per-head softmax attention, proj.
Module parameters are a dict with the state-dict names of bvc.attentive.AttentiveClassifier.
"""
import math

import torch
import torch.nn.functional as F

P = "pooler.cross_attention_block."


def standardise(x, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    return (x - mean) * rstd, rstd


def core(x, u, eps):
    """x [B][N][D], u [R][D] -> pooled [B][R][D], lse [B][R]"""
    xh, _ = standardise(x, eps)
    s = xh @ u.t()                                   # [B][N][R]
    lse = torch.logsumexp(s, dim=1)
    p = torch.exp(s - lse[:, None, :])
    return torch.einsum("bnr,bnd->brd", p, xh), lse


def core_backward(x, u, eps, dpooled):
    """(du [R][D], dx [B][N][D]) by the formulas of the design: dp = dP . xh, delta = dP . P, ds = p (dp - delta), .."""
    xh, rstd = standardise(x, eps)
    s = xh @ u.t()
    lse = torch.logsumexp(s, dim=1)
    p = torch.exp(s - lse[:, None, :])
    pooled = torch.einsum("bnr,bnd->brd", p, xh)
    dp = torch.einsum("brd,bnd->bnr", dpooled, xh)
    delta = (dpooled * pooled).sum(-1)               # [B][R]
    ds = p * (dp - delta[:, None, :])
    du = torch.einsum("bnr,bnd->rd", ds, xh)
    dxh = torch.einsum("bnr,brd->bnd", p, dpooled) + ds @ u
    dx = rstd * (dxh - dxh.mean(-1, keepdim=True) - xh * (dxh * xh).mean(-1, keepdim=True))
    return du, dx


def core_scales(x, u, eps, dpooled):
    """float64 magnitudes: dict with
    pooled [B][R][D] = sum_j p |xh|;  du [R][D] = sum_b sum_j p (|dp| + |delta|) |xh|;  dx [B][N][D] = rstd (|dxh| + mean |dxh| + |xh| mean
    |dxh . xh|) with |dxh| = sum_r p (|dP| + (|dp| + |delta|) |u|);  A [B][R] = max |s - lse| over tokens with p >= 2^-30;
    S [B][R] = max_j sum_d |xh u|."""
    xh, rstd = standardise(x, eps)
    s = xh @ u.t()
    lse = torch.logsumexp(s, dim=1)
    p = torch.exp(s - lse[:, None, :])
    pooled = torch.einsum("bnr,bnd->brd", p, xh)
    dp = torch.einsum("brd,bnd->bnr", dpooled, xh)
    delta = (dpooled * pooled).sum(-1)
    mag = p * (dp.abs() + delta.abs()[:, None, :])
    adxh = torch.einsum("bnr,brd->bnd", p, dpooled.abs()) + mag @ u.abs()
    a = (s - lse[:, None, :]).abs()
    a = torch.where(p >= 2.0 ** -30, a, torch.zeros_like(a))
    return {
        "pooled": torch.einsum("bnr,bnd->brd", p, xh.abs()),
        "du": torch.einsum("bnr,bnd->rd", mag, xh.abs()),
        "dx": rstd * (adxh + adxh.mean(-1, keepdim=True) + xh.abs() * (adxh * xh.abs()).mean(-1, keepdim=True)),
        "A": a.amax(dim=1),
        "S": (xh.abs() @ u.abs().t()).amax(dim=1),
    }


def make_params(D, H, num_classes, mlp_ratio=4.0, complete_block=True, qkv_bias=True, seed=0, dtype=torch.float64, spread=0.3):
    """A parameter dict with every entry well away from its initial value (biases and norm offsets included)."""
    g = torch.Generator().manual_seed(seed)
    hid = int(D * mlp_ratio)

    def rn(*shape, s=spread):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * s).to(dtype)

    sd = {"pooler.query_tokens": rn(1, 1, D, s=1.0),
          P + "norm1.weight": 1 + rn(D), P + "norm1.bias": rn(D),
          P + "xattn.q.weight": rn(D, D, s=spread / math.sqrt(D) * 4), P + "xattn.kv.weight": rn(2 * D, D, s=spread / math.sqrt(D) * 4),
          P + "xattn.proj.weight": rn(D, D, s=spread / math.sqrt(D) * 4), P + "xattn.proj.bias": rn(D)}
    if qkv_bias:
        sd[P + "xattn.q.bias"] = rn(D)
        sd[P + "xattn.kv.bias"] = rn(2 * D)
    if complete_block:
        sd.update({P + "norm2.weight": 1 + rn(D), P + "norm2.bias": rn(D),
                   P + "mlp.fc1.weight": rn(hid, D, s=spread / math.sqrt(D) * 4), P + "mlp.fc1.bias": rn(hid),
                   P + "mlp.fc2.weight": rn(D, hid, s=spread / math.sqrt(hid) * 4), P + "mlp.fc2.bias": rn(D)})
    sd["linear.weight"] = rn(num_classes, D)
    sd["linear.bias"] = rn(num_classes)
    return sd


def _tail(sd, q, eps):
    if P + "norm2.weight" in sd:
        D = q.shape[-1]
        h = F.layer_norm(q, (D,), sd[P + "norm2.weight"], sd[P + "norm2.bias"], eps)
        h = F.linear(F.gelu(F.linear(h, sd[P + "mlp.fc1.weight"], sd[P + "mlp.fc1.bias"])), sd[P + "mlp.fc2.weight"], sd[P + "mlp.fc2.bias"])
        q = q + h
    return F.linear(q, sd["linear.weight"], sd["linear.bias"])


def unfused_logits(sd, x, H, eps=1e-5, score_shift=None):
    """literal: K, V = kv(norm1(x)); per-head softmax(q K^T scale) V; proj; residual; (norm2 + MLP); linear.
    score_shift [H]: a constant added to every score of a head (must leave the result unchanged)."""
    B, N, D = x.shape
    d = D // H
    t = sd["pooler.query_tokens"][0, 0]
    xn = F.layer_norm(x, (D,), sd[P + "norm1.weight"], sd[P + "norm1.bias"], eps)
    q = F.linear(t, sd[P + "xattn.q.weight"], sd.get(P + "xattn.q.bias")).view(H, d)
    kv = F.linear(xn, sd[P + "xattn.kv.weight"], sd.get(P + "xattn.kv.bias"))
    k, v = kv[..., :D].reshape(B, N, H, d), kv[..., D:].reshape(B, N, H, d)
    s = torch.einsum("hd,bnhd->bhn", q, k) * d ** -0.5
    if score_shift is not None:
        s = s + score_shift[None, :, None]
    a = torch.softmax(s, dim=-1)
    out = torch.einsum("bhn,bnhd->bhd", a, v).reshape(B, D)
    y = F.linear(out, sd[P + "xattn.proj.weight"], sd[P + "xattn.proj.bias"])
    return _tail(sd, t + y, eps)


def folded_u(sd, H):
    D = sd["pooler.query_tokens"].shape[-1]
    d = D // H
    t = sd["pooler.query_tokens"][0, 0]
    q = F.linear(t, sd[P + "xattn.q.weight"], sd.get(P + "xattn.q.bias")).view(H, d)
    wk = sd[P + "xattn.kv.weight"][:D].view(H, d, D)
    return torch.einsum("hd,hdk->hk", q, wk) * (sd[P + "norm1.weight"] * d ** -0.5)


def folded_logits(sd, x, H, eps=1e-5, pool=None):
    """the form bvc.attentive computes: u, the core op (`pool`, default the reference core), the per-head Wv product"""
    B, N, D = x.shape
    d = D // H
    t = sd["pooler.query_tokens"][0, 0]
    u = folded_u(sd, H)
    pooled = core(x, u, eps)[0] if pool is None else pool(x, u, eps)
    z = pooled * sd[P + "norm1.weight"] + sd[P + "norm1.bias"]
    out = torch.einsum("bhk,hdk->bhd", z, sd[P + "xattn.kv.weight"][D:].view(H, d, D))
    if P + "xattn.kv.bias" in sd:
        out = out + sd[P + "xattn.kv.bias"][D:].view(H, d)
    y = F.linear(out.reshape(B, D), sd[P + "xattn.proj.weight"], sd[P + "xattn.proj.bias"])
    return _tail(sd, t + y, eps)


def loss_and_grads(fn, sd, x, labels, **kw):
    """(logits, loss, {name: grad}) of cross-entropy over `fn`(leaf copies of sd, x)"""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    logits = fn(leaves, x, **kw)
    loss = F.cross_entropy(logits, labels)
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return logits.detach(), loss.detach(), dict(zip(leaves.keys(), grads))
