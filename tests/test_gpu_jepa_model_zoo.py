"""The JEPA model zoo on the GPU: attention at head widths 96 and 128 (csrc/attention.hip, panel images), and training steps of the
ViT-H, ViT-g and ViT-Ti shapes (heads of 80 / 88 dims zero-padded to 96, the ViT-Ti predictor's 128-wide heads, LayerNorms of width
1280 / 1408) against the oracle.  Bars as in test_gpu_ops.py / test_gpu_jepa.py: attention ctx 1e-2, lse 2e-3, gradients 2e-2;
step loss 1e-3, activations 2e-2, per-tensor gradients 5e-2 relative L2."""
import copy
import dataclasses
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from oracle import jepa_oracle as jo   # noqa: E402
from oracle import videomae_oracle_bf16 as vb   # noqa: E402

bvc = G.bvc
L = G.L
dev = torch.device("cuda:0")
OWN_BAR = 5e-4      # |probe norm - bf16-operand oracle's| / norm (test_gpu_jepa.py's full-width bar; ViT-Ti's 224^2 case meets it too)


def _ref_attention(qkv, B, N, H, HD):
    x = qkv.float().view(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    s = (q @ k.transpose(-1, -2)) * HD ** -0.5
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * N, H * HD)
    return o, (torch.logsumexp(s, dim=-1) * math.log2(math.e)).reshape(B * H, N)


def _fwd(qkv, B, N, H, HD):
    ctx = torch.zeros(B * N, H * HD, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(B * H, N, device=dev)
    L.check(L.lib().bvc_op_attention_fwd(G.ptr(qkv), G.ptr(ctx), G.ptr(lse), B, N, H, HD, G.stream()), "attention_fwd")
    return ctx, lse


def _bwd(qkv, ctx, dctx, lse, B, N, H, HD):
    dqkv = torch.full((B * N, 3 * H * HD), float("nan"), device=dev, dtype=torch.bfloat16)
    delta = torch.zeros(B * H, N, device=dev)
    L.check(L.lib().bvc_op_attention_bwd(G.ptr(qkv), G.ptr(ctx), G.ptr(dctx), G.ptr(lse), G.ptr(delta), G.ptr(dqkv), B, N, H, HD,
                                         G.stream()), "attention_bwd")
    return dqkv


# N = 25 / 392: one owning wave in the last 128-row block (the tail split, gs = 4); 320: two (gs = 2); 125 / 500: a ragged last key tile
@pytest.mark.parametrize("HD", [96, 128])
@pytest.mark.parametrize("B,N,H", [(2, 25, 3), (2, 100, 2), (2, 125, 2), (1, 320, 2), (2, 392, 2), (1, 500, 3)])
def test_attention_wide_heads_forward_backward(B, N, H, HD):
    D = HD * H
    qkv = G.bf16_randn(B * N, 3 * D, seed=60 + HD)
    dctx = G.bf16_randn(B * N, D, seed=61)
    ctx, lse = _fwd(qkv, B, N, H, HD)
    dqkv = _bwd(qkv, ctx, dctx, lse, B, N, H, HD)
    ctx2, lse2 = _fwd(qkv, B, N, H, HD)
    dqkv2 = _bwd(qkv, ctx2, dctx, lse2, B, N, H, HD)
    torch.cuda.synchronize()
    assert torch.equal(ctx, ctx2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2), "two launches differ"
    x = qkv.float().requires_grad_(True)
    o, lse_ref = _ref_attention(x, B, N, H, HD)
    assert G.rel_err(ctx.float(), o.detach()) < 1e-2, G.rel_err(ctx.float(), o.detach())
    assert float((lse - lse_ref.detach()).abs().max()) < 2e-3
    (o * dctx.float()).sum().backward()
    got = dqkv.float()
    assert torch.isfinite(got).all()
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        e = G.rel_err(got[:, sl], x.grad[:, sl])
        assert e < 2e-2, (name, e)


def _modules(cfg, enc_p, pred_p, tgt_p):
    kw = dict(img_size=[cfg.image_size], patch_size=cfg.patch_size, num_frames=cfg.num_frames, tubelet_size=cfg.tubelet_size,
              embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio)
    enc = bvc.jepa.VisionTransformer(**kw)
    enc.load_state_dict(enc_p)
    tgt = copy.deepcopy(enc)
    tgt.load_state_dict(tgt_p)
    pred = bvc.jepa.vit_predictor(sequence_shape=enc.sequence_shape, embed_dim=cfg.embed_dim, predictor_embed_dim=cfg.pred_dim,
                                  depth=cfg.pred_depth, num_heads=enc.num_heads)
    pred.load_state_dict(pred_p)
    for p in tgt.parameters():
        p.requires_grad = False
    return enc.to(dev), pred.to(dev), tgt.to(dev)


def _params(cfg, seed):
    # the predictor keeps mlp_ratio 4 whatever the encoder's (vit_predictor, vision_transformer.py:538-541): ViT-g's 48/11 is the
    # encoder's alone
    pcfg = dataclasses.replace(cfg, mlp_ratio=4.0)
    return (jo.make_params(jo.encoder_shapes(cfg), cfg, seed), jo.make_params(jo.predictor_shapes(pcfg), pcfg, seed + 50),
            jo.make_params(jo.encoder_shapes(cfg), cfg, seed + 100))


def _step_case(cfg, B, n_ctx, n_pred, seed, tag):
    """_train_step_case of test_gpu_jepa.py without the reference-modules fixture: select targets, smooth-L1, backward, against the fp32
    oracle step and the bf16-operand one (vb.BUILD)."""
    enc_p, pred_p, tgt_p = _params(cfg, seed)
    imgs, m_enc, m_pred = jo.synthetic_inputs(cfg, B, seed, n_ctx, n_pred)
    scale = 1024.0
    rloss, rge, rgp, rz, rh = jo.step(cfg, enc_p, pred_p, tgt_p, imgs, m_enc, m_pred, grad_scale=scale)
    bloss, bge, _bgp, _bz, _bh = jo.step(cfg, enc_p, pred_p, tgt_p, imgs, m_enc, m_pred, grad_scale=scale, pol=vb.BUILD)
    enc, pred, tgt = _modules(cfg, enc_p, pred_p, tgt_p)
    x = imgs.to(dev)
    me, mp = [m.to(dev) for m in m_enc], [m.to(dev) for m in m_pred]
    with torch.no_grad():
        h = bvc.jepa.select_targets(tgt(x), mp)
    z = pred(enc(x, me), me, mp)
    loss = bvc.AllReduce.apply(bvc.jepa.smooth_l1_loss(z, h))
    (loss * scale).backward()
    torch.cuda.synchronize()
    eh, ez = G.rel_err(h.cpu(), rh), G.rel_err(z.detach().cpu(), rz)
    rel = abs(float(loss) - float(rloss)) / float(rloss)
    G.log_parity(f"[jepa zoo {tag}] loss hip {float(loss):.7f} oracle {float(rloss):.7f} rel {rel:.2e}; targets h rel {eh:.2e}, "
                 f"predictions z rel {ez:.2e}")
    assert eh < 2e-2 and ez < 2e-2, (eh, ez)
    assert rel < 1e-3, (float(loss), float(rloss))
    gmax = max(float(g.norm()) for g in list(rge.values()) + list(rgp.values()))
    worst = ("", 0.0)
    for mod, ref in ((enc, rge), (pred, rgp)):
        for k, p in mod.named_parameters():
            if not p.requires_grad:
                assert p.grad is None
                continue
            e = float((p.grad.float().cpu() - ref[k]).norm() / (ref[k].norm() + 1e-3 * gmax))
            worst = max(worst, (k, e), key=lambda t: t[1])
            assert e < 5e-2, (k, e)
    G.log_parity(f"[jepa zoo {tag}] worst per-tensor gradient rel L2 {worst[1]:.2e} ({worst[0]})")
    own_bar = OWN_BAR
    for k in ("blocks.0.attn.qkv.weight", f"blocks.{cfg.depth - 1}.attn.qkv.weight"):
        gn, rn, bn = float(dict(enc.named_parameters())[k].grad.norm()), float(rge[k].norm()), float(bge[k].norm())
        e, own = (gn - rn) / rn, (gn - bn) / bn
        G.log_parity(f"[jepa zoo {tag}] grad-norm {k}: hip vs fp32 {e:+.2e} (bar 5e-3) | hip vs bf16-operand oracle {own:+.2e} "
                     f"(own bar {own_bar:.0e})")
        assert abs(e) < 5e-3, (k, e)
        assert abs(own) < own_bar, (k, own)


HUGE_W = jo.JepaConfig(embed_dim=1280, num_heads=16, depth=2, pred_depth=2)                      # heads of 80 -> 96
GIANT_W = jo.JepaConfig(embed_dim=1408, num_heads=16, mlp_ratio=48 / 11, depth=2, pred_depth=2)   # heads of 88 -> 96, MLP 6144
TINY = jo.JepaConfig(embed_dim=192, num_heads=3, depth=2, pred_depth=2)                          # predictor heads of 128
VIT_H = jo.JepaConfig(embed_dim=1280, depth=32, num_heads=16)                                    # ViT-H/16 itself
VIT_G = jo.JepaConfig(embed_dim=1408, depth=40, num_heads=16, mlp_ratio=48 / 11)                 # ViT-g/16 itself


@pytest.mark.parametrize("tag,cfg", [("huge-width", HUGE_W), ("giant-width", GIANT_W), ("tiny", TINY)])
def test_train_step_matches_oracle(tag, cfg):
    _step_case(cfg, 2, 100, 25, 3, tag)


def test_train_step_full_depth_vit_h():
    """BASELINE config 4's shape with the ViT-H/16 encoder: B = 2, 224^2, 2 frames, N_ctx 100, N_pred 25."""
    _step_case(VIT_H, 2, 100, 25, 0, "vit_h")


def test_train_step_tiny_with_layernorm_inside_the_predictor_products():
    """The 384-wide predictor's LayerNorms inside the epilogues of its products (forced row_ln), at predictor head dim 128."""
    old = L.set_option("row_ln", 1)
    try:
        assert L.lib().bvc_op_row_ln_selected(1000, 384, 1536, 3) == 1
        _step_case(TINY, 2, 100, 25, 5, "tiny row_ln")
    finally:
        L.set_option("row_ln", old)


def test_vit_g_embedding_and_train_step():
    """Full-depth ViT-g/16: the embedding path of compute_embeddings_jepa.py:242 (encoder without masks, token mean) against the
    oracle, then one train step + EMA twice from the same state: finite, bit-identical, and the target moves by the EMA formula."""
    cfg = VIT_G
    B = 2
    enc_p, pred_p, tgt_p = _params(cfg, 9)
    imgs, m_enc, m_pred = jo.synthetic_inputs(cfg, B, 9, 100, 25)
    ref = jo.encoder_forward(cfg, enc_p, imgs).mean(1)
    x = imgs.to(dev)
    me, mp = [m.to(dev) for m in m_enc], [m.to(dev) for m in m_pred]

    def run():
        enc, pred, tgt = _modules(cfg, enc_p, pred_p, tgt_p)
        with torch.no_grad():
            emb = bvc.jepa.token_mean(enc(x))
        opt = bvc.optim.SGD([{"params": [p for p in enc.parameters() if p.requires_grad]},
                             {"params": [p for p in pred.parameters() if p.requires_grad]}], lr=0.05, momentum=0.9, nesterov=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with torch.no_grad():
                h = bvc.jepa.select_targets(tgt(x), mp)
            z = pred(enc(x, me), me, mp)
            loss = bvc.jepa.smooth_l1_loss(z, h)
        loss.backward()
        opt.step()
        opt.zero_grad()
        m = 0.996
        tgt_before = tgt.flat_parameters().detach().clone()
        bvc.jepa.ema_update(enc, tgt, m)
        torch.cuda.synchronize()
        want = tgt_before * m + enc.flat_parameters().detach() * (1 - m)
        ema_err = G.rel_err(tgt.flat_parameters().detach(), want)
        moved = G.rel_err(tgt.flat_parameters().detach(), tgt_before)
        out = (emb.cpu(), float(loss), enc.flat_parameters().detach().cpu(), tgt.flat_parameters().detach().cpu(), ema_err, moved)
        del enc, pred, tgt, opt
        return out

    emb, loss, enc_w, tgt_w, ema_err, moved = run()
    e = G.rel_err(emb, ref)
    G.log_parity(f"[jepa zoo vit_g] embedding rel {e:.2e}; loss {loss:.6f}; EMA rel {ema_err:.1e}, target moved {moved:.1e}")
    assert e < 2e-2, e
    assert math.isfinite(loss)
    assert ema_err < 1e-6 and moved > 0
    emb2, loss2, enc_w2, tgt_w2, _, _ = run()
    assert torch.equal(emb, emb2) and loss == loss2
    assert torch.equal(enc_w, enc_w2) and torch.equal(tgt_w, tgt_w2)
