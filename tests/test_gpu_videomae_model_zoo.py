"""The VideoMAE sizes on the GPU: attention at head dims 80 and 88 run in place (csrc/attention.hip) against the zero-padded hd-96
path, bitwise, and against fp32 torch; training steps of small, large and huge (full width, reduced depth; huge also at full depth)
against the fp32 oracle at test_gpu_videomae.py's bars; the huge embedding; a deterministic rerun; a GradScaler + SGD loop on large;
and the JEPA ViT-H step with head_pad 0 against 1."""
import copy
import dataclasses
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from tests.test_gpu_videomae import _check_step, _classifier, _fc_norm, _model   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402
from oracle import jepa_oracle as jo   # noqa: E402

bvc = G.bvc
L = G.L
dev = torch.device("cuda:0")


def _ref_attention(qkv, B, N, H, HD):
    x = qkv.float().view(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    s = (q @ k.transpose(-1, -2)) * HD ** -0.5
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * N, H * HD)
    return o, (torch.logsumexp(s, dim=-1) * math.log2(math.e)).reshape(B * H, N)


def _fwd(qkv, B, N, H, HD, scale=0.0):
    ctx = torch.full((B * N, H * HD), float("nan"), device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(B * H, N, device=dev)
    L.check(L.lib().bvc_op_attention_fwd_scaled(G.ptr(qkv), G.ptr(ctx), G.ptr(lse), B, N, H, HD, scale, G.stream()), "attention_fwd")
    return ctx, lse


def _bwd(qkv, ctx, dctx, lse, B, N, H, HD, scale=0.0):
    dqkv = torch.full((B * N, 3 * H * HD), float("nan"), device=dev, dtype=torch.bfloat16)
    delta = torch.zeros(B * H, N, device=dev)
    L.check(L.lib().bvc_op_attention_bwd_scaled(G.ptr(qkv), G.ptr(ctx), G.ptr(dctx), G.ptr(lse), G.ptr(delta), G.ptr(dqkv), B, N, H, HD,
                                                scale, G.stream()), "attention_bwd")
    return dqkv


def _pad(x, B, N, parts, H, HD):
    """[B*N][parts*H*HD] -> [B*N][parts*H*96], each head zero-padded at its end (what head_pad = 1 builds)"""
    y = torch.zeros(B * N, parts, H, 96, device=dev, dtype=x.dtype)
    y[..., :HD] = x.view(B * N, parts, H, HD)
    return y.view(B * N, parts * H * 96)


def _unpad(y, B, N, parts, H, HD):
    return y.view(B * N, parts, H, 96)[..., :HD].reshape(B * N, parts * H * HD)


# test_attention_wide_heads_forward_backward's cases (tail splits gs = 4 / 2, ragged key tiles), N = 160 (the encoder's visible tokens)
# and N = 1568 (the decoder)
CASES = [(2, 25, 3), (2, 100, 2), (2, 125, 2), (1, 320, 2), (2, 392, 2), (1, 500, 3), (2, 160, 16), (1, 1568, 8)]


@pytest.mark.parametrize("HD", [80, 88])
@pytest.mark.parametrize("B,N,H", CASES)
def test_attention_in_place_is_bitwise_the_padded_path(B, N, H, HD):
    D = HD * H
    qkv = G.bf16_randn(B * N, 3 * D, seed=70 + HD + N)
    dctx = G.bf16_randn(B * N, D, seed=71 + N)
    runs = []
    for _ in range(2):     # twice: the zeroed LDS chunks and the masked stores must not depend on what ran before
        ctx, lse = _fwd(qkv, B, N, H, HD)
        runs.append((ctx, lse, _bwd(qkv, ctx, dctx, lse, B, N, H, HD)))
    torch.cuda.synchronize()
    (ctx, lse, dqkv), (ctx2, lse2, dqkv2) = runs
    assert torch.equal(ctx, ctx2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2), "two launches differ"
    assert not torch.isnan(dqkv.float()).any() and not torch.isnan(ctx.float()).any(), "an in-place store left columns unwritten"
    # the padded path: heads zero-padded to 96 in HBM, the hd-96 kernels at the true width's scale, the padding dropped
    qp = _pad(qkv, B, N, 3, H, HD)
    cp, lp = _fwd(qp, B, N, H, 96, HD ** -0.5)
    dp = _bwd(qp, cp, _pad(dctx, B, N, 1, H, HD), lp, B, N, H, 96, HD ** -0.5)
    torch.cuda.synchronize()
    assert torch.equal(ctx, _unpad(cp, B, N, 1, H, HD)), "ctx differs from the padded path"
    assert torch.equal(lse, lp), "lse differs from the padded path"
    assert torch.equal(dqkv, _unpad(dp, B, N, 3, H, HD)), "dqkv differs from the padded path"
    x = qkv.float().requires_grad_(True)
    o, lse_ref = _ref_attention(x, B, N, H, HD)
    assert G.rel_err(ctx.float(), o.detach()) < 1e-2, G.rel_err(ctx.float(), o.detach())
    assert float((lse - lse_ref.detach()).abs().max()) < 2e-3
    (o * dctx.float()).sum().backward()
    got = dqkv.float()
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        e = G.rel_err(got[:, sl], x.grad[:, sl])
        assert e < 2e-2, (name, e)


def _cfg(arch, **kw):
    """oracle config of a VIDEOMAE_ARCHS size (16 frames of 224^2 unless overridden)"""
    c = bvc.videomae_config(arch, **kw)
    return dataclasses.replace(vo.BASE, **{f.name: getattr(c, f.name) for f in dataclasses.fields(vo.OracleConfig)
                                           if f.name != "decoder_norm_eps"})


def _fixture(golden_dir, name, cfg, B, seed):
    """tests/golden/videomae_<name>.json (tools/make_videomae_zoo_golden.py: transformers' own fp32 step), for this very case"""
    with open(os.path.join(golden_dir, f"videomae_{name}.json")) as f:
        fx = json.load(f)
    assert fx["config"] == cfg.__dict__ and (fx["batch"], fx["seed"], fx["weight_seed"], fx["mask_ratio"]) == (B, seed, 0, 0.9)
    return fx


def _check_fixture_grads(tag, model, fx, cfg):
    """the step's gradients against transformers': per-tensor L2 norms at the per-tensor bar 5e-2 (with the floor of _check_step),
    the three grad_logger probes at its probe bar (1e-3 from width 768 on, 2.5e-3 below).  _check_step asserted the loss (1e-3)."""
    named = dict(model.named_parameters())
    assert set(named) == set(fx["grad_l2"])
    gmax = max(fx["grad_l2"].values())
    worst = ("", 0.0)
    for k, want in fx["grad_l2"].items():
        e = abs(float(named[k].grad.double().norm()) - want) / (want + 1e-3 * gmax)
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e < 5e-2, (k, e)
    G.log_parity(f"[{tag}] worst per-tensor grad norm vs transformers fixture {worst[1]:.2e} ({worst[0]})")
    for k, want in fx["grad_probes"].items():
        e = abs(float(named[k].grad.double().norm()) - want) / want
        assert e < (1e-3 if cfg.hidden_size >= 768 else 2.5e-3), (k, e)


@pytest.mark.parametrize("arch", ["small", "large", "huge"])
def test_train_step_reduced_depth_matches_oracle_and_fixture(golden_dir, arch):
    """full width, 2 encoder layers and 1 decoder layer, 2 clips at mask 0.9"""
    cfg = _cfg(arch, num_hidden_layers=2, decoder_num_hidden_layers=1)
    fx = _fixture(golden_dir, f"{arch}_w_b2_s0", cfg, 2, 0)
    model = _check_step(f"{arch}_w", cfg, 2, 0, 0.9, fixture=fx)
    _check_fixture_grads(f"{arch}_w", model, fx, cfg)


def test_train_step_full_depth_huge_matches_oracle_and_fixture(golden_dir):
    cfg = _cfg("huge")
    fx = _fixture(golden_dir, "huge_b2_s1", cfg, 2, 1)
    model = _check_step("huge_full", cfg, 2, 1, 0.9, fixture=fx)
    _check_fixture_grads("huge_full", model, fx, cfg)


def test_huge_embedding_matches_oracle():
    cfg = _cfg("huge", num_hidden_layers=4)
    params = vo.make_params(cfg, seed=3)
    fw, fb = _fc_norm(cfg, 4)
    pixels, _ = vo.synthetic_batch(cfg, 2, 5, 0.9)
    with torch.no_grad():
        ref, ref_tok = vo.encode(cfg, params, pixels, fw, fb, 1e-6)
    out = _classifier(cfg, params, fw, fb)(pixel_values=pixels.to(dev), output_last_hidden_state=True)
    emb, tok = out.logits.float().cpu(), out.last_hidden_state.float().cpu()
    assert G.rel_err(emb, ref) < 2e-2 and G.rel_err(tok, ref_tok) < 2e-2, (G.rel_err(emb, ref), G.rel_err(tok, ref_tok))


def test_huge_step_deterministic_rerun():
    cfg = _cfg("huge", num_hidden_layers=2, decoder_num_hidden_layers=1)
    params = vo.make_params(cfg, seed=6)
    pixels, mask = vo.synthetic_batch(cfg, 3, 7, 0.9)
    old = bvc.are_deterministic_algorithms_enabled()
    bvc.use_deterministic_algorithms(True)
    try:
        res = []
        for _ in range(2):
            m = _model(cfg, params)
            out = m(pixels.to(dev), bool_masked_pos=mask.to(dev))
            out.loss.backward()
            torch.cuda.synchronize()
            res.append((out.loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    finally:
        bvc.use_deterministic_algorithms(old)
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_training_loop_large_with_gradscaler_and_sgd():
    cfg = _cfg("large", num_hidden_layers=2, decoder_num_hidden_layers=1)
    params = vo.make_params(cfg, seed=8)
    model = _model(cfg, params)
    model._ensure_flat(dev)
    opt = bvc.optim.SGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True, weight_decay=0.0)
    scaler = bvc.amp.GradScaler("cuda")
    ref = {k: v.clone() for k, v in params.items()}
    bufs = {}
    for it in range(3):
        pixels, mask = vo.synthetic_batch(cfg, 2, seed=200 + it, mask_ratio=0.9)
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model(pixels.to(dev), bool_masked_pos=mask.to(dev)).loss
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        rl, rg = vo.step(cfg, ref, pixels, mask)
        vo.sgd_nesterov_step(ref, rg, bufs, lr=0.1, momentum=0.9)
        rel = abs(float(loss) - float(rl)) / float(rl)
        assert math.isfinite(float(loss)) and rel < 2e-3, (it, float(loss), float(rl))
    sd = model.state_dict()
    e = max(G.rel_err(sd[k].cpu(), ref[k]) for k in ref if ref[k].dim() >= 2)
    assert e < 2e-2, e


def test_jepa_vit_h_head_pad_in_place_against_padded():
    """The ViT-H-width JEPA step (2 encoder / 2 predictor layers) under head_pad 0 (in place) and 1 (zero-padded to 96): same loss
    within 1e-3 and per-tensor gradients within the zoo bar 5e-2 of each other."""
    cfg = jo.JepaConfig(embed_dim=1280, num_heads=16, depth=2, pred_depth=2)
    pcfg = dataclasses.replace(cfg, mlp_ratio=4.0)
    enc_p, pred_p = jo.make_params(jo.encoder_shapes(cfg), cfg, 3), jo.make_params(jo.predictor_shapes(pcfg), pcfg, 53)
    tgt_p = jo.make_params(jo.encoder_shapes(cfg), cfg, 103)
    imgs, m_enc, m_pred = jo.synthetic_inputs(cfg, 2, 3, 100, 25)
    kw = dict(img_size=[cfg.image_size], patch_size=cfg.patch_size, num_frames=cfg.num_frames, tubelet_size=cfg.tubelet_size,
              embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio)
    out = {}
    for pad in (0, 1):
        old = L.set_option("head_pad", pad)
        try:
            assert L.lib().bvc_op_attention_width(80) == (96 if pad else 80)     # the width the stacks below are allocated at
            enc = bvc.jepa.VisionTransformer(**kw)
            enc.load_state_dict(enc_p)
            tgt = copy.deepcopy(enc)
            tgt.load_state_dict(tgt_p)
            for p in tgt.parameters():
                p.requires_grad = False
            pred = bvc.jepa.vit_predictor(sequence_shape=enc.sequence_shape, embed_dim=cfg.embed_dim, predictor_embed_dim=cfg.pred_dim,
                                          depth=cfg.pred_depth, num_heads=enc.num_heads)
            pred.load_state_dict(pred_p)
            enc, pred, tgt = enc.to(dev), pred.to(dev), tgt.to(dev)
            x = imgs.to(dev)
            me, mp = [m.to(dev) for m in m_enc], [m.to(dev) for m in m_pred]
            with torch.no_grad():
                h = bvc.jepa.select_targets(tgt(x), mp)
            loss = bvc.jepa.smooth_l1_loss(pred(enc(x, me), me, mp), h)
            (loss * 1024.0).backward()
            torch.cuda.synchronize()
            out[pad] = (float(loss), {k: p.grad.float().cpu() for k, p in list(enc.named_parameters()) + list(pred.named_parameters())
                                      if p.grad is not None})
        finally:
            L.set_option("head_pad", old)
    (l0, g0), (l1, g1) = out[0], out[1]
    # the two legs ran different products (K = 1280 against 1536 with zero columns, other tiles): not the same bits
    assert any(not torch.equal(g0[k], g1[k]) for k in g1), "head_pad = 1 ran the in-place path"
    assert abs(l0 - l1) / abs(l1) < 1e-3, (l0, l1)
    gmax = max(float(g.norm()) for g in g1.values())
    for k in g1:
        e = float((g0[k] - g1[k]).norm() / (g1[k].norm() + 1e-3 * gmax))
        assert e < 5e-2, (k, e)
