"""Stochastic depth and hidden dropout on the GPU: the gate on the two residual branches of every layer (include/bvc.h,
bvc_branch_drop), against tests/dropout_ref.py fed the gates the model reports.

Bars are the ungated steps', unchanged: tests/test_gpu_videomae_cls.py's for the fine-tuning step (loss 1e-3, logits 2e-2, encoder
per-tensor gradients 5e-2 with its floor, fc_norm / classifier 2e-2), tests/test_gpu_jepa.py's for the JEPA step (loss 1e-3, outputs
2e-2, per-tensor gradients 5e-2).  The schedule gives layer 0 rate 0, so a gate could go unexercised: every case runs on the first
of torch.manual_seed(0), (1), ... whose reported drop_path_scale holds both a zero and a nonzero entry among the layers with a
nonzero rate (a one-sample case: a zero in an MLP branch), and one of the first 32 seeds must qualify.
"""
import dataclasses
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from tests import dropout_ref as dr   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402
from oracle import jepa_oracle as jo   # noqa: E402
from tools.make_videomae_cls_golden import head_params   # noqa: E402

bvc = G.bvc
dg = bvc.dropgate
dev = torch.device("cuda:0")
NL = 10
SMALL = dataclasses.replace(vo.BASE, hidden_size=384, num_attention_heads=6, intermediate_size=1536)     # VIDEOMAE_ARCHS["small"]


def _heads(cfg, num_labels=NL, seed=5):
    return dict(zip(("fc_norm.weight", "fc_norm.bias", "classifier.weight", "classifier.bias"), head_params(cfg.hidden_size, num_labels, seed)))


def _model(cfg, params, heads, train=True, **drop):
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    m = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(num_labels=NL, **kw, **drop))
    sd = {k: v for k, v in params.items() if k.startswith("videomae.")}
    sd.update(heads)
    m.load_state_dict(sd)
    m.to(dev)
    return m.train() if train else m.eval()


# ----------------------------------------------------------------------------- 6: the mask op and its host twin
@pytest.mark.parametrize("M,N,p", [(37, 13, 0.1), (5, 3, 0.5), (1, 1, 0.9), (129, 130, 0.25), (1000, 384, 0.1)])
def test_dropout_mask_op_equals_host_twin(M, N, p):
    for seed, off, layer, branch in ((0, 0, 0, 0), (1234567890123, 4, 3, 1), (2 ** 63 + 5, 2 ** 40, 11, 0)):
        a = dg.dropout_mask(seed, off, layer, branch, M, N, p, dev).cpu()
        b = dg.dropout_mask_host(seed, off, layer, branch, M, N, p)
        assert torch.equal(a, b)
        assert set(a.unique().tolist()) <= {0, 1}


def test_gated_gemm_and_layernorm_backward_ops_match_torch():
    """The two kernels that apply the gate, alone: C = resid + g .* (A B^T + bias) on ragged M (every tile config), and the LayerNorm
    backward whose bf16 copy alone is gated."""
    M, N, K, rows, layer, branch, p = 333, 384, 256, 111, 2, 1, 0.5     # (p = 1 / 2: the gate's factors are powers of two, products exact)
    A, B = G.bf16_randn(M, K, seed=1), G.bf16_randn(N, K, scale=0.05, seed=2)
    bias, resid = torch.randn(N, device=dev), torch.randn(M, N, device=dev)
    scale = torch.tensor([[[1.0, 1.0, 1.0]] * 2] * 2 + [[[1.0, 1.0, 1.0], [2.0, 0.0, 2.0]]], device=dev)      # [3 layers][2][3 samples]
    drop = bvc._lib.branch_drop(p, 77, 8, scale, rows)
    keep = dg.dropout_mask(77, 8, layer, branch, M, N, p, dev).float()
    g = scale[layer, branch].repeat_interleave(rows)[:, None] * keep / (1 - p)
    ref = resid + g * (A.float() @ B.float().t() + bias)
    import ctypes
    for cfg_ in (-1, 0, 1, 2):
        C = torch.full((M, N), float("nan"), device=dev)
        d = G.gemm_desc(A, B, M, N, K, 15, C, bias=bias, resid=resid)
        bvc._lib.check(bvc._lib.lib().bvc_op_gemm_gate(ctypes.byref(d), ctypes.byref(drop), layer, branch, cfg_, G.stream()), "bvc_op_gemm_gate")
        assert G.rel_err(C, ref) < 1e-5, cfg_
        assert torch.equal(C[rows:2 * rows], resid[rows:2 * rows])          # the dropped sample: exactly the residual
    with pytest.raises(bvc._lib.BvcError, match="RESID_GATE"):
        G.run_gemm([G.gemm_desc(A, B, M, N, K, 15, C, bias=bias, resid=resid)], G.NT)
    # LayerNorm backward
    D = N
    x, dy = torch.randn(M, D, device=dev), G.bf16_randn(M, D, seed=3)
    gamma = torch.randn(D, device=dev)
    mean, var = x.mean(1), x.var(1, unbiased=False)
    rstd = (var + 1e-5).rsqrt()
    outs = []
    for gated in (False, True):
        dres, dbf = torch.randn(M, D, generator=torch.Generator(device=dev).manual_seed(1), device=dev), torch.empty(M, D, dtype=torch.bfloat16, device=dev)
        dgm, dbt = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        ws = torch.empty(int(bvc._lib.lib().bvc_op_layernorm_bwd_workspace(M, D)), device=dev)
        L = bvc._lib.lib()
        if gated:
            bvc._lib.check(L.bvc_op_layernorm_bwd_gate(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dres.data_ptr(),
                                                       1, dbf.data_ptr(), dgm.data_ptr(), dbt.data_ptr(), ws.data_ptr(), M, D, ctypes.byref(drop),
                                                       layer, branch, G.stream()), "ln_bwd_gate")
        else:
            bvc._lib.check(L.bvc_op_layernorm_bwd(dy.data_ptr(), x.data_ptr(), 0, 0, 0, mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dres.data_ptr(),
                                                  1, dbf.data_ptr(), dgm.data_ptr(), dbt.data_ptr(), ws.data_ptr(), M, D, G.stream()), "ln_bwd")
        outs.append((dres, dbf, dgm, dbt))
    (r0, b0, g0, t0), (r1, b1, g1, t1) = outs
    assert torch.equal(r0, r1)                                    # the residual gradient passes ungated
    # ... and so do the LayerNorm's parameter gradients (their partial rows are added by f32 atomics: equal to round-off)
    assert G.rel_err(g1, g0) < 1e-5 and G.rel_err(t1, t0) < 1e-5
    assert torch.equal(b0, r0.to(torch.bfloat16)) and torch.equal(b1, (r1 * g).to(torch.bfloat16))


# ----------------------------------------------------------------------------- 7: the fine-tuning step
def _seeded_step(m, pixels, labels, one_sample=False):
    """Forward + backward on the first seed whose reported gates are exercised."""
    px, y = pixels.to(dev), labels.to(dev)
    for seed in range(32):
        torch.manual_seed(seed)
        m.zero_grad(set_to_none=True)
        out = m(pixel_values=px, labels=y)
        if dr.scale_exercised(m.drop_path_scale, m._gate.rates, one_sample):
            out.loss.backward()
            torch.cuda.synchronize()
            return seed, out
    raise AssertionError("none of the first 32 seeds exercised the stochastic-depth gate")


def _cls_gates(m, cfg, B):
    seed, off, p = m.dropout_state
    M = B * cfg.seq_len
    fn = (lambda l, b: dg.dropout_mask(seed, off, l, b, M, cfg.hidden_size, p, dev)) if p > 0 else None
    return dr.make_gates(cfg.num_hidden_layers, B, cfg.seq_len, cfg.hidden_size, m.drop_path_scale, fn, p)


def _check_cls(tag, cfg, B, seed, hidden_p=0.1, drop_path=0.5):
    params, heads = vo.make_params(cfg, seed=0), _heads(cfg)
    pixels, _ = vo.synthetic_batch(cfg, B, seed, 0.9)
    labels = torch.arange(B) % NL
    m = _model(cfg, params, heads, hidden_dropout_prob=hidden_p, drop_path_rate=drop_path)
    used, out = _seeded_step(m, pixels, labels, one_sample=B == 1)
    assert m._train.h is not None and tuple(m.drop_path_scale.shape) == (cfg.num_hidden_layers, 2, B) and m.dropout_state[2] == hidden_p
    ref_loss, ref_logits, ref_grads = dr.cls_step(cfg, params, heads, pixels, lambda z: F.cross_entropy(z, labels), _cls_gates(m, cfg, B))
    rel = abs(float(out.loss.detach()) - float(ref_loss)) / abs(float(ref_loss))
    el = G.rel_err(out.logits.detach().float().cpu(), ref_logits)
    G.log_parity(f"[{tag}] seed {used} loss hip {float(out.loss.detach()):.7f} ref {float(ref_loss):.7f} rel {rel:.2e}; logits rel {el:.2e}; "
                 f"kept branches {int((m.drop_path_scale != 0).sum())} of {m.drop_path_scale.numel()}")
    assert rel < 1e-3 and el < 2e-2
    named = dict(m.named_parameters())
    gmax = max(float(g.norm()) for k, g in ref_grads.items() if k.startswith("videomae."))
    worst = ("", 0.0)
    for k, r in ref_grads.items():
        g = named[k].grad.float().cpu()
        assert torch.isfinite(g).all(), k
        if k.startswith("videomae."):
            e = float((g - r).norm() / (r.norm() + 1e-3 * gmax))
            worst = max(worst, (k, e), key=lambda t: t[1])
            assert e < 5e-2, (k, e)
        else:
            e = float((g - r).norm() / r.norm())
            assert e < 2e-2, (k, e)
    G.log_parity(f"[{tag}] worst encoder per-tensor grad rel {worst[1]:.2e} ({worst[0]})")
    return m


def test_tiny_gated_finetune_step_matches_reference():
    _check_cls("drop_cls_tiny", vo.TINY, 4, 0)


@pytest.mark.parametrize("frames,tubelet,image,patch,B", [(2, 1, 64, 16, 3), (8, 2, 96, 16, 2), (4, 4, 64, 16, 5), (4, 2, 128, 32, 1)])
def test_gated_finetune_config_matrix_small(frames, tubelet, image, patch, B):
    cfg = dataclasses.replace(vo.TINY, num_frames=frames, tubelet_size=tubelet, image_size=image, patch_size=patch)
    _check_cls(f"drop_cls_f{frames}_t{tubelet}_i{image}_p{patch}", cfg, B, seed=7)


def test_small_gated_finetune_step_matches_reference():
    """384 wide: the configuration whose LayerNorms would run inside the 384-wide products' epilogues - they step aside for the gate
    (forced on here as tests/test_gpu_jepa.py forces it, so the stepping aside is what is tested)."""
    old = bvc._lib.set_option("row_ln", 1)
    try:
        assert bvc._lib.lib().bvc_op_row_ln_selected(2 * 1568, 384, 1536, 6) == 1
        _check_cls("drop_cls_small_b2", SMALL, 2, 1)
    finally:
        bvc._lib.set_option("row_ln", old)


def test_base_gated_finetune_step_matches_reference():
    _check_cls("drop_cls_base_b2", vo.BASE, 2, 0)


# ----------------------------------------------------------------------------- 8: the JEPA step
def _jepa_modules(cfg, enc_p, pred_p, tgt_p, rate):
    kw = dict(img_size=[cfg.image_size], patch_size=cfg.patch_size, num_frames=cfg.num_frames, tubelet_size=cfg.tubelet_size,
              embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio)
    enc = bvc.jepa.VisionTransformer(drop_path_rate=rate, **kw)
    enc.load_state_dict(enc_p)
    tgt = bvc.jepa.VisionTransformer(**kw)
    tgt.load_state_dict(tgt_p)
    pred = bvc.jepa.vit_predictor(sequence_shape=enc.sequence_shape, embed_dim=cfg.embed_dim, predictor_embed_dim=cfg.pred_dim,
                                  depth=cfg.pred_depth, num_heads=enc.num_heads, drop_path_rate=rate)
    pred.load_state_dict(pred_p)
    for p in tgt.parameters():
        p.requires_grad = False
    return enc.to(dev).train(), pred.to(dev).train(), tgt.to(dev).eval()


@pytest.mark.parametrize("forced_row_ln", [False, True])
@pytest.mark.parametrize("name", ["TINY", "TINY_HD24"])
def test_gated_jepa_train_step_matches_reference(name, forced_row_ln):
    base = getattr(jo, name)
    cfg = dataclasses.replace(base, depth=max(base.depth, 2), pred_depth=max(base.pred_depth, 2))
    B, n_ctx, n_pred, nsets, scale = 4, 8, 4, 4, 1024.0
    enc_p = jo.make_params(jo.encoder_shapes(cfg), cfg, 11)
    pred_p = jo.make_params(jo.predictor_shapes(cfg), cfg, 61)
    tgt_p = jo.make_params(jo.encoder_shapes(cfg), cfg, 111)
    imgs, m_enc, m_pred = jo.synthetic_inputs(cfg, B, 11, n_ctx, n_pred, nsets)
    old = bvc._lib.set_option("row_ln", 1) if forced_row_ln else None
    try:
        enc, pred, tgt = _jepa_modules(cfg, enc_p, pred_p, tgt_p, 0.5)
        x, me, mp = imgs.to(dev), [m.to(dev) for m in m_enc], [m.to(dev) for m in m_pred]
        with torch.no_grad():
            h = bvc.jepa.select_targets(tgt(x), mp)
        for seed in range(32):
            torch.manual_seed(seed)
            enc.zero_grad(set_to_none=True)
            pred.zero_grad(set_to_none=True)
            z = pred(enc(x, me), me, mp)
            if dr.scale_exercised(enc.drop_path_scale, enc._gate.rates) and dr.scale_exercised(pred.drop_path_scale, pred._gate.rates):
                break
        else:
            raise AssertionError("none of the first 32 seeds exercised both stochastic-depth gates")
        loss = bvc.jepa.smooth_l1_loss(z, h)
        (loss * scale).backward()
        torch.cuda.synchronize()
    finally:
        if forced_row_ln:
            bvc._lib.set_option("row_ln", old)
    assert tuple(enc.drop_path_scale.shape) == (cfg.depth, 2, B) and tuple(pred.drop_path_scale.shape) == (cfg.pred_depth, 2, nsets * B)
    eg = dr.make_gates(cfg.depth, B, n_ctx, cfg.embed_dim, enc.drop_path_scale)
    pg = dr.make_gates(cfg.pred_depth, nsets * B, n_ctx + n_pred, cfg.pred_dim, pred.drop_path_scale)
    rloss, rge, rgp, rz, rh = dr.jepa_step(cfg, enc_p, pred_p, tgt_p, imgs, m_enc, m_pred, eg, pg, grad_scale=scale)
    eh, ez = G.rel_err(h.cpu(), rh), G.rel_err(z.detach().cpu(), rz)
    rel = abs(float(loss) - float(rloss)) / float(rloss)
    tag = f"drop_jepa {name}{' row_ln' if forced_row_ln else ''}"
    G.log_parity(f"[{tag}] seed {seed} loss hip {float(loss):.7f} ref {float(rloss):.7f} rel {rel:.2e}; h rel {eh:.2e}, z rel {ez:.2e}")
    assert eh < 2e-2 and ez < 2e-2 and rel < 1e-3
    gmax = max(float(g.norm()) for g in list(rge.values()) + list(rgp.values()))
    worst = ("", 0.0)
    for mod, ref in ((enc, rge), (pred, rgp)):
        for k, p in mod.named_parameters():
            if not p.requires_grad:
                continue
            e = float((p.grad.float().cpu() - ref[k]).norm() / (ref[k].norm() + 1e-3 * gmax))
            worst = max(worst, (k, e), key=lambda t: t[1])
            assert e < 5e-2, (k, e)
    G.log_parity(f"[{tag}] worst per-tensor gradient rel L2 {worst[1]:.2e} ({worst[0]})")


# ----------------------------------------------------------------------------- 9: exactness
def _grads(m):
    return [p.grad.clone() for p in m.parameters()]


def test_eval_mode_and_zero_rates_are_bit_identical_to_a_model_without_the_keywords():
    cfg = vo.TINY
    params, heads = vo.make_params(cfg, seed=1), _heads(cfg)
    px = vo.synthetic_batch(cfg, 3, 2, 0.9)[0].to(dev)
    y = torch.tensor([1, 4, 9], device=dev)
    plain = _model(cfg, params, heads)
    ref = plain(pixel_values=px, labels=y)
    ref.loss.backward()
    # (a) rates set, eval(): the same logits
    ev = _model(cfg, params, heads, train=False, hidden_dropout_prob=0.3, drop_path_rate=0.5)
    with torch.no_grad():
        assert torch.equal(ev(pixel_values=px).logits, ref.logits.detach())
    assert ev.drop_path_scale is None and ev.dropout_state is None
    # (b) train mode, all rates 0.0: loss, logits and every gradient
    zero = _model(cfg, params, heads, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0)
    out = zero(pixel_values=px, labels=y)
    out.loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(out.loss, ref.loss) and torch.equal(out.logits, ref.logits)
    assert all(torch.equal(a, b) for a, b in zip(_grads(zero), _grads(plain)))
    assert zero.drop_path_scale is None
    # ... and the selection of the ungated products is what it was: a residual product still names the kernel it always named
    import ctypes
    A, B = G.bf16_randn(256, 128), G.bf16_randn(128, 128)
    C = torch.zeros(256, 128, device=dev)
    d = G.gemm_desc(A, B, 256, 128, 128, G.EPI["RESID"], C, resid=C)
    name = ctypes.create_string_buffer(160)
    bvc._lib.check(bvc._lib.lib().bvc_op_gemm_kernel(ctypes.byref(d), 1, G.NT, -1, -1, name, 160), "bvc_op_gemm_kernel")
    assert b"gate" not in name.value and name.value.startswith(b"bvc::gemm")
    bvc._lib.check(bvc._lib.lib().bvc_op_gemm_gate_kernel(ctypes.byref(d), -1, name, 160), "bvc_op_gemm_gate_kernel")
    assert name.value.startswith(b"bvc::gemm_gate_kernel<")


def test_same_seed_is_bit_identical_in_deterministic_mode_and_another_seed_differs():
    cfg = vo.TINY
    params, heads = vo.make_params(cfg, seed=2), _heads(cfg)
    px = vo.synthetic_batch(cfg, 4, 3, 0.9)[0].to(dev)
    y = torch.tensor([1, 2, 3, 4], device=dev)
    bvc.use_deterministic_algorithms(True)
    try:
        runs = []
        for seed in (5, 5, 6):
            m = _model(cfg, params, heads, hidden_dropout_prob=0.1, drop_path_rate=0.5)
            torch.manual_seed(seed)
            out = m(pixel_values=px, labels=y)
            out.loss.backward()
            torch.cuda.synchronize()
            runs.append((out.loss.detach().clone(), out.logits.detach().clone(), _grads(m), m.drop_path_scale.clone(), m.dropout_state))
    finally:
        bvc.use_deterministic_algorithms(False)
    a, b, c = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(u, v) for u, v in zip(a[2], b[2]))
    assert torch.equal(a[3], b[3]) and a[4] == b[4]
    assert not torch.equal(a[3], c[3]) or a[4] != c[4]
    assert a[4][0] != c[4][0] and not torch.equal(a[1], c[1])


def test_a_dropped_mlp_branch_contributes_exactly_zero_to_its_bias_gradient():
    cfg = vo.TINY
    params, heads = vo.make_params(cfg, seed=3), _heads(cfg)
    px, y = vo.synthetic_batch(cfg, 1, 4, 0.9)[0], torch.tensor([3])
    m = _model(cfg, params, heads, hidden_dropout_prob=0.1, drop_path_rate=0.5)
    _seeded_step(m, px, y, one_sample=True)
    s = m.drop_path_scale.cpu()
    named = dict(m.named_parameters())
    seen = 0
    for layer in range(cfg.num_hidden_layers):
        for branch, key in ((0, "attention.output.dense.bias"), (1, "output.dense.bias")):
            g = named[f"videomae.encoder.layer.{layer}.{key}"].grad
            if float(s[layer, branch, 0]) == 0.0:
                assert float(g.abs().max()) == 0.0, (layer, branch)          # forward and backward used the same gate
                seen += branch
            else:
                assert float(g.abs().max()) > 0.0
    assert seen >= 1


def test_train_mode_inference_context_equals_the_finetuning_path_bit_for_bit():
    cfg = vo.TINY
    params, heads = vo.make_params(cfg, seed=4), _heads(cfg)
    px = vo.synthetic_batch(cfg, 3, 5, 0.9)[0].to(dev)
    m = _model(cfg, params, heads, hidden_dropout_prob=0.1, drop_path_rate=0.5)
    torch.manual_seed(9)
    a = m(pixel_values=px).logits.detach().clone()
    sa, da = m.drop_path_scale.clone(), m.dropout_state
    assert m._train.h is not None
    torch.manual_seed(9)
    with torch.no_grad():
        b = m(pixel_values=px).logits.clone()
    assert torch.equal(sa, m.drop_path_scale) and da == m.dropout_state
    assert torch.equal(a, b)
    m.eval()
    with torch.no_grad():
        c = m(pixel_values=px).logits
    assert not torch.equal(a, c)
    # a train-mode linear probe (frozen encoder): the inference context, gated alike
    m.train()
    for n, p in m.named_parameters():
        p.requires_grad = not n.startswith("videomae.")
    torch.manual_seed(9)
    d = m(pixel_values=px, labels=torch.tensor([0, 1, 2], device=dev))
    d.loss.backward()
    assert torch.equal(d.logits.detach(), a) and m.fc_norm.weight.grad is not None


# ----------------------------------------------------------------------------- 10: data-parallel training
def test_three_gated_optimiser_steps_under_ddp_single_rank(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setenv("BVC_COMM", "bvc")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29547"
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        cfg = vo.TINY
        params, heads = vo.make_params(cfg, seed=5), _heads(cfg)
        px = vo.synthetic_batch(cfg, 4, 4, 0.9)[0].to(dev)
        y = torch.tensor([0, 1, 2, 3], device=dev)
        model = _model(cfg, params, heads, hidden_dropout_prob=0.1, drop_path_rate=0.2)
        ddp = bvc.DistributedDataParallel(model, device_ids=[0], output_device=0, bucket_cap_mb=0.05, force_collectives=True)
        opt = torch.optim.SGD(ddp.parameters(), lr=0.05, momentum=0.9)
        ranges = []
        hook = model._bucket_hook
        model._bucket_hook = lambda off, cnt: (ranges.append((off, off + cnt)), hook(off, cnt))
        torch.manual_seed(0)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            ranges.clear()
            out = ddp(pixel_values=px, labels=y)
            out.loss.backward()
            opt.step()
            losses.append(float(out.loss))
            rs = sorted(ranges)          # every range once, together the whole flat buffer
            assert rs[0][0] == 0 and rs[-1][1] == model.flat_grads().numel() and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
            assert len(set(ranges)) == len(ranges)
        torch.cuda.synchronize()
        assert all(l == l and l != float("inf") for l in losses) and torch.isfinite(model.flat_parameters()).all()
        # the fixed batch under the eval-mode (ungated) model: the three steps lowered its loss
        model.eval()
        with torch.no_grad():
            after = float(model(pixel_values=px, labels=y).loss)
        before = float(_model(cfg, params, heads, train=False)(pixel_values=px, labels=y).loss)
        G.log_parity(f"[drop_ddp] gated step losses {losses}; eval loss on the batch {before:.5f} -> {after:.5f}")
        assert after < before and losses[-1] < losses[0]
    finally:
        bvc.comm.reset()
        dist.destroy_process_group()
