"""Fine-tuning VideoMAEForVideoClassification on the GPU: labels, loss and backward through the library's encoder.

Bars: loss within 1e-3 relative of the fp32 CPU oracle restated under autograd (vo.encode -> F.layer_norm -> F.linear -> loss);
encoder per-tensor gradients within 5e-2 relative L2 (with _check_step's floor for the tensors whose true gradient is ~0);
fc_norm and classifier gradients within 2e-2; logits within 2e-2 of the transformers fixture.
"""
import dataclasses
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402
from tools.make_videomae_cls_golden import head_params   # noqa: E402
from tests.test_gpu_videomae import _log   # noqa: E402  (the pre-training parity tests' report: one file for the whole suite)

bvc = G.bvc
dev = torch.device("cuda:0")
NL = 10


def _heads(cfg, num_labels=NL, seed=5):
    return dict(zip(("fc_norm.weight", "fc_norm.bias", "classifier.weight", "classifier.bias"), head_params(cfg.hidden_size, num_labels, seed)))


def _model(cfg, params, heads, num_labels=NL, train=True):
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    m = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(num_labels=num_labels, **kw))
    sd = {k: v for k, v in params.items() if k.startswith("videomae.")}
    sd.update({k: v for k, v in heads.items() if num_labels > 0 or k.startswith("fc_norm")})
    m.load_state_dict(sd)
    m.to(dev)
    return m.train() if train else m.eval()


def _oracle(cfg, params, heads, pixels, loss_fn):
    """fp32 CPU restatement under autograd: (loss, logits, grads)."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in params.items() if k.startswith("videomae.")}
    p.update({k: v.detach().clone().requires_grad_(True) for k, v in heads.items()})
    pooled, _ = vo.encode(cfg, p, pixels, p["fc_norm.weight"], p["fc_norm.bias"], 1e-5)
    logits = F.linear(pooled, p["classifier.weight"], p["classifier.bias"])
    loss = loss_fn(logits)
    loss.backward()
    return loss.detach(), logits.detach(), {k: v.grad for k, v in p.items()}


def _grad_errs(model, ref_grads, tag):
    named = dict(model.named_parameters())
    enc = {k: v for k, v in ref_grads.items() if k.startswith("videomae.")}
    gmax = max(float(g.norm()) for g in enc.values())
    worst = ("", 0.0)
    for k, r in ref_grads.items():
        g = named[k].grad
        assert g is not None, k
        g = g.float().cpu()
        assert torch.isfinite(g).all(), k
        if k.startswith("videomae."):
            e = float((g - r).norm() / (r.norm() + 1e-3 * gmax))
            if e > worst[1]:
                worst = (k, e)
            assert e < 5e-2, (k, e)
        else:
            e = float((g - r).norm() / r.norm())
            _log(f"[{tag}] grad {k} rel {e:.2e}")
            assert e < 2e-2, (k, e)
    _log(f"[{tag}] worst encoder per-tensor grad rel {worst[1]:.2e} ({worst[0]})")


def _check_cls(tag, cfg, B, seed):
    params = vo.make_params(cfg, seed=0)
    heads = _heads(cfg)
    pixels, _ = vo.synthetic_batch(cfg, B, seed, 0.9)
    labels = torch.arange(B) % NL
    ref_loss, ref_logits, ref_grads = _oracle(cfg, params, heads, pixels, lambda z: F.cross_entropy(z, labels))
    m = _model(cfg, params, heads)
    out = m(pixel_values=pixels.to(dev), labels=labels.to(dev))
    out.loss.backward()
    torch.cuda.synchronize()
    rel = abs(float(out.loss.detach()) - float(ref_loss)) / abs(float(ref_loss))
    el = G.rel_err(out.logits.detach().float().cpu(), ref_logits)
    _log(f"[{tag}] loss hip {float(out.loss.detach()):.7f} oracle {float(ref_loss):.7f} rel {rel:.2e}; logits rel {el:.2e}")
    assert rel < 1e-3 and el < 2e-2
    assert m._train.h is not None and m.config.problem_type == "single_label_classification"
    _grad_errs(m, ref_grads, tag)
    return m


def test_tiny_finetune_step_matches_oracle():
    _check_cls("cls_tiny", vo.TINY, 2, 0)


@pytest.mark.parametrize("frames,tubelet,image,patch,B", [(2, 1, 64, 16, 3), (8, 2, 96, 16, 2), (4, 4, 64, 16, 5), (4, 2, 128, 32, 1)])
def test_finetune_config_matrix_small(frames, tubelet, image, patch, B):
    """Ragged tile edges, one-clip batches, tube depth = all frames (test_config_matrix_small's geometries)."""
    cfg = dataclasses.replace(vo.TINY, num_frames=frames, tubelet_size=tubelet, image_size=image, patch_size=patch)
    _check_cls(f"cls_f{frames}_t{tubelet}_i{image}_p{patch}", cfg, B, seed=7)


def test_base_b2_matches_transformers_fixture(golden_dir):
    fx = json.load(open(os.path.join(golden_dir, "videomae_cls_base_b2_s0.json")))
    cfg = vo.BASE
    params = vo.make_params(cfg, seed=fx["weight_seed"])
    heads = _heads(cfg, fx["num_labels"], fx["head_seed"])
    pixels, _ = vo.synthetic_batch(cfg, fx["batch"], fx["seed"], 0.9)
    m = _model(cfg, params, heads, fx["num_labels"])
    out = m(pixel_values=pixels.to(dev), labels=torch.tensor(fx["labels"], device=dev))
    out.loss.backward()
    torch.cuda.synchronize()
    rel = abs(float(out.loss) - fx["loss"]) / fx["loss"]
    el = G.rel_err(out.logits.detach().float().cpu(), torch.tensor(fx["logits"]))
    _log(f"[cls_base_b2_s0] loss hip {float(out.loss):.7f} transformers {fx['loss']:.7f} rel {rel:.2e}; logits rel {el:.2e}")
    assert rel < 1e-3 and el < 2e-2
    named = dict(m.named_parameters())
    worst = ("", 0.0)
    gmax = max(fx["grad_l2"].values())
    for k, n in fx["grad_l2"].items():
        gn = float(named[k].grad.double().norm())
        e = abs(gn - n) / (n + 1e-3 * gmax)
        if e > worst[1]:
            worst = (k, e)
        assert e < 5e-2, (k, gn, n)
    pe = "videomae.embeddings.patch_embeddings.projection.weight"
    gpe = float(named[pe].grad.double().norm())
    _log(f"[cls_base_b2_s0] grad-norm {pe}: hip {gpe:.6e} transformers {fx['grad_l2'][pe]:.6e} "
         f"rel {(gpe - fx['grad_l2'][pe]) / fx['grad_l2'][pe]:+.2e}; worst grad-norm rel {worst[1]:.2e} ({worst[0]})")


def test_train_logits_equal_inference_and_uint8_bitwise():
    cfg = vo.TINY
    params, heads = vo.make_params(cfg, seed=1), _heads(cfg)
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (3, cfg.num_frames, cfg.num_channels, cfg.image_size, cfg.image_size), generator=g, dtype=torch.uint8)
    f32 = (u8.float() / 255.0 - 0.5) / 0.25
    labels = torch.tensor([1, 4, 9], device=dev)
    res = []
    for px in (f32, u8):
        m = _model(cfg, params, heads)
        out = m(pixel_values=px.to(dev), labels=labels, output_last_hidden_state=True)
        assert out.logits.requires_grad and not out.last_hidden_state.requires_grad
        out.loss.backward()
        torch.cuda.synchronize()
        res.append((out.loss.detach().cpu(), out.logits.detach().cpu(), m.flat_grads().cpu().clone(), m.fc_norm.weight.grad.cpu(),
                    out.last_hidden_state.cpu()))
        m.eval()
        ev = m(pixel_values=px.to(dev), output_last_hidden_state=True)
        with torch.no_grad():
            ng = m(pixel_values=px.to(dev))
        assert torch.equal(ev.logits.detach().cpu(), res[-1][1]) and torch.equal(ng.logits.cpu(), res[-1][1])
        assert torch.equal(ev.last_hidden_state.cpu(), res[-1][4])
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def test_path_selection_and_linear_probe():
    cfg = vo.TINY
    params, heads = vo.make_params(cfg, seed=2), _heads(cfg)
    pixels = vo.synthetic_batch(cfg, 2, 1, 0.9)[0].to(dev)
    y = torch.tensor([0, 5], device=dev)
    m = _model(cfg, params, heads, train=False)
    with pytest.warns(UserWarning, match="eval mode"):
        m(pixel_values=pixels, labels=y).loss.backward()
    assert m._train.h is None and all(p.grad is None for n, p in m.named_parameters() if n.startswith("videomae."))
    assert m.classifier.weight.grad is not None and m.fc_norm.weight.grad is not None
    m.train()
    with torch.no_grad():
        out = m(pixel_values=pixels, labels=y)
    assert m._train.h is None and not out.logits.requires_grad

    # set_parameter_requires_grad(model, feature_extracting=True) with the classifier re-enabled: classifier gradient as torch's
    for p in m.parameters():
        p.requires_grad = False
    for p in m.classifier.parameters():
        p.requires_grad = True
    for fc_trainable in (False, True):
        for p in m.fc_norm.parameters():
            p.requires_grad = fc_trainable
            p.grad = None
        m.classifier.zero_grad(set_to_none=True)
        out = m(pixel_values=pixels, labels=y, output_last_hidden_state=True)
        out.loss.backward()
        assert m._train.h is None and all(p.grad is None for n, p in m.named_parameters() if n.startswith("videomae."))
        tok = out.last_hidden_state.detach().mean(1)
        fw, fb = m.fc_norm.weight.detach().clone().requires_grad_(), m.fc_norm.bias.detach().clone().requires_grad_()
        cw, cb = m.classifier.weight.detach().clone().requires_grad_(), m.classifier.bias.detach().clone().requires_grad_()
        logits = F.linear(F.layer_norm(tok, (cfg.hidden_size,), fw, fb, 1e-5), cw, cb)
        assert G.rel_err(logits.detach(), out.logits.detach()) < 1e-5
        F.cross_entropy(logits, y).backward()
        assert G.rel_err(m.classifier.weight.grad, cw.grad) < 1e-5 and G.rel_err(m.classifier.bias.grad, cb.grad) < 1e-5
        if fc_trainable:
            assert G.rel_err(m.fc_norm.weight.grad, fw.grad) < 1e-4 and G.rel_err(m.fc_norm.bias.grad, fb.grad) < 1e-4
        else:
            assert m.fc_norm.weight.grad is None


def _restated_loop(cfg, params, heads, batches, make_opt):
    p = {k: v.detach().clone().requires_grad_(True) for k, v in params.items() if k.startswith("videomae.")}
    p.update({k: v.detach().clone().requires_grad_(True) for k, v in heads.items()})
    opt = make_opt(list(p.values()))
    losses = []
    for px, y in batches:
        opt.zero_grad()
        pooled, _ = vo.encode(cfg, p, px, p["fc_norm.weight"], p["fc_norm.bias"], 1e-5)
        loss = F.cross_entropy(F.linear(pooled, p["classifier.weight"], p["classifier.bias"]), y)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return losses, {k: v.detach() for k, v in p.items()}


@pytest.mark.parametrize("which", ["adamw_scaler", "sgd_nesterov"])
def test_three_step_training_loop(which):
    cfg = vo.TINY
    params, heads = vo.make_params(cfg, seed=3), _heads(cfg)
    batches = [(vo.synthetic_batch(cfg, 4, s, 0.9)[0], torch.tensor([s % NL, 3, 7, (2 * s) % NL])) for s in range(3)]
    if which == "adamw_scaler":
        mk_ref = lambda ps: torch.optim.AdamW(ps, lr=1e-3, weight_decay=0.05)       # noqa: E731
        mk = lambda ps: bvc.optim.AdamW(ps, lr=1e-3, weight_decay=0.05)            # noqa: E731
    else:
        mk_ref = lambda ps: torch.optim.SGD(ps, lr=0.05, momentum=0.9, nesterov=True)   # noqa: E731
        mk = mk_ref
    ref_losses, ref_params = _restated_loop(cfg, params, heads, batches, mk_ref)
    m = _model(cfg, params, heads)
    opt = mk(list(m.parameters()))
    scaler = torch.amp.GradScaler("cuda") if which == "adamw_scaler" else None
    for i, (px, y) in enumerate(batches):
        opt.zero_grad()
        out = m(pixel_values=px.to(dev), labels=y.to(dev))
        if scaler is not None:
            scaler.scale(out.loss).backward()
            scaler.step(opt)
            scaler.update()
        else:
            out.loss.backward()
            opt.step()
        rel = abs(float(out.loss) - ref_losses[i]) / ref_losses[i]
        _log(f"[cls_loop {which}] step {i} loss hip {float(out.loss):.7f} oracle {ref_losses[i]:.7f} rel {rel:.2e}")
        assert rel < 1e-3
    torch.cuda.synchronize()
    sd = m.state_dict()
    # AdamW moves every element by about lr per step whatever its gradient: tensors whose true gradient is ~0 (key.bias) take
    # bf16-noise-directed steps, so the distance is measured against |p| plus the size of three such steps (_check_step's floor)
    # The key biases are left out under AdamW: their exact gradient is zero (softmax is invariant to q . b_k), so both runs step them
    # by Adam-normalised round-off in unrelated directions.
    adam = which == "adamw_scaler"
    floor = (lambda v: 3 * 1e-3 * v.numel() ** 0.5) if adam else (lambda v: 0.0)
    worst = max((float((sd[k].float().cpu() - v).norm() / (v.norm() + floor(v))), k) for k, v in ref_params.items()
                if not (adam and k.endswith("attention.attention.key.bias")))
    _log(f"[cls_loop {which}] worst parameter rel after 3 steps {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < 2e-2


def test_gradient_accumulation_frozen_and_deterministic():
    cfg = vo.TINY
    params, heads = vo.make_params(cfg, seed=4), _heads(cfg)
    px = vo.synthetic_batch(cfg, 4, 2, 0.9)[0].to(dev)
    y = torch.tensor([1, 2, 3, 4], device=dev)
    one = _model(cfg, params, heads)
    one(pixel_values=px, labels=y).loss.backward()
    two = _model(cfg, params, heads)
    for sl in (slice(0, 2), slice(2, 4)):
        (0.5 * two(pixel_values=px[sl], labels=y[sl]).loss).backward()
    torch.cuda.synchronize()
    for (k, a), (_k, b) in zip(one.named_parameters(), two.named_parameters()):
        assert G.rel_err(b.grad, a.grad) < 1e-4, k

    # a frozen patch embedding keeps .grad None; the rest still trains
    fr = _model(cfg, params, heads)
    pe = fr.videomae.embeddings.patch_embeddings.projection
    pe.weight.requires_grad_(False)
    pe.bias.requires_grad_(False)
    fr(pixel_values=px, labels=y).loss.backward()
    assert pe.weight.grad is None and pe.bias.grad is None
    w = "videomae.encoder.layer.0.output.dense.weight"
    assert G.rel_err(dict(fr.named_parameters())[w].grad, dict(one.named_parameters())[w].grad) < 1e-6

    # deterministic mode: two runs, the same bits
    bvc.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            m = _model(cfg, params, heads)
            m(pixel_values=px, labels=y).loss.backward()
            torch.cuda.synchronize()
            runs.append([p.grad.clone() for p in m.parameters()])
        assert all(torch.equal(a, b) for a, b in zip(*runs))
    finally:
        bvc.use_deterministic_algorithms(False)


def test_ddp_single_rank_matches_unwrapped(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setenv("BVC_COMM", "torch")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29541"
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        cfg = vo.TINY
        params, heads = vo.make_params(cfg, seed=5), _heads(cfg)
        px = vo.synthetic_batch(cfg, 3, 4, 0.9)[0].to(dev)
        y = torch.tensor([0, 1, 2], device=dev)
        plain = _model(cfg, params, heads)
        plain(pixel_values=px, labels=y).loss.backward()
        model = _model(cfg, params, heads)
        ranges = []
        ddp = bvc.DistributedDataParallel(model, device_ids=[0], output_device=0, bucket_cap_mb=0.05, force_collectives=True)
        assert len(ddp._flats) == 1 and len(ddp._loose_grad) == 4       # fc_norm and classifier weight / bias
        hook = model._bucket_hook
        model._bucket_hook = lambda off, cnt: (ranges.append((off, off + cnt)), hook(off, cnt))
        ddp(pixel_values=px, labels=y).loss.backward()
        torch.cuda.synchronize()
        for (k, a), (_k, b) in zip(model.named_parameters(), plain.named_parameters()):
            assert G.rel_err(a.grad, b.grad) < 1e-6, k
        rs = sorted(ranges)
        assert rs[0][0] == 0 and rs[-1][1] == model.flat_grads().numel() and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
        assert [r for r in ranges] == sorted(ranges, reverse=True)           # tail first
    finally:
        bvc.comm.reset()
        dist.destroy_process_group()


def test_loss_types_follow_transformers():
    cfg = vo.TINY
    params = vo.make_params(cfg, seed=6)
    px = vo.synthetic_batch(cfg, 4, 3, 0.9)[0].to(dev)
    # regression
    m = _model(cfg, params, _heads(cfg, 1), num_labels=1)
    y = torch.randn(4, device=dev)
    out = m(pixel_values=px, labels=y)
    assert m.config.problem_type == "regression"
    assert torch.allclose(out.loss, F.mse_loss(out.logits.squeeze(), y.squeeze()), rtol=1e-6, atol=0)
    out.loss.backward()
    # single label, -100 ignored
    m = _model(cfg, params, _heads(cfg))
    y = torch.tensor([2, -100, 5, -100], device=dev)
    out = m(pixel_values=px, labels=y)
    assert m.config.problem_type == "single_label_classification"
    assert torch.allclose(out.loss, F.cross_entropy(out.logits[[0, 2]], y[[0, 2]]), rtol=1e-6, atol=0)
    out.loss.backward()
    # multi label
    m = _model(cfg, params, _heads(cfg))
    y = (torch.rand(4, NL, device=dev) > 0.5).float()
    out = m(pixel_values=px, labels=y)
    assert m.config.problem_type == "multi_label_classification"
    assert torch.allclose(out.loss, F.binary_cross_entropy_with_logits(out.logits, y), rtol=1e-6, atol=0)
    out.loss.backward()
    assert m.videomae.embeddings.patch_embeddings.projection.weight.grad is not None


def test_errors():
    cfg = vo.TINY
    params, heads = vo.make_params(cfg, seed=7), _heads(cfg)
    m = _model(cfg, params, heads)
    px = vo.synthetic_batch(cfg, 2, 0, 0.9)[0]
    with pytest.raises(bvc._lib.BvcError):
        m(pixel_values=px, labels=torch.tensor([0, 1]))
    # a backward after a newer forward
    y = torch.tensor([0, 1], device=dev)
    first = m(pixel_values=px.to(dev), labels=y)
    m(pixel_values=px.to(dev), labels=y)
    with pytest.raises(bvc._lib.BvcError, match="overwritten"):
        first.loss.backward()
    # an oversize batch is refused before anything is allocated, naming the limit (VideoMAE-base: 445 clips below 4 GiB)
    big = bvc.VideoMAEForVideoClassification(bvc.videomae_config("base", num_labels=NL))
    big._ensure_flat(dev)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(bvc._lib.BvcError, match="at most 445 clips"):
        big._get_train_ctx(446)
    assert big._train.h is None
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)
