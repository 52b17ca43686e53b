"""Bits of every model context, for comparing two builds of the library: each case runs in deterministic mode and prints one line
`<case> <tensor> <sha256>` per output, gradient buffer and final parameter set.  Run it once per build and diff the two outputs:

    python tools/ab/host_contexts_bits.py > this.txt
    BVC_LIB_PATH=/path/to/other/libbvc_hip.so python tools/ab/host_contexts_bits.py > other.txt

Cases: VideoMAE pre-training (TINY and base, 2 clips, 3 fused-SGD steps, with / without a decode mask, tail mode on / off, the
"dec<last>" tap), fine-tuning (drop gate, CutMix table, hidden states + attentions), the inference encode (with / without fc_norm,
fc_norm's backward), a JEPA step (ViT + predictor + target + EMA) and the SimCLR ViT composition."""
import copy
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402

bvc = ge.load_package()
from oracle import jepa_oracle as jo   # noqa: E402
from oracle import simclr_oracle as so   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402
from tools.make_videomae_cls_golden import head_params   # noqa: E402

dev = torch.device("cuda:0")
L = bvc._lib
NL = 10


def emit(case, name, t):
    torch.cuda.synchronize()
    a = t.detach().contiguous().cpu().reshape(-1)
    a = a.view(torch.uint8) if a.dtype != torch.uint8 else a
    print(case, name, hashlib.sha256(a.numpy().tobytes()).hexdigest(), flush=True)


def emit_state(case, name, module):
    for k, v in module.state_dict().items():
        emit(case, f"{name}.{k}", v)


def kwargs(cfg):
    return {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}


def pretrain(tag, cfg, params, ratio):
    batches = [vo.synthetic_batch(cfg, 2, seed=200 + it, mask_ratio=ratio) for it in range(3)]
    gen = bvc.DecoderSubsetGenerator(cfg.grid, 0.5, rng=np.random.RandomState(21))
    for dual in (0, 1):
        for tail in (0, 1):
            case = f"pretrain_{tag}_dual{dual}_tail{tail}"
            old = L.set_option("dec_tail", tail)
            model = bvc.VideoMAEForPreTraining(bvc.VideoMAEConfig(**kwargs(cfg)))
            model.load_state_dict(params)
            model.to(dev).train()
            model._ensure_flat(dev)
            opt = bvc.optim.SGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4)
            for it, (pixels, mask) in enumerate(batches):
                dec = torch.from_numpy(np.stack([gen(m) for m in mask.numpy()])).bool().to(dev) if dual else None
                opt.zero_grad()
                out = model(pixels.to(dev), bool_masked_pos=mask.to(dev), bool_decode_pos=dec, output_logits=True)
                emit(case, f"step{it}.loss", out.loss)
                emit(case, f"step{it}.logits", out.logits)
                emit(case, f"step{it}.tap_dec_last", model.tap(f"dec{cfg.decoder_num_hidden_layers - 1}"))
                out.loss.backward()
                emit(case, f"step{it}.grads", model.flat_grads())
                opt.step()
            emit_state(case, "params", model)
            L.set_option("dec_tail", old)
            del model, opt
            torch.cuda.empty_cache()


def classifier(cfg, params, heads, **extra):
    m = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(num_labels=NL, **kwargs(cfg), **extra))
    sd = {k: v for k, v in params.items() if k.startswith("videomae.")}
    sd.update(heads)
    m.load_state_dict(sd)
    return m.to(dev).train()


def emit_cls_step(case, m, out):
    emit(case, "loss", out.loss)
    emit(case, "logits", out.logits)
    out.loss.backward()
    emit(case, "grads", m.flat_grads())
    for k in ("fc_norm.weight", "fc_norm.bias", "classifier.weight", "classifier.bias"):
        emit(case, f"grad.{k}", dict(m.named_parameters())[k].grad)


def finetune(tag, cfg, params):
    heads = dict(zip(("fc_norm.weight", "fc_norm.bias", "classifier.weight", "classifier.bias"), head_params(cfg.hidden_size, NL, 5)))
    pixels, _ = vo.synthetic_batch(cfg, 2, seed=7, mask_ratio=0.9)
    px = pixels.to(dev)
    labels = torch.tensor([1, 4], device=dev)
    S = cfg.image_size

    m = classifier(cfg, params, heads, hidden_dropout_prob=0.1, drop_path_rate=0.5)
    torch.manual_seed(3)
    emit_cls_step(f"finetune_{tag}_drop", m, m(pixel_values=px, labels=labels))
    emit(f"finetune_{tag}_drop", "drop_path_scale", m.drop_path_scale)

    m = classifier(cfg, params, heads)
    m.config.problem_type = "soft_label_classification"
    box = (5, S - 21, 10, S - 27)
    mix = bvc.ClipMix([1, 0], [1.0, 1.0], [box, box], image_size=(S, S), device=dev)
    soft = torch.softmax(torch.randn(2, NL, generator=torch.Generator().manual_seed(8)), -1).to(dev)
    emit_cls_step(f"finetune_{tag}_cutmix", m, m(pixel_values=px, labels=soft, mix=mix))

    m = classifier(cfg, params, heads)
    out = m(pixel_values=px, labels=labels, output_hidden_states=True, output_attentions=True, output_last_hidden_state=True)
    case = f"finetune_{tag}_introspect"
    emit(case, "last_hidden_state", out.last_hidden_state)
    emit(case, "hidden_states", torch.stack(out.hidden_states))
    emit(case, "attentions", torch.stack(out.attentions))
    emit_cls_step(case, m, out)

    # the inference context: a frozen encoder under fc_norm's autograd (encode with fc_norm, then its backward), with everything
    # the encode can deliver; then the raw encode without fc_norm through the C ABI
    m = classifier(cfg, params, heads)
    for p in m.videomae.parameters():
        p.requires_grad = False
    out = m(pixel_values=px, labels=labels, output_hidden_states=True, output_attentions=True, output_last_hidden_state=True)
    case = f"encode_{tag}_fc_norm"
    emit(case, "logits", out.logits)
    emit(case, "last_hidden_state", out.last_hidden_state)
    emit(case, "hidden_states", torch.stack(out.hidden_states))
    emit(case, "attentions", torch.stack(out.attentions))
    out.loss.backward()
    for k in ("fc_norm.weight", "fc_norm.bias", "classifier.weight"):
        emit(case, f"grad.{k}", dict(m.named_parameters())[k].grad)
    h = m._get_ctx(2)
    pooled = torch.empty(2, cfg.hidden_size, device=dev)
    tokens = torch.empty(2, m.config.seq_length, cfg.hidden_size, device=dev)
    L.check(L.lib().bvc_videomae_encode(h, px.data_ptr(), 2, m._flat.data_ptr(), None, None, 0.0, tokens.data_ptr(), pooled.data_ptr(),
                                        L.current_stream_ptr()), "bvc_videomae_encode")
    emit(f"encode_{tag}_plain", "pooled", pooled)
    emit(f"encode_{tag}_plain", "tokens", tokens)
    del m
    torch.cuda.empty_cache()


def jepa_step():
    cfg = jo.TINY
    enc_p = jo.make_params(jo.encoder_shapes(cfg), cfg, 26)
    pred_p = jo.make_params(jo.predictor_shapes(cfg), cfg, 27)
    imgs, m_enc, m_pred = jo.synthetic_inputs(cfg, 4, 6, 8, 4)
    x, me, mp = imgs.to(dev), [m.to(dev) for m in m_enc], [m.to(dev) for m in m_pred]
    enc = bvc.jepa.VisionTransformer(img_size=[cfg.image_size], patch_size=cfg.patch_size, num_frames=cfg.num_frames, tubelet_size=cfg.tubelet_size,
                                     embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio)
    enc.load_state_dict(enc_p)
    tgt = copy.deepcopy(enc)
    pred = bvc.jepa.vit_predictor(sequence_shape=enc.sequence_shape, embed_dim=cfg.embed_dim, predictor_embed_dim=cfg.pred_dim,
                                  depth=cfg.pred_depth, num_heads=enc.num_heads)
    pred.load_state_dict(pred_p)
    for p in tgt.parameters():
        p.requires_grad = False
    enc, pred, tgt = enc.to(dev), pred.to(dev), tgt.to(dev)
    opt = bvc.optim.SGD([{"params": [p for p in enc.parameters() if p.requires_grad]},
                         {"params": [p for p in pred.parameters() if p.requires_grad]}], lr=0.05, momentum=0.9, nesterov=True)
    for it in range(3):
        with torch.no_grad():
            h = bvc.jepa.select_targets(tgt(x), mp)
        z = pred(enc(x, me), me, mp)
        loss = bvc.jepa.smooth_l1_loss(z, h)
        loss.backward()
        emit("jepa", f"step{it}.loss", loss)
        emit("jepa", f"step{it}.z", z)
        emit("jepa", f"step{it}.enc_grads", enc.flat_grads())
        emit("jepa", f"step{it}.pred_grads", pred.flat_grads())
        opt.step()
        opt.zero_grad()
        bvc.jepa.ema_update(enc, tgt, 0.9)
    for name, m in (("enc", enc), ("pred", pred), ("tgt", tgt)):
        emit_state("jepa", name, m)


def simclr_vit():
    cfg = jo.JepaConfig(image_size=64, patch_size=16, num_frames=1, embed_dim=128, depth=2, num_heads=2, pred_dim=64, pred_depth=1)
    B, D = 8, cfg.embed_dim
    imgs = torch.randn(2 * B, cfg.in_chans, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(21))
    model = bvc.simclr.SimCLRViT.__new__(bvc.simclr.SimCLRViT)
    torch.nn.Module.__init__(model)
    model.trunk = bvc.jepa.VisionTransformer(img_size=[cfg.image_size], patch_size=cfg.patch_size, num_frames=1, tubelet_size=1,
                                             embed_dim=D, depth=cfg.depth, num_heads=cfg.num_heads)
    model.fc = bvc.simclr.ProjectionHead(D, D)
    model.trunk.load_state_dict(jo.make_params(jo.encoder_shapes(cfg), cfg, seed=4))
    model.fc.load_state_dict(so.head_params(D, D, seed=9))
    model.to(dev).train()
    out = model(imgs.to(dev))
    loss = bvc.simclr.global_info_nce_loss(0.1, bvc.simclr.make_masks(B, dev), out)
    loss.backward()
    emit("simclr_vit", "features", out)
    emit("simclr_vit", "loss", loss)
    emit("simclr_vit", "trunk_grads", model.trunk.flat_grads())
    for k, p in model.fc.named_parameters():
        emit("simclr_vit", f"grad.fc.{k}", p.grad)


bvc.use_deterministic_algorithms(True)
print("# library", L.LIB_PATH, flush=True)
for tag, cfg, ratio in (("tiny", vo.TINY, 0.75), ("base", vo.BASE, 0.9)):
    params = vo.make_params(cfg, seed=0)
    pretrain(tag, cfg, params, ratio)
    finetune(tag, cfg, params)
jepa_step()
simclr_vit()
