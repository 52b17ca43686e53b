"""The two other BASELINE configurations as functions, for bench.py's `extra` block (one GPU, after the headline loop) and for
tools/bench_jepa.py / bench_simclr.py:
  jepa_leg   - config 4: I-JEPA training step (target encoder on all 392 tokens, context encoder, predictor, smooth-L1, backward,
               fused SGD-Nesterov, EMA; pretraining/predictive/pretrain_jepa.py:383-433), synthetic 2-frame 224^2 inputs;
  simclr_leg - config 5 on one GPU: ViT-B trunk + token mean + projection head + InfoNCE over the local rows (N > 1 gathers them
               first; pretraining/contrastive/pretrain_simclr.py:320-329), backward, fused SGD-Nesterov.
Each returns a dict with throughput, ms per step and TFLOP/s against the algorithmic FLOPs of SURVEY.md section 8d."""
import copy
import time

import numpy as np
import torch

JEPA_GFLOP = {"vit_base": 160.6, "vit_large": 473.2}     # per sample at N_ctx = 100, N_pred = 25
JEPA_GFLOP.update({"vit_tiny": 43.3, "vit_huge": 939.0, "vit_giant": 1476.8})   # jepa_gflop() of the three other factories
SIMCLR_GFLOP = 104.8                                      # per image, ViT-B/16 at 224^2


def jepa_gflop(embed_dim, depth, mlp_hidden, nctx=100, npred=25, nsets=4, tokens=392, patch_dim=768, pred_dim=384, pred_depth=6):
    """Algorithmic GFLOP of one JEPA training sample, SURVEY.md section 8d's counting: 2 FLOP per MAC, a transformer layer of N
    tokens is 8 N D^2 (qkv, proj) + 4 N D I (MLP) + 4 N^2 D (scores, context); train = target fwd + 3 x (context fwd + predictor fwd),
    with the patch embedding over all `tokens` in both encoder calls and the predictor's embed / proj over all `nsets` mask sets."""
    def layers(n, d, i, count):
        return count * (8 * n * d * d + 4 * n * d * i + 4 * n * n * d)
    embed = 2 * tokens * patch_dim * embed_dim
    target = embed + layers(tokens, embed_dim, mlp_hidden, depth)
    context = embed + layers(nctx, embed_dim, mlp_hidden, depth)
    predictor = nsets * (layers(nctx + npred, pred_dim, 4 * pred_dim, pred_depth) + 2 * nctx * embed_dim * pred_dim
                         + 2 * npred * pred_dim * embed_dim)
    return (target + 3 * (context + predictor)) / 1e9


def videomae_gflop(config, mask_ratio=0.9, decode_ratio=None):
    """Algorithmic GFLOP of one VideoMAE pre-training clip, BASELINE.md section 3's counting (202.295 for base): tube masking hides
    int(mask_ratio x patches per frame) patches of every frame; the patch embedding runs on the visible tokens and needs no input
    gradient (2x), everything else - encoder, encoder-to-decoder, decoder on all tokens, head on the masked ones - counts 3x.
    decode_ratio: the decoder reconstructs int(decode_ratio x masked per frame) masked patches of every frame (DecoderSubsetGenerator):
    it then runs on the visible and those tokens only, the head on those."""
    c = config
    g = c.image_size // c.patch_size
    per, T = g * g, c.num_frames // c.tubelet_size
    L = T * per
    nmask = T * int(mask_ratio * per)
    nvis = L - nmask
    ndec = nmask if decode_ratio is None else T * int(decode_ratio * int(mask_ratio * per))
    P = c.num_channels * c.tubelet_size * c.patch_size * c.patch_size

    def layers(n, d, i, count):
        return count * (8 * n * d * d + 4 * n * d * i + 4 * n * n * d)
    D, Dd = c.hidden_size, c.decoder_hidden_size
    patch = 2 * nvis * P * D
    rest = (layers(nvis, D, c.intermediate_size, c.num_hidden_layers) + 2 * nvis * D * Dd
            + layers(nvis + ndec, Dd, c.decoder_intermediate_size, c.decoder_num_hidden_layers) + 2 * ndec * Dd * P)
    return (2 * patch + 3 * rest) / 1e9


def _timed(step, warmup, steps):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, float(loss.detach())


def jepa_leg(bvc, dev, model="vit_large", batch=16, nctx=100, npred=25, warmup=6, steps=10, overlap_target=True):
    torch.manual_seed(0)
    enc, pred = bvc.jepa.get_model(dev, patch_size=16, tubelet_size=1, num_frames=2, model_name=model, image_size=224)
    tgt = copy.deepcopy(enc).to(dev)
    for p in tgt.parameters():
        p.requires_grad = False
    for m in (enc, pred, tgt):
        m._ensure_flat(dev)
    # the reference's optimiser (pretraining/predictive/helper.py:108-165 via pretrain_jepa.py:274): four groups, weight decay 1e-6 on the
    # weights only, SGD-Nesterov, GradScaler
    opt, scaler, _sched, _wd_sched = bvc.jepa.init_opt(enc, pred, iterations_per_epoch=1000, start_lr=0.1, ref_lr=0.1, momentum=0.9, warmup=0,
                                                       num_epochs=1, wd=1e-6, use_bfloat16=True)
    B = batch
    g = torch.Generator().manual_seed(1)
    imgs = ((torch.randint(0, 256, (B, 2, 3, 224, 224), generator=g, dtype=torch.uint8).float() / 255 - 0.5) / 0.25).to(dev)
    me = [torch.stack([torch.sort(torch.randperm(196, generator=g)[:nctx]).values for _ in range(B)]).to(dev)]
    mp = [(torch.stack([torch.sort(torch.randperm(196, generator=g)[:npred]).values for _ in range(B)]) + 196).to(dev) for _ in range(4)]

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if not overlap_target:
                with torch.no_grad():
                    h = bvc.jepa.select_targets(tgt(imgs), mp)
                z = pred(enc(imgs, me), me, mp)
            else:
                # the target encoder's forward has no consumer before the loss: on a second stream it runs beside the context encoder
                # and the predictor (bvc.jepa.forward_target_async: same kernels, same arithmetic)
                join = bvc.jepa.forward_target_async(tgt, imgs, mp)
                z = pred(enc(imgs, me), me, mp)
                h = join()
            loss = bvc.AllReduce.apply(bvc.jepa.smooth_l1_loss(z, h))
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        opt.zero_grad()
        bvc.jepa.ema_update(enc, tgt, 0.996)
        return loss

    dt, loss = _timed(step, warmup, steps)
    gf = JEPA_GFLOP.get(model, 0.0)
    return {"workload": f"I-JEPA {model}/16, 2x224^2 inputs, {B} samples/GPU, N_ctx {nctx}, N_pred {npred} x 4, full step (target + context "
                        "encoders, predictor, smooth-L1, bwd, SGD-Nesterov, EMA)" + ("; target forward on a second stream" if overlap_target else ""),
            "value": round(B / dt, 1), "unit": "samples/s", "ms_per_step": round(1e3 * dt, 3), "steps": steps,
            "tflops": round(gf * B / dt / 1e3, 1), "frac_of_mfma_peak": round(gf * B / dt / 1e3 / 2500.0, 4), "final_loss": round(loss, 5)}


def videomae_leg(bvc, dev, arch="base", batch=16, warmup=5, steps=10, mask_ratio=0.9, decode_ratio=None, clip_grad=None, clip_grad_torch=False):
    """VideoMAE pre-training step of one VIDEOMAE_ARCHS size: synthetic 16 x 224^2 clips, tube masking at mask_ratio, bf16 autocast,
    backward, fused SGD-Nesterov with GradScaler - the headline's step at another model size.  decode_ratio: the decoder reconstructs
    that share of every frame's masked patches (bool_decode_pos from DecoderSubsetGenerator); None = all of them, no decode mask.
    clip_grad: clip the gradients by their global norm - inside the fused step (max_grad_norm=), or, with clip_grad_torch, the route
    without it: scaler.unscale_ + torch.nn.utils.clip_grad_norm_ before the step."""
    torch.manual_seed(0)
    cfg = bvc.videomae_config(arch)
    model = bvc.VideoMAEForPreTraining(cfg).to(dev).train()
    model._ensure_flat(dev)
    # bench.py's optimiser and scaler: the fused SGD-Nesterov over the flat parameters, bvc.amp.GradScaler
    opt = bvc.optim.SGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True, weight_decay=0.0,
                        max_grad_norm=None if clip_grad_torch else clip_grad)
    torch_clip = clip_grad is not None and clip_grad_torch
    scaler = bvc.amp.GradScaler("cuda")
    B, T, g = batch, cfg.num_frames // cfg.tubelet_size, cfg.image_size // cfg.patch_size
    gen = torch.Generator().manual_seed(1234)
    clips = torch.randn(B, cfg.num_frames, 3, cfg.image_size, cfg.image_size, generator=gen).to(dev)
    mgen = bvc.TubeMaskingGenerator((T, g, g), mask_ratio, rng=np.random.RandomState(1234))
    masks = [mgen() for _ in range(B)]
    mask = torch.from_numpy(np.stack(masks)).bool().to(dev)
    kw = {}
    if decode_ratio is not None:
        dgen = bvc.DecoderSubsetGenerator((T, g, g), decode_ratio, rng=np.random.RandomState(4321))
        kw["bool_decode_pos"] = torch.from_numpy(np.stack([dgen(m) for m in masks])).bool().to(dev)

    def step():
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model(clips, bool_masked_pos=mask, **kw).loss
        scaler.scale(loss).backward()
        if torch_clip:
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip_grad)
        scaler.step(opt)
        scaler.update()
        return loss

    dt, loss = _timed(step, warmup, steps)
    gf = videomae_gflop(cfg, mask_ratio, decode_ratio)
    dual = "" if decode_ratio is None else f", decoder on {decode_ratio} of the masked patches ({int(kw['bool_decode_pos'][0].sum())} per clip)"
    return {"workload": f"VideoMAE-{arch} pre-training, 16x224^2 clips, mask {mask_ratio}{dual}, {B} clips/GPU, full step (fwd, bwd, SGD-Nesterov, "
                        "GradScaler)", "value": round(B / dt, 2), "unit": "clips/s", "ms_per_step": round(1e3 * dt, 3), "steps": steps,
            "gflop_per_clip": round(gf, 3), "tflops": round(gf * B / dt / 1e3, 1), "frac_of_mfma_peak": round(gf * B / dt / 1e3 / 2500.0, 4),
            "final_loss": round(loss, 5)}


def simclr_leg(bvc, dev, images=512, warmup=3, steps=10):
    torch.manual_seed(0)
    model = bvc.simclr.SimCLRViT("vit_base", image_size=224).to(dev).train()
    model.trunk._ensure_flat(dev)
    opt = bvc.optim.SGD([{"params": [p for p in model.trunk.parameters() if p.requires_grad]},
                         {"params": list(model.fc.parameters())}], lr=0.1, momentum=0.9, nesterov=True)
    scaler = torch.amp.GradScaler("cuda")
    n = images
    masks = bvc.simclr.make_masks(n // 2, dev)
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 256, (n, 3, 224, 224), generator=g, dtype=torch.uint8).to(dev)     # uint8 frames, normalised on the GPU

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = bvc.AllReduce.apply(bvc.simclr.global_info_nce_loss(0.1, masks, model(x)))
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        opt.zero_grad()
        return loss

    dt, loss = _timed(step, warmup, steps)
    return {"workload": f"SimCLR ViT-B/16 224^2, {n} images/GPU (global batch 4096 on 8 GPUs), full step (trunk, token mean, head, InfoNCE, "
                        "bwd, SGD-Nesterov)",
            "value": round(n / dt, 1), "unit": "images/s", "ms_per_step": round(1e3 * dt, 3), "steps": steps,
            "tflops": round(SIMCLR_GFLOP * n / dt / 1e3, 1), "frac_of_mfma_peak": round(SIMCLR_GFLOP * n / dt / 1e3 / 2500.0, 4),
            "final_loss": round(loss, 4)}
