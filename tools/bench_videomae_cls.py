"""Fine-tuning step time on one MI355X: VideoMAEForVideoClassification (train mode, labels) forward + backward + bvc.optim.AdamW step
on synthetic 16 x 224^2 clips, every one of the 1568 tokens through the encoder.  One JSON line:

    python tools/bench_videomae_cls.py --arch {small,base,large,huge} --batch B[,B2,...] [--steps K --warmup W]
                                       [--hidden-dropout P] [--drop-path R] [--layer-decay D]
                                       [--grad-scaler] [--clip-grad C [--clip-grad-torch]]

--hidden-dropout / --drop-path switch the gate on the residual branches on (config.hidden_dropout_prob / config.drop_path_rate);
left at 0 the step is the ungated one, kernel for kernel.  --layer-decay D builds the optimiser from
bvc.optim.layer_decay_param_groups (2 (layers + 2) parameter groups, layer-wise learning-rate decay D); without it the optimiser
has one group.  --clip-grad C clips the gradients by their global norm inside the fused step (bvc.optim.AdamW(max_grad_norm=C)); with
--clip-grad-torch it runs the route without it for the A/B: torch.nn.utils.clip_grad_norm_ before the step, after scaler.unscale_
where --grad-scaler puts the step under bvc.amp.GradScaler (scaled loss, inf check, scaler.step / update).  Several batch sizes give one line each.  `optimizer_launches_per_step` counts the kernels of one optimiser step
from the library calls it makes (a per-run Adam update is two: prepare + step; a by-value segment call two; a table call one plus
one writer per 64 groups).

Algorithmic cost per clip: forward = patch embedding 2 N D P (P = 1536 pixels per tube) + layers x (24 N D^2 + 4 N^2 D); a step
counts the encoder 3x (forward, dX, dW) and the patch embedding 2x (forward, dW; pixels need no gradient).  VideoMAE-base:
3.699 + 12 x 29.749 GFLOP forward, 1078.37 GFLOP per step.  `frac_peak` is against 2.5 PFLOP/s (dense bf16)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402

PEAK_TFLOPS = 2500.0


def gflop_per_clip(cfg):
    g = cfg.image_size // cfg.patch_size
    N = (cfg.num_frames // cfg.tubelet_size) * g * g
    D, P = cfg.hidden_size, cfg.num_channels * cfg.tubelet_size * cfg.patch_size ** 2
    pe = 2.0 * N * D * P
    layer = 24.0 * N * D * D + 4.0 * N * N * D
    return (3 * cfg.num_hidden_layers * layer + 2 * pe) / 1e9, pe / 1e9, layer / 1e9


OPT_ENTRY_POINTS = ("bvc_op_adam_prepare", "bvc_op_adam_step", "bvc_op_adam_step_segments", "bvc_op_adam_step_table",
                    "bvc_op_grad_sqnorm_items", "bvc_op_clip_finalize")


def optimizer_launches(bvc, opt):
    """Kernel launches of one opt.step(), from the library entry points it calls (gradients of the last backward are still there)."""
    lib = bvc._lib.lib()
    calls = {k: 0 for k in OPT_ENTRY_POINTS if hasattr(lib, k)}
    saved = {k: getattr(lib, k) for k in calls}
    for k, fn in saved.items():
        def counted(*a, _k=k, _fn=fn):
            calls[_k] += 1
            return _fn(*a)
        setattr(lib, k, counted)
    try:
        opt.step()
    finally:
        for k, fn in saved.items():
            setattr(lib, k, fn)
    writers = (len(opt.param_groups) + 63) // 64
    per_call = {"bvc_op_adam_prepare": 1, "bvc_op_adam_step": 1, "bvc_op_adam_step_segments": 2, "bvc_op_adam_step_table": 1 + writers,
                "bvc_op_grad_sqnorm_items": 2, "bvc_op_clip_finalize": 1}
    return sum(n * per_call[k] for k, n in calls.items()), calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="base", choices=["small", "base", "large", "huge"])
    ap.add_argument("--batch", default="16", help="batch size, or several separated by commas (one result line each)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--num-labels", type=int, default=400)
    ap.add_argument("--hidden-dropout", type=float, default=0.0)
    ap.add_argument("--drop-path", type=float, default=0.0)
    ap.add_argument("--layer-decay", type=float, default=None, help="layer-wise learning-rate decay: the optimiser gets 2 (layers + 2) groups")
    ap.add_argument("--grad-scaler", action="store_true", help="run the step under bvc.amp.GradScaler")
    ap.add_argument("--clip-grad", type=float, default=None, help="clip the gradients by their global norm at this value")
    ap.add_argument("--clip-grad-torch", action="store_true", help="with --clip-grad: torch.nn.utils.clip_grad_norm_ (after scaler.unscale_) instead of max_grad_norm=")
    args = ap.parse_args()
    ge.build()
    bvc = ge.load_package()
    for batch in (int(b) for b in str(args.batch).split(",")):
        run(bvc, args, batch)


def run(bvc, args, B):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    drop = {}
    if args.hidden_dropout:
        drop["hidden_dropout_prob"] = args.hidden_dropout
    if args.drop_path:
        drop["drop_path_rate"] = args.drop_path
    cfg = bvc.videomae_config(args.arch, num_labels=args.num_labels, **drop)
    free0 = torch.cuda.mem_get_info(dev)[0]
    m = bvc.VideoMAEForVideoClassification(cfg).to(dev).train()
    torch_clip = args.clip_grad is not None and args.clip_grad_torch
    clip = {} if args.clip_grad is None or torch_clip else {"max_grad_norm": args.clip_grad}
    if args.layer_decay is None:
        opt = bvc.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.05, **clip)
    else:
        opt = bvc.optim.AdamW(bvc.optim.layer_decay_param_groups(m, 1e-4, 0.05, args.layer_decay), lr=1e-4, **clip)
    scaler = bvc.amp.GradScaler("cuda") if args.grad_scaler else None
    g = torch.Generator().manual_seed(1)
    clips = torch.randint(0, 256, (B, cfg.num_frames, 3, cfg.image_size, cfg.image_size), generator=g, dtype=torch.uint8).to(dev)
    labels = torch.randint(0, args.num_labels, (B,), generator=g).to(dev)

    def step():
        opt.zero_grad()
        out = m(pixel_values=clips, labels=labels)
        if scaler is None:
            out.loss.backward()
            if torch_clip:
                torch.nn.utils.clip_grad_norm_(m.parameters(), args.clip_grad)
            opt.step()
            return out.loss
        scaler.scale(out.loss).backward()
        if torch_clip:
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(m.parameters(), args.clip_grad)
        scaler.step(opt)
        scaler.update()
        return out.loss

    for _ in range(args.warmup):
        loss = step()
    torch.cuda.synchronize()
    used = free0 - torch.cuda.mem_get_info(dev)[0]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    gf, pe, layer = gflop_per_clip(cfg)
    tflops = gf * B / dt / 1e3
    launches, calls = optimizer_launches(bvc, opt)
    torch.cuda.synchronize()
    print(json.dumps({"metric": f"VideoMAE-{args.arch} fine-tuning step (forward + backward + AdamW), all tokens, bf16 operands",
                      "arch": args.arch, "batch": B, "hidden_dropout": args.hidden_dropout, "drop_path": args.drop_path, "layer_decay": args.layer_decay,
                      "grad_scaler": bool(args.grad_scaler), "clip_grad": args.clip_grad, "clip_route": None if args.clip_grad is None else "torch" if torch_clip else "fused",
                      "optimizer_groups": len(opt.param_groups), "optimizer_launches_per_step": launches, "optimizer_calls": calls, "ms_per_step": round(1e3 * dt, 3), "clips_per_s": round(B / dt, 1),
                      "gflop_per_clip": round(gf, 2), "gflop_patch_embed_fwd": round(pe, 3), "gflop_layer_fwd": round(layer, 3),
                      "tflops": round(tflops, 1), "frac_peak": round(tflops / PEAK_TFLOPS, 4), "device_mem_gb": round(used / 1e9, 2),
                      "loss": round(float(loss), 4), "finite": bool(torch.isfinite(loss).all())}), flush=True)


if __name__ == "__main__":
    main()
