"""VideoMAE pre-training throughput of the VIDEOMAE_ARCHS sizes on one MI355X (tools/bench_legs.videomae_leg: synthetic 16 x 224^2
clips, tube mask 0.9, bf16 autocast, backward, fused SGD-Nesterov, GradScaler).  One JSON line per (arch, batch) on stdout.

    python tools/bench_videomae.py --arch small,base,large,huge --batch 16,64 [--steps 10] [--warmup 5] [--decode-ratio 0.5]
                                   [--clip-grad C [--clip-grad-torch]]

--decode-ratio R: the decoder reconstructs int(R x masked patches per frame) of every frame's masked patches (bool_decode_pos from
DecoderSubsetGenerator, VideoMAE V2's decoder masking); off by default, and then no decode mask is passed.
--clip-grad C: clip the gradients by their global norm inside the fused step (bvc.optim.SGD(max_grad_norm=C): the norm comes out of
the scaler's inf-check read); with --clip-grad-torch the route without it (scaler.unscale_ + torch.nn.utils.clip_grad_norm_), for the A/B."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402
from tools.bench_legs import videomae_leg   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--arch", default="base", help="comma-separated VIDEOMAE_ARCHS keys")
ap.add_argument("--batch", default="16", help="comma-separated clips per step")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--decode-ratio", type=float, default=None, help="share of the masked patches the decoder reconstructs (default: all, no decode mask)")
ap.add_argument("--clip-grad", type=float, default=None, help="clip the gradients by their global norm at this value")
ap.add_argument("--clip-grad-torch", action="store_true", help="with --clip-grad: scaler.unscale_ + torch.nn.utils.clip_grad_norm_ instead of max_grad_norm=")
args = ap.parse_args()
ge.build()
bvc = ge.load_package()
dev = torch.device("cuda:0")
for arch in args.arch.split(","):
    for b in (int(x) for x in args.batch.split(",")):
        r = videomae_leg(bvc, dev, arch=arch, batch=b, warmup=args.warmup, steps=args.steps, decode_ratio=args.decode_ratio,
                         clip_grad=args.clip_grad, clip_grad_torch=args.clip_grad_torch)
        extra = {} if args.decode_ratio is None else {"decode_ratio": args.decode_ratio}
        if args.clip_grad is not None:
            extra.update({"clip_grad": args.clip_grad, "clip_route": "torch" if args.clip_grad_torch else "fused"})
        print(json.dumps({"arch": arch, "batch": b, **extra, **r}), flush=True)
        torch.cuda.empty_cache()
