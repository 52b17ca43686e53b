"""First mode of the first decoder layer (bvc_set_option("dec_first")): same-process A (0: off) / B (1: on) / A' / B' of the
VideoMAE-base forward + backward, the headline's step without optimiser and loaders (they do not change with the mode).  One JSON line
per batch: the four times, the gain of the mean of B, B' over the mean of A, A', the spread max(|A - A'|, |B - B'|), and the two losses.

    python tools/bvc_tools.py ab dec_first [--steps 20] [--warmup 5] [--clips 16,64,256]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--clips", default="256")
args = ap.parse_args()
ge.build()
bvc = ge.load_package()
from oracle import videomae_oracle as vo   # noqa: E402

dev = torch.device("cuda:0")
cfg = vo.BASE
kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}


def timed(step, first):
    old = bvc._lib.set_option("dec_first", first)
    try:
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.steps):
            loss = step()
        t1.record()
        torch.cuda.synchronize()
    finally:
        bvc._lib.set_option("dec_first", old)
    return t0.elapsed_time(t1) / args.steps, float(loss)


for clips in [int(c) for c in args.clips.split(",") if c]:
    model = bvc.VideoMAEForPreTraining(bvc.VideoMAEConfig(**kw)).to(dev).train()
    pixels, mask = vo.synthetic_batch(cfg, clips, seed=5, mask_ratio=0.9)
    px, mk = pixels.to(dev), mask.to(dev)

    def step():
        for p in model.parameters():
            p.grad = None
        loss = model(px, bool_masked_pos=mk).loss
        loss.backward()
        return loss.detach()

    (a, la), (b, lb), (a2, _), (b2, _) = timed(step, 0), timed(step, 1), timed(step, 0), timed(step, 1)
    gain = 0.5 * (a + a2) - 0.5 * (b + b2)
    spread = max(abs(a - a2), abs(b - b2))      # the larger of the two repeats' differences: one coincidence cannot empty the bar
    print(json.dumps({"clips": clips, "off_ms": round(a, 4), "on_ms": round(b, 4), "off2_ms": round(a2, 4), "on2_ms": round(b2, 4),
                      "gain_ms": round(gain, 4), "spread_ms": round(spread, 4), "gain_over_spread": round(gain / spread, 2) if spread > 0 else None,
                      "loss_off": la, "loss_on": lb}), flush=True)
    del model, px, mk
    torch.cuda.empty_cache()
