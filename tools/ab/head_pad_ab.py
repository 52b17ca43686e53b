"""Cost of zero-padding 80 / 88-wide heads to 96 in HBM (bvc_set_option("head_pad", 1), the layout of earlier builds) against the
in-place attention (head_pad 0, the default): same-process A / B / A' / B' of the JEPA step (tools/bench_legs.jepa_leg) for ViT-H and
ViT-g.  head_pad is read when a model's stacks are allocated, so every leg builds its models afresh under its own setting.  One JSON
line per leg on stdout, then one summary line per model (B / A and A' / A).

    python tools/ab/head_pad_ab.py [--models vit_huge,vit_giant] [--batch 16] [--steps 10]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402
from tools.bench_legs import jepa_leg   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="vit_huge,vit_giant")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=4)
args = ap.parse_args()
ge.build()
bvc = ge.load_package()
dev = torch.device("cuda:0")
for model in args.models.split(","):
    ms = {}
    for leg, pad in (("A", 0), ("B", 1), ("A'", 0), ("B'", 1)):
        bvc._lib.set_option("head_pad", pad)
        r = jepa_leg(bvc, dev, model=model, batch=args.batch, warmup=args.warmup, steps=args.steps)
        ms[leg] = r["ms_per_step"]
        print(json.dumps({"model": model, "leg": leg, "head_pad": pad, **r}), flush=True)
        torch.cuda.empty_cache()
    bvc._lib.set_option("head_pad", 0)
    a = (ms["A"] + ms["A'"]) / 2
    print(json.dumps({"model": model, "batch": args.batch, "ms_in_place": a, "ms_padded": (ms["B"] + ms["B'"]) / 2,
                      "padded_over_in_place": round((ms["B"] + ms["B'"]) / 2 / a, 4),
                      "A_prime_over_A": round(ms["A'"] / ms["A"], 4), "B_prime_over_B": round(ms["B'"] / ms["B"], 4)}), flush=True)
