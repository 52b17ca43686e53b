"""Clip transforms (bvc.augment, csrc/augment.hip) at the benchmark's input size: 256 clips x 16 frames, 256 x 256 -> 224 x 224.

    python tools/bench_augment.py [--clips 256] [--frames 16] [--src 256] [--size 224] [--iters 10] [--rounds 5]

Configurations (tables drawn once, outside the timed window; every call uploads its table and launches the kernels):
  center_crop   Resize(224) + CenterCrop(224) of the whole frame, no colour (the VideoMAE loader)
  geometry      RandomResizedCrop(224, scale=(0.08, 1)) per clip + flip, no colour
  jitter        the same + all four ColorJitter stages on EVERY clip (jitter_p = 1, the worst case: three launches) + grayscale draws
  two_views     jitter, two views from the one source batch (twice the output)
  post_blur     the post stage (bvc_op_clip_post) alone on the 224 x 224 frames: Gaussian blur on EVERY frame, radius uniform in
                (0.1, 2.0) per clip
  post_rotate   the post stage alone: rotation on every frame, angle uniform in (-90, 90) per clip
  post_both     the post stage alone: both on every frame (two launches, the frames pass through the workspace)
  augment_cjbo  ClipAugment("cjbo") end to end: the `jitter` stage one without the extra gray, then the post stage with blur on half of
                the clips (blur_p = 0.5) and rotation on all
  d2d_copy      the yardstick: a device-to-device copy of the same input bytes plus a copy of the same output bytes (torch copy_),
                timed for the one-view and the two-view byte counts; d2d_copy_post is the post stage's: one copy of its 224 x 224 frames
One JSON line per configuration: milliseconds (median, min, max over rounds; HIP events around `iters` calls, after a warm-up of every
configuration; rounds alternate the configurations), the bytes the algorithm has to move (source region read once + output written
once; for `jitter` the second pass reads and writes the output again; every launch of the post stage reads and writes the frames
once) and that over the time.  `host_sample_ms` is the time
sample_params takes on the host for that table (one draw per clip).  Results: DESIGN.md, "Clip transforms".
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--src", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: no GPU (a timing taken elsewhere says nothing)")
    ge.build()
    bvc = ge.load_package()
    A = bvc.augment
    dev = torch.device("cuda:0")
    B, T, Hs, S = a.clips, a.frames, a.src, a.size
    g = torch.Generator().manual_seed(0)
    one = torch.randint(0, 256, (16, T, 3, Hs, Hs), generator=g, dtype=torch.uint8)
    src = one.repeat((B + 15) // 16, 1, 1, 1, 1)[:B].contiguous().to(dev)
    rng = np.random.default_rng(0)

    def sampled(**kw):
        t0 = time.perf_counter()
        t = A.sample_params(B, T, (Hs, Hs), S, generator=rng, **kw)
        return t, (time.perf_counter() - t0) * 1e3

    tables = {
        "center_crop": (A.center_crop_params(B * T, (Hs, Hs), S), 0.0),
        "geometry": sampled(augs="c", flip=0.5),
        "jitter": sampled(augs="cjg", flip=0.5, jitter_p=1.0),
        "two_views": sampled(augs="cjg", flip=0.5, jitter_p=1.0, views=2),
    }
    outs = {k: torch.empty(t.shape[0], 3, S, S, dtype=torch.uint8, device=dev) for k, (t, _) in tables.items()}
    src_copy = torch.empty_like(src)
    out_copy = torch.empty_like(outs["two_views"])
    runs = {k: (lambda k=k: A.clip_transform(src, tables[k][0], S, out=outs[k])) for k in tables}
    # the post stage: its input is the `jitter` output
    post_in, post_out = outs["jitter"], torch.empty_like(outs["jitter"])
    post = {"post_blur": A.sample_post_params(B, T, S, "b", blur_p=1.0, generator=rng),
            "post_rotate": A.sample_post_params(B, T, S, "o", generator=rng),
            "post_both": A.sample_post_params(B, T, S, "bo", blur_p=1.0, generator=rng)}
    for k in post:
        runs[k] = lambda k=k: A.clip_post(post_in, post[k], out=post_out)
    aug = A.ClipAugment(S, augs="cjbo", jitter_p=1.0, generator=rng)
    aug_tables = aug.sample(B, T, (Hs, Hs))
    runs["augment_cjbo"] = lambda: aug(src, tables=aug_tables)
    runs["d2d_copy_post"] = lambda: post_out.copy_(post_in)
    for views in (1, 2):
        n = views * B * T
        runs[f"d2d_copy_{views}view"] = lambda n=n: (src_copy.copy_(src), out_copy[:n].copy_(outs["two_views"][:n]))

    def launches(t):
        return int(bool(((t["blur_r"] >= 0) | (t["gray"] != 0)).any())) + int(bool((t["rotate"] != 0).any()))

    def moved(name):
        if name == "d2d_copy_post":
            return 2 * post_in.numel()
        if name in post:
            return 2 * post_in.numel() * launches(post[name])
        if name == "augment_cjbo":
            t = aug_tables[0]
            return int((t["w"].astype(np.int64) * t["h"]).sum()) * 3 + 3 * post_in.numel() + 2 * post_in.numel() * launches(aug_tables[1])
        if name.startswith("d2d"):
            n = int(name[9]) * B * T
            return 2 * src.numel() + 2 * n * 3 * S * S
        t = tables[name][0]
        rd = int((t["w"].astype(np.int64) * t["h"]).sum()) * 3
        wr = t.shape[0] * 3 * S * S
        second = 2 * wr if bool(((t["nops"] > 0)).any()) else 0
        return rd + wr + second

    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.iters)
    for k, t in times.items():
        med = statistics.median(t)
        line = {"what": "clip_transform", "config": k, "clips": B, "frames": T, "src": Hs, "size": S, "ms_median": round(med, 3),
                "ms_min": round(min(t), 3), "ms_max": round(max(t), 3), "bytes_moved": moved(k),
                "GB_per_s": round(moved(k) / med / 1e6, 1), "rounds": a.rounds, "iters": a.iters}
        if k in post:
            line["output_frames"] = int(post[k].shape[0])
            line["blurred_frames"] = int((post[k]["blur_r"] >= 0).sum())
            line["box_radius_counts"] = [int((post[k]["blur_r"] == r).sum()) for r in range(4)]
        if k == "augment_cjbo":
            line["output_frames"] = int(aug_tables[1].shape[0])
            line["blurred_frames"] = int((aug_tables[1]["blur_r"] >= 0).sum())
        if k in tables:
            line["output_frames"] = int(tables[k][0].shape[0])
            line["host_sample_ms"] = round(tables[k][1], 2)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
