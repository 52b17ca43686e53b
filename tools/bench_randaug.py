"""rand_augment on 64 x 16 frames of 224 x 224: a sampled rand-m7-n4-mstd0.5-inc1 table, four stages on every frame, each op alone, the
identity table, and clip_post on the same frames.  HIP events around every call (each call uploads its table), 3 warm-up calls, 20 or
10 samples; prints one JSON line per row with the median, the extremes and the 10th / 90th percentile in microseconds.

    python tools/bench_randaug.py [--out profiles/randaug_bench.jsonl]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

bvc = ge.load_package()
A = bvc.augment
dev = torch.device("cuda:0")
B, T, H, W = 64, 16, 224, 224
F = B * T
g = torch.Generator().manual_seed(0)
x = torch.randint(0, 256, (F, 3, H, W), generator=g, dtype=torch.uint8).to(dev)
out = torch.empty_like(x)
frame_bytes = 3 * H * W
log = open(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.devnull, "a")


def timed(fn, warm=3, n=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    return dict(median_us=float(np.median(ts)), min_us=float(ts.min()), p10_us=float(np.percentile(ts, 10)), p90_us=float(np.percentile(ts, 90)),
                max_us=float(ts.max()), samples=n)


def report(name, r, **kw):
    r = dict(name=name, frames=F, H=H, W=W, **kw, **r)
    line = json.dumps(r)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


need = int(bvc._lib.lib().bvc_op_clip_randaug_workspace(F, H, W))
work = torch.empty(need, dtype=torch.uint8, device=dev)

table = A.sample_randaug_params(B, T, (H, W), generator=np.random.default_rng(0), **A.parse_randaug("rand-m7-n4-mstd0.5-inc1"))
nops = table["nops"]
stage_frames = [int((nops > s).sum()) for s in range(int(nops.max()))]
stat_frames = [int(sum(1 for e in table if int(e["nops"]) > s and int(e["stage"][s]["op"]) in (0, 1, 7))) for s in range(int(nops.max()))]
moved = sum(2 * f * frame_bytes for f in stage_frames) + sum(f * frame_bytes for f in stat_frames) + int((nops == 0).sum()) * 2 * frame_bytes
r = timed(lambda: A.rand_augment(x, table, out=out, workspace=work))
report("rand_augment n4 sampled", r, stage_frames=stage_frames, stat_frames=stat_frames, bytes_moved=moved,
       bytes_over_8TBs_us=moved / 8.0e12 * 1e6, achieved_TBs=moved / (r["median_us"] * 1e-6) / 1e12)

table_p1 = A.sample_randaug_params(B, T, (H, W), prob=1.0, generator=np.random.default_rng(1))
r = timed(lambda: A.rand_augment(x, table_p1, out=out, workspace=work))
report("rand_augment n4 p1 (four stages on every frame)", r)

for name, p in [("AutoContrast", None), ("Equalize", None), ("Invert", None), ("Posterize", 2), ("Solarize", 77), ("SolarizeAdd", 77), ("Color", 1.6),
                ("Contrast", 1.6), ("Brightness", 1.6), ("Sharpness", 1.6), ("ShearX", 0.2), ("ShearY", 0.2), ("TranslateX", 30.5),
                ("TranslateY", 30.5), ("Rotate", 20.0)]:
    t1 = A.empty_randaug_table(F)
    t1[:] = A.randaug_entry([(name, p)], (H, W))
    stat = name in ("AutoContrast", "Equalize", "Contrast")
    mv = (3 if stat else 2) * F * frame_bytes
    r = timed(lambda: A.rand_augment(x, t1, out=out, workspace=work), n=10)
    report(f"one stage: {name}", r, bytes_moved=mv, bytes_over_8TBs_us=mv / 8.0e12 * 1e6, achieved_TBs=mv / (r["median_us"] * 1e-6) / 1e12)

r = timed(lambda: A.rand_augment(x, A.empty_randaug_table(F), out=out, workspace=work), n=10)
report("identity table (one copy)", r)

for augs in ("bo", "o", "b"):
    post = A.sample_post_params(B, T, (H, W), augs, generator=np.random.default_rng(2))
    r = timed(lambda: A.clip_post(x, post, out=out), n=10)
    report(f"clip_post augs={augs!r} sampled", r)
