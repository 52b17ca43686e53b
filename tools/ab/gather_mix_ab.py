"""Patch gather with Mixup / CutMix against the plain gather at the fine-tuning shape (16 x 224^2 clips, patch 16, tubelet 2).

    python tools/bvc_tools.py ab gather_mix [--batch 16,64] [--iters 50] [--rounds 5]        # op timing, HIP events, warmed
    python tools/bvc_tools.py ab gather_mix --step [--batch 16]                              # one fine-tuning step with / without mix=
    rocprofv3 --kernel-trace -d DIR -o gm -- python tools/ab/gather_mix_ab.py --trace-driver --batch 16
    python tools/ab/gather_mix_ab.py --trace-read DIR --batch 16                             # per-variant kernel times of that trace

Variants: plain (gather_patches_kernel), and gather_patches_mix_kernel under identity specs, CutMix (one box of half the image area,
partner = the batch flipped; its edges off every grid, and again with every edge on a multiple of 32 pixels) and Mixup (lam = 0.7, no
box), each from f32 and from uint8 clips.  The op-level plain gather takes f32
only, so its uint8 time comes from the kernel trace of a one-layer model's forward (the driver runs every variant in a fixed order,
the reader assigns the gather dispatches of the trace by that order).  Bytes per pixel: uint8 plain / identity / CutMix 1 + 2, Mixup
2 + 2; f32 4 + 2 and 8 + 2.  Rounds alternate the variants; each line gives the median over rounds and the min - max spread.
Results: profiles/mixup_gather.txt."""
import argparse
import csv
import ctypes
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402

T, C, S, TS, PS = 16, 3, 224, 2, 16
NTOK = (T // TS) * (S // PS) ** 2
K = C * TS * PS * PS
SPECS = ("plain", "identity", "cutmix", "cutmix_aligned", "mixup")


def make_mix(bvc, spec, B, dev):
    flip = [B - 1 - b for b in range(B)]
    if spec == "identity":
        return bvc.ClipMix(list(range(B)), [1.0] * B, [(0, 0, 0, 0)] * B, image_size=(S, S), device=dev)
    if spec == "cutmix":                       # 158 x 159 of 224 x 224: half the area, edges off every 8- and 16-pixel grid
        return bvc.ClipMix(flip, [1.0] * B, [(33, 191, 30, 189)] * B, image_size=(S, S), device=dev)
    if spec == "cutmix_aligned":               # 160 x 160, every edge on a multiple of 32 pixels: no 128-byte line is read from both clips
        return bvc.ClipMix(flip, [1.0] * B, [(32, 192, 32, 192)] * B, image_size=(S, S), device=dev)
    return bvc.ClipMix(flip, [0.7] * B, [(0, 0, 0, 0)] * B, image_size=(S, S), device=dev)


def clips(B, dev):
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (B, T, C, S, S), generator=g, dtype=torch.uint8).to(dev)
    return {"u8": u8, "f32": ((u8.float() / 255.0 - 0.5) / 0.25).contiguous()}


def bytes_moved(spec, dtype, B):
    px = B * T * C * S * S
    rd = {"u8": 1, "f32": 4}[dtype] * (2 if spec == "mixup" else 1)
    return px * (rd + 2)


def op_timing(bvc, batches, iters, rounds):
    L = bvc._lib
    dev = torch.device("cuda:0")
    for B in batches:
        src = clips(B, dev)
        idx = (torch.arange(B * NTOK, dtype=torch.int32, device=dev) % NTOK).contiguous()
        A = torch.zeros(B * NTOK, K, dtype=torch.bfloat16, device=dev)
        runs = {}
        for dtype in ("f32", "u8"):
            fmt = L.pixel_format(src[dtype], 0.5, 0.25, C)
            for spec in SPECS:
                if spec == "plain":
                    if dtype == "u8":
                        continue
                    runs[(spec, dtype)] = lambda p=src[dtype].data_ptr(): L.check(L.lib().bvc_op_gather_patches(
                        p, idx.data_ptr(), A.data_ptr(), B, NTOK, T, C, S, S, TS, PS, L.current_stream_ptr()), "gather")
                else:
                    mix = make_mix(bvc, spec, B, dev)
                    runs[(spec, dtype)] = lambda p=src[dtype].data_ptr(), f=fmt, m=mix: L.check(L.lib().bvc_op_gather_patches_mix(
                        p, ctypes.byref(f) if f is not None else None, idx.data_ptr(), A.data_ptr(), m.table.data_ptr(), B, NTOK, T, C, S, S,
                        TS, PS, L.current_stream_ptr()), "gather_mix")
        times = {k: [] for k in runs}
        for fn in runs.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / iters)
        base = statistics.median(times[("plain", "f32")])
        for (spec, dtype), t in times.items():
            med = statistics.median(t)
            print(json.dumps({"what": "op", "batch": B, "source": dtype, "spec": spec, "us_median": round(med, 2), "us_min": round(min(t), 2),
                              "us_max": round(max(t), 2), "GB_per_s": round(bytes_moved(spec, dtype, B) / med / 1e3, 1),
                              "ratio_to_plain_f32": round(med / base, 3), "rounds": rounds, "iters": iters}))


def narrow_model(bvc, dev):
    """the fine-tuning geometry with a one-layer, 64-wide encoder: its forward launches the gather of the full-size clips"""
    cfg = bvc.VideoMAEConfig(image_size=S, patch_size=PS, num_channels=C, num_frames=T, tubelet_size=TS, hidden_size=64, num_hidden_layers=1,
                             num_attention_heads=1, intermediate_size=64, num_labels=10)
    return bvc.VideoMAEForVideoClassification(cfg).to(dev).train()


TRACE_WARM, TRACE_ITERS = 3, 10


def trace_driver(bvc, B):
    dev = torch.device("cuda:0")
    m = narrow_model(bvc, dev)
    src = clips(B, dev)
    for dtype in ("f32", "u8"):
        for spec in SPECS:
            for _ in range(TRACE_WARM + TRACE_ITERS):
                m(pixel_values=src[dtype], mix=None if spec == "plain" else make_mix(bvc, spec, B, dev))
            torch.cuda.synchronize()


def trace_read(directory, B):
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "gather_patches" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    per = TRACE_WARM + TRACE_ITERS
    assert len(rows) == 2 * len(SPECS) * per, f"{len(rows)} gather dispatches in the trace, expected {2 * len(SPECS) * per}"
    i = 0
    for dtype in ("f32", "u8"):
        for spec in SPECS:
            chunk = rows[i + TRACE_WARM:i + per]
            i += per
            assert all(("mix" in n) == (spec != "plain") for _, _, n in chunk)
            t = [(e - s) / 1e3 for s, e, _ in chunk]
            med = statistics.median(t)
            print(json.dumps({"what": "kernel_trace", "batch": B, "source": dtype, "spec": spec, "us_median": round(med, 2),
                              "us_min": round(min(t), 2), "us_max": round(max(t), 2), "GB_per_s": round(bytes_moved(spec, dtype, B) / med / 1e3, 1),
                              "dispatches": len(t)}))


def step_timing(bvc, B, steps, rounds):
    dev = torch.device("cuda:0")
    model = bvc.VideoMAEForVideoClassification(bvc.videomae_config("base", num_labels=400)).to(dev).train()
    model.config.problem_type = "soft_label_classification"
    u8 = clips(B, dev)["u8"]
    labels = torch.arange(B, device=dev) % 400
    mixup = bvc.Mixup(num_classes=400, generator=__import__("numpy").random.default_rng(0))
    plain_soft = bvc.Mixup(num_classes=400, prob=0.0)(B, labels, (S, S), device=dev)[1]

    def step(mixed):
        if mixed:
            mix, soft = mixup(B, labels, image_size=(S, S), device=dev)
        else:
            mix, soft = None, plain_soft
        model(pixel_values=u8, labels=soft, mix=mix).loss.backward()

    for mixed in (False, True):
        for _ in range(3):
            step(mixed)
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for _ in range(rounds):
        for mixed in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step(mixed)
            e1.record()
            e1.synchronize()
            times[mixed].append(e0.elapsed_time(e1) / steps)
    for mixed, t in times.items():
        print(json.dumps({"what": "finetune_fwd_bwd", "arch": "base", "batch": B, "source": "u8", "mix": "Mixup(0.8, 1.0) per batch" if mixed else None,
                          "ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3),
                          "rounds": rounds, "steps": steps}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="16,64")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--trace-driver", action="store_true")
    ap.add_argument("--trace-read", default=None)
    a = ap.parse_args()
    batches = [int(b) for b in a.batch.split(",")]
    if a.trace_read:
        trace_read(a.trace_read, batches[0])
        return
    ge.build()
    bvc = ge.load_package()
    if a.trace_driver:
        trace_driver(bvc, batches[0])
    elif a.step:
        step_timing(bvc, batches[0], a.steps, a.rounds)
    else:
        op_timing(bvc, batches, a.iters, a.rounds)


if __name__ == "__main__":
    main()
