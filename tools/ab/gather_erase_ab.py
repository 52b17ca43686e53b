"""Patch gather with random erasing (gather_patches_aug_kernel) against the plain gather and the mix kernel at the fine-tuning shape
(16 x 224^2 clips, patch 16, tubelet 2, all 1568 tokens).

    python tools/bvc_tools.py ab gather_erase [--batch 16,64] [--iters 50] [--rounds 7] [--parent-lib PATH]    # op timing, HIP events, warmed
    python tools/bvc_tools.py ab gather_erase --step [--batch 16]                        # one fine-tuning step with / without erase=

Variants, each from f32 and from uint8 clips (the op-level plain gather takes f32 only):
    plain            gather_patches_kernel
    mix_identity     gather_patches_mix_kernel under identity entries
    aug_nobox        the new kernel, one empty box per clip, no mix
    aug_pixel        one pixel-mode box of 96 x 96 pixels per clip (18 % of the image, about 1/6), rows [37, 133) x columns [50, 146):
                     edges off every grid
    aug_pixel_al     the same area with every edge on a multiple of 32 pixels, rows [32, 128) x columns [64, 160)
    aug_*_cutmix     the same three with a CutMix armed as well (the box of tools/ab/gather_mix_ab.py, partner = the batch flipped)
    mix_cutmix       that CutMix on the mix kernel
With --parent-lib (a libbvc_hip.so built from the parent commit) plain, mix_identity and mix_cutmix are timed on that library too
(suffix @parent), in the same process and the same rounds: the A - A' of two builds of unchanged kernels.  Rounds alternate the variants;
each line gives the median over rounds and the min - max spread.  Results: profiles/erase_gather.txt."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402

T, C, S, TS, PS = 16, 3, 224, 2, 16
NTOK = (T // TS) * (S // PS) ** 2
K = C * TS * PS * PS
EMPTY = (0, 0, 0, 0)
ERASE = {"nobox": EMPTY, "pixel": (37, 133, 50, 146), "pixel_al": (32, 128, 64, 160)}
CUTMIX = (33, 191, 30, 189)
SEED, OFFSET = 0x9E3779B97F4A7C15, 1


def clips(B, dev):
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (B, T, C, S, S), generator=g, dtype=torch.uint8).to(dev)
    return {"u8": u8, "f32": ((u8.float() / 255.0 - 0.5) / 0.25).contiguous()}


def parent_library(path, L):
    """the two op entry points of another build of the library, with this build's argument types"""
    lib = ctypes.CDLL(path)
    for name in ("bvc_op_gather_patches", "bvc_op_gather_patches_mix"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SYMBOLS[name]
    return lib


def op_timing(bvc, batches, iters, rounds, parent):
    L = bvc._lib
    dev = torch.device("cuda:0")
    libs = {"": L.lib()}
    if parent:
        libs["@parent"] = parent_library(parent, L)
    for B in batches:
        src = clips(B, dev)
        idx = (torch.arange(B * NTOK, dtype=torch.int32, device=dev) % NTOK).contiguous()
        A = torch.zeros(B * NTOK, K, dtype=torch.bfloat16, device=dev)
        flip = [B - 1 - b for b in range(B)]
        ident = bvc.ClipMix(list(range(B)), [1.0] * B, [EMPTY] * B, image_size=(S, S), device=dev)
        cut = bvc.ClipMix(flip, [1.0] * B, [CUTMIX] * B, image_size=(S, S), device=dev)
        tabs = {k: bvc.ClipErase([[box]] * B, "pixel", seed=SEED, offset=OFFSET, image_size=(S, S), device=dev) for k, box in ERASE.items()}
        runs = {}
        for dtype in ("f32", "u8"):
            fmt = L.pixel_format(src[dtype], 0.5, 0.25, C)
            fp = ctypes.byref(fmt) if fmt is not None else None
            p = src[dtype].data_ptr()
            for tag, lib in libs.items():
                if dtype == "f32":
                    runs[("plain" + tag, dtype)] = lambda p=p, lib=lib: L.check(lib.bvc_op_gather_patches(
                        p, idx.data_ptr(), A.data_ptr(), B, NTOK, T, C, S, S, TS, PS, L.current_stream_ptr()), "gather")
                for name, mix in (("mix_identity", ident), ("mix_cutmix", cut)):
                    runs[(name + tag, dtype)] = lambda p=p, fp=fp, m=mix, lib=lib: L.check(lib.bvc_op_gather_patches_mix(
                        p, fp, idx.data_ptr(), A.data_ptr(), m.table.data_ptr(), B, NTOK, T, C, S, S, TS, PS, L.current_stream_ptr()), "gather_mix")
            for k, er in tabs.items():
                for suffix, mix in (("", None), ("_cutmix", cut)):
                    runs[("aug_" + k + suffix, dtype)] = lambda p=p, fp=fp, er=er, m=mix: L.check(L.lib().bvc_op_gather_patches_aug(
                        p, fp, idx.data_ptr(), A.data_ptr(), m.table.data_ptr() if m is not None else None, er.table.data_ptr(), 1, SEED, OFFSET,
                        B, NTOK, T, C, S, S, TS, PS, L.current_stream_ptr()), "gather_aug")
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
        for (spec, dtype), t in times.items():
            med = statistics.median(t)
            base = statistics.median(times[("mix_identity", dtype)])
            print(json.dumps({"what": "op", "batch": B, "source": dtype, "spec": spec, "us_median": round(med, 2), "us_min": round(min(t), 2),
                              "us_max": round(max(t), 2), "ratio_to_mix_identity": round(med / base, 3), "rounds": rounds, "iters": iters}), flush=True)


def step_timing(bvc, B, steps, rounds):
    dev = torch.device("cuda:0")
    model = bvc.VideoMAEForVideoClassification(bvc.videomae_config("base", num_labels=400)).to(dev).train()
    u8 = clips(B, dev)["u8"]
    labels = torch.arange(B, device=dev) % 400
    specs = {"none": None, "recipe p=0.25": bvc.RandomErasing(generator=np.random.default_rng(0)),
             "every clip p=1": bvc.RandomErasing(probability=1.0, generator=np.random.default_rng(0))}

    def step(re):
        model(pixel_values=u8, labels=labels, erase=re(B, image_size=(S, S), device=dev) if re is not None else None).loss.backward()

    for re in specs.values():
        for _ in range(3):
            step(re)
    torch.cuda.synchronize()
    times = {k: [] for k in specs}
    for _ in range(rounds):
        for k, re in specs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step(re)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / steps)
    for k, t in times.items():
        print(json.dumps({"what": "finetune_fwd_bwd", "arch": "base", "batch": B, "source": "u8", "erase": k, "ms_median": round(statistics.median(t), 3),
                          "ms_min": round(min(t), 3), "ms_max": round(max(t), 3), "rounds": rounds, "steps": steps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="16,64")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    batches = [int(b) for b in a.batch.split(",")]
    ge.build()
    bvc = ge.load_package()
    if a.step:
        step_timing(bvc, batches[0], a.steps, a.rounds)
    else:
        op_timing(bvc, batches, a.iters, a.rounds, a.parent_lib)


if __name__ == "__main__":
    main()
