"""Cost of the deterministic mode (bvc.use_deterministic_algorithms): same-process A / B / A' of the default and the deterministic
mode - VideoMAE-base forward + backward at 16, 64 and 256 clips, JEPA ViT-B/16 (context encoder + predictor + smooth-L1, forward +
backward) at 16 samples - and the bytes of the mode's workspace after each.  The optimiser, the EMA and the loaders do not change
with the mode and are left out.  One JSON line per case on stdout.

    python tools/bvc_tools.py ab deterministic [--steps 20] [--clips 16,64,256] [--no-jepa] [--det-only]
    (the workspace grows only: for the bytes one case needs alone, run it in a process of its own, e.g. --clips "" for JEPA only)"""
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
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--clips", default="16,64,256")
ap.add_argument("--no-jepa", action="store_true")
ap.add_argument("--det-only", action="store_true", help="deterministic mode only (for a rocprofv3 kernel-stats run)")
args = ap.parse_args()
ge.build()
bvc = ge.load_package()
from oracle import videomae_oracle as vo   # noqa: E402

dev = torch.device("cuda:0")


def timed(step, det):
    bvc.use_deterministic_algorithms(det)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    bvc.use_deterministic_algorithms(False)
    return t0.elapsed_time(t1) / args.steps


def ab(name, step):
    if args.det_only:
        b = timed(step, True)
        print(json.dumps({"case": name, "deterministic_ms": round(b, 4),
                          "workspace_bytes": int(bvc._lib.lib().bvc_deterministic_workspace_bytes())}), flush=True)
        return
    a = timed(step, False)
    b = timed(step, True)
    a2 = timed(step, False)
    ws = int(bvc._lib.lib().bvc_deterministic_workspace_bytes())
    base = 0.5 * (a + a2)
    print(json.dumps({"case": name, "default_ms": round(a, 4), "deterministic_ms": round(b, 4), "default2_ms": round(a2, 4),
                      "overhead": round(b / base - 1.0, 4), "spread_aa": round(abs(a2 - a) / base, 4), "workspace_bytes": ws}), flush=True)


cfg = vo.BASE
kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
for clips in [int(c) for c in args.clips.split(",") if c]:
    model = bvc.VideoMAEForPreTraining(bvc.VideoMAEConfig(**kw)).to(dev).train()
    pixels, mask = vo.synthetic_batch(cfg, clips, seed=5, mask_ratio=0.9)
    px, mk = pixels.to(dev), mask.to(dev)

    def vstep():
        for p in model.parameters():
            p.grad = None
        model(px, bool_masked_pos=mk).loss.backward()

    ab(f"videomae_base_b{clips}", vstep)
    del model, px, mk
    torch.cuda.empty_cache()

if not args.no_jepa:
    torch.manual_seed(0)
    enc, pred = bvc.jepa.get_model(dev, patch_size=16, tubelet_size=1, num_frames=2, model_name="vit_base", image_size=224)
    for m in (enc, pred):
        m._ensure_flat(dev)
    B = 16
    g = torch.Generator().manual_seed(1)
    imgs = ((torch.randint(0, 256, (B, 2, 3, 224, 224), generator=g, dtype=torch.uint8).float() / 255 - 0.5) / 0.25).to(dev)
    me = [torch.stack([torch.sort(torch.randperm(196, generator=g)[:100]).values for _ in range(B)]).to(dev)]
    mp = [(torch.stack([torch.sort(torch.randperm(196, generator=g)[:25]).values for _ in range(B)]) + 196).to(dev) for _ in range(4)]
    h = torch.randn(4 * B * 25, 768, device=dev)

    def jstep():
        for m in (enc, pred):
            for p in m.parameters():
                p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            z = pred(enc(imgs, me), me, mp)
            loss = torch.nn.functional.smooth_l1_loss(z.float(), h.view_as(z).float())
        loss.backward()

    ab("jepa_vit_base_b16", jstep)
