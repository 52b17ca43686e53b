"""Transformers fixtures for the VideoMAE sizes (bvc.VIDEOMAE_ARCHS small / large / huge)  --  runs on a CPU build machine only.

Builds transformers' VideoMAEForPreTraining (the installed version, 5.15.0 when these were made) with the oracle's deterministic
weights (oracle/videomae_oracle.py), runs its fp32 forward + backward on the oracle's synthetic batch, checks that the oracle's own
step agrees to fp32 round-off, and writes numbers only - loss, the three grad_logger probes, the L2 norm of every gradient tensor - to
tests/golden/videomae_{small,large,huge}_*.json:

    small_w_b2_s0, large_w_b2_s0, huge_w_b2_s0   full width, 2 encoder / 1 decoder layers, 2 clips, seed 0, mask 0.9
    huge_b2_s1                                   VideoMAE-H at full depth (32 / 4 layers), 2 clips, seed 1

    python tools/make_videomae_zoo_golden.py [--only small_w_b2_s0,...]

tests/test_gpu_videomae_model_zoo.py holds the GPU steps to these numbers.  Nothing under oracle/ is changed."""
import argparse
import dataclasses
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import videomae_oracle as vo   # noqa: E402
from oracle.make_golden import hf_model, summarize   # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
# (hidden, layers, heads, decoder hidden, decoder heads): bvc.VIDEOMAE_ARCHS (the test checks the configs agree)
ARCHS = {"small": (384, 12, 6, 192, 3), "large": (1024, 24, 16, 512, 8), "huge": (1280, 32, 16, 640, 8)}


def arch_config(arch, **kw):
    D, depth, heads, Dd, Hd = ARCHS[arch]
    base = dict(hidden_size=D, num_hidden_layers=depth, num_attention_heads=heads, intermediate_size=4 * D, decoder_hidden_size=Dd,
                decoder_num_attention_heads=Hd, decoder_num_hidden_layers=4, decoder_intermediate_size=4 * Dd)
    base.update(kw)
    return dataclasses.replace(vo.BASE, **base)


REDUCED = dict(num_hidden_layers=2, decoder_num_hidden_layers=1)
CASES = {
    "small_w_b2_s0": (arch_config("small", **REDUCED), 2, 0),
    "large_w_b2_s0": (arch_config("large", **REDUCED), 2, 0),
    "huge_w_b2_s0": (arch_config("huge", **REDUCED), 2, 0),
    "huge_b2_s1": (arch_config("huge"), 2, 1),
}


def case(name, cfg, batch, seed, wseed=0, ratio=0.9):
    params = vo.make_params(cfg, seed=wseed)
    pixels, mask = vo.synthetic_batch(cfg, batch, seed, ratio)
    model, ver = hf_model(cfg, params)
    out = model(pixels, bool_masked_pos=mask)
    out.loss.backward()
    loss = float(out.loss)
    hgrads = {k: v.grad.detach().clone() for k, v in model.named_parameters()}
    del out, model
    gc.collect()
    # pin: the oracle's step equals transformers' to fp32 round-off at this size too
    oloss, ograds = vo.step(cfg, params, pixels, mask)
    rel = abs(float(oloss) - loss) / abs(loss)
    gmax = max(float(g.norm()) for g in hgrads.values())
    worst = max(float((ograds[k] - g).norm() / (g.norm() + 1e-4 * gmax)) for k, g in hgrads.items())
    print(f"[{name}] transformers {ver}: loss {loss:.7f}; oracle loss rel {rel:.2e}, worst grad rel {worst:.2e}", flush=True)
    assert rel < 2e-6 and worst < 5e-5, (name, rel, worst)
    fx = {
        "case": name, "transformers": ver, "torch": torch.__version__,
        "config": cfg.__dict__, "batch": batch, "seed": seed, "weight_seed": wseed, "mask_ratio": ratio,
        "input": {"pixels": summarize(pixels), "mask_true": int(mask.sum())},
        "loss": loss,
        "grad_l2": {k: float(g.double().norm()) for k, g in hgrads.items()},
        "grad_probes": {k: float(hgrads[k].double().norm()) for k in vo.GRAD_PROBES},
    }
    with open(os.path.join(GOLD, f"videomae_{name}.json"), "w") as f:
        json.dump(fx, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="comma-separated case names (default: all)")
    args = ap.parse_args()
    torch.manual_seed(0)
    names = args.only.split(",") if args.only else list(CASES)
    for n in names:
        cfg, batch, seed = CASES[n]
        case(n, cfg, batch, seed)


if __name__ == "__main__":
    main()
