"""LARS.step against SGD(momentum=0.9).step and LAMB.step against AdamW.step on the VideoMAE-base flat layout (94 220 160 elements), one
group and the two-group split, HIP events around windows of steps, the four optimisers alternating.  --dry: shapes only (no GPU); --out FILE: the record as JSON."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from oracle import videomae_oracle as vo  # noqa: E402
from tests import layerwise_ref as lw  # noqa: E402

bvc = ge.load_package()
kw = {k: v for k, v in vo.BASE.__dict__.items() if k != "decoder_norm_eps"}
model = bvc.VideoMAEForPreTraining(bvc.VideoMAEConfig(**kw))
shapes = [tuple(p.shape) for _n, p in model.named_parameters() if p.requires_grad]
total = sum(int(torch.Size(s).numel()) for s in shapes)
print("tensors", len(shapes), "elements", total, "flat", model._numel)
del model
if "--dry" in sys.argv:
    sys.exit(0)

dev = torch.device("cuda:0")
WARM, ITERS, ROUNDS = 10, 200, 5


def make(kind, split):
    m = lw.FlatStandIn(bvc, dev, shadow=True, shapes=shapes)
    m._flat.mul_(0.02)
    m._shadow.copy_(m._flat.to(torch.bfloat16))
    m._flat_grad.copy_(0.01 * torch.randn(m.n, device=dev))
    if split:
        groups = [dict(params=[p for p in m.live if p.ndim > 1], weight_decay=0.05),
                  dict(params=[p for p in m.live if p.ndim <= 1], weight_decay=0.0)]
        if kind in ("lars", "lamb"):
            groups[1]["adapt"] = False
    else:
        groups = [dict(params=list(m.live), weight_decay=0.05)]
    opt = {"lars": lambda: bvc.optim.LARS(groups, lr=1e-4, momentum=0.9), "sgd": lambda: bvc.optim.SGD(groups, lr=1e-6, momentum=0.9),
           "lamb": lambda: bvc.optim.LAMB(groups, lr=1e-6), "adamw": lambda: bvc.optim.AdamW(groups, lr=1e-6)}[kind]()
    return m, opt


def window(opt, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        opt.step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


out = {"elements": total, "tensors": len(shapes), "iters_per_window": ITERS, "windows": ROUNDS}
for split in (False, True):
    cases = {k: make(k, split) for k in ("sgd", "lars", "adamw", "lamb")}
    for _m, opt in cases.values():
        window(opt, WARM)
    times = {k: [] for k in cases}
    for _ in range(ROUNDS):
        for k, (_m, opt) in cases.items():
            times[k].append(window(opt, ITERS))
    key = "two_groups" if split else "one_group"
    out[key] = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in times.items()}
    for k, (m, _opt) in cases.items():
        assert torch.isfinite(m._flat).all(), k
    print(key, json.dumps(out[key]))
    del cases
    torch.cuda.empty_cache()
if "--out" in sys.argv:      # --out FILE: the whole record as JSON (profiles/layerwise_step.json is one)
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
