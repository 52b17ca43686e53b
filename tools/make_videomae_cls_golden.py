"""Transformers fixture for VideoMAEForVideoClassification fine-tuning  --  runs on a CPU build machine only.

Builds transformers' VideoMAEForVideoClassification (the installed version, 5.15.0 when this was made) at VideoMAE-base with
num_labels = 10, the oracle's deterministic "videomae.*" weights (oracle/videomae_oracle.py make_params) and a seeded fc_norm /
classifier, runs its fp32 forward and backward (labels -> cross-entropy) on the oracle's synthetic pixels, checks that the oracle
restatement (vo.encode, F.layer_norm, F.linear, F.cross_entropy under autograd) agrees to fp32 round-off, and writes numbers only -
the loss, the logits, the L2 norm of every gradient tensor - to tests/golden/videomae_cls_base_b2_s0.json:

    python tools/make_videomae_cls_golden.py

tests/test_gpu_videomae_cls.py holds the GPU step to these numbers.  Nothing under oracle/ is changed."""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import videomae_oracle as vo   # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NUM_LABELS, BATCH, SEED, WEIGHT_SEED, HEAD_SEED = 10, 2, 0, 0, 5
LABELS = [3, 7]


def head_params(D, num_labels, seed):
    """fc_norm weight / bias and classifier weight / bias of the fixture (and of the GPU tests that read it): the classifier weight
    at transformers' initializer_range (0.02), as a fine-tune starts from it; fc_norm and the bias perturbed around their defaults."""
    g = torch.Generator().manual_seed(seed)
    fw = 1 + 0.1 * torch.randn(D, generator=g)
    fb = 0.05 * torch.randn(D, generator=g)
    cw = 0.02 * torch.randn(num_labels, D, generator=g)
    cb = 0.01 * torch.randn(num_labels, generator=g)
    return fw, fb, cw, cb


def main():
    import transformers
    cfg = vo.BASE
    params = vo.make_params(cfg, seed=WEIGHT_SEED)
    fw, fb, cw, cb = head_params(cfg.hidden_size, NUM_LABELS, HEAD_SEED)
    pixels, _ = vo.synthetic_batch(cfg, BATCH, SEED, 0.9)
    labels = torch.tensor(LABELS, dtype=torch.long)

    tc = transformers.VideoMAEConfig(
        image_size=cfg.image_size, patch_size=cfg.patch_size, num_channels=cfg.num_channels, num_frames=cfg.num_frames,
        tubelet_size=cfg.tubelet_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size, use_mean_pooling=True,
        num_labels=NUM_LABELS)
    model = transformers.VideoMAEForVideoClassification(config=tc)
    sd = {k: v for k, v in params.items() if k.startswith("videomae.")}
    sd.update({"fc_norm.weight": fw, "fc_norm.bias": fb, "classifier.weight": cw, "classifier.bias": cb})
    assert set(model.state_dict()) == set(sd), set(model.state_dict()) ^ set(sd)
    model.load_state_dict(sd)
    model.train()
    out = model(pixel_values=pixels, labels=labels)
    out.loss.backward()
    assert model.config.problem_type == "single_label_classification"
    loss, logits = float(out.loss.detach()), out.logits.detach().clone()
    hgrads = {k: v.grad.detach().clone() for k, v in model.named_parameters()}
    del out, model

    # the oracle restatement under autograd
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pooled, _ = vo.encode(cfg, p, pixels, p["fc_norm.weight"], p["fc_norm.bias"], 1e-5)
    ologits = F.linear(pooled, p["classifier.weight"], p["classifier.bias"])
    oloss = F.cross_entropy(ologits, labels)
    oloss.backward()
    rel = abs(float(oloss) - loss) / abs(loss)
    el = float((ologits.detach() - logits).norm() / logits.norm())
    gmax = max(float(g.norm()) for g in hgrads.values())
    worst = max(float((p[k].grad - g).norm() / (g.norm() + 1e-4 * gmax)) for k, g in hgrads.items())
    print(f"[cls_base_b2_s0] transformers {transformers.__version__}: loss {loss:.7f}; oracle loss rel {rel:.2e}, logits rel {el:.2e}, "
          f"worst grad rel {worst:.2e}", flush=True)
    assert rel < 2e-6 and el < 2e-5 and worst < 5e-5, (rel, el, worst)
    fx = {
        "case": "cls_base_b2_s0", "transformers": transformers.__version__, "torch": torch.__version__,
        "config": cfg.__dict__, "num_labels": NUM_LABELS, "batch": BATCH, "seed": SEED, "weight_seed": WEIGHT_SEED,
        "head_seed": HEAD_SEED, "labels": LABELS, "fc_norm_eps": 1e-5,
        "loss": loss,
        "logits": [[float(x) for x in row] for row in logits],
        "grad_l2": {k: float(g.double().norm()) for k, g in hgrads.items()},
    }
    with open(os.path.join(GOLD, "videomae_cls_base_b2_s0.json"), "w") as f:
        json.dump(fx, f, indent=1)


if __name__ == "__main__":
    main()
