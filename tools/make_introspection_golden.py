"""Transformers fixture for output_hidden_states / output_attentions  --  runs on a CPU build machine only.

Builds transformers' VideoMAEForVideoClassification (the installed version, 5.15.0 when this was made) with
attn_implementation="eager" at the oracle's TINY shape with its deterministic weights (vo.make_params(seed=0)) and the default
fc_norm, runs its fp32 forward on vo.synthetic_batch(cfg, 2, 0) with both outputs requested, checks that the float64 restatement
(tests/introspection_ref.encoder_states) agrees to fp32 round-off, and writes numbers only - per-layer hidden-state norms,
per-(layer, head) attention norms and a few full rows of each - to tests/golden/videomae_introspect_tiny.json:

    python tools/make_introspection_golden.py

tests/test_introspection_ref.py (CPU) and tests/test_gpu_videomae_introspect.py hold the references and the GPU outputs to these
numbers.  Nothing under oracle/ is changed."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import videomae_oracle as vo   # noqa: E402
from tests import introspection_ref as IR   # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
BATCH, SEED, WEIGHT_SEED = 2, 0, 0


def transformers_states(cfg, params, pixels):
    """(hidden_states, attentions) of transformers' eager VideoMAEForVideoClassification(num_labels=0), fp32, on the CPU."""
    import transformers
    tc = transformers.VideoMAEConfig(
        image_size=cfg.image_size, patch_size=cfg.patch_size, num_channels=cfg.num_channels, num_frames=cfg.num_frames,
        tubelet_size=cfg.tubelet_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size, use_mean_pooling=True,
        num_labels=0, attn_implementation="eager")
    model = transformers.VideoMAEForVideoClassification(config=tc)
    sd = {k: v for k, v in params.items() if k.startswith("videomae.")}
    sd.update({"fc_norm.weight": torch.ones(cfg.hidden_size), "fc_norm.bias": torch.zeros(cfg.hidden_size)})
    assert set(model.state_dict()) == set(sd), set(model.state_dict()) ^ set(sd)
    model.load_state_dict(sd)
    model.eval()
    with torch.no_grad():
        out = model(pixel_values=pixels, output_hidden_states=True, output_attentions=True)
    assert len(out.hidden_states) == cfg.num_hidden_layers + 1 and len(out.attentions) == cfg.num_hidden_layers
    return [h.detach() for h in out.hidden_states], [a.detach() for a in out.attentions]


def main():
    import transformers
    cfg = vo.TINY
    params = vo.make_params(cfg, seed=WEIGHT_SEED)
    pixels, _ = vo.synthetic_batch(cfg, BATCH, SEED)
    hs, att = transformers_states(cfg, params, pixels)
    rhs, ratt = IR.encoder_states(cfg, params, pixels)
    eh = max(float((a.double() - b).abs().max()) for a, b in zip(hs, rhs))
    ea = max(float((a.double() - b).abs().max()) for a, b in zip(att, ratt))
    print(f"[introspect_tiny] transformers {transformers.__version__}: restatement differs by {eh:.2e} (hidden states, absolute), "
          f"{ea:.2e} (attentions)", flush=True)
    assert eh < 2e-5 and ea < 1e-7, (eh, ea)
    fx = {"case": "introspect_tiny", "transformers": transformers.__version__, "torch": torch.__version__,
          "config": cfg.__dict__, "batch": BATCH, "seed": SEED, "weight_seed": WEIGHT_SEED, "rows": list(IR.FIXTURE_ROWS)}
    view = IR.fixture_view(hs, att)

    def short(v):      # float32 values: 9 significant digits restore them exactly
        return [short(x) for x in v] if isinstance(v, list) else float(f"{v:.9g}")
    fx.update({k: short(v) for k, v in view.items()})
    with open(os.path.join(GOLD, IR.FIXTURE), "w") as f:
        json.dump(fx, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
