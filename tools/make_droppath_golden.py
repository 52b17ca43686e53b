"""Drop-path fixture from the reference's own modules  --  runs on a CPU build machine that holds a reference checkout.

Imports pretraining/predictive/vision_transformer.py of the reference (torch / numpy only), builds its VisionTransformer and
vit_predictor with drop_path_rate > 0 and the oracle's deterministic weights, runs the train-step arithmetic of
pretrain_jepa.py:383-402 in train mode under torch.manual_seed, and records numbers only: the uniform draws its drop_path() took (in
call order: encoder blocks, then predictor blocks; attention branch before MLP branch; blocks whose rate is 0 draw nothing), the loss,
a digest of the predictions and the L2 norm of every gradient tensor - to tests/golden/jepa_droppath.json:

    python tools/make_droppath_golden.py --reference /path/to/baby-vision-curriculum

tests/test_dropout_ref.py holds tests/dropout_ref.py (fed the recorded draws through bvc.dropgate.path_scale_from_uniform) to these
numbers.  Nothing under oracle/ is changed."""
import argparse
import dataclasses
import json
import os
import sys
from functools import partial

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import jepa_oracle as jo   # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
RATE = 0.5
# (name, config, B, n_ctx, n_pred, mask sets, weight seed, torch seed): every stack at least two layers deep (layer 0 never drops)
SPECS = [("tiny", dataclasses.replace(jo.TINY, pred_depth=2), 3, 6, 4, 4, 0, 0),
         ("tiny_hd24", dataclasses.replace(jo.TINY_HD24, depth=3), 2, 7, 5, 2, 2, 1)]


def digest(t):
    t = t.detach().double()
    return {"l2": float(t.norm()), "mean": float(t.mean()), "head": [float(v) for v in t.flatten()[:8]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("BVC_REFERENCE"), help="checkout of the reference repository")
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit("give --reference (or BVC_REFERENCE): the checkout whose pretraining/predictive/vision_transformer.py is imported")
    sys.path.insert(0, os.path.join(args.reference, "pretraining", "predictive"))
    for m in ("mask", "tensors", "vision_transformer"):
        sys.modules.pop(m, None)
    import vision_transformer as rvit
    import tensors as rten

    cases = []
    for name, cfg, B, n_ctx, n_pred, nsets, wseed, tseed in SPECS:
        enc_p = jo.make_params(jo.encoder_shapes(cfg), cfg, wseed)
        pred_p = jo.make_params(jo.predictor_shapes(cfg), cfg, wseed + 50)
        tgt_p = jo.make_params(jo.encoder_shapes(cfg), cfg, wseed + 100)
        imgs, m_enc, m_pred = jo.synthetic_inputs(cfg, B, wseed, n_ctx, n_pred, nsets)
        kw = dict(img_size=[cfg.image_size], patch_size=cfg.patch_size, num_frames=cfg.num_frames, tubelet_size=cfg.tubelet_size,
                  embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, qkv_bias=True,
                  norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
        enc = rvit.VisionTransformer(drop_path_rate=RATE, **kw)
        tgt = rvit.VisionTransformer(**kw)
        pred = rvit.vit_predictor(sequence_shape=enc.sequence_shape, embed_dim=cfg.embed_dim, predictor_embed_dim=cfg.pred_dim,
                                  depth=cfg.pred_depth, num_heads=enc.num_heads, drop_path_rate=RATE)
        enc.load_state_dict(enc_p); tgt.load_state_dict(tgt_p); pred.load_state_dict(pred_p)
        enc.train(); pred.train(); tgt.eval()
        with torch.no_grad():
            h = rten.repeat_interleave_batch(rten.apply_masks(F.layer_norm(tgt(imgs), (cfg.embed_dim,)), m_pred), B, repeat=len(m_enc))
        draws, real_rand = [], torch.rand

        def recording_rand(*a, **k):
            u = real_rand(*a, **k)
            draws.append(u.flatten().tolist())
            return u

        torch.manual_seed(tseed)
        torch.rand = recording_rand
        try:
            zc = enc(imgs, m_enc)
            n_enc = len(draws)
            z = pred(zc, m_enc, m_pred)
        finally:
            torch.rand = real_rand
        loss = F.smooth_l1_loss(z, h)
        loss.backward()

        def table(flat, depth, samples):      # call order -> [depth][2][samples]; None for the layers that drew nothing (rate 0)
            rates = [x.item() for x in torch.linspace(0, RATE, depth)]
            it = iter(flat)
            out = [[next(it), next(it)] if r > 0 else None for r in rates]
            assert next(it, None) is None and all(len(u) == samples for pair in out if pair for u in pair)
            return out

        eu, pu = table(draws[:n_enc], cfg.depth, B), table(draws[n_enc:], cfg.pred_depth, nsets * B)
        for tab in (eu, pu):       # a fixture whose gates are all kept (or all dropped) would pin nothing
            rates = [x.item() for x in torch.linspace(0, RATE, len(tab))]
            flags = [u < rates[i] for i, pair in enumerate(tab) if pair for row in pair for u in row]      # dropped: floor(1 - rate + u) = 0
            assert any(flags) and not all(flags), name
        cases.append({"case": name, "config": dataclasses.asdict(cfg), "B": B, "n_ctx": n_ctx, "n_pred": n_pred, "nsets": nsets,
                      "weight_seed": wseed, "torch_seed": tseed, "drop_path_rate": RATE, "enc_draws": eu, "pred_draws": pu,
                      "loss": float(loss.detach()), "z": digest(z), "zc": digest(zc),
                      "enc_grad_l2": {k: float(p.grad.double().norm()) for k, p in enc.named_parameters() if p.grad is not None},
                      "pred_grad_l2": {k: float(p.grad.double().norm()) for k, p in pred.named_parameters() if p.grad is not None}})
        print(f"[droppath {name}] loss {float(loss):.7f}, {n_enc} + {len(draws) - n_enc} draws")
    with open(os.path.join(GOLD, "jepa_droppath.json"), "w") as f:
        json.dump({"source": "pretraining/predictive/vision_transformer.py:145-164,213-231,332,465 (drop_path, Block, the rate schedules), "
                             "tensors.py, pretrain_jepa.py:383-402", "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
