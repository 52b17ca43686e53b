"""tests/dropout_ref.py (the fp32 reference of the gated stacks that the GPU tests use) pinned on the CPU: to the oracle with every
gate one, to transformers' VideoMAEForVideoClassification with its nn.Dropout modules replaced by the same masks, and to the
fixture the reference's own vision_transformer.py wrote for drop path (tools/make_droppath_golden.py).  Bar: fp32 round-off,
assert_close with rtol = atol = 1e-6 (what tests/test_oracle_golden.py holds a restatement to)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as ge
from oracle import jepa_oracle as jo
from oracle import videomae_oracle as vo
from tests import dropout_ref as dr
from tools.make_videomae_cls_golden import head_params

TOL = dict(rtol=1e-6, atol=1e-6)


@pytest.fixture(scope="module")
def bvc():
    ge.build()
    return ge.load_package()


def _ones(depth):
    return [(torch.ones(1), torch.ones(1)) for _ in range(depth)]


@pytest.mark.parametrize("ones", [False, True])
def test_all_gates_one_is_the_oracle(ones):
    cfg = vo.TINY
    p = vo.make_params(cfg, seed=0)
    fw, fb, _, _ = head_params(cfg.hidden_size, 3, 5)
    px, _ = vo.synthetic_batch(cfg, 3, 1, 0.9)
    a = dr.videomae_encode(cfg, p, px, fw, fb, 1e-5, _ones(cfg.num_hidden_layers) if ones else None)
    b = vo.encode(cfg, p, px, fw, fb, 1e-5)
    for x, y in zip(a, b):
        torch.testing.assert_close(x, y, **TOL)
    for jc in (jo.TINY, jo.TINY_HD24):
        ep = jo.make_params(jo.encoder_shapes(jc), jc, 2)
        pp = jo.make_params(jo.predictor_shapes(jc), jc, 52)
        imgs, m_enc, m_pred = jo.synthetic_inputs(jc, 3, 2, 6, 4)
        za = dr.jepa_encoder_forward(jc, ep, imgs, m_enc, _ones(jc.depth) if ones else None)
        zb = jo.encoder_forward(jc, ep, imgs, m_enc)
        torch.testing.assert_close(za, zb, **TOL)
        torch.testing.assert_close(dr.jepa_encoder_forward(jc, ep, imgs), jo.encoder_forward(jc, ep, imgs), **TOL)
        torch.testing.assert_close(dr.jepa_predictor_forward(jc, pp, zb, m_enc, m_pred, _ones(jc.pred_depth) if ones else None),
                                   jo.predictor_forward(jc, pp, zb, m_enc, m_pred), **TOL)


class _FixedDropout(torch.nn.Module):
    """nn.Dropout with the mask given: x * keep / (1 - p)."""

    def __init__(self, keep, p):
        super().__init__()
        self.keep, self.p = keep, p

    def forward(self, x):
        return x * (self.keep.view_as(x).to(x.dtype) / (1.0 - self.p))


def test_hidden_dropout_matches_transformers_with_the_same_masks(bvc):
    transformers = pytest.importorskip("transformers")
    cfg, B, p_drop, NL = vo.TINY, 3, 0.1, 10
    params = vo.make_params(cfg, seed=0)
    heads = dict(zip(("fc_norm.weight", "fc_norm.bias", "classifier.weight", "classifier.bias"), head_params(cfg.hidden_size, NL, 5)))
    px, _ = vo.synthetic_batch(cfg, B, 0, 0.9)
    labels = torch.tensor([3, 7, 1])
    M = B * cfg.seq_len
    masks = {(l, b): bvc.dropgate.dropout_mask_host(9, 4, l, b, M, cfg.hidden_size, p_drop) for l in range(cfg.num_hidden_layers) for b in (0, 1)}
    assert all(0 < int(m.sum()) < m.numel() for m in masks.values())
    tc = transformers.VideoMAEConfig(
        image_size=cfg.image_size, patch_size=cfg.patch_size, num_channels=cfg.num_channels, num_frames=cfg.num_frames,
        tubelet_size=cfg.tubelet_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size, use_mean_pooling=True,
        num_labels=NL, hidden_dropout_prob=p_drop, attention_probs_dropout_prob=0.0)
    model = transformers.VideoMAEForVideoClassification(config=tc)
    sd = {k: v for k, v in params.items() if k.startswith("videomae.")}
    sd.update(heads)
    model.load_state_dict(sd)
    model.train()
    drops = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Dropout)]
    assert len(drops) == 2 * cfg.num_hidden_layers, drops          # SelfOutput.dropout and Output.dropout of every layer, nothing else
    for l, layer in enumerate(model.videomae.encoder.layer):
        layer.attention.output.dropout = _FixedDropout(masks[(l, 0)].view(B, cfg.seq_len, -1), p_drop)
        layer.output.dropout = _FixedDropout(masks[(l, 1)].view(B, cfg.seq_len, -1), p_drop)
    out = model(pixel_values=px, labels=labels)
    out.loss.backward()
    gates = dr.make_gates(cfg.num_hidden_layers, B, cfg.seq_len, cfg.hidden_size, None, lambda l, b: masks[(l, b)], p_drop)
    loss, logits, grads = dr.cls_step(cfg, params, heads, px, lambda z: F.cross_entropy(z, labels), gates)
    torch.testing.assert_close(loss, out.loss.detach(), **TOL)
    torch.testing.assert_close(logits, out.logits.detach(), **TOL)
    for k, prm in model.named_parameters():
        torch.testing.assert_close(grads[k], prm.grad, **TOL, msg=lambda s, k=k: f"{k}: {s}")
    # and the masks matter: the ungated step is another loss
    assert abs(float(dr.cls_step(cfg, params, heads, px, lambda z: F.cross_entropy(z, labels))[0]) - float(loss)) > 1e-4


def _draw_tensor(table, samples):
    return torch.tensor([pair if pair else [[0.0] * samples] * 2 for pair in table], dtype=torch.float32)


def test_drop_path_matches_the_reference_modules_fixture(bvc, golden_dir):
    fx = json.load(open(os.path.join(golden_dir, "jepa_droppath.json")))
    assert len(fx["cases"]) >= 2
    for c in fx["cases"]:
        cfg = jo.JepaConfig(**c["config"])
        B, nsets, rate = c["B"], c["nsets"], c["drop_path_rate"]
        enc_p = jo.make_params(jo.encoder_shapes(cfg), cfg, c["weight_seed"])
        pred_p = jo.make_params(jo.predictor_shapes(cfg), cfg, c["weight_seed"] + 50)
        tgt_p = jo.make_params(jo.encoder_shapes(cfg), cfg, c["weight_seed"] + 100)
        imgs, m_enc, m_pred = jo.synthetic_inputs(cfg, B, c["weight_seed"], c["n_ctx"], c["n_pred"], nsets)
        # the recorded draws through the product's own host arithmetic (what turns torch.rand into path_scale on the device)
        es = bvc.dropgate.path_scale_from_uniform(_draw_tensor(c["enc_draws"], B), bvc.dropgate.drop_path_schedule(rate, cfg.depth))
        ps = bvc.dropgate.path_scale_from_uniform(_draw_tensor(c["pred_draws"], nsets * B), bvc.dropgate.drop_path_schedule(rate, cfg.pred_depth))
        assert bool((es == 0).any()) and bool((ps == 0).any()) and bool((es[1:] != 0).any()) and bool((ps[1:] != 0).any())
        eg = dr.make_gates(cfg.depth, B, c["n_ctx"], cfg.embed_dim, es)
        pg = dr.make_gates(cfg.pred_depth, nsets * B, c["n_ctx"] + c["n_pred"], cfg.pred_dim, ps)
        loss, ge_, gp_, z, _h = dr.jepa_step(cfg, enc_p, pred_p, tgt_p, imgs, m_enc, m_pred, eg, pg)
        t = lambda v: torch.tensor(v, dtype=torch.float64)       # noqa: E731
        torch.testing.assert_close(loss.double(), t(c["loss"]), **TOL)
        torch.testing.assert_close(z.double().flatten()[:8], t(c["z"]["head"]), **TOL)
        torch.testing.assert_close(z.double().norm(), t(c["z"]["l2"]), **TOL)
        torch.testing.assert_close(z.double().mean(), t(c["z"]["mean"]), **TOL)
        for got, want in ((ge_, c["enc_grad_l2"]), (gp_, c["pred_grad_l2"])):
            assert want
            for k, n in want.items():
                torch.testing.assert_close(got[k].double().norm(), t(n), **TOL, msg=lambda s, k=k: f"{c['case']} {k}: {s}")
        # the ungated step is another loss: the fixture does pin the gates
        assert abs(float(jo.step(cfg, enc_p, pred_p, tgt_p, imgs, m_enc, m_pred)[0]) - c["loss"]) > 1e-4
