"""Pins tests/introspection_ref.py on the CPU: the float64 restatement of the encoder's per-layer outputs and the bf16 rounding
models, against the committed transformers fixture (tests/golden/videomae_introspect_tiny.json), against the oracle, and - where
transformers is installed - against transformers' eager VideoMAEForVideoClassification itself."""
import json
import os

import pytest
import torch

from oracle import videomae_oracle as vo
from tests import attention_ref as R
from tests import introspection_ref as IR

CFG = vo.TINY


@pytest.fixture(scope="module")
def case():
    params = vo.make_params(CFG, seed=0)
    pixels, _ = vo.synthetic_batch(CFG, 2, 0)
    hs, att = IR.encoder_states(CFG, params, pixels)
    return params, pixels, hs, att


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return json.load(open(os.path.join(golden_dir, IR.FIXTURE)))


def _flat(v):
    return torch.tensor(v, dtype=torch.float64).flatten()


def test_fixture_is_small_numbers_only(golden_dir, fixture):
    assert os.path.getsize(os.path.join(golden_dir, IR.FIXTURE)) < 50 * 1024
    assert fixture["rows"] == list(IR.FIXTURE_ROWS) and fixture["config"] == CFG.__dict__
    L, H, N, D, B, R_ = CFG.num_hidden_layers, CFG.num_attention_heads, CFG.seq_len, CFG.hidden_size, 2, len(IR.FIXTURE_ROWS)
    assert _flat(fixture["hidden_norm"]).numel() == L + 1 and _flat(fixture["attention_norm"]).numel() == L * H
    assert _flat(fixture["hidden_rows"]).numel() == (L + 1) * B * R_ * D
    assert _flat(fixture["attention_rows"]).numel() == L * B * H * R_ * N


def test_restatement_matches_the_transformers_fixture(case, fixture):
    """Agreement measured when the fixture was made: 5.3e-6 absolute on the hidden states, 8.5e-9 on the attentions (fp32
    transformers against the float64 restatement)."""
    _, _, hs, att = case
    view = IR.fixture_view(hs, att)
    assert float((_flat(view["hidden_rows"]) - _flat(fixture["hidden_rows"])).abs().max()) < 2e-5
    assert float((_flat(view["attention_rows"]) - _flat(fixture["attention_rows"])).abs().max()) < 1e-7
    for name in ("hidden_norm", "attention_norm"):
        a, b = _flat(view[name]), _flat(fixture[name])
        assert float(((a - b).abs() / b).max()) < 1e-6, name


def test_restatement_matches_the_oracle(case):
    params, pixels, hs, att = case
    pooled, last = vo.encode(CFG, params, pixels)
    assert float((hs[-1] - last.double()).abs().max()) < 2e-5
    assert len(hs) == CFG.num_hidden_layers + 1 and len(att) == CFG.num_hidden_layers
    B, N = pixels.shape[0], CFG.seq_len
    for h in hs:
        assert h.shape == (B, N, CFG.hidden_size) and h.dtype == torch.float64
    for i, a in enumerate(att):
        assert a.shape == (B, CFG.num_attention_heads, N, N)
        assert float((a.sum(-1) - 1).abs().max()) < 1e-12
        # one layer from its own input is that layer of the whole
        assert torch.equal(IR.layer_attention(CFG, params, i, hs[i]), a)


def test_rounding_models_are_near_and_not_equal(case, fixture):
    """The bf16 models sit at bf16 distance from the reference: far above float32 round-off, far below a wrong key or head."""
    params, pixels, hs, att = case
    bh, ba = IR.encoder_states_bf16(CFG, params, pixels)
    for i, a in enumerate(att):
        one = IR.layer_attention_bf16(CFG, params, i, hs[i].float())
        e1, _ = R.row_err(one, a)
        e2, _ = R.row_err(ba[i], a)
        assert 1e-5 < e1 < 2e-3 and 1e-5 < e2 < 1e-2, (i, e1, e2)
        assert float((one.sum(-1) - 1).abs().max()) < 1e-5
    for i, h in enumerate(hs):
        e = float((bh[i].double() - h).norm() / h.norm())
        assert 1e-5 < e < 2e-2, (i, e)
    # layer 0 of the end-to-end model = the one-layer model on the end-to-end model's own embedding
    assert torch.equal(IR.layer_attention_bf16(CFG, params, 0, bh[0]), ba[0])
    # the end-to-end model against the fixture's rows, the comparison the GPU test makes
    view = IR.fixture_view(bh, ba)
    assert float((_flat(view["attention_rows"]) - _flat(fixture["attention_rows"])).abs().max()) < 1e-3


@pytest.mark.parametrize("kind", R.KINDS)
def test_probs_model_against_reference(kind):
    """The op's model (float32 exp2(s2 - lse2)) against the float64 softmax: worst row 4.6e-7 ... 1.8e-6 for gauss / shift /
    headscale and up to 9.0e-6 for sharp over the GPU test's shapes; always below 1e-5, and every row sums to 1."""
    B, H = 2, 3
    for HD, N in ((32, 33), (64, 160), (88, 97), (128, 257)):
        qkv, _ = R.inputs(kind, B, N, H, HD, seed=11 * HD + N)
        ref, mod = IR.probs_reference(qkv, B, N, H, HD), IR.probs_model(qkv, B, N, H, HD)
        assert ref.shape == mod.shape == (B, H, N, N) and ref.dtype == torch.float64 and mod.dtype == torch.float32
        e, at = R.row_err(mod, ref)
        assert 0 < e < 1e-5, (kind, HD, N, e, at)
        assert float((mod.double().sum(-1) - 1).abs().max()) < 1e-5
        # the reference is attention_ref's: its lse is the log of the same row sums
        _, lse2, *_ = R.reference(qkv, torch.zeros(B * N, H * HD), B, N, H, HD)
        q, k, _ = R._split(qkv, B, N, H, HD, torch.float64)
        s2 = (q @ k.transpose(-1, -2)) * HD ** -0.5 * IR.LOG2E
        assert float((torch.exp2(s2 - lse2.view(B, H, N, 1)) - ref).abs().max()) < 1e-12


def test_probs_reference_explicit_scale():
    B, N, H, HD = 1, 17, 2, 32
    qkv, _ = R.inputs("gauss", B, N, H, HD, seed=3)
    a = IR.probs_reference(qkv, B, N, H, HD, scale=24 ** -0.5)
    q, k, _ = R._split(qkv, B, N, H, HD, torch.float64)
    assert torch.allclose(a, torch.softmax(q @ k.transpose(-1, -2) / 24 ** 0.5, dim=-1), rtol=0, atol=1e-15)
    assert not torch.allclose(a, IR.probs_reference(qkv, B, N, H, HD), atol=1e-6)


def test_restatement_matches_transformers_directly(case):
    pytest.importorskip("transformers")
    from tools.make_introspection_golden import transformers_states
    params, pixels, hs, att = case
    ths, tatt = transformers_states(CFG, params, pixels)
    assert max(float((a.double() - b).abs().max()) for a, b in zip(ths, hs)) < 2e-5
    assert max(float((a.double() - b).abs().max()) for a, b in zip(tatt, att)) < 1e-7
