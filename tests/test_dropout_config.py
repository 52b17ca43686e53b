"""Stochastic depth / hidden dropout without a GPU: the configuration surface, the rate schedule, what stays refused, and the
counter-based generator's host twin (bvc_dropout_mask_host)."""
import math

import pytest
import torch

import __graft_entry__ as ge


@pytest.fixture(scope="module")
def bvc():
    ge.build()
    return ge.load_package()


def test_config_fields_default_to_zero_and_round_trip(bvc):
    c = bvc.VideoMAEConfig()
    assert (c.hidden_dropout_prob, c.attention_probs_dropout_prob, c.drop_path_rate) == (0.0, 0.0, 0.0)
    c = bvc.VideoMAEConfig(hidden_dropout_prob=0.1, drop_path_rate=0.2, num_labels=7)
    d = bvc.VideoMAEConfig(**{k: v for k, v in c.__dict__.items() if k != "decoder_norm_eps"})
    assert (d.hidden_dropout_prob, d.attention_probs_dropout_prob, d.drop_path_rate, d.num_labels) == (0.1, 0.0, 0.2, 7)
    assert bvc.videomae_config("small", drop_path_rate=0.1).drop_path_rate == 0.1
    m = bvc.VideoMAEForVideoClassification(bvc.videomae_config("small", num_hidden_layers=3, hidden_dropout_prob=0.1, drop_path_rate=0.2))
    assert m._gate.hidden_p == pytest.approx(0.1) and m._gate.enabled and m.drop_path_scale is None and m.dropout_state is None
    assert not bvc.VideoMAEForVideoClassification(bvc.videomae_config("small", num_hidden_layers=2))._gate.enabled


@pytest.mark.parametrize("rate,depth", [(0.1, 12), (0.2, 24), (0.5, 2), (0.3, 1), (0.0, 4)])
def test_schedule_is_linspace(bvc, rate, depth):
    got = bvc.dropgate.drop_path_schedule(rate, depth)
    assert got == [x.item() for x in torch.linspace(0, rate, depth)] and got[0] == 0.0 and len(got) == depth
    if depth > 1:
        assert got[-1] == pytest.approx(rate)


def test_jepa_modules_accept_drop_path_rate(bvc):
    enc = bvc.jepa.vit_tiny(drop_path_rate=0.1)          # raised ValueError before this feature
    assert enc.drop_path_rate == 0.1 and enc._gate.rates == bvc.dropgate.drop_path_schedule(0.1, 12) and enc.drop_path_scale is None
    pred = bvc.jepa.vit_predictor(sequence_shape=enc.sequence_shape, embed_dim=enc.embed_dim, depth=3, num_heads=3, drop_path_rate=0.2)
    assert pred._gate.rates == bvc.dropgate.drop_path_schedule(0.2, 3)
    import copy
    tgt = copy.deepcopy(enc)            # pretrain_jepa.py:258: the copy keeps the rate (and follows ITS training flag)
    assert tgt.drop_path_rate == 0.1 and tgt._gate.rates == enc._gate.rates and tgt._gate is not enc._gate
    e2, p2 = bvc.jepa.get_model("cpu", model_name="vit_tiny", pred_depth=2, drop_path_rate=0.3)
    assert e2._gate.drop_path_rate == 0.3 and p2._gate.drop_path_rate == 0.3
    e3, p3 = bvc.jepa.get_model("cpu", model_name="vit_tiny", pred_depth=2)
    assert not e3._gate.enabled and not p3._gate.enabled


def test_what_stays_refused_names_its_field(bvc):
    with pytest.raises(ValueError, match="attention_probs_dropout_prob"):       # built silently before this feature
        bvc.VideoMAEConfig(attention_probs_dropout_prob=0.1)
    cfg = bvc.videomae_config("small", num_hidden_layers=1)
    cfg.attention_probs_dropout_prob = 0.1       # (set behind the constructor's back, as a loaded config object could be)
    for cls in (bvc.VideoMAEForVideoClassification, bvc.VideoMAEForPreTraining):
        with pytest.raises(ValueError, match="attention_probs_dropout_prob"):
            cls(cfg)
    for field in ("hidden_dropout_prob", "drop_path_rate"):
        with pytest.raises(ValueError, match=field):
            bvc.VideoMAEForPreTraining(bvc.videomae_config("small", num_hidden_layers=1, **{field: 0.1}))
        with pytest.raises(ValueError, match=field):
            bvc.VideoMAEConfig(**{field: 1.0})
    bvc.VideoMAEForPreTraining(bvc.videomae_config("small", num_hidden_layers=1, decoder_num_hidden_layers=1))        # all zero: as ever
    for field in ("drop_rate", "attn_drop_rate"):
        with pytest.raises(ValueError, match=field):
            bvc.jepa.vit_tiny(**{field: 0.1})
        with pytest.raises(ValueError, match=field):
            bvc.jepa.vit_predictor(sequence_shape=(2, 4, 4), embed_dim=192, depth=1, num_heads=3, **{field: 0.1})


def test_path_scale_from_uniform_is_the_reference_arithmetic(bvc):
    rates = bvc.dropgate.drop_path_schedule(0.5, 3)
    u = torch.rand(3, 2, 64, generator=torch.Generator().manual_seed(0))
    s = bvc.dropgate.path_scale_from_uniform(u, rates)
    assert torch.equal(s[0], torch.ones(2, 64))                                  # rate 0: never gated, exactly 1
    for i in (1, 2):
        keep = 1 - rates[i]
        want = (keep + u[i]).floor() / keep                                      # drop_path(): x.div(keep) * floor(keep + rand)
        assert torch.equal(s[i], want) and set(s[i].unique().tolist()) <= {0.0, float(torch.tensor(1.0) / keep)}
    assert bool((s[2] == 0).any()) and bool((s[2] != 0).any())


def test_host_mask_is_a_function_of_its_whole_key(bvc):
    f = bvc.dropgate.dropout_mask_host
    base = dict(seed=11, offset=4, layer=3, branch=1)
    a = f(rows=37, cols=13, p=0.5, **base)
    assert a.dtype == torch.uint8 and tuple(a.shape) == (37, 13) and set(a.unique().tolist()) == {0, 1}
    assert torch.equal(a, f(rows=37, cols=13, p=0.5, **base))
    for k, v in (("seed", 12), ("offset", 8), ("layer", 2), ("branch", 0), ("seed", 11 + 2 ** 32), ("offset", 4 + 2 ** 32)):
        assert not torch.equal(a, f(rows=37, cols=13, p=0.5, **{**base, k: v})), k
    # the mask of the first rows does not depend on how many rows follow; p moves a threshold over the same draws
    assert torch.equal(f(rows=10, cols=13, p=0.5, **base), a[:10])
    lo, hi = f(rows=37, cols=13, p=0.1, **base), f(rows=37, cols=13, p=0.9, **base)
    assert bool((lo >= a).all()) and bool((a >= hi).all())
    assert bool(f(rows=5, cols=7, p=0.0, **base).all())


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_host_mask_keeps_its_share(bvc, p):
    rows, cols = 1568, 384
    n = rows * cols
    for key in ((0, 0, 0, 0), (2 ** 40 + 1, 12, 11, 1)):
        kept = int(bvc.dropgate.dropout_mask_host(*key, rows, cols, p).sum())
        assert abs(kept - n * (1 - p)) <= 6 * math.sqrt(n * p * (1 - p)), (key, kept)
