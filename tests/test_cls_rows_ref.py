"""tests/cls_rows_ref.py (references, cases and mutants of the fine-tuning step's per-row bars) pinned on the CPU before any GPU test
relies on it.  The rule, the judges and the caps are tests/model_rows_ref.py's, pinned by tests/test_model_rows_ref.py.

  * the float64 step is tests/dropout_ref.cls_step to f32 round-off (run in f32: to the bit), plain, gated and mixed; the policy step with
    every Policy switch off is it too; all gates one == no gates and an identity mix == plain, bit for bit, in both steps;
  * the twin - the policy carried in float64 - is inside every bar on every case and variant with gates from fixed host inputs, and the
    factors in force are what the rule gives for it under the unchanged caps (4, 4, 12);
  * the bars discriminate: six mutants of the policy step of C1.  Four are invisible to the whole-tensor bars (2e-2 / 5e-2) and over a row
    bar; two (a clip's stochastic-depth factor, a head's keys) move a third of a three-clip batch and are seen by the whole-tensor bars
    as well - recorded, with how much further over the row bars they are.

Measured here (one host; the ratios move in the second digit with the thread count):
  twin, worst over the ten runs: token rows 1.03 (rule: 4), pooled / logits rows 1.01, matrix rows / columns 1.84 (rule: 4), vector elements
  6.25 (rule: 16, cap: 12).
  mutants at C1, worst ratio on the tensor that must catch them: pool_row layer-1 proj bias 46.6 (bar 12); mask_row_late hs1 row 431:
  17.2 (4); weight_gradient fc2.weight columns 35.7 (4); patch_unmixed hs0 row 17: 193 (4); drop_path_clip layer-1 fc2 bias 1307 (12);
  key_row layer-1 query.weight rows 309 (4).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import videomae_oracle_bf16 as vb
from tests import cls_rows_ref as C
from tests import dropout_ref as dr
from tests import mixup_ref as mr
from tests import model_rows_ref as M
from tests.test_model_rows_ref import _f32_roundoff      # the bars of the same statement about the pre-training step


def _same_bits(a, b):
    return (torch.equal(a["loss"], b["loss"]) and all(torch.equal(a["taps"][k], b["taps"][k]) for k in a["taps"])
            and all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"]))


def _cls_step(name, variant):
    """tests/dropout_ref.cls_step in fp32 on the inputs of a case and variant: (loss, logits, grads)."""
    c = C.case(name)
    gates, mix = C.variant_inputs(name, variant)
    if mix is None:
        return dr.cls_step(c.cfg, c.params, c.heads, c.pixels, lambda z: F.cross_entropy(z, c.labels), gates)
    soft = C.soft_labels(c, mix)
    return dr.cls_step(c.cfg, c.params, c.heads, mr.mix_clips(c.u8_f32, *mix), lambda z: C.soft_target_cross_entropy(z, soft), gates)


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("name,variant", [("C1", "plain"), ("C1", "gated"), ("C1", "mixed"), ("C5", "gated")])
def test_float64_step_is_cls_step_to_round_off(name, variant, bvc):
    c = C.case(name)
    ref, _ = C.references(name, variant)
    assert ref["loss"].dtype == torch.float64 and all(g.dtype == torch.float64 for g in ref["grads"].values())
    assert list(ref["taps"]) == C.tap_names(c.cfg) and set(ref["grads"]) == set(c.params) | set(c.heads)
    l32, z32, g32 = _cls_step(name, variant)
    _f32_roundoff(ref["loss"], ref["grads"], l32, g32)
    assert float((z32.double() - ref["taps"]["logits"]).norm() / ref["taps"]["logits"].norm()) < 1e-5
    # ... and the same code in f32 is cls_step to the bit: nothing but the taps was added
    gates, mix = C.variant_inputs(name, variant)
    r32 = C.float64_step(c, gates, mix, dtype=torch.float32)
    assert torch.equal(r32["loss"], l32) and torch.equal(r32["taps"]["logits"], z32) and all(torch.equal(r32["grads"][k], g32[k]) for k in g32)


@pytest.mark.parametrize("name,variant", [("C1", "plain"), ("C1", "gated"), ("C2", "mixed")])
def test_policy_step_with_every_switch_off_is_cls_step(name, variant, bvc):
    c = C.case(name)
    gates, mix = C.variant_inputs(name, variant)
    got = C.policy_step(c, gates, mix, pol=vb.F32)
    l32, z32, g32 = _cls_step(name, variant)
    _f32_roundoff(l32, g32, got["loss"], got["grads"])
    assert float((z32 - got["taps"]["logits"]).norm() / z32.norm()) < 1e-5
    ref, _ = C.references(name, variant)
    for n, t in ref["taps"].items():
        assert got["taps"][n].shape == t.shape and float((got["taps"][n].double() - t).norm() / t.norm()) < 1e-5, n


def test_dtypes_of_the_three_executions():
    ref, pol = C.references("C5")
    tw = C.twin("C5")
    assert all(t.dtype == torch.float32 for t in [pol["loss"]] + list(pol["taps"].values()) + list(pol["grads"].values()))
    assert all(t.dtype == torch.float64 for t in [tw["loss"]] + list(tw["taps"].values()) + list(tw["grads"].values()))
    assert not torch.equal(pol["taps"]["hs0"].double(), ref["taps"]["hs0"])          # the policy did round
    # the loss is what F.cross_entropy gives on the f32 logits, no cast in between
    assert torch.equal(pol["loss"], F.cross_entropy(pol["taps"]["logits"], C.case("C5").labels))


@pytest.mark.parametrize("step", [C.policy_step, C.float64_step])
def test_all_gates_one_and_the_identity_mix_are_the_plain_step_bit_for_bit(step):
    c = C.case("C1")
    plain = step(c)
    ones = dr.make_gates(c.cfg.num_hidden_layers, c.B, c.N, c.cfg.hidden_size)
    assert all(bool((g == 1).all()) for pair in ones for g in pair)
    assert _same_bits(plain, step(c, gates=ones))
    identity = (list(range(c.B)), [1.0] * c.B, [(0, 0, 0, 0)] * c.B)           # lam 1, empty box, hard targets (no smoothing)
    assert _same_bits(plain, step(c, mix=identity, pixels=c.pixels, smoothing=0.0))
    assert not _same_bits(plain, step(c, mix=C.host_mix(c), pixels=c.pixels, smoothing=0.0))


def test_cases_and_host_inputs(bvc):
    want = {"C1": (3, 144, 192, 64, 2), "C2": (2, 196, 128, 64, 2), "C3": (3, 144, 384, 64, 1), "C4": (3, 144, 320, 80, 2), "C5": (1, 32, 128, 64, 2)}
    for n in C.CASES:
        c = C.case(n)
        cfg = c.cfg
        assert (c.B, c.N, cfg.hidden_size, cfg.hidden_size // cfg.num_attention_heads, cfg.num_hidden_layers) == want[n], n
        s = C.host_scale(c)
        for layer in range(cfg.num_hidden_layers):       # every layer holds both zeros and 1 / (1 - rate)
            assert sorted(set(s[layer].flatten().tolist())) == [0.0, 2.0], (n, layer)
    assert set(C.VARIANTS["gated"]) >= {"C1", "C3", "C5"} and set(C.VARIANTS["mixed"]) >= {"C1", "C2"} and C.VARIANTS["plain"] == C.CASES
    assert C.case("C2").N == 128 + 68 and C.case("C2").N > 160 >= C.case("C1").N        # the whole-head attention backward's limit
    # the gates: make_gates of the explicit scale and the host twin of the mask at a fixed (seed, offset)
    c = C.case("C1")
    g = C.host_gates("C1")
    keep = bvc.dropgate.dropout_mask_host(C.HOST_SEED, C.HOST_OFFSET, 1, 0, c.B * c.N, 192, C.HIDDEN_P)
    assert 0.05 < 1.0 - float(keep.float().mean()) < 0.15
    assert torch.equal(g[1][0], C.host_scale(c)[1, 0].view(3, 1, 1) * keep.view(3, c.N, 192).float() / (1.0 - C.HIDDEN_P))
    # the mix: a blend whose weight is no dyadic number, a box whose edges cut patches, a clip left alone
    for n in C.VARIANTS["mixed"]:
        c = C.case(n)
        partner, lam, box = C.host_mix(c)
        assert lam[0] == C.LAM and (C.LAM * 2 ** 24) % 1 != 0 and box[0] == (0, 0, 0, 0) and partner[0] != 0
        assert lam[1] == 1.0 and partner[1] != 1 and all(v % c.cfg.patch_size for v in box[1]) and box[1][1] <= c.cfg.image_size
        if c.B > 2:
            assert (partner[2], lam[2], box[2]) == (2, 1.0, (0, 0, 0, 0))
        mixed = mr.mix_clips(c.u8_f32, partner, lam, box)
        assert not torch.equal(mixed[0], c.u8_f32[0]) and not torch.equal(mixed[1], c.u8_f32[1]) and torch.equal(mixed[2:], c.u8_f32[2:])
        soft = C.soft_labels(c, (partner, lam, box))
        assert torch.allclose(soft.sum(1), torch.ones(c.B)) and c.u8.dtype == torch.uint8


# ------------------------------------------------------------------------------------------------ the twin and the factors
@functools.lru_cache(maxsize=None)
def _twin_verdicts(name, variant):
    ref, pol = C.references(name, variant)
    return C.judge(C.twin(name, variant), pol, ref)


@pytest.mark.parametrize("name,variant", C.RUNS)
def test_twin_is_inside_every_bar(name, variant, bvc):
    acts, grads = _twin_verdicts(name, variant)
    ref, _ = C.references(name, variant)
    assert [v.tensor for v in acts] == C.tap_names(C.case(name).cfg)
    assert len(grads) == sum(2 if M.is_matrix(k, g) else 1 for k, g in ref["grads"].items())
    w = C.worst(acts, grads)
    heads = max(v.worst for v in acts if v.tensor in ("pooled", "logits"))
    print(f"[cls rows twin {name}/{variant}] worst ratio: activation rows {w['act']:.3f} (pooled / logits rows {heads:.3f}; factor {C.F_ACT:g}); "
          f"gradient rows {w['row']:.3f}, columns {w['col']:.3f} (factor {C.F_MAT:g}); vector elements {w['vec']:.3f} (factor {C.F_VEC:g})")
    assert not M.failures(acts + grads), M.failures(acts + grads)[:5]
    assert not M.whole_tensor_failures(C.twin(name, variant), ref)
    tw = C.twin(name, variant)
    assert abs(float(tw["loss"]) - float(ref["loss"])) < 1e-3 * abs(float(ref["loss"]))


def test_factors_are_what_the_rule_gives_for_the_twin_and_inside_the_caps(bvc):
    worst = {"act": 0.0, "mat": 0.0, "vec": 0.0}
    for name, variant in C.RUNS:
        w = C.worst(*_twin_verdicts(name, variant))
        worst = {k: max(v, w[k]) for k, v in worst.items()}
    rule = {k: float(2.0 ** torch.tensor(2.0 * v).log2().ceil()) for k, v in worst.items()}
    print(f"[cls rows factors] twin worst over {len(C.RUNS)} runs {worst}; rule (2 x worst, next power of two) {rule}; caps {M.CAPS}; "
          f"in force {dict(act=C.F_ACT, mat=C.F_MAT, vec=C.F_VEC)}")
    assert M.CAPS == {"act": 4.0, "mat": 4.0, "vec": 12.0}
    assert C.F_ACT == M.factor_from(worst["act"], M.CAPS["act"]) <= M.CAPS["act"]
    assert C.F_MAT == M.factor_from(worst["mat"], M.CAPS["mat"]) <= M.CAPS["mat"]
    assert C.F_VEC == M.factor_from(worst["vec"], M.CAPS["vec"]) <= M.CAPS["vec"]
    # the twin itself is under every cap: the rule fits every tensor of this step, pooled and logits (one to three rows) included
    assert all(worst[k] < M.CAPS[k] for k in worst)


# ------------------------------------------------------------------------------------------------ the bars discriminate
_L0, _L1 = "videomae.encoder.layer.0.", "videomae.encoder.layer.1."
# mutant -> (the tensor and axis that must catch it, invisible to the whole-tensor bars?)
_MUTANT = {"pool_row": (_L1 + "attention.output.dense.bias", "elem", True),
           "mask_row_late": ("hs1", "row", True),
           "weight_gradient": (_L0 + "output.dense.weight", "col", True),
           "patch_unmixed": ("hs0", "row", True),
           "drop_path_clip": (_L1 + "output.dense.bias", "elem", False),
           "key_row": (_L1 + "attention.attention.query.weight", "row", False)}


@functools.lru_cache(maxsize=None)
def _mutant(which):
    ref, pol = C.references("C1", C.MUTANT_VARIANT[which])
    got = C.mutant_step("C1", which)
    return got, [v for v in sum(C.judge(got, pol, ref), []) if not v.ok]


@pytest.mark.parametrize("which", [m for m in C.MUTANTS if _MUTANT[m][2]])
def test_mutant_passes_the_whole_tensor_bars_and_fails_a_row_bar(which, bvc):
    tensor, axis, _ = _MUTANT[which]
    c = C.case("C1")
    ref, pol = C.references("C1", C.MUTANT_VARIANT[which])
    got, bad = _mutant(which)
    assert not M.whole_tensor_failures(got, ref), M.whole_tensor_failures(got, ref)      # invisible to 2e-2 / 5e-2: the point of the row bars
    assert abs(float(got["loss"]) - float(ref["loss"])) < 1e-3 * abs(float(ref["loss"]))
    hit = [v for v in bad if v.tensor == tensor and v.axis == axis]
    assert hit, (which, [v.line() for v in bad][:5])
    print(f"[cls rows mutant {which} at C1] caught by {len(bad)} bars; {hit[0].line()}")
    last = c.B * c.N - 1
    if which == "pool_row":            # the forward is untouched: no activation bar moves
        assert all(torch.equal(got["taps"][n], pol["taps"][n]) for n in pol["taps"])
    if which == "mask_row_late":       # the last 8 token rows, and only they, are over the bar of layer 0's output
        assert hit[0].failed == 8 and hit[0].where >= last - 7
        e = M.row_errors(got["taps"]["hs1"].reshape(-1, 192), pol["taps"]["hs1"].reshape(-1, 192))
        assert float(e[:-8].max()) == 0.0 and float(e[-8:].min()) > 0.0
    if which == "weight_gradient":     # that tensor alone
        assert {v.tensor for v in bad} == {tensor}
    if which == "patch_unmixed":       # one row of the embedding output, the unmixed token of clip 0
        assert hit[0].failed == 1 and hit[0].where == C.UNMIXED_TOKEN


@pytest.mark.parametrize("which", [m for m in C.MUTANTS if not _MUTANT[m][2]])
def test_mutant_the_whole_tensor_bars_see_too_is_far_over_a_row_bar(which, bvc):
    """Two of the listed defects are not subtle at C1: with three clips, a clip that takes its neighbour's stochastic-depth factor in the
    last MLP branch (0 for 2) loses or gains a third of the batch's branch, and a head of three that reads another clip's keys moves a ninth
    of the layer's attention.  The whole-tensor bars see both (drop_path_clip: hs2 8.8e-2 against 2e-2, the layer-1 MLP gradients 0.7
    against 5e-2; key_row: query.weight / key.weight 8.8e-2 against 5e-2).  They are kept, not dropped: what is recorded is that the row
    bars see them too, and from much further away - over 25 times the bar where the whole-tensor bars are over by 1.8 to 15 times."""
    tensor, axis, _ = _MUTANT[which]
    c = C.case("C1")
    ref, pol = C.references("C1", C.MUTANT_VARIANT[which])
    got, bad = _mutant(which)
    whole = M.whole_tensor_failures(got, ref)
    assert whole
    hit = [v for v in bad if v.tensor == tensor and v.axis == axis]
    assert hit, (which, [v.line() for v in bad][:5])
    print(f"[cls rows mutant {which} at C1] whole-tensor bars over on {len(whole)} tensors, worst {max(e for _, e in whole):.3g}; "
          f"caught by {len(bad)} row bars; {hit[0].line()}")
    assert hit[0].worst > 25 * hit[0].factor
    n, D = c.N, c.cfg.hidden_size
    e = M.row_errors(got["taps"]["hs2"].reshape(-1, D), pol["taps"]["hs2"].reshape(-1, D))
    if which == "key_row":             # clip 1's rows only: clips 0 and 2 keep the policy step's bits
        assert float(e[:n].max()) == 0.0 and float(e[2 * n:].max()) == 0.0 and float(e[n:2 * n].min()) > 0.0
    if which == "drop_path_clip":      # clip 0's rows only, and every one of them over its bar
        assert float(e[n:].max()) == 0.0 and float(e[:n].min()) > 0.0
        v = [v for v in bad if v.tensor == "hs2"][0]
        assert v.failed == n and v.where < n
