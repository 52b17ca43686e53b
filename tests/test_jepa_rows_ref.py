"""tests/jepa_rows_ref.py (references, cases and mutants of the JEPA step's per-row bars) pinned on the CPU before any GPU test relies on
it.  The rule, the judges and the caps are tests/model_rows_ref.py's, pinned by tests/test_model_rows_ref.py.

  * the float64 step is jo.step (gated: dropout_ref.jepa_step) to f32 round-off, and run in f32 it is that step to the bit; the policy
    step is jo.step(pol=POLICY) to the bit in the loss, h, z and every parameter gradient (the one place it states differently - where dz
    is rounded - moves the `dz` tap alone); with every Policy switch off it is the fp32 step; all gates one == no gates, bit for bit;
  * the twin - the policy carried in float64 - is inside every bar on every case and variant, further than 1.2 x from every cap, and the
    factors in force are what the rule gives for it under the unchanged caps (4, 4, 12);
  * judged as ONE (3D, D) tensor, the fused qkv weight gradient of the same twin is outside the cap on four of the six cases (seven of the nine runs): the reason
    the gradients are judged through split_qkv stays on record here;
  * Policy.p_unnormalised, the one place where the policy step departs from BUILD, is the attention kernel's form and is pinned;
  * the bars discriminate: seven mutants of the policy step, each over the row bar of the tensor named for it, with its verdict under
    the whole-tensor bars of tests/test_gpu_jepa.py recorded as seen or passed.

Measured here (one host; the ratios move in the second digit with the thread count):
  twin, worst over the nine runs: h / zc / z rows 1.08, dz rows 1.19 (rule: 4); split matrix rows 3.20 (J6; 3.15 J3 gated, <= 2.58
  elsewhere), columns 1.67 (rule: 8, cap: 4); vector elements 5.73 (rule: 16, cap: 12).  J6 (one sample, one set, one predicted row) is
  inside the caps with the 1.2 x margin (3.20 x 1.2 = 3.84), so it is judged by the bars like the rest.
  unsplit, worst qkv.weight row ratio of the twin: J1 2.66, J2 8.34, J3 12.49, J4 13.81, J5 3.22, J6 10.59 (cap 4); gated J1 6.75, J2 6.34,
  J3 4.31.
  mutants, worst ratio on the tensor that must catch them (bar 4; mask_token 12):
    pred_pos (J2)       z row 67: 210          whole-tensor bars: SEEN in z only (4.8e-2 against 2e-2), every gradient passes
    ctx_grad_copy (J2)  dz row 51: 55          whole-tensor bars: pass
    ctx_sample (J1)     dz row 27: 81 (all)    whole-tensor bars: SEEN (patch_embed.proj.weight 0.21, predictor_embed.weight 7.6e-2); z is not
                                               (at initialisation a prediction hardly depends on whose context it reads)
    mask_token (J1)     element 15: 37.4       whole-tensor bars: pass
    patch_gather (J1)   zc row 35: 596         whole-tensor bars: SEEN in patch_embed.proj.weight alone (0.14); h, z and the rest pass
    v_unpad (J2)        v.weight row 69: 1726  whole-tensor bars: SEEN (that layer's qkv.weight 1.47, qkv.bias 1.37)
    key_sequence (J1)   q.weight row 7: 29.2   whole-tensor bars: pass (z included: near-uniform attention at initialisation)
"""
import functools

import pytest
import torch

from oracle import jepa_oracle as jo
from oracle import videomae_oracle_bf16 as vb
from tests import dropout_ref as dr
from tests import jepa_rows_ref as J
from tests import model_rows_ref as M
from tests.test_model_rows_ref import _f32_roundoff


def _same_bits(a, b):
    return (torch.equal(a["loss"], b["loss"]) and all(torch.equal(a["taps"][k], b["taps"][k]) for k in a["taps"])
            and all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"]))


def _oracle_step(c, gates=None, pol=None):
    """jo.step (plain, either policy) or dropout_ref.jepa_step (gated, fp32): (loss, {every gradient}, z, h)."""
    args = (c.cfg, c.enc, c.pred, c.tgt, c.imgs, c.m_enc, c.m_pred)
    loss, ge, gp, z, h = jo.step(*args, pol=pol) if gates is None else dr.jepa_step(*args, gates[0], gates[1])
    return loss, {k: v for k, v in {**ge, **gp}.items() if k not in J.FROZEN}, z, h


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("name,variant", [("J1", "plain"), ("J1", "gated"), ("J2", "plain")])
def test_float64_step_is_the_oracle_step(name, variant):
    c = J.case(name)
    gates = J.variant_gates(name, variant)
    ref, _ = J.references(name, variant)
    assert ref["loss"].dtype == torch.float64 and all(g.dtype == torch.float64 for g in ref["grads"].values())
    assert list(ref["taps"]) == list(J.ACT_TAPS)
    assert set(ref["grads"]) == (set(c.enc) | set(c.pred)) - set(J.FROZEN)
    l32, g32, z32, h32 = _oracle_step(c, gates)
    _f32_roundoff(ref["loss"], ref["grads"], l32, g32)
    for k, t in (("z", z32), ("h", h32)):
        assert float((t.double() - ref["taps"][k]).norm() / ref["taps"][k].norm()) < 1e-5
    # ... and the same code in f32 is that step to the bit: nothing but the taps was added
    r32 = J.float64_step(c, gates, dtype=torch.float32)
    assert torch.equal(r32["loss"], l32) and torch.equal(r32["taps"]["z"], z32) and torch.equal(r32["taps"]["h"], h32)
    assert all(torch.equal(r32["grads"][k], g32[k]) for k in g32)


@pytest.mark.parametrize("name", ["J1", "J2"])
def test_policy_step_is_the_oracles_policy_step_bit_for_bit(name):
    """jo.step(pol=BUILD) states every place of the policy table but one: it rounds dz as predictor_embed's dX, the build (and
    policy_step) rounds the f32 dz at the head of the encoder's backward.  The same number reaches the same LayerNorm backward: loss, h,
    z and every parameter gradient keep their bits; the dz tap is the unrounded f32 product, and rounding it gives bf16 values."""
    c = J.case(name)
    _, pol = J.references(name)
    loss, grads, z, h = _oracle_step(c, pol=J.POLICY)
    assert torch.equal(pol["loss"], loss) and torch.equal(pol["taps"]["z"], z) and torch.equal(pol["taps"]["h"], h)
    assert [k for k in grads if not torch.equal(pol["grads"][k], grads[k])] == []
    dz = pol["taps"]["dz"]
    assert dz.dtype == torch.float32 and not torch.equal(dz.bfloat16().float(), dz)


def test_policy_step_with_every_switch_off_is_the_fp32_step():
    c = J.case("J1")
    for variant in ("plain", "gated"):
        gates = J.variant_gates("J1", variant)
        got = J.policy_step(c, gates, pol=vb.F32)
        l32, g32, z32, h32 = _oracle_step(c, gates)
        _f32_roundoff(l32, g32, got["loss"], got["grads"])
        assert float((z32 - got["taps"]["z"]).norm() / z32.norm()) < 1e-5 and float((h32 - got["taps"]["h"]).norm() / h32.norm()) < 1e-5


def test_dtypes_and_shapes_of_the_three_executions():
    c = J.case("J1")
    ref, pol = J.references("J1")
    tw = J.twin("J1")
    assert all(t.dtype == torch.float32 for t in [pol["loss"]] + list(pol["taps"].values()) + list(pol["grads"].values()))
    assert all(t.dtype == torch.float64 for t in [tw["loss"]] + list(tw["taps"].values()) + list(tw["grads"].values()))
    D = c.cfg.embed_dim
    assert {k: tuple(v.shape) for k, v in ref["taps"].items()} == {"h": (c.S, c.Np, D), "zc": (c.B, c.Nc, D), "z": (c.S, c.Np, D),
                                                                     "dz": (c.B, c.Nc, D)}
    assert not torch.equal(pol["taps"]["zc"].double(), ref["taps"]["zc"])          # the policy did round
    assert bool((ref["taps"]["dz"].reshape(-1, D).norm(dim=1) > 0).all())            # every context token has a gradient


@pytest.mark.parametrize("step", [J.policy_step, J.float64_step])
def test_all_gates_one_are_the_plain_step_bit_for_bit(step):
    c = J.case("J1")
    ones = J.gates_from(c, torch.ones(c.cfg.depth, 2, c.B), torch.ones(c.cfg.pred_depth, 2, c.S))
    assert _same_bits(step(c), step(c, ones))
    assert not _same_bits(step(c), step(c, J.host_gates("J1")))


def test_cases_and_host_gates():
    #        B  Nc   Np nsets  D   enc hd  Dp  pred hd  layers
    want = {"J1": (3, 12, 4, 4, 128, 64, 64, 32, (2, 1)),
            "J2": (3, 40, 12, 4, 512, 64, 192, 24, (1, 2)),
            "J3": (3, 40, 10, 4, 384, 32, 384, 32, (1, 1)),
            "J4": (2, 170, 20, 2, 128, 64, 128, 64, (1, 1)),
            "J5": (3, 12, 4, 4, 192, 96, 64, 32, (2, 1)),
            "J6": (1, 9, 1, 1, 128, 64, 64, 32, (2, 1))}
    assert set(want) == set(J.CASES)
    for n in J.CASES:
        c = J.case(n)
        cfg = c.cfg
        assert (c.B, c.Nc, c.Np, c.nsets, cfg.embed_dim, cfg.embed_dim // cfg.num_heads, cfg.pred_dim, cfg.pred_dim // cfg.num_heads,
                (cfg.depth, cfg.pred_depth)) == want[n], n
        assert (cfg.num_frames, cfg.tubelet_size, cfg.patch_size) == (2, 1, 16)
        assert c.u8.dtype == torch.uint8 and tuple(c.u8.shape) == tuple(c.imgs.shape)
        per = cfg.seq_len // 2
        assert int(c.m_enc[0].max()) < per <= int(min(m.min() for m in c.m_pred))     # context in frame 0, predictions in frame 1
    assert J.case("J1").B != J.case("J1").nsets                                      # what tells set-major from sample-major
    c4 = J.case("J4")
    assert c4.Nc > 160 and c4.Nc + c4.Np > 160 and c4.Nc % 128 and (c4.Nc + c4.Np) % 128    # above the whole-head backward's limit, ragged
    assert J.VARIANTS["plain"] == J.CASES and set(J.VARIANTS["gated"]) >= {"J1", "J2", "J3"}
    for n in J.VARIANTS["gated"]:
        c = J.case(n)
        es, ps = J.host_scales(c)
        assert tuple(es.shape) == (c.cfg.depth, 2, c.B) and tuple(ps.shape) == (c.cfg.pred_depth, 2, c.S)
        for s in (es, ps):
            for layer in range(s.shape[0]):
                for branch in (0, 1):
                    assert sorted(set(s[layer, branch].tolist())) == [0.0, 2.0], (n, layer, branch)
        eg, pg = J.host_gates(n)
        assert tuple(eg[0][0].shape) == (c.B, 1, 1) and tuple(pg[0][1].shape) == (c.S, 1, 1)      # one factor per SEQUENCE in the predictor


def test_split_qkv_round_trips():
    ref, _ = J.references("J2")
    g = ref["grads"]
    s = J.split_qkv(g)
    D, Dp = 512, 192
    assert "blocks.0.attn.qkv.weight" not in s and len(s) == len(g) + 2 * 2 * 3       # 3 blocks x (weight, bias), each one -> three
    assert tuple(s["blocks.0.attn.q.weight"].shape) == (D, D) and tuple(s["predictor_blocks.1.attn.v.bias"].shape) == (Dp,)
    assert torch.equal(s["predictor_blocks.1.attn.k.weight"], g["predictor_blocks.1.attn.qkv.weight"][Dp:2 * Dp])
    assert torch.equal(s["blocks.0.attn.v.bias"], g["blocks.0.attn.qkv.bias"][2 * D:])
    back = J.join_qkv(s)
    assert list(back) == list(g) and all(torch.equal(back[k], g[k]) for k in g)
    assert all(s[k] is g[k] for k in g if ".attn.qkv." not in k)


# ------------------------------------------------------------------------------------------------ the twin and the factors
@functools.lru_cache(maxsize=None)
def _twin_verdicts(name, variant, split=True):
    ref, pol = J.references(name, variant)
    return J.judge(J.twin(name, variant), pol, ref, split=split)


@pytest.mark.parametrize("name,variant", J.RUNS)
def test_twin_is_inside_every_bar_and_clear_of_every_cap(name, variant):
    acts, grads = _twin_verdicts(name, variant)
    ref, _ = J.references(name, variant)
    tw = J.twin(name, variant)
    assert [v.tensor for v in acts] == list(J.ACT_TAPS)
    split = J.split_qkv(ref["grads"])
    assert len(grads) == sum(2 if M.is_matrix(k, g) else 1 for k, g in split.items())
    assert not any(".attn.qkv." in v.tensor for v in grads)
    w = J.worst(acts, grads)
    print(f"[jepa rows twin {name}/{variant}] worst ratio: activation rows {w['act']:.3f} (factor {J.F_ACT:g}); gradient rows {w['row']:.3f}, "
          f"columns {w['col']:.3f} (factor {J.F_MAT:g}); vector elements {w['vec']:.3f} (factor {J.F_VEC:g})")
    assert not M.failures(acts + grads), M.failures(acts + grads)[:5]
    assert not J.whole_tensor_failures(tw, ref)
    assert abs(float(tw["loss"]) - float(ref["loss"])) < 1e-3 * abs(float(ref["loss"]))
    # admissible: no closer than 1.2 x to a cap (a case that is would have to be made larger)
    for k in ("act", "mat", "vec"):
        assert w[k] * J.ADMISSIBLE < M.CAPS[k], (name, variant, k, w[k])


def test_factors_are_what_the_rule_gives_for_the_twin_and_inside_the_caps():
    worst = {"act": 0.0, "mat": 0.0, "vec": 0.0}
    for name, variant in J.RUNS:
        w = J.worst(*_twin_verdicts(name, variant))
        worst = {k: max(v, w[k]) for k, v in worst.items()}
    rule = {k: float(2.0 ** torch.tensor(2.0 * v).log2().ceil()) for k, v in worst.items()}
    print(f"[jepa rows factors] twin worst over {len(J.RUNS)} runs {worst}; rule (2 x worst, next power of two) {rule}; caps {M.CAPS}; "
          f"in force {dict(act=J.F_ACT, mat=J.F_MAT, vec=J.F_VEC)}")
    assert M.CAPS == {"act": 4.0, "mat": 4.0, "vec": 12.0}
    assert J.F_ACT == M.factor_from(worst["act"], M.CAPS["act"]) <= M.CAPS["act"]
    assert J.F_MAT == M.factor_from(worst["mat"], M.CAPS["mat"]) <= M.CAPS["mat"]
    assert J.F_VEC == M.factor_from(worst["vec"], M.CAPS["vec"]) <= M.CAPS["vec"]
    assert all(worst[k] < M.CAPS[k] for k in worst)


def test_the_fused_qkv_gradient_cannot_be_judged_as_one_tensor():
    """Unsplit, the twin is over the row bar of a qkv.weight on at least one case - always on rows of the v block, whose gradients are far
    larger than the q / k rows that set the median - while the same twin judged as q / k / v blocks is inside every bar."""
    over = {}
    for name, variant in J.RUNS:
        _, grads = _twin_verdicts(name, variant, False)
        bad = [v for v in grads if not v.ok]
        assert all(v.tensor.endswith("attn.qkv.weight") and v.axis == "row" for v in bad), [v.line() for v in bad]
        ref, _ = J.references(name, variant)
        for v in bad:
            assert v.where >= 2 * ref["grads"][v.tensor].shape[0] // 3, v.line()          # the worst row is a v row
        if bad:
            over[(name, variant)] = max(v.worst for v in bad)
        assert not M.failures(sum(_twin_verdicts(name, variant), []))
    print(f"[jepa rows unsplit qkv] the twin's worst qkv.weight row ratio where it is over the cap of {M.CAPS['mat']:g}: "
          + ", ".join(f"{n}/{v} {r:.2f}" for (n, v), r in over.items()))
    assert ("J2", "plain") in over and len(over) >= 3


def test_attention_forward_as_the_kernel_forms_it():
    """Policy.p_unnormalised (the form of fwd_subtile in attention.hip: r(exp(s - rowmax)) V divided by the f32 row sum) against the
    normalised form r(softmax) V.  On generic scores the two agree to a bf16 rounding.  On 9 keys of equal score - a freshly initialised
    model at J6 - r(1/9) = 0.111328 is 0.195 % over for every key, so the normalised form's context is 0.2 % over in EVERY element, while
    exp(0) = 1 is exact and the kernel's form gives the mean of v to one rounding.  Off by default: today's callers keep their bits."""
    assert vb.Policy().p_unnormalised is False and vb.BUILD.p_unnormalised is False and J.POLICY.p_unnormalised is True
    assert {f: getattr(J.POLICY, f) for f in ("weights", "acts", "grads", "gelu_grad", "autocast_outputs")} == \
        {f: getattr(vb.BUILD, f) for f in ("weights", "acts", "grads", "gelu_grad", "autocast_outputs")}
    g = torch.Generator().manual_seed(0)
    r = lambda t: t.bfloat16().double()      # noqa: E731
    q, k, v = (r(torch.randn(2, 2, 9, 64, generator=g, dtype=torch.float64)) for _ in range(3))
    exact = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v
    a, b = vb._Attention.apply(q, k, v, vb.BUILD), vb._Attention.apply(q, k, v, J.POLICY)
    for o in (a, b):
        assert float((o - exact).norm() / exact.norm()) < 2.0 ** -8
    assert not torch.equal(a, b)
    zero = torch.zeros_like(q)                # equal scores: p = 1 / 9 for every key
    mean = v.mean(dim=-2, keepdim=True).expand_as(v)
    off = float(r(torch.tensor(1.0 / 9.0, dtype=torch.float64)) * 9.0 - 1.0)
    assert abs(off - 1.95e-3) < 1e-5
    a, b = vb._Attention.apply(zero, k, v, vb.BUILD), vb._Attention.apply(zero, k, v, J.POLICY)
    assert torch.equal(b, r(mean))                                             # one rounding of the exact mean
    big = mean.abs() > 0.05
    rel = ((a - mean) / mean)[big]
    assert float(rel.mean()) > 0.5 * off and float((rel > 0).float().mean()) > 0.7      # over everywhere, by about r(1/9) * 9 - 1
    # the backward is the same function of its saved tensors in both forms
    qa, qb = q.clone().requires_grad_(True), q.clone().requires_grad_(True)
    vb._Attention.apply(qa, k, v, vb.BUILD).sum().backward()
    vb._Attention.apply(qb, k, v, J.POLICY).sum().backward()
    assert float((qa.grad - qb.grad).norm() / qa.grad.norm()) < 0.1


# ------------------------------------------------------------------------------------------------ the bars discriminate
# mutant -> do the whole-tensor bars of tests/test_gpu_jepa.py see it (and on which tensors alone)?
_WHOLE = {"pred_pos": {"z"},
          "ctx_grad_copy": set(),
          "ctx_sample": None,                 # seen, on several gradient tensors
          "mask_token": set(),
          "patch_gather": {"patch_embed.proj.weight"},
          "v_unpad": {"predictor_blocks.1.attn.qkv.weight", "predictor_blocks.1.attn.qkv.bias"},
          "key_sequence": set()}


@functools.lru_cache(maxsize=None)
def _mutant(which):
    name = J.MUTANTS[which][0]
    ref, pol = J.references(name)
    got = J.mutant_step(name, which)
    return got, [v for v in sum(J.judge(got, pol, ref), []) if not v.ok]


@pytest.mark.parametrize("which", list(J.MUTANTS))
def test_mutant_fails_the_row_bar_of_its_named_tensor(which):
    name, (tensor, axis) = J.MUTANTS[which]
    c = J.case(name)
    ref, pol = J.references(name)
    got, bad = _mutant(which)
    hit = [v for v in bad if v.tensor == tensor and v.axis == axis]
    assert hit, (which, [v.line() for v in bad][:5])
    whole = J.whole_tensor_failures(got, ref)
    print(f"[jepa rows mutant {which} at {name}] whole-tensor bars: {'SEEN ' + str([(n, round(e, 4)) for n, e in whole]) if whole else 'pass'}; "
          f"caught by {len(bad)} row bars; {hit[0].line()}")
    seen = {n for n, _ in whole}
    if _WHOLE[which] is None:
        assert seen and "z" not in seen and "h" not in seen
    else:
        assert seen == _WHOLE[which], seen
    D = c.cfg.embed_dim
    same = lambda k: M.row_errors(got["taps"][k].reshape(-1, D), pol["taps"][k].reshape(-1, D)) == 0      # noqa: E731
    if which == "pred_pos":            # that row of z alone; h and zc untouched
        assert hit[0].failed == 1 and hit[0].where == J.POS_SEQ * c.Np + J.POS_TOKEN
        assert bool(same("h").all()) and bool(same("zc").all())
    if which == "ctx_grad_copy":       # the forward is untouched; one row of dz
        assert all(bool(same(k).all()) for k in ("h", "zc", "z"))
        assert hit[0].failed == 1 and hit[0].where == (J.CTX_SEQ % c.B) * c.Nc + J.CTX_TOKEN
        e = ~same("dz")
        assert int(e.sum()) == 1
    if which == "mask_token":          # the forward is untouched and that tensor alone is over a bar
        assert all(bool(same(k).all()) for k in ("h", "zc", "z")) and {v.tensor for v in bad} == {"mask_token"}
    if which == "patch_gather":        # the last sample's rows of zc (attention spreads the one wrong token over them), nobody else's
        e = ~same("zc")
        assert not bool(e[:(c.B - 1) * c.Nc].any()) and bool(e[(c.B - 1) * c.Nc:].all()) and hit[0].where == c.B * c.Nc - 1
    if which == "v_unpad":             # the forward and every other gradient keep their bits
        assert all(bool(same(k).all()) for k in J.ACT_TAPS)
        assert {v.tensor for v in bad} == {"predictor_blocks.1.attn.v.weight", "predictor_blocks.1.attn.v.bias"} and hit[0].failed == c.cfg.pred_dim
    if which == "key_sequence":        # sequence 1's rows of z move, the others keep their bits - by less than the bar: the gradients catch it
        e = ~same("z")
        assert bool(e[c.Np:2 * c.Np].all()) and not bool(e[:c.Np].any()) and not bool(e[2 * c.Np:].any())
        assert not [v for v in bad if v.tensor == "z"]
    if which == "ctx_sample":          # every sample's dz is the sum over the wrong sequences
        assert hit[0].failed > c.B * c.Nc // 2 and hit[0].worst > 10 * hit[0].factor
