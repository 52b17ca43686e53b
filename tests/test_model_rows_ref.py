"""tests/model_rows_ref.py (references, per-row bars and factors of a model step) pinned on the CPU before any GPU test relies on it.

  * the float64 step is the fp32 oracle's step to f32 round-off; the bf16-operand oracle keeps its f32 bits, runs in float64 when
    handed float64 (the twin), and takes a decoder subset (== tests/dual_mask_ref.step with every policy switch off);
  * the twin - the same operand policy carried in float64 - is inside every bar on every case, and the factors in force are what the
    rule gives for it: twice the twin's worst ratio, rounded up to a power of two, never above the caps (4, 4, 12);
  * the bars discriminate: five mutants of the policy step, each one defect of the kind a kernel change can introduce, each still
    inside the whole-tensor bars of tests/test_gpu_videomae.py::_check_step (2e-2 / 5e-2), each over at least one row bar.

Measured here (one host; bf16 roundings may flip with the thread count, the ratios move in the second digit):
  twin, worst over the five cases: activations 1.12 (-> 4), matrix rows / columns 2.48 (rule: 8, cap: 4), vector elements 6.27
  (rule: 16, cap: 12).  Where the cap binds, the headroom over the twin is 1.6x / 1.9x instead of the rule's 2x to 4x.
  mutants at S1, worst ratio on the tensor that catches them: context_row dec1 row 431: 109 (bar 4); weight_gradient fc1.weight
  rows: 26 (4); bias_gradient fc1.bias: 15.8 (12); key_row enc layer 1 query.weight rows: 210 (4).
  mask_token SURVIVES at S1 (one of 3 x 108 decoded rows: 9.7 against 12) and is caught at S1 with two clips (14.3) and at S2 (one of
  2 x 120 rows, 64 wide: 31.5 against 12), where it is pinned: a single mask-token row is visible up to about 250 decoded rows.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import videomae_oracle as vo
from oracle import videomae_oracle_bf16 as vb
from tests import dual_mask_ref as dr
from tests import model_rows_ref as M


def _f32_roundoff(l0, g0, l1, g1):
    """Two f32-or-better executions of the same arithmetic: the bars of tests/test_oracle_bf16.py (loss 1e-6, gradients 2e-5 relative L2
    with a floor of 1e-3 of the largest gradient norm)."""
    assert abs(float(l0) - float(l1)) < 1e-6 * abs(float(l0))
    gmax = max(float(g.norm()) for g in g0.values())
    for k in g0:
        assert float((g0[k].double() - g1[k].double()).norm()) < 2e-5 * (float(g0[k].norm()) + 1e-3 * gmax), k


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("name", ["S2", "S1"])
def test_float64_step_is_the_fp32_step_to_round_off(name):
    c = M.case(name)
    ref, _ = M.references(name)
    assert ref["loss"].dtype == torch.float64 and all(g.dtype == torch.float64 for g in ref["grads"].values())
    taps = {}
    if c.dec is None:
        l32, g32 = vo.step(c.cfg, c.params, c.pixels, c.mask, taps=taps)
    else:
        l32, g32 = dr.step(c.cfg, c.params, c.pixels, c.mask, c.dec, taps=taps)
    _f32_roundoff(ref["loss"], ref["grads"], l32, g32)
    for n, t in taps.items():
        assert float((t.detach().double() - ref["taps"][n]).norm() / ref["taps"][n].norm()) < 1e-5, n


def test_rounding_keeps_the_dtype_and_the_f32_bits():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4096, generator=g) * torch.logspace(-20, 20, 4096)
    assert vb._r(x).dtype == torch.float32 and torch.equal(vb._r(x), x.to(torch.bfloat16).float())
    x64 = torch.randn(4096, generator=g, dtype=torch.float64)
    r = vb._r(x64)
    assert r.dtype == torch.float64 and torch.equal(r, r.to(torch.bfloat16).double())          # on the bf16 grid, carried in f64
    assert float((r - x64).abs().max()) <= 2.0 ** -8 * float(x64.abs().max())
    assert vb._r(x64, False) is x64
    # the whole step: float32 in, float32 out (loss, activations, gradients); float64 in, float64 out
    c = M.case("S2")
    _, pol = M.references("S2")
    tw = M.twin("S2")
    assert pol["loss"].dtype == torch.float32 and tw["loss"].dtype == torch.float64
    assert all(t.dtype == torch.float32 for t in list(pol["taps"].values()) + list(pol["grads"].values()))
    assert all(t.dtype == torch.float64 for t in list(tw["taps"].values()) + list(tw["grads"].values()))
    # the loss is what F.mse_loss gives on the f32 logits, no cast in between
    assert torch.equal(pol["loss"], F.mse_loss(pol["taps"]["logits"], pol["taps"]["labels"]))
    assert c.dec is not None and pol["taps"]["logits"].shape[1] == c.ndec


def test_decoder_subset_with_every_switch_off_is_the_dual_mask_reference():
    c = M.case("S2")
    t0, t1 = {}, {}
    l0, g0 = dr.step(c.cfg, c.params, c.pixels, c.mask, c.dec, grad_scale=8.0, taps=t0)
    l1, g1 = vb.step(c.cfg, c.params, c.pixels, c.mask, vb.F32, grad_scale=8.0, taps=t1, bool_decode_pos=c.dec)
    _f32_roundoff(l0, g0, l1, g1)
    assert set(t0) == set(t1)
    for n in t0:
        assert t0[n].shape == t1[n].shape and float((t0[n] - t1[n]).detach().norm() / t0[n].detach().norm()) < 1e-5, n
    assert torch.equal(t0["labels"], t1["labels"])
    # decode-all through the new argument is the step without it, bit for bit
    la, ga = vb.step(c.cfg, c.params, c.pixels, c.mask, vb.BUILD)
    lb, gb = vb.step(c.cfg, c.params, c.pixels, c.mask, vb.BUILD, bool_decode_pos=c.mask.clone())
    assert torch.equal(la, lb) and all(torch.equal(ga[k], gb[k]) for k in ga)


def test_case_shapes():
    want = {"S1": (3, 36, 108), "S2": (2, 52, 120), "S3": (3, 32, 256), "S3_subset": (3, 32, 200), "S4": (3, 36, 108)}
    for n in M.CASES:
        c = M.case(n)
        assert (c.pixels.shape[0], c.nvis, c.ndec) == want[n], n
        if c.dec is not None:
            assert not bool((c.dec & ~c.mask).any()) and bool((c.dec.sum(1) == c.ndec).all())
    assert M.S4.hidden_size // M.S4.num_attention_heads == 80 and M.S1.hidden_size // M.S1.num_attention_heads == 64


def test_s4_is_the_narrowest_encoder_with_heads_of_80_the_library_builds(bvc):
    """Two heads of 80 (160 wide) are refused at context creation - hidden sizes are multiples of 64 - so S4 has four (320 wide)."""
    import ctypes
    import dataclasses
    L = bvc._lib.lib()
    c = M.case("S4")

    def create(cfg):
        kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
        cc = bvc.VideoMAEConfig(**kw).to_c()
        h = ctypes.c_void_p()
        return L.bvc_videomae_create(ctypes.byref(cc), 3, c.ndec, ctypes.byref(h)), h

    rc, h = create(dataclasses.replace(M.S4, hidden_size=160, num_attention_heads=2))
    assert rc != 0 and h.value is None and b"multiples of 64" in L.bvc_last_error()
    assert M.S4.hidden_size == 320 and [w for w in range(80, 321, 80) if w % 64 == 0] == [320]


# ------------------------------------------------------------------------------------------------ the rules themselves
def test_row_rule_median_guard_and_exact_row_floor():
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(64, 32, generator=g, dtype=torch.float64)
    noise = torch.randn(64, 32, generator=g, dtype=torch.float64) * 1e-3
    pol = ref + noise
    pol[:40] = ref[:40]                                  # 40 of 64 rows reproduced exactly: the median is 0, the floor carries them
    ulp = float(M._ulp32(ref[3].abs().max()))
    got = pol.clone()
    assert M.judge_rows("t", got, pol, ref, 4.0).ok
    got[3, 0] += 3.9 * ulp
    assert M.judge_rows("t", got, pol, ref, 4.0).ok
    got[3, 0] += 0.2 * ulp
    v = M.judge_rows("t", got, pol, ref, 4.0)
    assert not v.ok and v.failed == 1 and v.where == 3
    got = ref + 3.9 * noise
    got[:40] = ref[:40]
    assert M.judge_rows("t", got, pol, ref, 4.0).ok
    got[50] = ref[50] + 4.1 * noise[50]
    v = M.judge_rows("t", got, pol, ref, 4.0)
    assert not v.ok and v.where == 50 and abs(v.worst - 4.1) < 1e-6
    # a row whose own policy error is small is judged against the median, not against itself
    pol = ref + noise
    pol[7] = ref[7] + 1e-3 * noise[7]
    med = float(torch.quantile(M.row_errors(pol, ref), 0.5))
    got = pol.clone()
    got[7] = ref[7] + noise[7] * (0.99 * med / float(noise[7].norm()))        # ~1000 x the row's own policy error, below the median
    assert M.judge_rows("t", got, pol, ref, 1.0).ok
    got[7] = ref[7] + noise[7] * (1.01 * med / float(noise[7].norm()))
    assert not M.judge_rows("t", got, pol, ref, 1.0).ok


def test_element_rule_has_no_relative_term():
    ref = torch.zeros(100, dtype=torch.float64)             # a gradient that is truly 0
    pol = torch.full((100,), 1e-6, dtype=torch.float64)
    got = -pol
    assert M.judge_elements("b", got, pol, ref, 12.0).ok
    got[17] = 1.3e-5
    v = M.judge_elements("b", got, pol, ref, 12.0)
    assert not v.ok and v.where == 17 and v.failed == 1


def test_on_against_off_rule_rows_and_vectors():
    g = torch.Generator().manual_seed(2)
    ref = {"w": torch.randn(48, 32, generator=g, dtype=torch.float64), "b": torch.randn(48, generator=g, dtype=torch.float64)}
    pol = {k: v + 1e-3 * torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in ref.items()}
    off = {k: v + 1e-3 * torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in ref.items()}
    on = {k: v + 1e-5 * torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in off.items()}
    v = M.judge_on_against_off(on, off, pol, ref, {"w"})
    assert [(x.tensor, x.axis) for x in v] == [("w", "row"), ("w", "col"), ("b", "vec")] and all(x.ok for x in v)
    on["w"][11] = off["w"][11] + 2.0 * (off["w"][11] - ref["w"][11])          # one row moved by twice its own error
    v = M.judge_on_against_off(on, off, pol, ref, {"w"})
    assert not v[0].ok and v[0].where == 11 and v[0].failed == 1 and 1.0 < v[0].worst <= 2.0 + 1e-9 and v[1].ok and v[2].ok
    # why a vector is one row and its elements are not rows: two correct executions of the policy - float32- and float64-carried -
    # as `off` and `on`.  key.bias has a true gradient of 0, so every element of every execution is summation noise: element by
    # element they differ by more than max(|off - ref|, rms(pol - ref)), as whole vectors they satisfy the rule.
    ref, pol = M.references("S3")
    tw = M.twin("S3")
    keys = [k for k in ref["grads"] if k.endswith("key.bias")]
    assert len(keys) == 3 and all(float(ref["grads"][k].norm()) < 1e-15 for k in keys)
    sub = lambda d: {k: d["grads"][k] for k in keys}      # noqa: E731
    assert all(x.ok and x.axis == "vec" for x in M.judge_on_against_off(sub(tw), sub(pol), sub(pol), sub(ref)))
    worst = 0.0
    for k in keys:
        a, b, r = tw["grads"][k].double(), pol["grads"][k].double(), ref["grads"][k]
        worst = max(worst, float(((a - b).abs() / torch.maximum((b - r).abs(), (b - r).pow(2).mean().sqrt())).max()))
    assert worst > 1.5, worst


# ------------------------------------------------------------------------------------------------ the twin and the factors
@functools.lru_cache(maxsize=None)
def _twin_verdicts(name):
    ref, pol = M.references(name)
    tw = M.twin(name)
    return (M.judge_activations(tw["taps"], pol["taps"], ref["taps"]), M.judge_gradients(tw["grads"], pol["grads"], ref["grads"]))


@pytest.mark.parametrize("name", M.CASES)
def test_twin_is_inside_every_bar(name):
    acts, grads = _twin_verdicts(name)
    ref, _ = M.references(name)
    assert [v.tensor for v in acts] == M.activation_names(M.case(name).cfg) + ["labels"]
    assert len(grads) == sum(2 if M.is_matrix(k, g) else 1 for k, g in ref["grads"].items())
    w = {**M.worst(acts, ("row",)), **{"g" + k: v for k, v in M.worst(grads).items()}}
    print(f"[rows twin {name}] worst ratio: activation rows {w['row']:.3f} (factor {M.F_ACT:g}); gradient rows {w['grow']:.3f}, columns "
          f"{w['gcol']:.3f} (factor {M.F_MAT:g}); vector elements {w['gelem']:.3f} (factor {M.F_VEC:g})")
    assert not M.failures(acts + grads), M.failures(acts + grads)[:5]
    assert not M.whole_tensor_failures(M.twin(name), ref)


def test_factors_are_what_the_rule_gives_for_the_twin_and_inside_the_caps():
    worst = {"act": 0.0, "mat": 0.0, "vec": 0.0}
    for name in M.CASES:
        acts, grads = _twin_verdicts(name)
        g = M.worst(grads)
        worst["act"] = max(worst["act"], M.worst(acts, ("row",))["row"])
        worst["mat"] = max(worst["mat"], g["row"], g["col"])
        worst["vec"] = max(worst["vec"], g["elem"])
    rule = {k: float(2.0 ** torch.tensor(2.0 * v).log2().ceil()) for k, v in worst.items()}
    print(f"[rows factors] twin worst over {len(M.CASES)} cases {worst}; rule (2 x worst, next power of two) {rule}; caps {M.CAPS}; "
          f"in force {dict(act=M.F_ACT, mat=M.F_MAT, vec=M.F_VEC)}")
    assert M.CAPS == {"act": 4.0, "mat": 4.0, "vec": 12.0}
    assert M.F_ACT <= M.CAPS["act"] and M.F_MAT <= M.CAPS["mat"] and M.F_VEC <= M.CAPS["vec"]
    assert M.F_ACT == M.factor_from(worst["act"], M.CAPS["act"])
    assert M.F_MAT == M.factor_from(worst["mat"], M.CAPS["mat"])
    assert M.F_VEC == M.factor_from(worst["vec"], M.CAPS["vec"])


# ------------------------------------------------------------------------------------------------ the bars discriminate
# mutant -> (case, the tensor and axis that must catch it)
_MUTANT_CASE = {"context_row": ("S1", "dec1", "row"),
                "weight_gradient": ("S1", "decoder.decoder_layers.0.intermediate.dense.weight", "row"),
                "bias_gradient": ("S1", "decoder.decoder_layers.0.intermediate.dense.bias", "elem"),
                # (weights drawn at 0.02 make the softmax nearly uniform: the wrong keys move enc1's rows by less than the policy's own
                # error; the query-weight gradient reads the keys directly and shows them 50 times over the bar)
                "key_row": ("S1", "videomae.encoder.layer.1.attention.attention.query.weight", "row"),
                "mask_token": ("S2", "mask_token", "elem")}


@pytest.mark.parametrize("which", M.MUTANTS)
def test_mutant_passes_the_whole_tensor_bars_and_fails_a_row_bar(which):
    name, tensor, axis = _MUTANT_CASE[which]
    c = M.case(name)
    ref, pol = M.references(name)
    got = M.mutant_step(c, which)
    assert not M.whole_tensor_failures(got, ref), M.whole_tensor_failures(got, ref)      # invisible to 2e-2 / 5e-2: the point of the row bars
    verdicts = M.judge_activations(got["taps"], pol["taps"], ref["taps"]) + M.judge_gradients(got["grads"], pol["grads"], ref["grads"])
    bad = [v for v in verdicts if not v.ok]
    hit = [v for v in bad if v.tensor == tensor and v.axis == axis]
    assert hit, (which, [v.line() for v in bad][:5])
    print(f"[rows mutant {which} at {name}] caught by {len(bad)} bars; {hit[0].line()}")
    if which == "context_row":      # the zeroed context row is the LAST token row, and only that activation row is over its bar
        assert hit[0].where == ref["taps"]["dec1"].shape[0] * ref["taps"]["dec1"].shape[1] - 1 and hit[0].failed == 1
    if which == "key_row":          # clip 1's rows only: clip 0 and clip 2 are untouched
        n = c.nvis
        e = M.row_errors(got["taps"]["enc1"].reshape(-1, c.cfg.hidden_size), pol["taps"]["enc1"].reshape(-1, c.cfg.hidden_size))
        assert float(e[:n].max()) == 0.0 and float(e[2 * n:].max()) == 0.0 and float(e[n:2 * n].min()) > 0.0


def test_mask_token_mutant_margin_at_s1_is_recorded():
    """One of 324 mask-token rows missing moves an element of the mask_token gradient by less than F_VEC x the policy error's rms: the
    mutant survives at S1 and is pinned at S2 instead (above).  This test records the margin, and that the defect sits within a factor
    of two of the bar (three times the twin's own ratio on this tensor), not far inside it."""
    ref, pol = M.references("S1")
    got = M.mutant_step(M.case("S1"), "mask_token")
    v = [v for v in M.judge_gradients(got["grads"], pol["grads"], ref["grads"]) if v.tensor == "mask_token"][0]
    print(f"[rows mutant mask_token at S1] {v.line()}")
    assert v.worst > 0.5 * M.F_VEC            # close to the bar: 2.5x the twin's own ratio on this tensor, not far inside
