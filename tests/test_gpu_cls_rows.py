"""The fine-tuning step (VideoMAEForVideoClassification in train mode) on the GPU, judged per row: every token row of every hidden
state, the rows of pooled and of the logits, every row and column of every weight gradient - encoder, fc_norm, classifier - and every
element of every vector gradient, against the float64 step, with the rule and caps of tests/model_rows_ref.py and the references, cases
and factors of tests/cls_rows_ref.py (pinned on the CPU by tests/test_cls_rows_ref.py; DESIGN.md, "How the fine-tuning step is judged"):

    E_got(r) <= F * max(E_pol(r), med)          F_ACT = 4 (token rows, pooled, logits), F_MAT = 4 (weight rows and columns)
    |got - ref| <= F_VEC * rms(pol - ref)       F_VEC = 12 (vector elements)

The references are computed on the host with exactly the gates the run reports (drop_path_scale, and dropout_state through
dropgate.dropout_mask) and the mix it was given.  The whole-tensor bars of test_gpu_videomae_cls.py / test_gpu_dropout.py stay where they
are; these sit inside them.

Cases: C1 (3 x 144 rows, heads of 64: the whole-head attention backward) on every path an option forces; C2 (N = 196: the two-kernel
backward, ragged); C3 (384 wide: LayerNorm epilogues on and off, and stepping aside for a gate); C4 (heads of 80); C5 (one clip of 32
rows).  Variants: plain, gated (stochastic depth 0.5, hidden dropout 0.1), mixed (Mixup + CutMix in the patch gather, f32 and uint8
pixels).  Then four exact properties with no tolerance: clip independence, a dropped clip is untouched, linearity in the upstream
gradient, train context == inference context.

One line per case, path and tensor goes to the parity report (tests/gpu_util.log_parity; a copy: profiles/cls_rows_parity_report.txt).
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from tests import cls_rows_ref as C   # noqa: E402
from tests import dropout_ref as dr   # noqa: E402
from tests import model_rows_ref as M   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402
from tests.test_gpu_model_rows import _Options   # noqa: E402

bvc = G.bvc
L = G.L
dg = bvc.dropgate
dev = torch.device("cuda:0")
_log = G.log_parity

#  path             options              deterministic  grad_scale
PATHS = {"selected":      ({}, False, 1.0),
         "gemm8":         ({"gemm8": 1}, False, 1.0),
         "row_ln0":       ({"row_ln": 0}, False, 1.0),
         "row_ln1":       ({"row_ln": 1}, False, 1.0),
         "deterministic": ({}, True, 1.0),
         "det_scale1024": ({}, True, 1024.0),
         "scale65536":    ({}, False, 65536.0)}


def _model(c, variant):
    kw = {k: v for k, v in c.cfg.__dict__.items() if k != "decoder_norm_eps"}
    drop = dict(hidden_dropout_prob=C.HIDDEN_P, drop_path_rate=C.DROP_PATH) if variant == "gated" else {}
    m = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(num_labels=C.NL, **kw, **drop))
    m.load_state_dict({**c.params, **c.heads})
    if variant.startswith("mixed"):
        m.config.problem_type = "soft_label_classification"
    return m.to(dev).train()


def _forward(m, c, variant, pixels=None, **kw):
    """One train-mode forward with every hidden state: (output, {tap: f32 CPU tensor}).  `pooled` is what the classifier was handed."""
    seen = []
    hook = m.classifier.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].detach()))
    try:
        if variant.startswith("mixed"):
            mix = C.host_mix(c)
            px = c.u8 if variant == "mixed_u8" else c.u8_f32
            out = m(pixel_values=px.to(dev), labels=C.soft_labels(c, mix).to(dev), output_hidden_states=True,
                    mix=bvc.ClipMix(*mix, image_size=(c.cfg.image_size,) * 2, device=dev), **kw)
        else:
            px = c.pixels if pixels is None else pixels
            out = m(pixel_values=px.to(dev), labels=c.labels[:px.shape[0]].to(dev), output_hidden_states=True, **kw)
    finally:
        hook.remove()
    torch.cuda.synchronize()
    assert len(out.hidden_states) == c.cfg.num_hidden_layers + 1 and len(seen) == 1
    taps = {f"hs{i}": h.float().cpu() for i, h in enumerate(out.hidden_states)}
    taps["pooled"], taps["logits"] = seen[0].float().cpu(), out.logits.detach().float().cpu()
    return out, taps


def _run_gates(m, c):
    """The gates the last forward used, as dropout_ref.make_gates builds them from what the model reports."""
    seed, off, p = m.dropout_state
    assert p == C.HIDDEN_P and tuple(m.drop_path_scale.shape) == (c.cfg.num_hidden_layers, 2, c.B)
    fn = lambda l, b: dg.dropout_mask(seed, off, l, b, c.B * c.N, c.cfg.hidden_size, p, dev)      # noqa: E731
    return dr.make_gates(c.cfg.num_hidden_layers, c.B, c.N, c.cfg.hidden_size, m.drop_path_scale, fn, p)


def _exercised(m, c):
    """test_gpu_dropout._seeded_step's condition.  A one-layer stack has rate 0 in its only layer (dropgate.drop_path_schedule): its
    stochastic-depth factors are exactly one and the gate is the hidden dropout alone, on any seed."""
    if all(r == 0 for r in m._gate.rates):
        assert c.cfg.num_hidden_layers == 1 and bool((m.drop_path_scale == 1).all())
        return True
    return dr.scale_exercised(m.drop_path_scale, m._gate.rates, c.B == 1)


@functools.lru_cache(maxsize=None)
def _gpu_step(name, variant, path):
    """One forward and backward of a case and variant on a path: {"loss", "taps", "grads", "gates", "seed", "scale"} on the CPU, gradients
    still multiplied by the path's grad_scale.  Computed once and shared (the exact-property tests read the runs the bar tests judged)."""
    c = C.case(name)
    opts, det, scale = PATHS[path]
    with _Options(deterministic=det, **opts):
        m = _model(c, variant)
        used = None
        for seed in range(32 if variant == "gated" else 1):
            torch.manual_seed(seed)
            out, taps = _forward(m, c, variant)
            if variant != "gated" or _exercised(m, c):
                used = seed
                break
        assert used is not None, "none of the first 32 seeds exercised the stochastic-depth gate"
        assert m._train.h is not None                 # the fine-tuning context ran
        (out.loss * scale).backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.float().cpu().clone() for k, p in m.named_parameters()}
        gates = _run_gates(m, c) if variant == "gated" else None
        ds = m.drop_path_scale.cpu().clone() if variant == "gated" else None
    return {"loss": out.loss.detach().float().cpu(), "taps": taps, "grads": grads, "gates": gates, "seed": used, "scale": ds}


@functools.lru_cache(maxsize=None)
def _references(name, variant, path):
    """(ref, pol) on the host with exactly the gates the run used (gated), or the shared ones of the case (plain, mixed)."""
    if variant != "gated":
        return C.references(name, "mixed" if variant.startswith("mixed") else "plain")
    c = C.case(name)
    gates = _gpu_step(name, variant, path)["gates"]
    return C.float64_step(c, gates), C.policy_step(c, gates)


def _judge(name, variant="plain", path="selected"):
    c = C.case(name)
    got = _gpu_step(name, variant, path)
    ref, pol = _references(name, variant, path)
    scale = PATHS[path][2]
    assert set(got["grads"]) == set(ref["grads"])
    for k, t in ref["taps"].items():
        assert tuple(got["taps"][k].shape) == tuple(t.shape), (k, tuple(got["taps"][k].shape), tuple(t.shape))
    assert all(bool(torch.isfinite(g).all()) for g in got["grads"].values())
    unscaled = {"taps": got["taps"], "grads": {k: g.double() / scale for k, g in got["grads"].items()}}      # a power of two: exact
    acts, grads = C.judge(unscaled, pol, ref)
    rel = abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    tag = f"cls rows {name}/{variant}/{path}"
    _log(f"[{tag}] {c.B} clips of {c.N} rows, seed {got['seed']}: loss hip {float(got['loss']):.7f} float64 {float(ref['loss']):.7f} "
         f"policy {float(pol['loss']):.7f} rel {rel:.2e}")
    for line in M.report_lines(acts + grads):
        _log(f"[{tag}] {line}")
    w = C.worst(acts, grads)
    _log(f"[{tag}] worst: activation rows {w['act']:.3f} (factor {C.F_ACT:g}); gradient rows {w['row']:.3f}, columns {w['col']:.3f} "
         f"(factor {C.F_MAT:g}); vector elements {w['vec']:.3f} (factor {C.F_VEC:g})")
    bad = M.failures(acts + grads)
    assert not bad, (len(bad), bad[:6])
    assert rel < 1e-3, rel
    assert not M.whole_tensor_failures(unscaled, ref)
    return got


# ------------------------------------------------------------------------------------------------ what the launcher selects
def _row_ln(c):
    cfg = c.cfg
    return L.lib().bvc_op_row_ln_selected(c.B * c.N, cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads)


def _qkv_kernel(c):
    """the instantiation the launcher runs a qkv product of this stack on, under the options in force (nothing is launched)"""
    rows, width = c.B * c.N, c.cfg.hidden_size
    a, w = torch.empty(rows, width, dtype=torch.bfloat16, device=dev), torch.empty(3 * width, width, dtype=torch.bfloat16, device=dev)
    out = torch.empty(rows, 3 * width, dtype=torch.bfloat16, device=dev)
    return G.gemm_kernel_name(G.gemm_desc(a, w, rows, 3 * width, width, G.EPI["BF16"], out), G.NT)


def _gate_kernel(c):
    """the instantiation a gated branch product (proj: rows x width x width, RESID_GATE) of this stack runs on"""
    rows, width = c.B * c.N, c.cfg.hidden_size
    a, w = torch.empty(rows, width, dtype=torch.bfloat16, device=dev), torch.empty(width, width, dtype=torch.bfloat16, device=dev)
    out = torch.empty(rows, width, device=dev)
    d = G.gemm_desc(a, w, rows, width, width, G.EPI["RESID_GATE"], out, resid=out)
    name = ctypes.create_string_buffer(160)
    L.check(L.lib().bvc_op_gemm_gate_kernel(ctypes.byref(d), -1, name, 160), "bvc_op_gemm_gate_kernel")
    return name.value.decode()


def _whole_head_backward(c):
    """Does bvc_op_attention_bwd run the whole-head kernel at this stack's (B, N, H, head width)?  Asked of the launcher by a launch on
    zeros: the whole-head kernel leaves the delta scratch untouched, the two-kernel form writes it (tests/test_gpu_attention_edges.py)."""
    B, N, H = c.B, c.N, c.cfg.num_attention_heads
    D = c.cfg.hidden_size
    bf = dict(dtype=torch.bfloat16, device=dev)
    qkv, dctx, ctx, dqkv = torch.zeros(B * N, 3 * D, **bf), torch.zeros(B * N, D, **bf), torch.zeros(B * N, D, **bf), torch.zeros(B * N, 3 * D, **bf)
    lse, delta = torch.zeros(B * H, N, device=dev), torch.full((B * H, N), -7.0, device=dev)
    L.check(L.lib().bvc_op_attention_fwd(G.ptr(qkv), G.ptr(ctx), G.ptr(lse), B, N, H, D // H, G.stream()), "attention_fwd")
    L.check(L.lib().bvc_op_attention_bwd(G.ptr(qkv), G.ptr(ctx), G.ptr(dctx), G.ptr(lse), G.ptr(delta), G.ptr(dqkv), B, N, H, D // H, G.stream()),
            "attention_bwd")
    torch.cuda.synchronize()
    return bool((delta == -7.0).all())


# ------------------------------------------------------------------------------------------------ C1 on every path
def test_c1_as_the_launcher_selects():
    c = C.case("C1")
    assert L.lib().bvc_get_option(b"gemm8") == 0 and L.lib().bvc_get_option(b"row_ln") == 0
    assert _row_ln(c) == 0 and "gemm8" not in _qkv_kernel(c)
    assert _whole_head_backward(c)                          # N = 144 <= 160, heads of 64
    _judge("C1")


def test_c1_on_gemm8():
    c = C.case("C1")
    plain = _qkv_kernel(c)
    with _Options(gemm8=1):
        forced = _qkv_kernel(c)
    _log(f"[cls rows C1/plain/gemm8] qkv product 432 x 576 x 192: {plain} -> {forced}")
    assert forced != plain and "gemm8" not in plain, (plain, forced)       # the option reaches this stack's products
    _judge("C1", path="gemm8")
    assert _qkv_kernel(c) == plain


def test_c1_deterministic_mode():
    _judge("C1", path="deterministic")


def test_c1_grad_scale_65536():
    """a GradScaler-sized upstream gradient: the references are those of scale 1 (a power of two commutes with every rounding)"""
    _judge("C1", path="scale65536")


def test_c1_gated():
    got = _judge("C1", "gated")
    s = got["scale"]
    assert bool((s[0] == 1).all()) and bool((s[1] == 0).any()) and bool((s[1] == 2).any())


@pytest.mark.parametrize("variant", ["mixed_f32", "mixed_u8"])
def test_c1_mixup_cutmix_and_a_clip_left_alone(variant):
    _judge("C1", variant)


# ------------------------------------------------------------------------------------------------ C2, C4, C5
def test_c2_ragged_above_the_whole_head_limit():
    c = C.case("C2")
    assert c.N == 196 and not _whole_head_backward(c)       # the two-kernel backward
    _judge("C2")


@pytest.mark.parametrize("variant", ["mixed_f32", "mixed_u8"])
def test_c2_mixed(variant):
    _judge("C2", variant)


def test_c4_heads_of_80_in_place():
    c = C.case("C4")
    assert c.cfg.hidden_size // c.cfg.num_attention_heads == 80 and L.lib().bvc_op_attention_width(80) == 80
    assert not _whole_head_backward(c)                      # the whole-head kernel exists for heads of 64 only
    _judge("C4")


@pytest.mark.parametrize("variant", ["plain", "gated"])
def test_c5_one_clip_fewer_rows_than_a_tile(variant):
    c = C.case("C5")
    assert (c.B, c.N) == (1, 32) and _whole_head_backward(c)
    got = _judge("C5", variant)
    if variant == "gated":
        assert bool((got["scale"][:, 1] == 0).any())       # a zero in an MLP branch of the one clip


# ------------------------------------------------------------------------------------------------ C3: the 384-wide LayerNorm epilogues
@pytest.mark.parametrize("variant", ["plain", "gated"])
@pytest.mark.parametrize("row_ln", [0, 1])
def test_c3_layernorm_passes_and_epilogues(row_ln, variant):
    c = C.case("C3")
    with _Options(row_ln=row_ln):
        assert _row_ln(c) == row_ln
        if variant == "gated":       # the branch products of a gated run: the gated kernel, which has no LayerNorm epilogue
            assert _gate_kernel(c).startswith("bvc::gemm_gate_kernel<"), _gate_kernel(c)
    _judge("C3", variant, f"row_ln{row_ln}")


def test_c3_epilogues_run_without_a_gate_and_step_aside_for_one():
    """The same seed with row_ln forced to 0 and to 1.  Plain: the two forms differ in bits somewhere (the epilogue form did run).
    Gated: every hidden state, pooled and the logits are the same bits (the epilogue form is not the one that ran: both ran the separate
    LayerNorm passes around the gated products)."""
    p0, p1 = _gpu_step("C3", "plain", "row_ln0"), _gpu_step("C3", "plain", "row_ln1")
    g0, g1 = _gpu_step("C3", "gated", "row_ln0"), _gpu_step("C3", "gated", "row_ln1")
    assert any(not torch.equal(p0["taps"][k], p1["taps"][k]) for k in p0["taps"])
    assert g0["seed"] == g1["seed"] and torch.equal(g0["scale"], g1["scale"])
    for k in g0["taps"]:
        assert torch.equal(g0["taps"][k], g1["taps"][k]), k


# ------------------------------------------------------------------------------------------------ exact properties
def _forward_only(c, variant, pixels=None, seed=0, no_grad=False):
    m = _model(c, variant)
    torch.manual_seed(seed)
    if no_grad:
        with torch.no_grad():
            _, taps = _forward(m, c, variant, pixels)
        assert m._train.h is None                     # the inference context
    else:
        _, taps = _forward(m, c, variant, pixels)
        assert m._train.h is not None
    return taps, m


def test_clip_independence_bit_for_bit():
    """Gates off, C1: clips 0 and 2 of the batch sit at positions 2 and 0 of another batch whose middle clip is new.  Every hidden-state
    row and the pooled row of a clip are the same bits in both.  The forward is first shown to be bit-stable run to run."""
    c = C.case("C1")
    a, _ = _forward_only(c, "plain")
    again, _ = _forward_only(c, "plain")
    for k in a:
        assert torch.equal(a[k], again[k]), f"forward not bit-stable run to run: {k}"
    other, _ = vo.synthetic_batch(c.cfg, 1, 977, 0.9)
    b, _ = _forward_only(c, "plain", torch.cat([c.pixels[2:3], other, c.pixels[0:1]]))
    for k in a:
        if k == "logits":
            continue
        assert not torch.equal(a[k][1], b[k][1]), k               # the middle clips do differ
        for i, j in ((0, 2), (2, 0)):
            same = (a[k][i] == b[k][j]).reshape(-1, a[k].shape[-1]).all(dim=-1)
            assert bool(same.all()), f"{k}: clip {i} differs at position {j} in rows {torch.nonzero(~same).flatten()[:8].tolist()}"


def test_a_dropped_clip_is_untouched_bit_for_bit():
    """A gated run of C1 on the first seed below 32 that holds a (layer, clip) whose two branches both have factor 0: that clip's rows of
    the layer's output are its rows of the layer's input, bit for bit."""
    c = C.case("C1")
    m = _model(c, "gated")
    for seed in range(32):
        torch.manual_seed(seed)
        _, taps = _forward(m, c, "gated")
        both = (m.drop_path_scale == 0).all(dim=1).cpu()          # [layers, clips]
        if bool(both.any()) and _exercised(m, c):
            break
    else:
        raise AssertionError("none of the first 32 seeds dropped both branches of a clip in one layer")
    pairs = torch.nonzero(both).tolist()
    for layer, clip in pairs:
        assert torch.equal(taps[f"hs{layer + 1}"][clip], taps[f"hs{layer}"][clip]), (seed, layer, clip)
    kept = torch.nonzero(~both).tolist()
    assert kept and all(not torch.equal(taps[f"hs{l + 1}"][b], taps[f"hs{l}"][b]) for l, b in kept)
    _log(f"[cls rows C1/gated/dropped clip] seed {seed}: (layer, clip) with both branches dropped {pairs}: output rows == input rows")


def test_gradients_are_linear_in_the_upstream_gradient_bit_for_bit():
    """Deterministic mode, C1: every gradient at upstream scale 1024 is 1024 x the gradient at scale 1, bit for bit."""
    one, big = _gpu_step("C1", "plain", "deterministic"), _gpu_step("C1", "plain", "det_scale1024")
    assert torch.equal(one["loss"], big["loss"]) and all(torch.equal(one["taps"][k], big["taps"][k]) for k in one["taps"])
    bad = [k for k in one["grads"] if not torch.equal(one["grads"][k] * 1024.0, big["grads"][k])]
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("variant", ["plain", "gated"])
def test_train_context_equals_inference_context_bit_for_bit(variant):
    """The same seed: the L + 1 hidden states of the fine-tuning context equal those of the inference context (the same module under
    torch.no_grad() in train mode), as do pooled and the logits."""
    c = C.case("C1")
    a, ma = _forward_only(c, variant, seed=9)
    b, mb = _forward_only(c, variant, seed=9, no_grad=True)
    if variant == "gated":
        assert torch.equal(ma.drop_path_scale, mb.drop_path_scale) and ma.dropout_state == mb.dropout_state
    for k in a:
        assert torch.equal(a[k], b[k]), k
