"""Per-row float64 bars for the FINE-TUNING step (VideoMAEForVideoClassification in train mode)  --  TEST INFRASTRUCTURE ONLY, CPU only.

The rule, the judges and the caps are those of tests/model_rows_ref.py ("How a model step is judged"); this file supplies the
three executions of one classification step they need, each {"loss", "taps", "grads"} as model_rows_ref._result gives it:

  ref    float64_step: tests/dropout_ref.cls_step's arithmetic (its videomae_layer, conv3d patch embedding, mean pool, fc_norm, linear
         classifier) on .double() parameters, pixels and gates, keeping its taps
  pol    policy_step: the same step under the build's operand policy (oracle/videomae_oracle_bf16.BUILD) in float32
  twin   policy_step(dtype=torch.float64): the same operand roundings, everything else carried in float64

Taps: "hs0" (the embedding output), "hs1" .. "hs<L>" (every layer's output - the L + 1 tensors output_hidden_states returns), "pooled"
(after fc_norm) and "logits".  Gradients: every encoder parameter, fc_norm and the classifier.

Gates and mixes are INPUTS, identical in all three executions: `gates` is what dropout_ref.make_gates builds ([(g1, g2)] per layer, f32),
`mix` is (partner, lam, box) per clip - the clip that enters the patch embedding is tests/mixup_ref.mix_clips of the normalised f32
clip, the targets are mixup_ref.soft_targets and the loss is the package's soft_target_cross_entropy.

The policy of the classification step, as read from the code (every place is repeated where policy_step states it):

  * the patch gather rounds the (mixed) f32 pixel to bf16 once: gather_patches_kernel / gather_patches_mix_kernel (rowops.hip) blend in
    f32 and pack to bf16 - the `acts` rounding of the first product's operand;
  * a gated branch is C = resid + g .* (A B^T + bias) with the gate applied to the f32 accumulator plus bias, in f32, before the f32
    residual is added: EPI_RESID_GATE in gemm_kernel_body.inc through layer_forward (stack.hip).  No rounding follows it;
  * in the backward the f32 residual gradient passes ungated; the bf16 copy that feeds a branch is bf16(g .* dres), the gate applied in
    f32 before the one rounding: ln_bwd_gate_kernel (rowops.hip) for the attention branch and for the MLP branch of the layer below,
    fcnorm_bwd_bcast_gate_kernel for the last layer's MLP branch (layer_backward in stack.hip, bvc_videomae_cls_backward in videomae.hip);
  * the mean pool sums f32 rows and divides by N (token_mean_kernel), fc_norm is an f32 LayerNorm of the B pooled rows (launch_ln_fwd
    from bvc_videomae_cls_forward_px): nothing is rounded;
  * fc_norm's backward and the broadcast of dpooled_pre / N run in f32 (fcnorm_bwd_bcast_kernel); dres of the last layer is that f32
    row for every token, its bf16 copy (gated or not) is the dY operand of the last fc2's dX and dW products;
  * the classifier and the loss are torch f32 modules: f32 products here.
"""
import dataclasses
import functools

import torch
import torch.nn.functional as F

from oracle import videomae_oracle as vo
from oracle import videomae_oracle_bf16 as vb
from tests import dropout_ref as dr
from tests import mixup_ref as mr
from tests import model_rows_ref as M
from tools.make_videomae_cls_golden import head_params

NL = 10                      # classes
SMOOTHING = 0.1              # label smoothing of the soft targets
HIDDEN_P, DROP_PATH = 0.1, 0.5
PIXEL_MEAN, PIXEL_STD = 0.5, 0.25     # VideoMAEForVideoClassification.pixel_mean / pixel_std for uint8 clips

# twice the worst twin ratio over every case and variant, rounded up to a power of two, at most the cap (M.CAPS; tests/test_cls_rows_ref.py
# re-derives and pins them).  `pooled` and `logits` have one row per clip, one to three in all, so their median is over one to three
# numbers: the twin is inside the row rule there all the same (worst ratio 1.01 - it shares the policy's roundings), so the rule stays.
F_ACT, F_MAT, F_VEC = 4.0, 4.0, 12.0

# ------------------------------------------------------------------------------------------------ cases
_ENC = dict(decoder_hidden_size=64, decoder_num_attention_heads=2, decoder_intermediate_size=128, decoder_num_hidden_layers=1)
C1 = dataclasses.replace(M.S1, **_ENC)                                     # N = 144, 192 wide, 3 heads of 64, 2 layers
C2 = dataclasses.replace(M.S2, **_ENC)                                     # N = 196 = 128 + 68, TINY widths (128 wide, 2 heads of 64)
C3 = dataclasses.replace(C1, hidden_size=384, num_attention_heads=6, intermediate_size=1536, num_hidden_layers=1)
C4 = dataclasses.replace(M.S4, **_ENC)                                     # C1 at 320 wide with 4 heads of 80
C5 = dataclasses.replace(vo.TINY, **_ENC)                                  # N = 32

#        name   cfg  B  clip seed
_SPEC = {"C1": (C1, 3, 11), "C2": (C2, 2, 7), "C3": (C3, 3, 5), "C4": (C4, 3, 11), "C5": (C5, 1, 3)}
CASES = tuple(_SPEC)
# which cases carry which variant (the minimums: plain everywhere; gated on C1, C3, C5; mixed on C1, C2)
VARIANTS = {"plain": CASES, "gated": ("C1", "C3", "C5"), "mixed": ("C1", "C2")}
RUNS = tuple((n, v) for v, names in VARIANTS.items() for n in names)


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    cfg: vo.OracleConfig
    params: dict             # the encoder's parameters (videomae.*)
    heads: dict              # fc_norm.* and classifier.*
    pixels: torch.Tensor     # f32 [B, T, C, H, W]: the clips of the plain and gated variants
    u8: torch.Tensor         # uint8 clips of the mixed variants ...
    u8_f32: torch.Tensor     # ... and their normalised f32 form, (u8 / 255 - mean) / std as load_pixels4 (rowops.hip) computes it
    labels: torch.Tensor

    @property
    def B(self):
        return self.pixels.shape[0]

    @property
    def N(self):
        return self.cfg.seq_len


@functools.lru_cache(maxsize=None)
def case(name):
    cfg, B, seed = _SPEC[name]
    params = {k: v for k, v in vo.make_params(cfg, seed=0).items() if k.startswith("videomae.")}
    heads = dict(zip(("fc_norm.weight", "fc_norm.bias", "classifier.weight", "classifier.bias"), head_params(cfg.hidden_size, NL, 5)))
    pixels, _ = vo.synthetic_batch(cfg, B, seed, 0.9)
    g = torch.Generator().manual_seed(31 + seed)
    u8 = torch.randint(0, 256, tuple(pixels.shape), generator=g, dtype=torch.uint8)
    u8_f32 = (u8.float() / 255.0 - PIXEL_MEAN) / PIXEL_STD
    return Case(name, cfg, params, heads, pixels, u8, u8_f32, torch.arange(B) % NL)


# ------------------------------------------------------------------------------------------------ gates and mixes (inputs)
def host_scale(c):
    """An explicit drop_path_scale [depth, 2, B]: every layer holds both zeros and 1 / (1 - rate) = 2."""
    s = torch.empty(c.cfg.num_hidden_layers, 2, c.B)
    for layer in range(s.shape[0]):
        for branch in (0, 1):
            for b in range(c.B):
                zero = (layer + branch + b) % 3 == 0 if c.B >= 3 else (layer + branch + b) % 2 == 1
                s[layer, branch, b] = 0.0 if zero else 1.0 / (1.0 - DROP_PATH)
    return s


HOST_SEED, HOST_OFFSET = 1234567890123, 8


def host_mask_fn(c, seed=HOST_SEED, offset=HOST_OFFSET):
    import __graft_entry__ as ge
    dg = ge.load_package().dropgate
    return lambda layer, branch: dg.dropout_mask_host(seed, offset, layer, branch, c.B * c.N, c.cfg.hidden_size, HIDDEN_P)


def gates_from(c, scale, mask_fn):
    return dr.make_gates(c.cfg.num_hidden_layers, c.B, c.N, c.cfg.hidden_size, scale, mask_fn, HIDDEN_P if mask_fn is not None else 0.0)


@functools.lru_cache(maxsize=None)
def host_gates(name):
    """The gates of the CPU pinning: fixed host inputs (host_scale, dropout_mask_host at a fixed seed and offset)."""
    c = case(name)
    return gates_from(c, host_scale(c), host_mask_fn(c))


LAM = 0.7310586              # not a dyadic number


def host_mix(c):
    """(partner, lam, box) per clip: clip 0 a Mixup blend, clip 1 a CutMix box whose edges cut patches, a third clip left alone."""
    S = c.cfg.image_size
    box = (5, S - 21, 10, S - 27)                       # 96: (5, 75, 10, 69); 112: (5, 91, 10, 85) - no edge on a multiple of 16
    assert all(v % c.cfg.patch_size for v in box)
    partner, lam, boxes = [c.B - 1, 0], [LAM, 1.0], [(0, 0, 0, 0), box]
    for b in range(2, c.B):
        partner.append(b), lam.append(1.0), boxes.append((0, 0, 0, 0))
    return partner[:c.B], lam[:c.B], boxes[:c.B]


def target_lam(c, mix):
    """The weight of a clip's own label, as ClipMix computes it: lam x (1 - box area / image area)."""
    S = c.cfg.image_size
    return [float(l) * (1.0 - max(y1 - y0, 0) * max(x1 - x0, 0) / float(S * S)) for l, (y0, y1, x0, x1) in zip(mix[1], mix[2])]


def soft_labels(c, mix, smoothing=SMOOTHING):
    return mr.soft_targets(c.labels, mix[0], target_lam(c, mix), NL, smoothing)


def soft_target_cross_entropy(logits, target):
    import __graft_entry__ as ge
    return ge.load_package().videomae.soft_target_cross_entropy(logits, target)


def _inputs(c, mix, pixels, composed=False, smoothing=SMOOTHING):
    """(the f32 clip that enters the patch embedding, loss function of the logits); `composed`: `pixels` is the mixed clip already"""
    if mix is None:
        px = c.pixels if pixels is None else pixels
        return px, lambda z: F.cross_entropy(z, c.labels)
    px = pixels if composed else mr.mix_clips(c.u8_f32 if pixels is None else pixels, *mix)
    soft = soft_labels(c, mix, smoothing)
    return px, lambda z: soft_target_cross_entropy(z, soft.to(z.dtype))


def tap_names(cfg):
    return [f"hs{i}" for i in range(cfg.num_hidden_layers + 1)] + ["pooled", "logits"]


def _leaves(c, dtype):
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in c.params.items()}
    p.update({k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in c.heads.items()})
    return p


def _cast(gates, dtype):
    return None if gates is None else [tuple(g.to(dtype) for g in pair) for pair in gates]


def _finish(p, loss, taps):
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}
    return M._result(loss, grads, taps)


# ------------------------------------------------------------------------------------------------ ref
def float64_step(c, gates=None, mix=None, pixels=None, dtype=torch.float64, smoothing=SMOOTHING):
    """`ref`: dropout_ref.cls_step's arithmetic (videomae_encode + F.linear + the loss) with its taps kept."""
    cfg = c.cfg
    px, loss_fn = _inputs(c, mix, pixels, smoothing=smoothing)
    p, g = _leaves(c, dtype), _cast(gates, dtype)
    D, L = cfg.hidden_size, cfg.seq_len
    x = F.conv3d(px.to(dtype).permute(0, 2, 1, 3, 4), p["videomae.embeddings.patch_embeddings.projection.weight"],
                 p["videomae.embeddings.patch_embeddings.projection.bias"],
                 stride=(cfg.tubelet_size, cfg.patch_size, cfg.patch_size)).flatten(2).transpose(1, 2)
    x = x + vo.sinusoid_table(L, D)[None]
    taps = {"hs0": x}
    for i in range(cfg.num_hidden_layers):
        x = dr.videomae_layer(x, p, f"videomae.encoder.layer.{i}.", cfg.num_attention_heads, cfg.layer_norm_eps, *dr._pair(g, i))
        taps[f"hs{i + 1}"] = x
    pooled = F.layer_norm(x.mean(1), (D,), p["fc_norm.weight"], p["fc_norm.bias"], 1e-5)
    logits = F.linear(pooled, p["classifier.weight"], p["classifier.bias"])
    taps["pooled"], taps["logits"] = pooled, logits
    return _finish(p, loss_fn(logits), taps)


# ------------------------------------------------------------------------------------------------ pol / twin
def _gated_layer(x, p, prefix, heads, eps, pol, g1, g2):
    """vb._layer with the two gates.  vb.linear / vb._Attention are looked up at call time (the mutants patch them)."""
    B, N, D = x.shape
    d = D // heads
    a = prefix + "attention.attention."
    h = F.layer_norm(x, (D,), p[prefix + "layernorm_before.weight"], p[prefix + "layernorm_before.bias"], eps)

    def proj(nm):
        y = vb.linear(h, p[a + nm + ".weight"], p[a + nm + ".bias"], pol)
        return vb._Round.apply(y, pol).view(B, N, heads, d).transpose(1, 2)
    ctxv = vb._Attention.apply(proj("query"), proj("key"), proj("value"), pol).transpose(1, 2).reshape(B, N, D)
    # EPI_RESID_GATE (gemm_kernel_body.inc; launch_gemm_gate from layer_forward, stack.hip): the gate multiplies the f32 accumulator plus
    # bias, then the f32 residual is added - nothing is rounded.  Backward: autograd hands linear's backward g .* dres in f32, which it
    # rounds once to bf16 - ln_bwd_gate_kernel (rowops.hip) writes dhb = bf16(gate_apply4(dres)) next to the ungated f32 dres.
    x = x + dr._gate(vb.linear(ctxv, p[prefix + "attention.output.dense.weight"], p[prefix + "attention.output.dense.bias"], pol), g1)
    h = F.layer_norm(x, (D,), p[prefix + "layernorm_after.weight"], p[prefix + "layernorm_after.bias"], eps)
    pre = vb.linear(h, p[prefix + "intermediate.dense.weight"], p[prefix + "intermediate.dense.bias"], pol)
    act = vb._Gelu.apply(pre, pol)
    # the MLP branch: the same epilogue with the gate of branch 1.  Backward: the bf16 dY of fc2 is bf16(g2 .* dres), written by the
    # ln_bwd_gate_kernel of the layer ABOVE (g_below in layer_backward, stack.hip) or, for the last layer, by
    # fcnorm_bwd_bcast_gate_kernel (top_gate in bvc_videomae_cls_backward, videomae.hip); dX of fc2 is not rounded on its own (vb._layer)
    return x + dr._gate(vb.linear(act, p[prefix + "output.dense.weight"], p[prefix + "output.dense.bias"], pol, round_dx=False), g2)


def policy_step(c, gates=None, mix=None, pixels=None, dtype=torch.float32, pol=vb.BUILD, pool_keep=None, composed=False,
                smoothing=SMOOTHING):
    """`pol` (float32) or the twin (float64): the classification step under the operand policy `pol`.
    `pool_keep` ([B, N, 1] bool; mutants only): token rows the mean pool's backward reaches."""
    cfg = c.cfg
    px, loss_fn = _inputs(c, mix, pixels, composed, smoothing)
    p, g = _leaves(c, dtype), _cast(gates, dtype)
    B, T, C, H, W = px.shape
    D, L, ts, ps = cfg.hidden_size, cfg.seq_len, cfg.tubelet_size, cfg.patch_size
    # gather_patches_kernel / gather_patches_mix_kernel (rowops.hip): the normalised (and mixed, in f32) pixel is packed to bf16 - the
    # rounding vb.linear applies to its activation operand; k order (c, dt, dy, dx) = the Conv3d weight's own layout
    patches = mr.tokens_to_rows(px.to(dtype), T, C, H, W, ts, ps)
    w = p["videomae.embeddings.patch_embeddings.projection.weight"].reshape(D, -1)
    x = vb.linear(patches, w, p["videomae.embeddings.patch_embeddings.projection.bias"], pol)
    x = x + vo.sinusoid_table(L, D)[None]                 # f32 table added to the f32 accumulator (the POS epilogue of PatchFront::embed)
    taps = {"hs0": x}
    for i in range(cfg.num_hidden_layers):
        x = _gated_layer(x, p, f"videomae.encoder.layer.{i}.", cfg.num_attention_heads, cfg.layer_norm_eps, pol, *dr._pair(g, i))
        taps[f"hs{i + 1}"] = x
    # token_mean_kernel (rowops.hip): f32 sums of the f32 residual stream divided by N; its backward inside fcnorm_bwd_bcast_kernel:
    # dres = dpooled_pre / N in f32 for every token row, rounded once where the last fc2's backward reads it (vb.linear's backward)
    xk = x if pool_keep is None else torch.where(pool_keep, x, x.detach())
    # launch_ln_fwd on the B pooled rows (bvc_videomae_cls_forward_px, videomae.hip): an f32 LayerNorm with eps 1e-5, nothing rounded
    pooled = F.layer_norm(xk.mean(1), (D,), p["fc_norm.weight"], p["fc_norm.bias"], 1e-5)
    # the classifier (nn.Linear) and the loss are torch f32 modules on the GPU: f32 products
    logits = F.linear(pooled, p["classifier.weight"], p["classifier.bias"])
    taps["pooled"], taps["logits"] = pooled, logits
    return _finish(p, loss_fn(logits), taps)


def variant_inputs(name, variant):
    """(gates, mix) of the CPU pinning for a case and variant."""
    c = case(name)
    assert name in VARIANTS[variant], (name, variant)
    return (host_gates(name) if variant == "gated" else None), (host_mix(c) if variant == "mixed" else None)


@functools.lru_cache(maxsize=None)
def references(name, variant="plain"):
    """(ref, pol) of a case and variant with the host inputs, computed once per process; nobody writes to them."""
    gates, mix = variant_inputs(name, variant)
    return float64_step(case(name), gates, mix), policy_step(case(name), gates, mix)


@functools.lru_cache(maxsize=None)
def twin(name, variant="plain"):
    gates, mix = variant_inputs(name, variant)
    return policy_step(case(name), gates, mix, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ the judgement
def judge(got, pol, ref, scale=1.0):
    """Every bar of one execution: (activations, gradients).  Token rows of hs0 .. hs<L> and the B rows of pooled and of logits by the
    row rule (F_ACT); weight gradients over rows and columns (F_MAT), vector gradients per element (F_VEC).  `scale`: the upstream
    gradient `got` ran with (a power of two; the references are those of scale 1)."""
    acts = M.judge_activations(got["taps"], pol["taps"], ref["taps"], F_ACT, names=list(ref["taps"]))
    grads = M.judge_gradients(got["grads"], pol["grads"], ref["grads"], F_MAT, F_VEC, scale)
    return acts, grads


def worst(acts, grads):
    g = M.worst(grads)
    return {"act": M.worst(acts, ("row",))["row"], "mat": max(g["row"], g["col"]), "vec": g["elem"], "row": g["row"], "col": g["col"]}


# ------------------------------------------------------------------------------------------------ mutants of the policy step
MUTANTS = ("pool_row", "drop_path_clip", "mask_row_late", "weight_gradient", "patch_unmixed", "key_row")
MUTANT_VARIANT = {"pool_row": "plain", "drop_path_clip": "gated", "mask_row_late": "gated", "weight_gradient": "plain",
                  "patch_unmixed": "mixed", "key_row": "plain"}
_FC2 = "videomae.encoder.layer.0.output.dense.weight"
UNMIXED_TOKEN = 17           # the patch of clip 0 (the blended clip) that patch_unmixed gathers from the clip itself


def mutant_step(name, which):
    """The policy step (float32, BUILD) of a case with one defect of the kind a kernel change can introduce:

      pool_row         the backward of the mean pool leaves out the last token row of the last clip
      drop_path_clip   clip 0 takes clip 1's stochastic-depth factor in layer 1's MLP branch
      mask_row_late    the keep mask of layer 0's attention branch is read one row late in the last 8 rows
      weight_gradient  layer 0's fc2 weight gradient is formed without the last token row
      patch_unmixed    one patch of the blended clip is gathered unmixed
      key_row          head 0 of clip 1 reads clip 0's keys in layer 1
    """
    assert which in MUTANTS, which
    c = case(name)
    cfg = c.cfg
    gates, mix = variant_inputs(name, MUTANT_VARIANT[which])
    kw = {}
    real_attention, real_linear = vb._Attention, vb.linear
    calls = [0]
    box = {}

    class Attention:
        @staticmethod
        def apply(qh, kh, vh, pol):
            i = calls[0]
            calls[0] += 1
            if which == "key_row" and i == 1:
                kh = kh.clone()
                kh[1, 0] = kh[0, 0]
            return real_attention.apply(qh, kh, vh, pol)

    def linear(x, w, b, pol, round_dx=True):
        # (the fc2 weight reaches linear as the leaf itself; the leaves are made inside policy_step, so it is told by its shape and call)
        if which != "weight_gradient" or tuple(w.shape) != (cfg.hidden_size, cfg.intermediate_size) or box.setdefault("seen", w) is not w:
            return real_linear(x, w, b, pol, round_dx)
        x2 = x.reshape(-1, x.shape[-1])
        y = torch.cat([real_linear(x2[:-1], w, b, pol, round_dx), real_linear(x2[-1:], w.detach(), b, pol, round_dx)])
        return y.reshape(*x.shape[:-1], y.shape[-1])

    if which == "pool_row":
        keep = torch.ones(c.B, c.N, 1, dtype=torch.bool)
        keep[-1, -1] = False
        kw["pool_keep"] = keep
    if which == "drop_path_clip":
        scale = host_scale(c)
        assert float(scale[1, 1, 0]) != float(scale[1, 1, 1])
        scale[1, 1, 0] = scale[1, 1, 1]
        gates = gates_from(c, scale, host_mask_fn(c))
    if which == "mask_row_late":
        real_mask = host_mask_fn(c)

        def mask_fn(layer, branch):
            m = real_mask(layer, branch).clone()
            if (layer, branch) == (0, 0):
                m[-8:] = real_mask(layer, branch)[-9:-1]
            return m
        gates = gates_from(c, host_scale(c), mask_fn)
    if which == "patch_unmixed":
        mixed = mr.mix_clips(c.u8_f32, *mix)
        t, hp, wp = cfg.grid
        tp, yp, xp = UNMIXED_TOKEN // (hp * wp), (UNMIXED_TOKEN // wp) % hp, UNMIXED_TOKEN % wp
        ts, ps = cfg.tubelet_size, cfg.patch_size
        sl = (0, slice(tp * ts, (tp + 1) * ts), slice(None), slice(yp * ps, (yp + 1) * ps), slice(xp * ps, (xp + 1) * ps))
        assert not torch.equal(mixed[sl], c.u8_f32[sl])
        mixed[sl] = c.u8_f32[sl]
        kw.update(pixels=mixed, composed=True)       # the clip as gathered, with the soft targets of the real mix
    with M._patched(_Attention=Attention, linear=linear):
        return policy_step(c, gates, mix, **kw)
