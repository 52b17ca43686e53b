"""Per-row float64 bars for the JEPA train step (context encoder, predictor, targets, smooth-L1)  --  TEST INFRASTRUCTURE ONLY, CPU only.

The rule, the judges and the caps are those of tests/model_rows_ref.py ("How a model step is judged"); this file supplies the
three executions of one JEPA step they need, each {"loss", "taps", "grads"} as model_rows_ref._result gives it:

  ref    float64_step: oracle/jepa_oracle.py's arithmetic (jo.targets, jo.encoder_forward, jo.predictor_forward; with gates, the gated
         restatement of the same blocks in tests/dropout_ref.py) on .double() parameters, frames and gates
  pol    policy_step: the same step under the build's operand policy (POLICY below: oracle/videomae_oracle_bf16.BUILD with the
         attention forward stated as the kernel forms it) in float32
  twin   policy_step(dtype=torch.float64): the same operand roundings, everything else carried in float64

Taps: "h" (the target rows, set-major: sequence s = i * B + b), "zc" (the context encoder's output, one row per kept token), "z" (the
prediction rows, ordered like h) and "dz" (zc.grad: what the predictor hands the context encoder, one row per kept token).  Gradients:
every parameter of encoder and predictor in ONE dict (their names do not collide) without the frozen tables pos_embed and
predictor_pos_embed.  Every gradient judgement goes through split_qkv: the fused (3D, D) qkv gradient is judged as its three (D, D)
blocks, the bias as three vectors - the tensors the VideoMAE steps judge.  Unsplit, the median of E_pol over the 3D rows is a number of
the q / k rows (whose gradients are far smaller than v's at initialisation) and gives the v rows no floor: the twin itself is then
outside the cap (tests/test_jepa_rows_ref.py keeps the numbers).

Gates (stochastic depth only: the JEPA modules refuse hidden dropout) are INPUTS, identical in all three executions: `gates` is
(encoder gates, predictor gates), each what dropout_ref.make_gates builds from a drop_path_scale - [depth, 2, B] for the encoder,
[pred_depth, 2, nsets * B] for the predictor (one factor per SEQUENCE: take_drop(c->drop, S, T) in jepa.hip).

The policy of the JEPA step, as read from jepa.hip (each place is repeated where policy_step states it; "jo" = jo.step(pol=POLICY) states
the same place, "here" = stated by this file):

  * patch gather -> bf16 once (PatchFront::embed): the `acts` rounding of the first product's operand; pos_embed is added to the f32
    accumulator (EPI_POS).  jo (as a product over all patches, gathered afterwards: the same rows).
  * every block: LayerNorm f32 -> bf16 operand; qkv stored bf16; softmax f32 with scale 1 / sqrt(hd) of the TRUE head width (a 24-wide
    head runs zero-padded to 32 with sm_scale passed explicitly: stack.hip); probabilities, context, GELU output bf16; residual stream
    f32.  jo (_block_bf16: vb._Attention scales by q.shape[-1] ** -0.5, the unpadded width).
  * the attention forward (fwd_subtile, attention.hip): the probability operand of P V is the UNNORMALISED exp2(s c - m) rounded to
    bf16, the f32 accumulator is divided by the f32 row sum of the unrounded values, then rounded to bf16.  BUILD rounds the
    normalised p instead, which is not the same thing where many keys share a probability: with 9 keys near p = 1/9 every r(p) is
    0.2 % over, the context row with them, and through delta = rowsum(dO * O) every dS row no longer sums to ~0 - a common-mode
    error in dq that a fresh model's large mean key amplifies.  Policy.p_unnormalised states the kernel's form (the backward is
    unchanged: it recomputes the normalised P from lse, as BUILD says).  Found on the GPU: against BUILD, J6 had one q.weight row at
    4.21 and J1 rows / elements at 3.51 / 8.15; against POLICY they are 3.20 and 1.64 / 4.09.
  * a gated branch is resid + g .* (A B^T + bias) on the f32 accumulator (EPI_RESID_GATE), backward bf16(g .* dres).  here (_block).
  * the encoder's final LayerNorm writes f32 zc; the predictor rounds it ONCE to bf16 (z_bf, launch_gather_rows_bf16) as the operand of
    predictor_embed; + bias + predictor_pos_embed[idx_ctx] on the f32 accumulator (EPI_POS).  jo.
  * pred_assemble_kernel copies f32 rows: context rows of sequence s from sample s % B, tail rows mask_token + pos[idx_pred[i][b]].  jo.
  * the final LayerNorm over the tail rows (RowMap{Np, T, Nc}) writes bf16 lnf, the operand of predictor_proj (f32 out + bias).  jo.
  * backward: dout -> bf16 (dout_bf); predictor_proj dW = dout_bf^T lnf, dX -> bf16 (dln, EPI_BF16); LayerNorm backward in f32 into the
    tail rows of dres, the context rows zero.  jo (vb.linear's backward).
  * mask_token's gradient: the f32 column sum of dres over the tail rows (launch_colsum_f32).  jo (autograd's sum).
  * dxe: pred_ctx_grad_kernel sums dres over the nsets copies in f32, then rounds ONCE to bf16; dxe is the dY operand of BOTH
    predictor_embed products (dW with z_bf, and dX = dz).  jo (x.repeat's backward, then vb.linear's rounding of dy).
  * dz = dxe W_emb is written in f32 (EPI_F32) and handed to autograd; bvc_vit_backward rounds it to bf16 (dout_bf) BEFORE the final
    LayerNorm's backward.  jo rounds the same number at the same point of the chain but as predictor_embed's dX (round_dx), so its
    zc.grad is the rounded value; here the product is left in f32 (round_dx=False) and _RoundGrad rounds it at the encoder's output:
    every parameter gradient keeps jo.step's bits (pinned), and the `dz` tap is the f32 product, as on the GPU.
"""
import dataclasses
import functools

import torch
import torch.nn.functional as F

from oracle import jepa_oracle as jo
from oracle import videomae_oracle_bf16 as vb
from tests import dropout_ref as dr
from tests import model_rows_ref as M
from tests.model_rows_ref import CAPS, factor_from      # noqa: F401  (the judges, the caps and the rule are model_rows_ref's)

# twice the worst twin ratio over every case and variant, rounded up to a power of two, at most the cap (tests/test_jepa_rows_ref.py
# re-derives and pins them)
F_ACT, F_MAT, F_VEC = 4.0, 4.0, 12.0
ADMISSIBLE = 1.2             # a case whose twin is within this factor of a cap is not admissible
# the build's operand policy with the attention forward stated as attention.hip forms it (see the last entry of the table above)
POLICY = dataclasses.replace(vb.BUILD, p_unnormalised=True)
DROP_PATH = 0.5
ACT_TAPS = ("h", "zc", "z", "dz")
FROZEN = ("pos_embed", "predictor_pos_embed")

# ------------------------------------------------------------------------------------------------ cases
# all: 2 frames, tubelet 1, patch 16.  Context indices lie in frame 0, the prediction sets in frame 1 (jo.synthetic_inputs).
J1 = jo.TINY                                                                 # 128 wide, heads of 64; predictor 64 wide, heads of 32
J2 = dataclasses.replace(jo.TINY_HD24, image_size=112)                       # 512 wide, 8 heads of 64; predictor 192 wide, 8 heads of 24, 2 layers
J3 = jo.JepaConfig(image_size=112, embed_dim=384, depth=1, num_heads=12, pred_dim=384, pred_depth=1)     # the width the LayerNorm epilogues exist at
# 196 tokens per frame; predictor 128 wide so that its heads are 64 wide too and T = 190 is what keeps it off the whole-head backward
J4 = jo.JepaConfig(image_size=224, embed_dim=128, depth=1, num_heads=2, pred_dim=128, pred_depth=1)
J5 = dataclasses.replace(jo.TINY, embed_dim=192)                             # encoder heads of 96, unpadded
J6 = jo.TINY

#        name  cfg  B  seed  n_ctx  n_pred  nsets
_SPEC = {"J1": (J1, 3, 3, 12, 4, 4),
         "J2": (J2, 3, 5, 40, 12, 4),
         "J3": (J3, 3, 7, 40, 10, 4),
         "J4": (J4, 2, 9, 170, 20, 2),
         "J5": (J5, 3, 3, 12, 4, 4),
         "J6": (J6, 1, 13, 9, 1, 1)}
CASES = tuple(_SPEC)
VARIANTS = {"plain": CASES, "gated": ("J1", "J2", "J3")}
RUNS = tuple((n, v) for v, names in VARIANTS.items() for n in names)


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    cfg: jo.JepaConfig
    enc: dict                # the context encoder's parameters
    pred: dict               # the predictor's
    tgt: dict                # the target encoder's
    imgs: torch.Tensor       # f32 [B, T, C, H, W] = (u8 / 255 - 0.5) / 0.25
    u8: torch.Tensor         # the uint8 frames `imgs` was normalised from
    m_enc: list              # [idx [B, Nc]] int64
    m_pred: list             # nsets x idx [B, Np] int64

    @property
    def B(self):
        return self.imgs.shape[0]

    @property
    def Nc(self):
        return self.m_enc[0].shape[1]

    @property
    def Np(self):
        return self.m_pred[0].shape[1]

    @property
    def nsets(self):
        return len(self.m_pred)

    @property
    def S(self):
        return self.nsets * self.B


@functools.lru_cache(maxsize=None)
def case(name):
    cfg, B, seed, n_ctx, n_pred, nsets = _SPEC[name]
    enc = jo.make_params(jo.encoder_shapes(cfg), cfg, seed)
    pred = jo.make_params(jo.predictor_shapes(cfg), cfg, seed + 50)
    tgt = jo.make_params(jo.encoder_shapes(cfg), cfg, seed + 100)
    imgs, m_enc, m_pred = jo.synthetic_inputs(cfg, B, seed, n_ctx, n_pred, nsets)
    # the uint8 frames behind `imgs`: the first draw of jo.synthetic_inputs' generator
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, tuple(imgs.shape), generator=g, dtype=torch.uint8)
    assert torch.equal((u8.float() / 255.0 - 0.5) / 0.25, imgs)
    return Case(name, cfg, enc, pred, tgt, imgs, u8, m_enc, m_pred)


# ------------------------------------------------------------------------------------------------ gates (inputs)
def host_scales(c):
    """Explicit drop_path_scale tensors of the CPU pinning, ([depth, 2, B], [pred_depth, 2, nsets * B]): every layer and branch holds
    both zeros and 1 / (1 - rate) = 2 (a superset of what a run reports: the schedule gives layer 0 rate 0)."""
    out = []
    for depth, samples in ((c.cfg.depth, c.B), (c.cfg.pred_depth, c.S)):
        s = torch.empty(depth, 2, samples)
        for layer in range(depth):
            for branch in (0, 1):
                for b in range(samples):
                    s[layer, branch, b] = 0.0 if (layer + branch + b) % 3 == 0 else 1.0 / (1.0 - DROP_PATH)
        out.append(s)
    return tuple(out)


def gates_from(c, enc_scale, pred_scale):
    """(encoder gates, predictor gates) from two drop_path_scale tensors (either may be None: no gate on that module)."""
    cfg = c.cfg
    eg = None if enc_scale is None else dr.make_gates(cfg.depth, c.B, c.Nc, cfg.embed_dim, enc_scale)
    pg = None if pred_scale is None else dr.make_gates(cfg.pred_depth, c.S, c.Nc + c.Np, cfg.pred_dim, pred_scale)
    return eg, pg


@functools.lru_cache(maxsize=None)
def host_gates(name):
    c = case(name)
    return gates_from(c, *host_scales(c))


def _cast(gates, dtype):
    return None if gates is None else [tuple(g.to(dtype) for g in pair) for pair in gates]


# ------------------------------------------------------------------------------------------------ the step
def _leaves(c, dtype):
    ep = {k: v.detach().to(dtype).clone().requires_grad_(k != "pos_embed") for k, v in c.enc.items()}
    pp = {k: v.detach().to(dtype).clone().requires_grad_(k != "predictor_pos_embed") for k, v in c.pred.items()}
    tp = {k: v.detach().to(dtype) for k, v in c.tgt.items()}
    return ep, pp, tp


def _finish(ep, pp, h, zc_tap, zc_in, z, grad_scale=1.0):
    """loss, backward, the result dict.  zc_in: the tensor the predictor consumed (its .grad is dz)."""
    zc_in.retain_grad()
    loss = F.smooth_l1_loss(z, h)
    (loss * grad_scale).backward()
    grads = {}
    for p in (ep, pp):
        for k, v in p.items():
            if k in FROZEN:
                assert v.grad is None
                continue
            grads[k] = v.grad if v.grad is not None else torch.zeros_like(v)
    return M._result(loss, grads, {"h": h, "zc": zc_tap, "z": z, "dz": zc_in.grad})


def float64_step(c, gates=None, dtype=torch.float64):
    """`ref`: the fp32 oracle's own code on float64 inputs (dtype=torch.float32: jo.step / dropout_ref.jepa_step to the bit)."""
    cfg = c.cfg
    ep, pp, tp = _leaves(c, dtype)
    imgs = c.imgs.to(dtype)
    h = jo.targets(cfg, tp, imgs, c.m_enc, c.m_pred)
    if gates is None:
        zc = jo.encoder_forward(cfg, ep, imgs, c.m_enc)
        z = jo.predictor_forward(cfg, pp, zc, c.m_enc, c.m_pred)
    else:
        zc = dr.jepa_encoder_forward(cfg, ep, imgs, c.m_enc, _cast(gates[0], dtype))
        z = dr.jepa_predictor_forward(cfg, pp, zc, c.m_enc, c.m_pred, _cast(gates[1], dtype))
    return _finish(ep, pp, h, zc, zc, z)


class _RoundGrad(torch.autograd.Function):
    """identity forward, r(dy) backward: launch_gather_rows_bf16(dout, ..., c->dout_bf) at the head of bvc_vit_backward"""

    @staticmethod
    def forward(ctx, x, pol):
        ctx.pol = pol
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        return vb._r(dy, ctx.pol.grads), None


def _block(x, p, prefix, heads, eps, pol, g1=None, g2=None):
    """jo._block_bf16 with the two gates.  vb.linear / vb._Attention are looked up at call time (the mutants patch them).
    EPI_RESID_GATE (gemm_kernel_body.inc; launch_gemm_gate from layer_forward, stack.hip): the per-sequence gate multiplies the f32
    accumulator plus bias, then the f32 residual is added - nothing is rounded.  Backward: autograd hands vb.linear's backward
    g .* dres in f32, which it rounds once to bf16 (ln_bwd_gate_kernel writes bf16(gate(dres)) next to the ungated f32 dres)."""
    B, N, D = x.shape
    d = D // heads
    h = F.layer_norm(x, (D,), p[prefix + "norm1.weight"], p[prefix + "norm1.bias"], eps)
    qkv = vb._Round.apply(vb.linear(h, p[prefix + "attn.qkv.weight"], p[prefix + "attn.qkv.bias"], pol), pol)
    qkv = qkv.reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    # the softmax scale is d ** -0.5 of the true width d inside vb._Attention: a 24-wide head runs zero-padded to 32 with that scale
    y = vb._Attention.apply(qkv[0], qkv[1], qkv[2], pol).transpose(1, 2).reshape(B, N, D)
    x = x + dr._gate(vb.linear(y, p[prefix + "attn.proj.weight"], p[prefix + "attn.proj.bias"], pol), g1)
    h = F.layer_norm(x, (D,), p[prefix + "norm2.weight"], p[prefix + "norm2.bias"], eps)
    h = vb._Gelu.apply(vb.linear(h, p[prefix + "mlp.fc1.weight"], p[prefix + "mlp.fc1.bias"], pol), pol)
    return x + dr._gate(vb.linear(h, p[prefix + "mlp.fc2.weight"], p[prefix + "mlp.fc2.bias"], pol, round_dx=False), g2)


def _encoder(cfg, p, imgs, masks, pol, gates=None, wrong_patch=None):
    """jo.encoder_forward(pol=...) with gates.  wrong_patch (mutants only): (sample, kept position) whose PIXELS come from the patch of
    index + 1 while its position row is the right one."""
    B, T, C, H, W = imgs.shape
    ts, ps = cfg.tubelet_size, cfg.patch_size
    # PatchFront::embed gathers the kept patches and packs them to bf16 (vb.linear's rounding of its activation operand); k order
    # (c, dt, dy, dx) = the Conv3d weight's own layout; bias and pos_embed[idx] join the f32 accumulator (EPI_POS)
    pt = imgs.permute(0, 2, 1, 3, 4).reshape(B, C, T // ts, ts, H // ps, ps, W // ps, ps)
    pt = pt.permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, -1, C * ts * ps * ps)
    raw = vb.linear(pt, p["patch_embed.proj.weight"].reshape(cfg.embed_dim, -1), p["patch_embed.proj.bias"], pol)
    x = jo.apply_masks(raw + p["pos_embed"], masks)
    if wrong_patch is not None:
        b, t = wrong_patch
        j = int(masks[0][b, t])
        keep = torch.ones(B, x.shape[1], 1, dtype=torch.bool)
        keep[b, t] = False
        x = torch.where(keep, x, (raw[b, j + 1] + p["pos_embed"][0, j]).expand_as(x))
    for i in range(cfg.depth):
        x = _block(x, p, f"blocks.{i}.", cfg.num_heads, cfg.eps, pol, *dr._pair(gates, i))
    # launch_ln_fwd(..., out): an f32 LayerNorm, f32 rows out
    return F.layer_norm(x, (cfg.embed_dim,), p["norm.weight"], p["norm.bias"], cfg.eps)


def _predictor(cfg, p, zc, masks_x, masks, pol, gates=None, mut=None):
    """jo.predictor_forward(pol=...) with gates and the hooks of the mutants (mut: dict)."""
    mut = mut or {}
    B, nsets = len(zc), len(masks)
    # z_bf: zc rounded once to bf16 (vb.linear's rounding of x); + bias + pos[idx_ctx] on the f32 accumulator.  Backward: dy = the f32
    # sum over the nsets copies (autograd's backward of repeat), rounded ONCE (dxe) for both products; dz stays f32 (round_dx=False)
    x = vb.linear(zc, p["predictor_embed.weight"], p["predictor_embed.bias"], pol, round_dx=False)
    x = x + jo.apply_masks(p["predictor_pos_embed"].repeat(B, 1, 1), masks_x)
    n_ctx = x.shape[1]
    pos = jo.repeat_interleave_batch(jo.apply_masks(p["predictor_pos_embed"].repeat(B, 1, 1), mut.get("pos_masks", masks)), B,
                                     repeat=len(masks_x))
    tok = p["mask_token"].repeat(pos.size(0), pos.size(1), 1)
    if "token_keep" in mut:          # [S, Np, 1] bool: tail rows the mask_token gradient's column sum reaches
        tok = torch.where(mut["token_keep"], tok, tok.detach())
    pred = tok + pos
    if "ctx_source" in mut:          # sequence s reads its context rows from sample ctx_source[s] (pred_assemble_kernel: s % B)
        ctx = x[mut["ctx_source"]]
    else:
        ctx = x.repeat(nsets, 1, 1)
    if "ctx_keep" in mut:            # [S, Nc, 1] bool: copies pred_ctx_grad_kernel's sum over the sets reaches
        ctx = torch.where(mut["ctx_keep"], ctx, ctx.detach())
    x = torch.cat([ctx, pred], dim=1)
    for i in range(cfg.pred_depth):
        x = _block(x, p, f"predictor_blocks.{i}.", cfg.num_heads, cfg.eps, pol, *dr._pair(gates, i))
    # the final LayerNorm over the tail rows (RowMap{Np, T, Nc}) in f32, stored bf16 (lnf) as predictor_proj's operand; backward:
    # dout -> bf16 (dout_bf), dX -> bf16 (dln) into the f32 LayerNorm backward, context rows of dres zero
    x = F.layer_norm(x, (cfg.pred_dim,), p["predictor_norm.weight"], p["predictor_norm.bias"], cfg.eps)
    return vb.linear(x[:, n_ctx:], p["predictor_proj.weight"], p["predictor_proj.bias"], pol)


def policy_step(c, gates=None, dtype=torch.float32, pol=POLICY, mut=None):
    """`pol` (float32) or the twin (float64): the JEPA step under the operand policy `pol`.  mut: hooks of mutant_step."""
    cfg = c.cfg
    mut = mut or {}
    ep, pp, tp = _leaves(c, dtype)
    imgs = c.imgs.to(dtype)
    eg, pg = (None, None) if gates is None else (_cast(gates[0], dtype), _cast(gates[1], dtype))
    h = jo.targets(cfg, tp, imgs, c.m_enc, c.m_pred, pol)            # target encoder (ungated, no_grad), F.layer_norm, the sets' rows
    zc = _encoder(cfg, ep, imgs, c.m_enc, pol, eg, mut.get("wrong_patch"))
    zc_in = _RoundGrad.apply(zc, pol)                                  # dout_bf of bvc_vit_backward
    z = _predictor(cfg, pp, zc_in, c.m_enc, c.m_pred, pol, pg, mut)
    return _finish(ep, pp, h, zc, zc_in, z)


def variant_gates(name, variant):
    assert name in VARIANTS[variant], (name, variant)
    return host_gates(name) if variant == "gated" else None


@functools.lru_cache(maxsize=None)
def references(name, variant="plain"):
    """(ref, pol) of a case and variant with the host gates, computed once per process; nobody writes to them."""
    g = variant_gates(name, variant)
    return float64_step(case(name), g), policy_step(case(name), g)


@functools.lru_cache(maxsize=None)
def twin(name, variant="plain"):
    return policy_step(case(name), variant_gates(name, variant), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ qkv as three blocks
def split_qkv(grads):
    """`...attn.qkv.weight` (3D, D) -> `...attn.q.weight`, `.k.`, `.v.` (chunk(3, dim=0)); the bias likewise.  Order kept."""
    out = {}
    for k, g in grads.items():
        if ".attn.qkv." in k:
            for nm, part in zip("qkv", g.chunk(3, dim=0)):
                out[k.replace(".attn.qkv.", f".attn.{nm}.")] = part
        else:
            out[k] = g
    return out


def join_qkv(grads):
    """the inverse of split_qkv"""
    out = {}
    for k, g in grads.items():
        if ".attn.q." in k:
            out[k.replace(".attn.q.", ".attn.qkv.")] = torch.cat([g, grads[k.replace(".attn.q.", ".attn.k.")], grads[k.replace(".attn.q.", ".attn.v.")]])
        elif ".attn.k." not in k and ".attn.v." not in k:
            out[k] = g
    return out


# ------------------------------------------------------------------------------------------------ the judgement
def judge(got, pol, ref, scale=1.0, split=True):
    """Every bar of one execution: (activations, gradients).  Rows of h, zc, z and dz by the row rule (F_ACT); the split weight gradients
    over rows and columns (F_MAT); vectors and mask_token per element (F_VEC).  `scale`: the upstream gradient `got` ran with (a power
    of two; the references are those of scale 1): dz and the gradients are divided by it.  split=False: qkv as one tensor (the CPU test
    keeps on record why that is not done)."""
    taps = dict(got["taps"])
    taps["dz"] = taps["dz"].double() / scale
    acts = M.judge_activations(taps, pol["taps"], ref["taps"], F_ACT, names=list(ACT_TAPS))
    f = split_qkv if split else (lambda g: g)
    grads = M.judge_gradients(f(got["grads"]), f(pol["grads"]), f(ref["grads"]), F_MAT, F_VEC, scale)
    return acts, grads


def worst(acts, grads):
    g = M.worst(grads)
    return {"act": M.worst(acts, ("row",))["row"], "mat": max(g["row"], g["col"]), "vec": g["elem"], "row": g["row"], "col": g["col"]}


def whole_tensor_failures(got, ref):
    """The bars of tests/test_gpu_jepa.py on a result dict: h and z 2e-2 relative L2, every gradient tensor (unsplit) 5e-2 with a floor
    of 1e-3 of the largest gradient norm.  Returns the tensors over a bar (empty: passes)."""
    pick = lambda r: {"taps": {k: r["taps"][k] for k in ("h", "z")}, "grads": r["grads"]}      # noqa: E731
    return M.whole_tensor_failures(pick(got), pick(ref))


# ------------------------------------------------------------------------------------------------ mutants of the policy step
#          mutant          case  (the tensor, the axis that must catch it)
MUTANTS = {"pred_pos":      ("J2", ("z", "row")),
           "ctx_grad_copy": ("J2", ("dz", "row")),
           "ctx_sample":    ("J1", ("dz", "row")),
           "mask_token":    ("J1", ("mask_token", "elem")),
           "patch_gather":  ("J1", ("zc", "row")),
           "v_unpad":       ("J2", ("predictor_blocks.1.attn.v.weight", "row")),
           "key_sequence":  ("J1", ("predictor_blocks.0.attn.q.weight", "row"))}
POS_SEQ, POS_TOKEN = 5, 7          # pred_pos: sequence (set 1, sample 2) and its predicted token
CTX_SEQ, CTX_TOKEN = 7, 11         # ctx_grad_copy: the copy of (set 2, sample 1), context token 11


def mutant_step(name, which):
    """The policy step (float32, BUILD) of a case with one defect of the kind a kernel change can introduce:

      pred_pos       one predicted token takes pos[idx + 1] (pred_assemble_kernel)
      ctx_grad_copy  one context token's gradient loses one set's copy (pred_ctx_grad_kernel)
      ctx_sample     context rows of sequence s read from sample s // nsets instead of s % B (set-major / sample-major; B != nsets)
      mask_token     the mask_token gradient's column sum misses the last tail row of the last sequence
      patch_gather   the last kept token of the last sample gathered from the patch of index + 1 in the context encoder (jepa.hip's
                     index-masked gather), its position row the right one
      v_unpad        the v block of predictor layer 1's qkv weight gradient comes out as layer 0's (launch_unpad_head_grads reading the
                     scratch of the layer before)
      key_sequence   head 0 of sequence 1 reads sequence 0's keys in predictor layer 0
    """
    assert which in MUTANTS and MUTANTS[which][0] == name, (name, which)
    c = case(name)
    cfg = c.cfg
    mut = {}
    if which == "pred_pos":
        i, b = POS_SEQ // c.B, POS_SEQ % c.B
        masks = [m.clone() for m in c.m_pred]
        assert int(masks[i][b, POS_TOKEN]) + 1 < cfg.seq_len
        masks[i][b, POS_TOKEN] += 1
        mut["pos_masks"] = masks
    if which == "ctx_grad_copy":
        keep = torch.ones(c.S, c.Nc, 1, dtype=torch.bool)
        keep[CTX_SEQ, CTX_TOKEN] = False
        mut["ctx_keep"] = keep
    if which == "ctx_sample":
        assert c.B != c.nsets
        mut["ctx_source"] = torch.tensor([s // c.nsets for s in range(c.S)])
        assert mut["ctx_source"].tolist() != [s % c.B for s in range(c.S)]
    if which == "mask_token":
        keep = torch.ones(c.S, c.Np, 1, dtype=torch.bool)
        keep[-1, -1] = False
        mut["token_keep"] = keep
    if which == "patch_gather":
        assert int(c.m_enc[0][-1, -1]) + 1 < cfg.seq_len
        mut["wrong_patch"] = (c.B - 1, c.Nc - 1)
    real_attention = vb._Attention
    calls = [0]

    class Attention:
        @staticmethod
        def apply(qh, kh, vh, pol):
            i = calls[0]
            calls[0] += 1
            if which == "key_sequence" and i == 2 * cfg.depth:      # after the target encoder's and the context encoder's layers
                assert kh.shape[0] == c.S
                kh = kh.clone()
                kh[1, 0] = kh[0, 0]
            return real_attention.apply(qh, kh, vh, pol)

    with M._patched(_Attention=Attention):
        got = policy_step(c, mut=mut)
    assert calls[0] == 2 * cfg.depth + cfg.pred_depth
    if which == "v_unpad":
        assert cfg.pred_dim // cfg.num_heads == 24 and cfg.pred_depth >= 2
        D = cfg.pred_dim
        for kind in ("weight", "bias"):
            g0, g1 = (got["grads"][f"predictor_blocks.{i}.attn.qkv.{kind}"] for i in (0, 1))
            got["grads"][f"predictor_blocks.1.attn.qkv.{kind}"] = torch.cat([g1[:2 * D], g0[2 * D:]])
    return got
