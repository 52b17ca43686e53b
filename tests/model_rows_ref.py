"""Per-row float64 bars for a model step (activations, logits, gradients)  --  TEST INFRASTRUCTURE ONLY, CPU only.

A model step is a composition of kernels that are each held to float64 bars on their own; this file holds the COMPOSITION to bars of
the same kind, one per token row / weight row / weight column / vector element, so that a dropped row, a row read from the wrong
source or a ragged tile left out of a weight gradient cannot hide inside a whole-tensor norm.

Three executions of the same step on the CPU ("How a model step is judged"):

  ref    the float64 step: oracle.videomae_oracle.step (tests/dual_mask_ref.step with a decoder subset) on .double() inputs
  pol    the policy step: oracle.videomae_oracle_bf16.step(pol=BUILD) in float32, the plain reference of the build's operand policy
  twin   a second implementation of that policy: the same module on .double() inputs - the same operand roundings to bf16, every
         product, LayerNorm, softmax and the loss carried out in float64

and, for a tensor T of the execution under test (`got`), with E_x(r) = || x_r - ref_r ||_2 over row r and med = median_r E_pol(r):

  activations, logits   one row = one token of one clip:   E_got(r) <= F_ACT * max(E_pol(r), med)       for every row
                        (a row the policy step reproduces exactly, E_pol(r) == 0, gets a floor of 4 ulp(f32) of its largest |ref|)
  2-D gradients         reshaped to (out, in): the same rule with F_MAT, once over the rows and once over the columns
  1-D gradients and     per element:   |got - ref| <= F_VEC * rms(pol - ref)      (no division by |ref|: key.bias, whose true gradient
  mask_token            is ~0, needs no special case)
  labels                relative L2 1e-5, as in tests/test_gpu_videomae.py::_check_step

The factors are measured, not chosen: tests/test_model_rows_ref.py runs the twin as `got` over every case below and pins each factor
to twice the worst ratio seen, rounded up to a power of two and held under its cap (F_ACT <= 4, F_MAT <= 4, F_VEC <= 12).  An
execution that needs more than a cap departs from the declared policy or is wrong; the cap is not what gives.

The helpers take plain dicts of tensors (name -> tensor), so other model steps can be judged the same way.
"""
import contextlib
import dataclasses
import functools

import numpy as np
import torch

from oracle import videomae_oracle as vo
from oracle import videomae_oracle_bf16 as vb
from tests import dual_mask_ref as dr

CAPS = {"act": 4.0, "mat": 4.0, "vec": 12.0}
# twice the worst twin ratio over CASES, rounded up to a power of two, at most the cap (test_model_rows_ref.py re-derives and pins them)
F_ACT, F_MAT, F_VEC = 4.0, 4.0, 12.0
LABELS_BAR = 1e-5


def factor_from(worst, cap):
    """Twice the worst ratio seen, rounded up to a power of two; never above the cap."""
    return min(float(2.0 ** np.ceil(np.log2(2.0 * worst))), cap)


# ------------------------------------------------------------------------------------------------ cases
# S1: 4 slots of 6 x 6 positions = 144 tokens, 27 of 36 masked per slot -> nvis 36, nmask 108.  3 clips: 108 encoder rows (below one
# 128-row tile), 432 decoder rows (144 per clip: two query blocks, inside the whole-head attention backward's limit of 160 rows).
# Encoder 192 wide with 3 heads of 64; decoder 384 wide (the width at which the LayerNorm epilogues exist) with 6 heads.
S1 = dataclasses.replace(vo.BASE, num_frames=8, tubelet_size=2, image_size=96, patch_size=16,
                         hidden_size=192, num_attention_heads=3, intermediate_size=768, num_hidden_layers=2,
                         decoder_hidden_size=384, decoder_num_attention_heads=6, decoder_intermediate_size=1536, decoder_num_hidden_layers=2)
# S2: RAGGED of tests/test_gpu_dual_mask.py with its "ragged172" subset: Ld = 52 + 120 = 172 rows per clip, above the whole-head limit
S2 = dataclasses.replace(vo.TINY, num_frames=8, tubelet_size=2, image_size=112, patch_size=16)
# S3: SMALL of tests/test_gpu_decoder_tail.py: nvis 32, ndec 256 ("small") or 200 ("small_subset") per clip
S3 = dataclasses.replace(vo.BASE, image_size=96, num_frames=16, tubelet_size=2, patch_size=16, hidden_size=384, num_attention_heads=6,
                         intermediate_size=1536, num_hidden_layers=1, decoder_num_hidden_layers=2)
# S4: S1 with encoder heads of 80, the unpadded head width of the S / L / H models.  The narrowest such encoder the library builds is
# 320 wide with 4 heads (hidden sizes are multiples of 64: 160 = 2 x 80 is refused by bvc_videomae_create, pinned in
# tests/test_model_rows_ref.py)
S4 = dataclasses.replace(S1, hidden_size=320, num_attention_heads=4)


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    cfg: vo.OracleConfig
    params: dict
    pixels: torch.Tensor
    mask: torch.Tensor
    dec: "torch.Tensor | None"      # decoder subset ([B, L] bool) or None: every masked token is decoded

    @property
    def nvis(self):
        return int((~self.mask[0]).sum())

    @property
    def ndec(self):
        return int((self.mask if self.dec is None else self.dec)[0].sum())


def _subset(cfg, mask, decode_ratio, seed):
    """The decoder subsets of tests/test_gpu_dual_mask.py / test_gpu_decoder_tail.py: the package's own generator (numpy only)."""
    import __graft_entry__ as ge
    gen = ge.load_package().DecoderSubsetGenerator(cfg.grid, decode_ratio, rng=np.random.RandomState(seed))
    return torch.from_numpy(np.stack([gen(m) for m in mask.numpy()])).bool()


#        name            cfg  B  clip seed  mask ratio  weight seed  (decode ratio, subset seed)
_SPEC = {"S1":           (S1, 3, 11, 0.75, 0, None),
         "S2":           (S2, 2, 7, 0.75, 0, (0.84, 21)),
         "S3":           (S3, 3, 5, 0.89, 0, None),
         "S3_subset":    (S3, 3, 5, 0.89, 0, (0.8, 31)),
         "S4":           (S4, 3, 11, 0.75, 0, None)}
CASES = tuple(_SPEC)


@functools.lru_cache(maxsize=None)
def case(name):
    cfg, B, seed, ratio, wseed, sub = _SPEC[name]
    params = vo.make_params(cfg, seed=wseed)
    pixels, mask = vo.synthetic_batch(cfg, B, seed, ratio)
    dec = _subset(cfg, mask, *sub) if sub is not None else None
    return Case(name, cfg, params, pixels, mask, dec)


def _result(loss, grads, taps):
    return {"loss": loss.detach(), "grads": grads, "taps": {k: v.detach() for k, v in taps.items()}}


def float64_step(c):
    """`ref`: the fp32 oracle's own code on float64 parameters and pixels."""
    p = {k: v.double() for k, v in c.params.items()}
    taps = {}
    if c.dec is None:
        loss, grads = vo.step(c.cfg, p, c.pixels.double(), c.mask, taps=taps)
    else:
        loss, grads = dr.step(c.cfg, p, c.pixels.double(), c.mask, c.dec, taps=taps)
    return _result(loss, grads, taps)


def policy_step(c, dtype=torch.float32, pol=vb.BUILD):
    """`pol` (float32) or the twin (float64): the bf16-operand oracle under the build's policy, in `dtype`."""
    p = {k: v.to(dtype) for k, v in c.params.items()}
    taps = {}
    loss, grads = vb.step(c.cfg, p, c.pixels.to(dtype), c.mask, pol, taps=taps, bool_decode_pos=c.dec)
    return _result(loss, grads, taps)


@functools.lru_cache(maxsize=None)
def references(name):
    """(ref, pol) of a case, computed once per process and shared by every test that needs them; nobody writes to them."""
    c = case(name)
    return float64_step(c), policy_step(c)


@functools.lru_cache(maxsize=None)
def twin(name):
    return policy_step(case(name), torch.float64)


# ------------------------------------------------------------------------------------------------ bars
@dataclasses.dataclass
class Verdict:
    tensor: str
    axis: str           # "row" (token rows / weight rows), "col" (weight columns), "elem" (vector elements), "vec" (a vector as one row), "rel" (labels)
    worst: float        # worst E_got / max(E_pol, med)   (elem: |got - ref| / rms(pol - ref); rel: relative L2)
    where: int          # the row / column / element it fell on
    factor: float       # the factor (bar) in force
    failed: int         # rows / columns / elements over their bar
    count: int

    @property
    def ok(self):
        return self.failed == 0

    def line(self):
        return (f"{self.tensor} [{self.axis}] worst {self.worst:.3f} at {self.where} of {self.count} (factor {self.factor:g}, "
                f"margin {self.factor / max(self.worst, 1e-30):.2f}x{'' if self.ok else f', {self.failed} OVER THE BAR'})")


def _ulp32(x):
    x = x.to(torch.float32)
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def row_errors(x, ref):
    """E_x(r): the L2 distance from `ref` (float64) of every row of a 2-D view."""
    return (x.double() - ref.double()).norm(dim=1)


def _verdict(name, axis, e_got, denom, floor, factor):
    """e_got(r) <= max(factor * denom(r), floor(r)) for every r; the reported ratio is e_got / denom (0 where the floor admits the row)."""
    over = e_got > torch.maximum(factor * denom, floor)
    ratio = torch.where(e_got <= floor, torch.zeros_like(e_got), e_got / denom.clamp_min(1e-300))
    w = int(ratio.argmax())
    return Verdict(name, axis, float(ratio[w]), w, factor, int(over.sum()), ratio.numel())


def judge_rows(name, got, pol, ref, factor, axis="row"):
    """E_got(r) <= factor * max(E_pol(r), med) for every row of the 2-D tensors got / pol / ref; rows with E_pol(r) == 0 get a floor of
    4 ulp(f32) of the row's largest |ref|."""
    ref = ref.double()
    e_got, e_pol = row_errors(got, ref), row_errors(pol, ref)
    med = torch.quantile(e_pol, 0.5)
    floor = torch.where(e_pol == 0, 4.0 * _ulp32(ref.abs().amax(dim=1)), torch.zeros_like(e_pol))
    return _verdict(name, axis, e_got, torch.maximum(e_pol, med), floor, factor)


def judge_elements(name, got, pol, ref, factor):
    """|got - ref| <= factor * rms(pol - ref) for every element of a vector."""
    ref = ref.double().reshape(-1)
    e_got = (got.double().reshape(-1) - ref).abs()
    rms = (pol.double().reshape(-1) - ref).pow(2).mean().sqrt()
    return _verdict(name, "elem", e_got, rms.expand_as(e_got), torch.zeros_like(e_got), factor)


def activation_names(cfg):
    return (["embed"] + [f"enc{i}" for i in range(cfg.num_hidden_layers)] + ["x_full"]
            + [f"dec{i}" for i in range(cfg.decoder_num_hidden_layers)] + ["logits"])


def judge_activations(got, pol, ref, f_act=None, names=None):
    """got / pol / ref: dicts name -> [B, rows, width] (any shape with the width last).  Returns one Verdict per tensor; 'labels', when
    `got` has it, is held to its relative-L2 bar."""
    f_act = F_ACT if f_act is None else f_act
    out = []
    for n in (names if names is not None else [k for k in ref if k != "labels"]):
        r = ref[n]
        w = r.shape[-1]
        out.append(judge_rows(n, got[n].reshape(-1, w), pol[n].reshape(-1, w), r.reshape(-1, w), f_act))
    if names is None and "labels" in got and "labels" in ref:
        e = float((got["labels"].double().reshape(-1) - ref["labels"].double().reshape(-1)).norm() / ref["labels"].double().norm())
        out.append(Verdict("labels", "rel", e, 0, LABELS_BAR, int(not e < LABELS_BAR), 1))
    return out


def is_matrix(name, t):
    return t.dim() >= 2 and name != "mask_token"


def judge_gradients(got, pol, ref, f_mat=None, f_vec=None, scale=1.0):
    """got / pol / ref: dicts parameter name -> gradient.  `scale`: the upstream gradient `got` was computed with (a power of two; the
    references are those of scale 1).  Matrices are judged over rows and over columns, vectors and mask_token per element."""
    f_mat, f_vec = F_MAT if f_mat is None else f_mat, F_VEC if f_vec is None else f_vec
    out = []
    for k, r in ref.items():
        g = got[k].double() / scale
        if is_matrix(k, r):
            g2, p2, r2 = (t.reshape(r.shape[0], -1) for t in (g, pol[k], r))
            out.append(judge_rows(k, g2, p2, r2, f_mat, "row"))
            out.append(judge_rows(k, g2.t(), p2.t(), r2.t(), f_mat, "col"))
        else:
            out.append(judge_elements(k, g, pol[k], r, f_vec))
    return out


def judge_on_against_off(on, off, pol, ref, matrices=()):
    """Two executions of one step that differ only in scheduling (tail mode on against off), per row:
    || on_r - off_r || <= max(E_off(r), med), med = the median of E_pol as everywhere.  Tensors named in `matrices` are 2-D gradients
    (rows and columns); other tensors with a width are activations (token rows).  A vector (or mask_token) is ONE row - the column
    of its (out, 1) view: || on - off || <= max(|| off - ref ||, || pol - ref ||).  Its elements are not rows: a norm over a row
    averages the scheduling noise of its elements, a single element has nothing to average, and where the true value is 0 (key.bias)
    every execution's element IS such noise - two correct CPU executions of the policy (float32- and float64-carried) differ there
    by up to 3.3 x max(|off - ref|, rms) per element while their norms satisfy the rule (tests/test_model_rows_ref.py)."""
    out = []
    for k, r in ref.items():
        if k == "labels":
            continue
        if r.dim() >= 2 and k != "mask_token":
            shp = (r.shape[0], -1) if k in matrices else (-1, r.shape[-1])
            a, b, p2, r2 = (t.double().reshape(shp) for t in (on[k], off[k], pol[k], r))
            for axis, (a_, b_, p_, r_) in (("row", (a, b, p2, r2)), ("col", (a.t(), b.t(), p2.t(), r2.t())))[: 2 if k in matrices else 1]:
                e_off, med = row_errors(b_, r_), torch.quantile(row_errors(p_, r_), 0.5)
                out.append(_verdict(k, axis, (a_ - b_).norm(dim=1), torch.maximum(e_off, med), torch.zeros_like(e_off), 1.0))
        else:
            a, b, p1, r1 = (t.double().reshape(1, -1) for t in (on[k], off[k], pol[k], r))
            e_off = row_errors(b, r1)
            out.append(_verdict(k, "vec", (a - b).norm(dim=1), torch.maximum(e_off, row_errors(p1, r1)), torch.zeros_like(e_off), 1.0))
    return out


def failures(verdicts):
    return [v.line() for v in verdicts if not v.ok]


def report_lines(verdicts, what="E_got / max(E_pol, med)"):
    """One line per tensor for the parity report: the worst ratio per axis, where it fell, the factor in force."""
    by_tensor = {}
    for v in verdicts:
        by_tensor.setdefault(v.tensor, []).append(v)
    out = []
    for name, vs in by_tensor.items():
        parts = [f"{v.axis} {v.worst:.3g} at {v.where} of {v.count}" + ("" if v.ok else f" ({v.failed} OVER)") for v in vs]
        out.append(f"{name}: worst {what} " + ", ".join(parts) + f" (factor {vs[0].factor:g})")
    return out


def mask_ratio(name):
    return _SPEC[name][3]


def worst(verdicts, axes=("row", "col", "elem")):
    """{axis: worst ratio} over a list of verdicts."""
    return {a: max([v.worst for v in verdicts if v.axis == a], default=0.0) for a in axes}


# ------------------------------------------------------------------------------------------------ the whole-tensor bars (existing)
def whole_tensor_failures(got, ref):
    """The bars of tests/test_gpu_videomae.py::_check_step on {"taps", "grads"} dicts: activations and logits 2e-2 relative L2, every
    gradient tensor 5e-2 with a floor of 1e-3 of the largest gradient norm.  Returns the list of tensors over a bar (empty: passes)."""
    bad = []
    for n, r in ref["taps"].items():
        if n == "labels":
            continue
        e = float((got["taps"][n].double() - r.double()).norm() / r.double().norm())
        if not e < 2e-2:
            bad.append((n, e))
    gmax = max(float(g.double().norm()) for g in ref["grads"].values())
    for k, r in ref["grads"].items():
        e = float((got["grads"][k].double() - r.double()).norm() / (r.double().norm() + 1e-3 * gmax))
        if not e < 5e-2:
            bad.append((k, e))
    return bad


# ------------------------------------------------------------------------------------------------ mutants of the policy step
MUTANTS = ("context_row", "weight_gradient", "bias_gradient", "key_row", "mask_token")
_FC1 = "decoder.decoder_layers.0.intermediate.dense."


@contextlib.contextmanager
def _patched(**attrs):
    old = {k: getattr(vb, k) for k in attrs}
    for k, v in attrs.items():
        setattr(vb, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(vb, k, v)


def mutant_step(c, which):
    """The policy step (float32, BUILD) with one defect of the kind a kernel change can introduce:

      context_row      the attention context of the last token of the last clip is zeroed in the last decoder layer
      weight_gradient  the fc1 weight gradient of decoder layer 0 is formed without the last token row
      bias_gradient    the same omission for that layer's fc1 bias gradient
      key_row          head 0 of clip 1 reads clip 0's keys in encoder layer 1
      mask_token       the mask_token gradient misses the last decoded row of clip 1
    """
    assert which in MUTANTS, which
    cfg = c.cfg
    p = {k: v.detach().clone().requires_grad_(True) for k, v in c.params.items()}
    q = dict(p)
    real_attention, real_linear = vb._Attention, vb.linear
    calls = [0]

    class Attention:
        @staticmethod
        def apply(qh, kh, vh, pol):
            i = calls[0]
            calls[0] += 1
            if which == "key_row" and i == 1:
                kh = kh.clone()
                kh[1, 0] = kh[0, 0]
            o = real_attention.apply(qh, kh, vh, pol)
            if which == "context_row" and i == cfg.num_hidden_layers + cfg.decoder_num_hidden_layers - 1:
                keep = torch.ones(o.shape[0], 1, o.shape[2], 1, dtype=o.dtype)
                keep[-1, :, -1] = 0
                o = o * keep
            return o

    def linear(x, w, b, pol, round_dx=True):
        if which not in ("weight_gradient", "bias_gradient") or w is not p[_FC1 + "weight"]:
            return real_linear(x, w, b, pol, round_dx)
        x2 = x.reshape(-1, x.shape[-1])
        wl, bl = (w.detach(), b) if which == "weight_gradient" else (w, b.detach())
        y = torch.cat([real_linear(x2[:-1], w, b, pol, round_dx), real_linear(x2[-1:], wl, bl, pol, round_dx)])
        return y.reshape(*x.shape[:-1], y.shape[-1])

    if which == "mask_token":
        keep = torch.ones(c.pixels.shape[0], c.ndec, 1, dtype=torch.bool)
        keep[1, -1] = False
        q["mask_token"] = torch.where(keep, p["mask_token"], p["mask_token"].detach())
    taps = {}
    with _patched(_Attention=Attention, linear=linear):
        loss, _, _ = vb.forward(cfg, q, c.pixels, c.mask, vb.BUILD, taps, c.dec)
        loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}
    return _result(loss, grads, taps)
