"""First mode of the VideoMAE pre-training step (option "dec_first", stack.h LayerFirst): the first decoder layer computes LayerNorm 1
and the qkv row of the mask rows once per position, and in the backward derives their share of the qkv weight / bias gradients, of
LayerNorm 1's and of the mask token's gradient from per-position sums of d qkv.  On against off (same process, same weights, same
clips), each on the bars of tests/model_rows_ref.py - no tolerance of this file's own:

  * the loss of the two paths is equal, or one f32 ulp apart;
  * the on path passes the per-row float64 bars the off path is held to (judge_activations / judge_gradients);
  * || on_r - off_r || <= max(E_off(r), med) for every activation row, every row and column of every weight gradient and every vector
    gradient as one row (judge_on_against_off: the rule tail mode is held to).

Cases: S1, S3 and S3_subset of model_rows_ref (a decoder subset leaves positions neither visible nor decoded), S1 with one clip (every
position has at most one contributor), S1 with one position masked in all three clips and one visible in all three (S[p] = 0: its table
row is unused), each under row_ln 0 / 1 x dec_tail 0 / 1; the benchmark's geometry (160 + 1408 rows, base widths) at 2 and 3 clips as
selected and with tail mode on; a one-layer decoder, which must fall back.  The reduction kernel alone against a float64 index_add,
and the deterministic mode.
"""
import dataclasses
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from tests import model_rows_ref as M   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402

bvc = G.bvc
L = G.L
dev = torch.device("cuda:0")
_log = G.log_parity

QKV0 = "decoder.decoder_layers.0.attention.attention.query.weight"
# the gradients the by-position backward produces or feeds (all others are judged too)
NAMED = ("mask_token", "decoder.decoder_layers.0.layernorm_before.weight", "decoder.decoder_layers.0.layernorm_before.bias", QKV0,
         "decoder.decoder_layers.0.attention.attention.query.bias", "encoder_to_decoder.weight",
         "videomae.encoder.layer.0.attention.attention.query.weight")


def _model(cfg, params):
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    m = bvc.VideoMAEForPreTraining(bvc.VideoMAEConfig(**kw))
    m.load_state_dict(params)
    return m.to(dev).train()


class _Options:
    def __init__(self, deterministic=False, **kw):
        self.kw, self.old, self.det = kw, {}, deterministic

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = L.set_option(k, v)
        if self.det:
            bvc.use_deterministic_algorithms(True)

    def __exit__(self, *exc):
        if self.det:
            bvc.use_deterministic_algorithms(False)
            L.lib()
        for k, v in self.old.items():
            L.set_option(k, v)


# ------------------------------------------------------------------------------------------------ cases
# the benchmark's geometry (1568 tokens, 160 visible, 1408 decoded), base widths, depth 1 + 2: BENCH2 of tests/test_gpu_decoder_tail.py
BENCH = dataclasses.replace(vo.BASE, num_hidden_layers=1, decoder_num_hidden_layers=2)
P_MASKED, P_VISIBLE = 5, 17      # S1_hand: masked in every clip / visible in every clip


def _hand_mask(mask):
    """The S1 masks with position P_MASKED masked and P_VISIBLE visible in all clips; every clip keeps its counts (one swap each)."""
    mask = mask.clone()
    for b in range(mask.shape[0]):
        for p, want in ((P_MASKED, True), (P_VISIBLE, False)):
            if bool(mask[b, p]) != want:
                q = next(int(i) for i in torch.nonzero(mask[b] == want).flatten() if int(i) not in (P_MASKED, P_VISIBLE))
                mask[b, p], mask[b, q] = want, not want
    return mask


@functools.lru_cache(maxsize=None)
def _case(name):
    if name in M.CASES:
        return M.case(name)
    s1 = M.case("S1")
    if name == "S1_b1":
        return M.Case(name, s1.cfg, s1.params, s1.pixels[:1].clone(), s1.mask[:1].clone(), None)
    if name == "S1_hand":
        return M.Case(name, s1.cfg, s1.params, s1.pixels, _hand_mask(s1.mask), None)
    if name in ("BENCH_b2", "BENCH_b3"):
        pixels, mask = vo.synthetic_batch(BENCH, int(name[-1]), 3, 0.9)
        return M.Case(name, BENCH, vo.make_params(BENCH, seed=0), pixels, mask, None)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _references(name):
    """(ref, pol): shared with tests/test_gpu_model_rows.py for its cases, computed once here for the others; nobody writes to them."""
    if name in M.CASES:
        return M.references(name)
    c = _case(name)
    return M.float64_step(c), M.policy_step(c)


def _names(cfg):
    return [n for n in M.activation_names(cfg) if n != "logits"]


@functools.lru_cache(maxsize=None)
def _gpu_step(name, first, tail, row_ln, det=False, run=0):
    c = _case(name)
    with _Options(deterministic=det, dec_first=first, dec_tail=tail, row_ln=row_ln):
        model = _model(c.cfg, c.params)
        kw = {} if c.dec is None else {"bool_decode_pos": c.dec.to(dev)}
        out = model(c.pixels.to(dev), bool_masked_pos=c.mask.to(dev), output_logits=True, **kw)
        B = c.pixels.shape[0]
        taps = {}
        for n in _names(c.cfg):
            width = c.cfg.hidden_size if n == "embed" or n.startswith("enc") else c.cfg.decoder_hidden_size
            taps[n] = model.tap(n).view(B, -1, width).float().cpu()
        taps["logits"] = out.logits.float().cpu()
        out.loss.backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.float().cpu().clone() for k, p in model.named_parameters()}
    return {"loss": out.loss.detach().float().cpu(), "taps": taps, "grads": grads}


def _ulps(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float32).reshape(1), torch.as_tensor(b, dtype=torch.float32).reshape(1)
    return abs(int(a.view(torch.int32)) - int(b.view(torch.int32)))


def _on_against_off(name, tail, row_ln, engaged=True):
    c = _case(name)
    ref, pol = _references(name)
    on, off = _gpu_step(name, 1, tail, row_ln), _gpu_step(name, 0, tail, row_ln)
    tag = f"first {name}/tail{tail}/row_ln{row_ln}"
    d_ulp = _ulps(on["loss"], off["loss"])
    _log(f"[{tag}] {c.pixels.shape[0]} clips of {c.nvis} + {c.ndec} rows: loss on {float(on['loss']):.9g} off {float(off['loss']):.9g} ({d_ulp} ulp) "
         f"float64 {float(ref['loss']):.9g}")
    # the on path on the bars of the off path
    for which, got in (("on", on), ("off", off)):
        assert all(bool(torch.isfinite(g).all()) for g in got["grads"].values())
        acts = M.judge_activations(got["taps"], pol["taps"], ref["taps"])
        grads = M.judge_gradients(got["grads"], pol["grads"], ref["grads"])
        w = {**M.worst(acts, ("row",)), **{"g" + k: v for k, v in M.worst(grads).items()}}
        _log(f"[{tag}] {which}: worst activation rows {w['row']:.3f} (factor {M.F_ACT:g}); gradient rows {w['grow']:.3f}, columns {w['gcol']:.3f} "
             f"(factor {M.F_MAT:g}); vector elements {w['gelem']:.3f} (factor {M.F_VEC:g})")
        for v in grads:
            if v.tensor in NAMED:
                _log(f"[{tag}] {which}: {v.line()}")
        if which == "on":
            bad = M.failures(acts + grads)
            assert not bad, (len(bad), bad[:6])
            assert not M.whole_tensor_failures(got, ref)
    # on against off, per row
    matrices = {k for k, g in ref["grads"].items() if M.is_matrix(k, g)}
    acts = M.judge_on_against_off(on["taps"], off["taps"], pol["taps"], ref["taps"])
    grads = M.judge_on_against_off(on["grads"], off["grads"], pol["grads"], ref["grads"], matrices)
    for line in M.report_lines([v for v in acts + grads if v.tensor in NAMED or v.tensor in on["taps"]], "|| on - off || / max(E_off, med)"):
        _log(f"[{tag}] {line}")
    w = M.worst(acts + grads, ("row", "col", "vec"))
    _log(f"[{tag}] worst || on - off || / max(E_off, med): rows {w['row']:.3f}, columns {w['col']:.3f}, whole vectors {w['vec']:.3f} (bar 1)")
    assert d_ulp <= 1, (float(on["loss"]), float(off["loss"]), d_ulp)
    bad = M.failures(acts + grads)
    assert not bad, (len(bad), bad[:6])
    if engaged:
        assert not torch.equal(on["grads"][QKV0], off["grads"][QKV0]), "first mode did not engage: the qkv weight gradient has the same bits"


COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]      # (dec_tail, row_ln)


@pytest.mark.parametrize("tail,row_ln", COMBOS)
@pytest.mark.parametrize("name", ["S1", "S1_b1", "S1_hand", "S3", "S3_subset"])
def test_on_against_off(name, tail, row_ln):
    _on_against_off(name, tail, row_ln)


def test_hand_masks_are_what_they_claim():
    c = _case("S1_hand")
    assert bool(c.mask[:, P_MASKED].all()) and not bool(c.mask[:, P_VISIBLE].any())
    assert c.mask.sum(dim=1).tolist() == M.case("S1").mask.sum(dim=1).tolist()
    assert _case("S1_b1").pixels.shape[0] == 1
    sub = _case("S3_subset")
    assert bool((sub.mask & ~sub.dec).any()), "the subset leaves no position masked and undecoded"


# ------------------------------------------------------------------------------------------------ the benchmark's geometry
@pytest.mark.parametrize("tail,row_ln", [(0, 0), (1, 1)])
@pytest.mark.parametrize("name", ["BENCH_b2", "BENCH_b3"])
def test_benchmark_geometry_on_against_off(name, tail, row_ln):
    """160 + 1408 rows per clip (11 whole 128-row units: tail mode engages), base widths, depth 1 + 2, at 2 and 3 clips: as the launcher
    selects, and with tail mode and the LayerNorm epilogues on"""
    c = _case(name)
    assert (c.nvis, c.ndec) == (160, 1408)
    _on_against_off(name, tail, row_ln)


# ------------------------------------------------------------------------------------------------ fall-back, deterministic mode
def test_one_layer_decoder_falls_back_bit_identically():
    """a decoder of one layer: that layer may be the tail layer, first mode yields, and the switch changes nothing (bits compared in the
    deterministic mode, where a step has them)"""
    s1 = M.case("S1")
    cfg = dataclasses.replace(s1.cfg, decoder_num_hidden_layers=1)
    params = vo.make_params(cfg, seed=0)
    got = {}
    for first in (1, 0):
        with _Options(deterministic=True, dec_first=first):
            model = _model(cfg, params)
            out = model(s1.pixels.to(dev), bool_masked_pos=s1.mask.to(dev), output_logits=True)
            out.loss.backward()
            torch.cuda.synchronize()
            got[first] = (out.loss.detach().cpu(), out.logits.cpu(), {k: p.grad.cpu().clone() for k, p in model.named_parameters()})
    assert torch.equal(got[1][0], got[0][0]) and torch.equal(got[1][1], got[0][1])
    for k in got[1][2]:
        assert torch.equal(got[1][2][k], got[0][2][k]), k


@pytest.mark.parametrize("name,tail,row_ln", [("S1", 0, 0), ("S3", 1, 1), ("S3_subset", 1, 1)])
def test_deterministic_mode_with_first_mode_is_bitwise_reproducible(name, tail, row_ln):
    a, b = _gpu_step(name, 1, tail, row_ln, True, 0), _gpu_step(name, 1, tail, row_ln, True, 1)
    assert torch.equal(a["loss"], b["loss"])
    for k in a["taps"]:
        assert torch.equal(a["taps"][k], b["taps"][k]), k
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    ref = _references(name)[0]
    assert abs(float(a["loss"]) - float(ref["loss"])) / abs(float(ref["loss"])) < 1e-3


# ------------------------------------------------------------------------------------------------ the index and the reduction alone
def _slots(B, Lp, ndec, seed):
    """dec_idx [B][ndec] ascending, none of them position `hole`; dec_slot [B][Lp] with -1 elsewhere"""
    g = torch.Generator().manual_seed(seed)
    hole = Lp // 2
    idx = torch.empty(B, ndec, dtype=torch.int32)
    slot = torch.full((B, Lp), -1, dtype=torch.int32)
    for b in range(B):
        cand = torch.tensor([p for p in range(Lp) if p != hole])
        pick = cand[torch.randperm(len(cand), generator=g)[:ndec]].sort().values
        idx[b] = pick.int()
        slot[b, pick] = torch.arange(ndec, dtype=torch.int32)
    return idx, slot, hole


@pytest.mark.parametrize("Lp", [8, 33, 1568])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_reduction_kernel_against_float64_index_add(B, Lp):
    """S[p] = sum over clips of dqkv[b][nvis + dec_slot[b][p]] (1152 columns): |S - S64| <= B * 2^-24 * sum |x| per element (B f32
    additions of exactly representable bf16 terms), the same bits on two runs, a position no clip decodes stays zero; the bf16 pair is
    hi = bf16(S), lo = bf16(S - hi) exactly."""
    W, nvis = 1152, 3
    ndec = max(1, (Lp - nvis) * 3 // 4)
    Ld = nvis + ndec
    idx, slot, hole = _slots(B, Lp, ndec, 100 * B + Lp)
    x = G.bf16_randn(B, Ld, W, seed=B + Lp)
    idx_d, slot_d = idx.to(dev), torch.full((B, Lp), 7, dtype=torch.int32, device=dev)
    L.check(L.lib().bvc_op_dec_slot(G.ptr(idx_d), G.ptr(slot_d), B, Lp, ndec, G.stream()), "op_dec_slot")
    assert torch.equal(slot_d.cpu(), slot)
    runs = []
    for _ in range(2):
        S = torch.full((Lp, W), float("nan"), device=dev)
        hi = torch.zeros(Lp, W, dtype=torch.bfloat16, device=dev)
        lo = torch.zeros(Lp, W, dtype=torch.bfloat16, device=dev)
        L.check(L.lib().bvc_op_first_reduce(G.ptr(x), G.ptr(slot_d), B, Lp, Ld, nvis, W, G.ptr(S), G.ptr(hi), G.ptr(lo), G.stream()), "op_first_reduce")
        torch.cuda.synchronize()
        runs.append((S.cpu(), hi.cpu(), lo.cpu()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    S, hi, lo = runs[0]
    xc = x.cpu().double()
    S64, A64 = torch.zeros(Lp, W, dtype=torch.float64), torch.zeros(Lp, W, dtype=torch.float64)
    for b in range(B):
        S64.index_add_(0, idx[b].long(), xc[b, nvis:])
        A64.index_add_(0, idx[b].long(), xc[b, nvis:].abs())
    err = (S.double() - S64).abs()
    bound = B * 2.0 ** -24 * A64
    assert bool((err <= bound).all()), float((err - bound).max())
    assert bool((S[hole] == 0).all())
    assert torch.equal(hi, S.to(torch.bfloat16))
    assert torch.equal(lo, (S - hi.float()).to(torch.bfloat16))
