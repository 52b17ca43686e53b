"""The VideoMAE pre-training step on the GPU, judged per row: every token row of every activation and of the logits, every row and
column of every weight gradient, every element of every vector gradient, against the float64 step, with the bars of
tests/model_rows_ref.py (pinned on the CPU by tests/test_model_rows_ref.py; DESIGN.md, "How a model step is judged"):

    E_got(r) <= F * max(E_pol(r), med)          F_ACT = 4 (token rows), F_MAT = 4 (weight rows and columns)
    |got - ref| <= F_VEC * rms(pol - ref)       F_VEC = 12 (vector elements, mask_token)

where `pol` is the plain float32 reference of the build's operand policy and the factors are what a second, float64-carried
implementation of that policy needs, doubled, under fixed caps.  The whole-tensor bars of test_gpu_videomae.py / test_gpu_dual_mask.py /
test_gpu_decoder_tail.py stay where they are; these sit inside them.

Cases (tests/model_rows_ref.py): S1 (108 encoder rows, 3 x 144 decoder rows, decoder 384 wide) as the launcher selects and on every
path an option forces; S2 (Ld = 172: the two-kernel attention backward, a decoder subset); S3 (tail mode on and off, ndec 256 and
200); S4 (encoder heads of 80).  Then three exact properties of the step, with no tolerance: clip independence, masked / visible pixel
independence, linearity in the upstream gradient.

One line per case and tensor goes to the parity report (tests/gpu_util.log_parity; a copy: profiles/model_rows_parity_report.txt).
"""
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


def _model(cfg, params):
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    m = bvc.VideoMAEForPreTraining(bvc.VideoMAEConfig(**kw))
    m.load_state_dict(params)
    return m.to(dev).train()


class _Options:
    """process-wide switches (and the deterministic mode) for the duration of a step"""
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


#  path             options                      deterministic  grad_scale
PATHS = {"selected":      ({}, False, 1.0),
         "gemm8":         ({"gemm8": 1}, False, 1.0),
         "row_ln0":       ({"row_ln": 0}, False, 1.0),
         "row_ln1":       ({"row_ln": 1}, False, 1.0),
         "deterministic": ({}, True, 1.0),
         "det_scale1024": ({}, True, 1024.0),
         "scale65536":    ({}, False, 65536.0),
         "tail_on":       ({"row_ln": 1, "dec_tail": 1}, False, 1.0),
         "tail_off":      ({"row_ln": 1, "dec_tail": 0}, False, 1.0)}


def _forward(model, pixels, mask, dec, names):
    """One forward; returns (output, {tap name: f32 CPU tensor [B, rows, width]})."""
    kw = {} if dec is None else {"bool_decode_pos": dec.to(dev)}
    out = model(pixels.to(dev), bool_masked_pos=mask.to(dev), output_logits=True, **kw)
    torch.cuda.synchronize()
    B, cfg = pixels.shape[0], model.config
    taps = {}
    for n in names:
        if n == "labels":
            width = out.logits.shape[-1]
        else:
            width = cfg.hidden_size if n == "embed" or n.startswith("enc") else cfg.decoder_hidden_size
        taps[n] = model.tap(n).view(B, -1, width).float().cpu()
    taps["logits"] = out.logits.float().cpu()
    return out, taps


@functools.lru_cache(maxsize=None)
def _gpu_step(name, path):
    """One forward and backward of a case on a path: {"loss", "taps", "grads"} on the CPU, gradients still multiplied by the path's
    grad_scale.  Computed once and shared (the on / off and linearity tests read the same runs the bar tests judged)."""
    c = M.case(name)
    opts, det, scale = PATHS[path]
    names = [n for n in M.activation_names(c.cfg) if n != "logits"] + ["labels"]
    with _Options(deterministic=det, **opts):
        model = _model(c.cfg, c.params)
        out, taps = _forward(model, c.pixels, c.mask, c.dec, names)
        (out.loss * scale).backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.float().cpu().clone() for k, p in model.named_parameters()}
    return {"loss": out.loss.detach().float().cpu(), "taps": taps, "grads": grads}


def _judge(name, path):
    c = M.case(name)
    ref, pol = M.references(name)
    got = _gpu_step(name, path)
    scale = PATHS[path][2]
    for k, t in ref["taps"].items():
        assert tuple(got["taps"][k].shape) == tuple(t.shape), (k, tuple(got["taps"][k].shape), tuple(t.shape))
    assert all(bool(torch.isfinite(g).all()) for g in got["grads"].values())
    unscaled = {"taps": got["taps"], "grads": {k: g.double() / scale for k, g in got["grads"].items()}}      # a power of two: exact
    acts = M.judge_activations(got["taps"], pol["taps"], ref["taps"])
    grads = M.judge_gradients(unscaled["grads"], pol["grads"], ref["grads"])
    rel = abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    tag = f"rows {name}/{path}"
    _log(f"[{tag}] {c.pixels.shape[0]} clips of {c.nvis} + {c.ndec} rows: loss hip {float(got['loss']):.7f} float64 {float(ref['loss']):.7f} "
         f"policy {float(pol['loss']):.7f} rel {rel:.2e}")
    for line in M.report_lines(acts + grads):
        _log(f"[{tag}] {line}")
    w = {**M.worst(acts, ("row",)), **{"g" + k: v for k, v in M.worst(grads).items()}}
    _log(f"[{tag}] worst: activation rows {w['row']:.3f} (factor {M.F_ACT:g}); gradient rows {w['grow']:.3f}, columns {w['gcol']:.3f} "
         f"(factor {M.F_MAT:g}); vector elements {w['gelem']:.3f} (factor {M.F_VEC:g})")
    bad = M.failures(acts + grads)
    assert not bad, (len(bad), bad[:6])
    assert rel < 1e-3, rel
    assert not M.whole_tensor_failures(unscaled, ref)
    return got


def _dec_rows(c):
    return c.pixels.shape[0] * (c.nvis + c.ndec)


def _row_ln(c):
    cfg = c.cfg
    return L.lib().bvc_op_row_ln_selected(_dec_rows(c), cfg.decoder_hidden_size, cfg.decoder_intermediate_size, cfg.decoder_num_attention_heads)


def _qkv_kernel(rows, width):
    """the instantiation the launcher runs a qkv product of this stack on, under the options in force (nothing is launched)"""
    a, w = torch.empty(rows, width, dtype=torch.bfloat16, device=dev), torch.empty(3 * width, width, dtype=torch.bfloat16, device=dev)
    out = torch.empty(rows, 3 * width, dtype=torch.bfloat16, device=dev)
    return G.gemm_kernel_name(G.gemm_desc(a, w, rows, 3 * width, width, G.EPI["BF16"], out), G.NT)


# ------------------------------------------------------------------------------------------------ S1 on every path
def test_s1_as_the_launcher_selects():
    c = M.case("S1")
    assert L.lib().bvc_get_option(b"gemm8") == 0 and L.lib().bvc_get_option(b"row_ln") == 0
    assert _row_ln(c) == 0                                             # 432 rows: separate LayerNorm passes
    assert "gemm8" not in _qkv_kernel(c.pixels.shape[0] * c.nvis, c.cfg.hidden_size)
    _judge("S1", "selected")


def test_s1_on_gemm8():
    c = M.case("S1")
    rows, width = c.pixels.shape[0] * c.nvis, c.cfg.hidden_size
    with _Options(gemm8=1):
        assert _qkv_kernel(rows, width).startswith("bvc::gemm8_kernel<"), _qkv_kernel(rows, width)      # 108 x 576 x 192 on the 256-row kernel
        assert _row_ln(c) == 1                                         # and with it the decoder's LayerNorms in the 384-wide epilogues
    _judge("S1", "gemm8")
    assert "gemm8" not in _qkv_kernel(rows, width)


@pytest.mark.parametrize("row_ln", [0, 1])
def test_s1_layernorm_passes_and_epilogues(row_ln):
    c = M.case("S1")
    with _Options(row_ln=row_ln):
        assert _row_ln(c) == row_ln
    _judge("S1", f"row_ln{row_ln}")


def test_s1_deterministic_mode():
    _judge("S1", "deterministic")


def test_s1_grad_scale_65536():
    """a GradScaler-sized upstream gradient: the references are those of scale 1 (a power of two commutes with every rounding)"""
    _judge("S1", "scale65536")


# ------------------------------------------------------------------------------------------------ S2, S4 as selected
def test_s2_ragged_decoder_subset_above_the_whole_head_limit():
    c = M.case("S2")
    from tests import test_gpu_dual_mask as T      # the same shape and subset as its "ragged172" case
    assert c.cfg == T.RAGGED and torch.equal(c.dec, T._generated(c.cfg, c.mask, 0.84, 21))
    assert (c.nvis, c.ndec, c.nvis + c.ndec) == (52, 120, 172)
    _judge("S2", "selected")


def test_s4_encoder_heads_of_80_in_place():
    c = M.case("S4")
    assert c.cfg.hidden_size // c.cfg.num_attention_heads == 80 and L.lib().bvc_op_attention_width(80) == 80
    _judge("S4", "selected")


# ------------------------------------------------------------------------------------------------ S3: tail mode
@pytest.mark.parametrize("name", ["S3", "S3_subset"])
@pytest.mark.parametrize("tail", ["tail_on", "tail_off"])
def test_s3_tail_mode(name, tail):
    c = M.case(name)
    with _Options(row_ln=1):
        assert _row_ln(c) == 1
    _judge(name, tail)


@pytest.mark.parametrize("name", ["S3", "S3_subset"])
def test_s3_tail_on_against_off_per_row(name):
    """|| on_r - off_r || <= max(E_off(r), med) for every row of every activation and of the logits, every row and column of every
    weight gradient, and every vector gradient as one row: the per-row form of test_gpu_decoder_tail.py's whole-tensor rule."""
    ref, pol = M.references(name)
    on, off = _gpu_step(name, "tail_on"), _gpu_step(name, "tail_off")
    matrices = {k for k, g in ref["grads"].items() if M.is_matrix(k, g)}
    acts = M.judge_on_against_off(on["taps"], off["taps"], pol["taps"], ref["taps"])
    grads = M.judge_on_against_off(on["grads"], off["grads"], pol["grads"], ref["grads"], matrices)
    tag = f"rows {name}/tail on-off"
    for line in M.report_lines(acts + grads, "|| on - off || / max(E_off, med)"):
        _log(f"[{tag}] {line}")
    w = M.worst(acts + grads, ("row", "col", "vec"))
    _log(f"[{tag}] worst || on - off || / max(E_off, med): rows {w['row']:.3f}, columns {w['col']:.3f}, whole vectors {w['vec']:.3f} (bar 1)")
    if name == "S3":          # 256 decoded rows per clip: tail mode engages, and the two paths differ in bits
        assert not torch.equal(on["taps"]["logits"], off["taps"]["logits"]), "tail mode did not engage"
    bad = M.failures(acts + grads)
    assert not bad, (len(bad), bad[:6])


# ------------------------------------------------------------------------------------------------ exact properties
def _forward_only(name, pixels, mask, dec, **opts):
    c = M.case(name)
    names = [n for n in M.activation_names(c.cfg) if n != "logits"] + ["labels"]
    with _Options(**opts), torch.no_grad():
        model = _model(c.cfg, c.params)
        out, taps = _forward(model, pixels, mask, dec, names)
    taps["loss"] = out.loss.detach().float().cpu()
    return taps


@pytest.mark.parametrize("name,opts", [("S1", {}), ("S3", {"row_ln": 1, "dec_tail": 1})])
def test_clip_independence_bit_for_bit(name, opts):
    """Clips 0 and 2 of the case's batch sit at positions 2 and 0 of another batch whose middle clip (and its mask) is new: every
    activation row, logits row and label row of a clip is the same bits in both - nothing of a clip's forward depends on its position
    or its neighbours.  As the launcher selects: the forward is first shown to be bit-stable run to run."""
    c = M.case(name)
    assert c.dec is None and c.pixels.shape[0] == 3
    a = _forward_only(name, c.pixels, c.mask, None, **opts)
    again = _forward_only(name, c.pixels, c.mask, None, **opts)
    for k in a:
        assert torch.equal(a[k], again[k]), f"forward not bit-stable run to run: {k}"
    other_px, other_mask = vo.synthetic_batch(c.cfg, 1, 977, M.mask_ratio(name))
    assert int(other_mask.sum()) == c.ndec and not torch.equal(other_mask[0], c.mask[1])
    px = torch.cat([c.pixels[2:3], other_px, c.pixels[0:1]])
    mk = torch.cat([c.mask[2:3], other_mask, c.mask[0:1]])
    b = _forward_only(name, px, mk, None, **opts)
    for k in a:
        if k == "loss":
            continue
        assert not torch.equal(a[k][1], b[k][1]), k               # the middle clips do differ
        for i, j in ((0, 2), (2, 0)):
            same = (a[k][i] == b[k][j]).all(dim=-1)
            assert bool(same.all()), f"{name} {k}: clip {i} differs at position {j} in rows {torch.nonzero(~same).flatten()[:8].tolist()}"


def _pixel_mask(cfg, token_mask):
    """[B, L] token mask -> [B, T, 1, H, W] mask of the pixels those tokens' tubes cover"""
    B = token_mask.shape[0]
    t, h, w = cfg.grid
    m = token_mask.view(B, t, h, w)
    m = m.repeat_interleave(cfg.tubelet_size, 1).repeat_interleave(cfg.patch_size, 2).repeat_interleave(cfg.patch_size, 3)
    return m[:, :, None]


def test_masked_and_visible_pixels_reach_only_what_they_should():
    """New pixels in the masked patches only: embed, enc<i> and the visible rows of x_full keep their bits (the encoder never sees
    them).  New pixels in the visible patches only: the labels keep their bits."""
    c = M.case("S1")
    cfg, nvis = c.cfg, c.nvis
    other, _ = vo.synthetic_batch(cfg, c.pixels.shape[0], 978, 0.75)
    masked_px = _pixel_mask(cfg, c.mask)
    base = _forward_only("S1", c.pixels, c.mask, None)
    a = _forward_only("S1", torch.where(masked_px, other, c.pixels), c.mask, None)
    for k in ["embed"] + [f"enc{i}" for i in range(cfg.num_hidden_layers)]:
        assert torch.equal(a[k], base[k]), k
    assert torch.equal(a["x_full"][:, :nvis], base["x_full"][:, :nvis])
    assert not torch.equal(a["labels"], base["labels"])                       # the change did arrive somewhere
    b = _forward_only("S1", torch.where(masked_px, c.pixels, other), c.mask, None)
    assert torch.equal(b["labels"], base["labels"])
    assert not torch.equal(b["embed"], base["embed"])


def test_gradients_are_linear_in_the_upstream_gradient_bit_for_bit():
    """Deterministic mode, S1: every gradient at grad_scale 1024 is 1024 x the gradient at scale 1, bit for bit - the backward is
    linear in its upstream gradient, and a power of two commutes with bf16 and f32 rounding away from under- and overflow."""
    one, big = _gpu_step("S1", "deterministic"), _gpu_step("S1", "det_scale1024")
    assert torch.equal(one["loss"], big["loss"])
    bad = [k for k in one["grads"] if not torch.equal(one["grads"][k] * 1024.0, big["grads"][k])]
    assert not bad, (len(bad), bad[:8])
