"""Tail mode of the VideoMAE pre-training step (option "dec_tail", stack.h LayerTail): the last decoder layer runs everything behind
its qkv product on the decoded rows only.  On against off (same process, same weights, same clips) and both against the fp32 oracle.

Bars.  Both paths are bf16 executions of the same mathematics, and what tail mode leaves out were exact zeros (the gradients of the
visible rows) or rows nobody reads; they differ in summation order and in which query block a row falls in.  So
  * the tail path's deviation from the fp32 oracle stays inside the bars of tests/test_gpu_videomae.py::_check_step (loss 1e-3,
    logits and activations 2e-2 relative L2, per-tensor gradients 5e-2 with its floor of 1e-3 of the largest gradient norm), and
  * the on / off difference of a tensor (loss, logits, every gradient tensor) is at most the off path's own deviation from the oracle
    for that tensor (L2 norms).
The measured values are logged through tests/gpu_util.log_parity (a copy: profiles/decoder_tail_parity.txt).
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from tests import dual_mask_ref as dr   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402

bvc = G.bvc
L = G.L
dev = torch.device("cuda:0")
_log = G.log_parity

# shape 1: 8 slots of 6 x 6 positions = 288 tokens, 32 of 36 masked per slot -> nvis = 32, ndec = 256 = 2 x 128; 3 clips: a unit
# boundary falls on a clip boundary, nvis is no multiple of a 128-row query block
SMALL = dataclasses.replace(vo.BASE, image_size=96, num_frames=16, tubelet_size=2, patch_size=16, hidden_size=384, num_attention_heads=6,
                            intermediate_size=1536, num_hidden_layers=1, decoder_num_hidden_layers=2)
# shape 2: the benchmark's geometry (1568 tokens, 160 visible, 1408 = 11 x 128 decoded), base widths, depth 1 + 2
BENCH2 = dataclasses.replace(vo.BASE, num_hidden_layers=1, decoder_num_hidden_layers=2)


def _model(cfg, params):
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    m = bvc.VideoMAEForPreTraining(bvc.VideoMAEConfig(**kw))
    m.load_state_dict(params)
    return m.to(dev).train()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(cfg, params, pixels, mask, decode mask or None, reference loss, gradients and taps): the fp32 reference, computed once."""
    if name == "small":
        cfg, B, seed, ratio, dec = SMALL, 3, 5, 0.89, None
    elif name == "bench2":
        cfg, B, seed, ratio, dec = BENCH2, 2, 3, 0.9, None
    elif name == "small_subset":      # 25 of the 32 masked positions of a slot decoded: ndec = 200, no multiple of 128
        cfg, B, seed, ratio, dec = SMALL, 3, 5, 0.89, 0.8
    else:
        raise KeyError(name)
    params = vo.make_params(cfg, seed=0)
    pixels, mask = vo.synthetic_batch(cfg, B, seed, ratio)
    taps = {}
    if dec is None:
        dmask = None
        ref_loss, ref_grads = vo.step(cfg, params, pixels, mask, taps=taps)
    else:
        gen = bvc.DecoderSubsetGenerator(cfg.grid, dec, rng=np.random.RandomState(31))
        dmask = torch.from_numpy(np.stack([gen(m) for m in mask.numpy()])).bool()
        ref_loss, ref_grads = dr.step(cfg, params, pixels, mask, dmask, taps=taps)
    return cfg, params, pixels, mask, dmask, ref_loss.detach(), ref_grads, {k: v.detach() for k, v in taps.items()}


class _Options:
    """process-wide switches for the duration of a test"""
    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = L.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            L.set_option(k, v)


def _step(name, tail, taps=()):
    cfg, params, pixels, mask, dmask, *_ = _case(name)
    with _Options(dec_tail=1 if tail else 0):
        model = _model(cfg, params)
        kw = {} if dmask is None else {"bool_decode_pos": dmask.to(dev)}
        out = model(pixels.to(dev), bool_masked_pos=mask.to(dev), output_logits=True, **kw)
        out.loss.backward()
        torch.cuda.synchronize()
        got = {n: model.tap(n).float().cpu() for n in taps}
    grads = {k: p.grad.float().cpu().clone() for k, p in model.named_parameters()}
    return out.loss.detach().float().cpu(), out.logits.float().cpu(), grads, got


def _on_against_off(tag, name, expect):
    cfg, params, pixels, mask, dmask, ref_loss, ref_grads, taps = _case(name)
    nvis, ndec = int((~mask[0]).sum()), int(mask[0].sum())
    assert (nvis, ndec) == expect, (nvis, ndec)
    assert L.lib().bvc_op_row_ln_selected(pixels.shape[0] * (nvis + ndec), cfg.decoder_hidden_size, cfg.decoder_intermediate_size,
                                          cfg.decoder_num_attention_heads) == 1
    loss_on, logits_on, g_on, _ = _step(name, True)
    loss_off, logits_off, g_off, _ = _step(name, False)
    ref_logits = taps["logits"]
    # the tail path against the oracle: the bars of test_gpu_videomae.py::_check_step
    rel = abs(float(loss_on) - float(ref_loss)) / abs(float(ref_loss))
    e_log = G.rel_err(logits_on, ref_logits)
    _log(f"[tail {tag}] nvis {nvis} ndec {ndec}: loss on {float(loss_on):.7f} off {float(loss_off):.7f} oracle {float(ref_loss):.7f}; on vs oracle rel {rel:.2e}; "
         f"logits on vs oracle rel {e_log:.2e}")
    gmax = max(float(g.norm()) for g in ref_grads.values())
    worst_abs, worst_ratio = ("", 0.0), ("", 0.0, 0.0, 0.0)
    fails = []
    for k, r in ref_grads.items():
        assert torch.isfinite(g_on[k]).all(), k
        e = float((g_on[k] - r).norm() / (r.norm() + 1e-3 * gmax))
        if e > worst_abs[1]:
            worst_abs = (k, e)
        if not e < 5e-2:
            fails.append(("oracle", k, e))
        d, own = float((g_on[k] - g_off[k]).norm()), float((g_off[k] - r).norm())
        if own == 0.0 or d / own > worst_ratio[1]:
            worst_ratio = (k, d / own if own > 0 else float("inf"), d, own)
        if not d <= own:
            fails.append(("on/off", k, d, own))
    d_loss, own_loss = abs(float(loss_on) - float(loss_off)), abs(float(loss_off) - float(ref_loss))
    d_log, own_log = float((logits_on - logits_off).norm()), float((logits_off - ref_logits).norm())
    _log(f"[tail {tag}] worst per-tensor grad rel vs oracle {worst_abs[1]:.2e} ({worst_abs[0]})")
    _log(f"[tail {tag}] on/off: |loss| {d_loss:.2e} (off vs oracle {own_loss:.2e}); logits L2 {d_log:.3e} (off vs oracle {own_log:.3e}); "
         f"worst gradient tensor {worst_ratio[2]:.3e} of {worst_ratio[3]:.3e} = {worst_ratio[1]:.3f} ({worst_ratio[0]})")
    assert rel < 1e-3, rel
    assert e_log < 2e-2, e_log
    assert d_log > 0.0, "on and off gave the same logits bit for bit: tail mode did not engage"
    assert d_loss <= own_loss, (d_loss, own_loss)
    assert d_log <= own_log, (d_log, own_log)
    assert not fails, fails[:5]


def test_small_fused_path_on_against_off():
    """3 clips of 32 visible + 256 decoded rows, 384 wide, 6 heads, 1 + 2 layers, LayerNorm epilogues forced on"""
    with _Options(row_ln=1):
        _on_against_off("small 3 x (32 + 256)", "small", (32, 256))


def test_benchmark_geometry_on_against_off():
    """2 clips of the benchmark's 160 + 1408 rows (11 exact units per clip), base widths, depth 1 + 2"""
    with _Options(row_ln=1):
        _on_against_off("bench 2 x (160 + 1408)", "bench2", (160, 1408))


def test_decode_count_off_the_unit_grid_falls_back_bit_identically():
    """ndec = 200 per clip: tail mode must yield, and then the switch changes nothing.  Bits are compared where a step has them, in
    the deterministic mode (the default weight-gradient kernels add by f32 atomics in scheduling order)."""
    cfg, params, pixels, mask, dmask, *_ = _case("small_subset")
    assert int(dmask[0].sum()) == 200 and int((~mask[0]).sum()) == 32
    bvc.use_deterministic_algorithms(True)
    try:
        with _Options(row_ln=1):
            on = _step("small_subset", True)
            off = _step("small_subset", False)
    finally:
        bvc.use_deterministic_algorithms(False)
        L.lib()
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    for k in on[2]:
        assert torch.equal(on[2][k], off[2][k]), k


def test_deterministic_mode_in_tail_mode_is_bitwise_reproducible():
    bvc.use_deterministic_algorithms(True)
    try:
        with _Options(row_ln=1):
            a = _step("small", True)
            b = _step("small", True)
    finally:
        bvc.use_deterministic_algorithms(False)
        L.lib()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    ref_loss = _case("small")[5]
    assert abs(float(a[0]) - float(ref_loss)) / abs(float(ref_loss)) < 1e-3


def test_last_decoder_tap_in_tail_mode_has_every_row():
    """tap("dec<last>") keeps nvis + ndec rows per clip: the visible rows are completed on demand and held to the oracle like the rest"""
    cfg, params, pixels, mask, dmask, ref_loss, ref_grads, taps = _case("small")
    last = f"dec{cfg.decoder_num_hidden_layers - 1}"
    with _Options(row_ln=1):
        _, _, _, got = _step("small", True, taps=(last, "dec0"))
    ref = taps[last]
    B, nvis = pixels.shape[0], 32
    assert tuple(ref.shape) == (B, 288, cfg.decoder_hidden_size) and got[last].numel() == ref.numel()
    x = got[last].view(ref.shape)
    e_all, e_vis, e_dec = G.rel_err(x, ref), G.rel_err(x[:, :nvis], ref[:, :nvis]), G.rel_err(x[:, nvis:], ref[:, nvis:])
    e0 = G.rel_err(got["dec0"].view(taps["dec0"].shape), taps["dec0"])
    _log(f"[tail tap {last}] rel vs oracle: all rows {e_all:.2e}, visible rows {e_vis:.2e}, decoded rows {e_dec:.2e}; dec0 {e0:.2e}")
    assert e_all < 2e-2 and e_vis < 2e-2 and e_dec < 2e-2 and e0 < 2e-2, (e_all, e_vis, e_dec, e0)
