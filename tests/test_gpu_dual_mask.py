"""VideoMAE pre-training with a decoder subset (``bool_decode_pos``: VideoMAE V2's decoder masking) on the GPU against the fp32
reference tests/dual_mask_ref.py (pinned on the CPU by tests/test_dual_mask_ref.py).

Bars are those of tests/test_gpu_videomae.py::_check_step: activations and logits 2e-2 relative L2 (bf16 operands), labels 1e-5,
loss 1e-3, per-tensor gradients 5e-2 with a floor of 1e-3 of the largest gradient norm, the three grad_logger probes 1e-3 at
width >= 768 and 2.5e-3 below.
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
dev = torch.device("cuda:0")
_log = G.log_parity

# case c: TINY widths on 4 slots of 7 x 7 positions: L = 196, 36 masked per slot -> nvis = 52, nmask = 144
RAGGED = dataclasses.replace(vo.TINY, num_frames=8, tubelet_size=2, image_size=112, patch_size=16)
# case d: base widths (decoder 384 wide: the LayerNorm epilogues exist), two layers each
BASE2 = dataclasses.replace(vo.BASE, num_hidden_layers=2, decoder_num_hidden_layers=2)


def _model(cfg, params):
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    m = bvc.VideoMAEForPreTraining(bvc.VideoMAEConfig(**kw))
    m.load_state_dict(params)
    return m.to(dev).train()


def _generated(cfg, mask, decode_ratio, seed):
    gen = bvc.DecoderSubsetGenerator(cfg.grid, decode_ratio, rng=np.random.RandomState(seed))
    return torch.from_numpy(np.stack([gen(m) for m in mask.numpy()])).bool()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(cfg, params, pixels, mask, decode mask, grad_scale, reference loss, reference grads, reference taps), computed once per case."""
    if name == "tiny":            # a: B = 3, ratio 0.75, every second masked token
        cfg, B, seed, ratio, wseed, scale = vo.TINY, 3, 1, 0.75, 1, 65536.0
        pick = dr.every_second
    elif name == "ragged172":     # c: 30 of 36 per slot -> ndec = 120, Ld = 172 (one full 128-row block + 44 rows, two-kernel backward)
        cfg, B, seed, ratio, wseed, scale = RAGGED, 2, 7, 0.75, 0, 1.0
        pick = lambda m: _generated(cfg, m, 0.84, 21)
    elif name == "ragged160":     # c: 27 of 36 per slot -> ndec = 108, Ld = 160 (the whole-head backward's limit)
        cfg, B, seed, ratio, wseed, scale = RAGGED, 2, 7, 0.75, 0, 1.0
        pick = lambda m: _generated(cfg, m, 0.75, 22)
    elif name == "base864":       # d: 88 of 176 per slot -> ndec = 704, Ld = 864
        cfg, B, seed, ratio, wseed, scale = BASE2, 2, 3, 0.9, 0, 1.0
        pick = lambda m: _generated(cfg, m, 0.5, 23)
    else:
        raise KeyError(name)
    params = vo.make_params(cfg, seed=wseed)
    pixels, mask = vo.synthetic_batch(cfg, B, seed, ratio)
    dec = pick(mask)
    taps = {}
    ref_loss, ref_grads = dr.step(cfg, params, pixels, mask, dec, grad_scale=scale, taps=taps)
    return cfg, params, pixels, mask, dec, scale, ref_loss, ref_grads, {k: v.detach() for k, v in taps.items()}


def _check_dual_step(tag, name, expect=None):
    cfg, params, pixels, mask, dec, grad_scale, ref_loss, ref_grads, taps = _case(name)
    B = pixels.shape[0]
    nvis, nmask, ndec = int((~mask[0]).sum()), int(mask[0].sum()), int(dec[0].sum())
    if expect is not None:
        assert (nvis, nmask, ndec, nvis + ndec) == expect, (nvis, nmask, ndec)
    assert 0 < ndec < nmask
    model = _model(cfg, params)
    out = model(pixels.to(dev), bool_masked_pos=mask.to(dev), bool_decode_pos=dec.to(dev), output_logits=True)
    (out.loss * grad_scale).backward()
    torch.cuda.synchronize()
    assert tuple(out.logits.shape) == (B, ndec, cfg.patch_dim), tuple(out.logits.shape)
    loss = float(out.loss)
    rel = abs(loss - float(ref_loss)) / abs(float(ref_loss))
    _log(f"[dual {tag}] nvis {nvis} nmask {nmask} ndec {ndec} Ld {nvis + ndec}: loss hip {loss:.7f} reference {float(ref_loss):.7f} rel {rel:.2e}")
    Dd = cfg.decoder_hidden_size
    names = ["embed"] + [f"enc{i}" for i in range(cfg.num_hidden_layers)] + ["x_full"] + [f"dec{i}" for i in range(cfg.decoder_num_hidden_layers)]
    for n in names:
        ref = taps[n]
        if n == "x_full" or n.startswith("dec"):
            assert tuple(ref.shape) == (B, nvis + ndec, Dd)
        got = model.tap(n)
        assert got.numel() == ref.numel(), (n, got.numel(), ref.numel())       # x_full / dec<i>: B * Ld rows
        e = G.rel_err(got.view(ref.shape).float().cpu(), ref)
        _log(f"[dual {tag}] act {n:7s} rel {e:.2e}")
        assert e < 2e-2, (n, e)
    got = model.tap("labels")
    assert got.numel() == B * ndec * cfg.patch_dim
    e = G.rel_err(got.view(taps["labels"].shape).float().cpu(), taps["labels"])
    _log(f"[dual {tag}] labels rel {e:.2e}")
    assert e < 1e-5
    e = G.rel_err(out.logits.float().cpu(), taps["logits"])
    _log(f"[dual {tag}] logits rel {e:.2e}")
    assert e < 2e-2
    assert rel < 1e-3, rel
    named = dict(model.named_parameters())
    gmax = max(float(g.norm()) for g in ref_grads.values())
    worst = ("", 0.0)
    for k, r in ref_grads.items():
        g = named[k].grad.float().cpu()
        assert torch.isfinite(g).all(), k
        e = float((g - r).norm() / (r.norm() + 1e-3 * gmax))
        if e > worst[1]:
            worst = (k, e)
        assert e < 5e-2, (k, e)
    _log(f"[dual {tag}] worst per-tensor grad rel {worst[1]:.2e} ({worst[0]})")
    for k in vo.GRAD_PROBES:
        gn, rn = float(named[k].grad.norm()), float(ref_grads[k].norm())
        e = abs(gn - rn) / rn
        _log(f"[dual {tag}] grad-norm {k}: hip {gn:.6e} reference {rn:.6e} rel {e:.2e}")
        assert e < (1e-3 if cfg.hidden_size >= 768 else 2.5e-3), (k, e)
    return model


# ------------------------------------------------------------------ a
def test_tiny_step_with_every_second_masked_token_decoded():
    """Fails without the feature: the keyword then vanishes into **kwargs and logits comes back [B, nmask, P]."""
    _check_dual_step("tiny", "tiny", expect=(8, 24, 12, 20))


# ------------------------------------------------------------------ b
def _one_step(cfg, params, pixels, mask, dec):
    model = _model(cfg, params)
    kw = {} if dec is None else {"bool_decode_pos": dec.to(dev)}
    out = model(pixels.to(dev), bool_masked_pos=mask.to(dev), output_logits=True, **kw)
    out.loss.backward()
    torch.cuda.synchronize()
    return out.loss.detach().cpu(), out.logits.cpu(), model.flat_grads().detach().cpu().clone()


@pytest.mark.parametrize("shape", ["tiny", "f8_t2_i96_p16"])
def test_decode_all_through_the_new_entry_points_is_bit_identical(shape):
    if shape == "tiny":
        cfg, B, seed, ratio = vo.TINY, 3, 1, 0.75
    else:       # one case of test_gpu_videomae.py::test_config_matrix_small
        cfg, B, seed, ratio = dataclasses.replace(vo.TINY, num_frames=8, tubelet_size=2, image_size=96, patch_size=16), 2, 7, 0.9
    params = vo.make_params(cfg, seed=0)
    pixels, mask = vo.synthetic_batch(cfg, B, seed, ratio)
    # as selected: the forward has no scheduling-order sums, so loss and logits have one set of bits.  The weight gradients of the
    # default kernels add by f32 atomics and differ between two runs of the SAME step (test_gpu_videomae.py::
    # test_gradient_run_to_run_spread_at_64_clips), so their bits are compared where a step has them: in the deterministic mode.
    # In the default mode the two gradients agree within the run-to-run spread the project pins for one step run twice: 5e-6 of the
    # largest element (test_gpu_deterministic.py::test_deterministic_and_default_gradients_agree_at_the_spread_bar).
    plain = _one_step(cfg, params, pixels, mask, None)
    dual = _one_step(cfg, params, pixels, mask, mask.clone())
    assert torch.equal(plain[0], dual[0]), (plain[0], dual[0])
    assert torch.equal(plain[1], dual[1])
    spread, gmax = float((plain[2] - dual[2]).abs().max()), float(plain[2].abs().max())
    _log(f"[dual decode-all {shape}] default mode: {100 * float((plain[2] != dual[2]).float().mean()):.3f} % of the gradient elements differ, "
         f"max abs {spread:.2e} of {gmax:.2e}")
    assert torch.isfinite(dual[2]).all() and spread <= 5e-6 * gmax, (spread, gmax)
    if shape == "tiny":      # 96 decoder rows, one row tile per product: no element differed in any recorded run (0.011 % at the other shape)
        assert torch.equal(plain[2], dual[2])
    bvc.use_deterministic_algorithms(True)
    try:
        plain = _one_step(cfg, params, pixels, mask, None)
        dual = _one_step(cfg, params, pixels, mask, mask.clone())
    finally:
        bvc.use_deterministic_algorithms(False)
    assert torch.equal(plain[0], dual[0]), (plain[0], dual[0])
    assert torch.equal(plain[1], dual[1])
    assert torch.equal(plain[2], dual[2]), f"{100 * float((plain[2] != dual[2]).float().mean()):.3f} % of the gradient elements differ"


# ------------------------------------------------------------------ c
def test_ragged_decoder_length_above_the_whole_head_limit():
    _check_dual_step("ragged Ld 172", "ragged172", expect=(52, 144, 120, 172))


def test_ragged_decoder_length_at_the_whole_head_limit():
    _check_dual_step("ragged Ld 160", "ragged160", expect=(52, 144, 108, 160))


# ------------------------------------------------------------------ d
@pytest.mark.parametrize("row_ln", [None, 1])
def test_decoder_width_384_with_the_layernorm_epilogues_both_ways(row_ln):
    """Ld = 864 at 2 clips (1728 rows: 13 full 128-row tiles and one of 64): once as the launcher selects (separate LayerNorm passes
    at this size), once with the LayerNorms in the epilogues of the 384-wide products (gemm8's 128 x 384 tile, EC 4 / 5)."""
    rows = 2 * 864
    assert G.L.lib().bvc_op_row_ln_selected(rows, 384, 1536, 6) == 0
    old = G.L.set_option("row_ln", row_ln) if row_ln is not None else None
    try:
        if row_ln:
            assert G.L.lib().bvc_op_row_ln_selected(rows, 384, 1536, 6) == 1
        _check_dual_step(f"base Ld 864 row_ln {row_ln}", "base864", expect=(160, 1408, 704, 864))
    finally:
        if row_ln is not None:
            G.L.set_option("row_ln", old)


# ------------------------------------------------------------------ e
def _leaky(mask, dec):
    """dec with one visible token of clip 1 set and one decoded token cleared: the count stays, the subset condition breaks."""
    bad = dec.clone()
    bad[1, int(torch.nonzero(~mask[1])[0])] = True
    bad[1, int(torch.nonzero(dec[1])[0])] = False
    assert int(bad[1].sum()) == int(dec[1].sum()) and bool((bad & ~mask).any())
    return bad


def test_decoded_token_visible_to_the_encoder_makes_the_loss_nan_or_raises():
    cfg = vo.TINY
    model = _model(cfg, vo.make_params(cfg))
    pixels, mask = vo.synthetic_batch(cfg, 2, 0, 0.75)
    dec = dr.every_second(mask)
    px, mk = pixels.to(dev), mask.to(dev)
    good = model(px, bool_masked_pos=mk, bool_decode_pos=dec.to(dev))
    assert torch.isfinite(good.loss)
    bad = _leaky(mask, dec).to(dev)
    out = model(px, bool_masked_pos=mk, bool_decode_pos=bad)
    assert torch.isnan(out.loss)                     # the status word of the index kernel, no host sync
    with pytest.raises(ValueError):                  # ... and the asynchronous check reports it on the following step
        model(px, bool_masked_pos=mk, bool_decode_pos=dec.to(dev))
    assert torch.isfinite(model(px, bool_masked_pos=mk, bool_decode_pos=dec.to(dev)).loss)
    model.strict_mask_check = True
    with pytest.raises(ValueError):
        model(px, bool_masked_pos=mk, bool_decode_pos=bad)
    uneven = dec.clone()
    uneven[1, int(torch.nonzero(dec[1])[0])] = False
    with pytest.raises(ValueError):                  # strict: another count in one clip raises on the spot
        model(px, bool_masked_pos=mk, bool_decode_pos=uneven.to(dev))


def test_decode_count_that_changes_at_one_shape_raises_on_the_following_step():
    cfg = vo.TINY
    model = _model(cfg, vo.make_params(cfg))
    pixels, mask = vo.synthetic_batch(cfg, 2, 0, 0.75)
    dec = dr.every_second(mask)
    px, mk = pixels.to(dev), mask.to(dev)
    assert torch.isfinite(model(px, bool_masked_pos=mk, bool_decode_pos=dec.to(dev)).loss)
    fewer = dec.clone()
    for b in range(2):
        fewer[b, int(torch.nonzero(dec[b])[0])] = False
    out = model(px, bool_masked_pos=mk, bool_decode_pos=fewer.to(dev))      # cached count: the library sees a wrong count
    assert torch.isnan(out.loss)
    with pytest.raises(ValueError):
        model(px, bool_masked_pos=mk, bool_decode_pos=fewer.to(dev))
    out = model(px, bool_masked_pos=mk, bool_decode_pos=fewer.to(dev))      # the cache entry is gone: counted anew
    assert torch.isfinite(out.loss) and model._ctx_key[3] == int(fewer[0].sum())


# ------------------------------------------------------------------ f
def test_deterministic_mode_gives_the_same_bits_twice():
    cfg, params, pixels, mask, dec, *_ = _case("ragged172")
    bvc.use_deterministic_algorithms(True)
    try:
        a = _one_step(cfg, params, pixels, mask, dec)
        b = _one_step(cfg, params, pixels, mask, dec)
    finally:
        bvc.use_deterministic_algorithms(False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert torch.isfinite(a[0]) and torch.isfinite(a[2]).all()


# ------------------------------------------------------------------ the index kernel on its own
def test_dual_mask_index_kernel_lists_and_status():
    B, L, nvis, ndec = 3, 196, 52, 61          # L is no multiple of the wave's 64 lanes
    g = torch.Generator().manual_seed(0)
    mask = torch.zeros(B, L, dtype=torch.bool)
    dec = torch.zeros(B, L, dtype=torch.bool)
    for b in range(B):
        perm = torch.randperm(L, generator=g)
        mask[b, perm[nvis:]] = True
        dec[b, perm[nvis:nvis + ndec]] = True

    def run(m, d):
        vis = torch.full((B, nvis), -1, dtype=torch.int32, device=dev)
        didx = torch.full((B, ndec), -1, dtype=torch.int32, device=dev)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        md, dd = m.to(dev).contiguous(), d.to(dev).contiguous()
        G.L.check(G.L.lib().bvc_op_dual_mask_index(md.data_ptr(), dd.data_ptr(), B, L, nvis, ndec, vis.data_ptr(), didx.data_ptr(),
                                                   status.data_ptr(), G.stream()), "bvc_op_dual_mask_index")
        torch.cuda.synchronize()
        return vis.cpu(), didx.cpu(), int(status[0])

    vis, didx, status = run(mask, dec)
    assert status == 0
    for b in range(B):
        assert torch.equal(vis[b].long(), torch.nonzero(~mask[b]).flatten())
        assert torch.equal(didx[b].long(), torch.nonzero(dec[b]).flatten())
    more = dec.clone()
    more[2, int(torch.nonzero(mask[2] & ~dec[2])[0])] = True          # one decoded token too many: nothing is written past the list
    vis, didx, status = run(mask, more)
    assert status == 1 and torch.equal(didx[2].long(), torch.nonzero(more[2]).flatten()[:ndec])
    assert run(mask, _leaky(mask, dec))[2] == 1                         # right count, one decoded token visible
    wrong_vis = mask.clone()
    wrong_vis[0, int(torch.nonzero(mask[0] & ~dec[0])[0])] = False      # one visible token too many
    assert run(wrong_vis, dec)[2] == 1
