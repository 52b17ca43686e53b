"""tests/dual_mask_ref.py (the fp32 reference of the decoder-subset step that the GPU tests use) pinned on the CPU, the mask generator,
and the library's argument checks that need no GPU.

Bars: decode-all is the oracle's own step, bit for bit; a strict subset agrees with transformers' own modules composed by hand to
1e-5 relative (fp32 round-off of two implementations of the same arithmetic; 2.4e-7 measured)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import videomae_oracle as vo
from tests import dual_mask_ref as dr


def test_decode_all_is_the_oracle_step_bit_for_bit():
    cfg = vo.TINY
    params = vo.make_params(cfg, seed=0)
    pixels, mask = vo.synthetic_batch(cfg, 3, 0, 0.9)
    t0, t1 = {}, {}
    l0, g0 = vo.step(cfg, params, pixels, mask, taps=t0)
    l1, g1 = dr.step(cfg, params, pixels, mask, mask.clone(), taps=t1)
    assert torch.equal(l0, l1)
    assert set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert set(t0) == set(t1) and all(torch.equal(t0[k], t1[k]) for k in t0)


def test_strict_subset_matches_transformers_modules_composed_by_hand():
    transformers = pytest.importorskip("transformers")
    cfg, B = vo.TINY, 3
    params = vo.make_params(cfg, seed=0)
    pixels, mask = vo.synthetic_batch(cfg, B, 0, 0.9)
    dec = dr.every_second(mask)
    ndec = int(dec[0].sum())
    assert 0 < ndec < int(mask[0].sum()) and bool((dec.sum(1) == ndec).all()) and not bool((dec & ~mask).any())
    tc = transformers.VideoMAEConfig(
        image_size=cfg.image_size, patch_size=cfg.patch_size, num_channels=cfg.num_channels, num_frames=cfg.num_frames,
        tubelet_size=cfg.tubelet_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size, use_mean_pooling=True,
        decoder_num_attention_heads=cfg.decoder_num_attention_heads, decoder_hidden_size=cfg.decoder_hidden_size,
        decoder_num_hidden_layers=cfg.decoder_num_hidden_layers, decoder_intermediate_size=cfg.decoder_intermediate_size,
        norm_pix_loss=cfg.norm_pix_loss, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    hf = transformers.VideoMAEForPreTraining(tc)
    res = hf.load_state_dict(params)
    assert not res.missing_keys and not res.unexpected_keys
    hf.eval()
    with torch.no_grad():
        x = hf.encoder_to_decoder(hf.videomae(pixels, bool_masked_pos=mask).last_hidden_state)
        Dd = x.shape[-1]
        pos = hf.position_embeddings.expand(B, -1, -1).type_as(pixels)
        x = torch.cat([x + pos[~mask].reshape(B, -1, Dd), hf.mask_token + pos[dec].reshape(B, -1, Dd)], dim=1)
        ref = hf.decoder(x, return_token_num=ndec).logits
        loss, logits, labels = dr.forward(cfg, params, pixels, mask, dec)
    assert tuple(logits.shape) == (B, ndec, cfg.patch_dim) == tuple(ref.shape) == tuple(labels.shape)
    e = float((logits - ref).norm() / ref.norm())
    print(f"dual-mask reference vs transformers composition: logits rel {e:.2e}")
    assert e < 1e-5, e
    assert abs(float(loss) - float(torch.nn.functional.mse_loss(ref, labels))) / float(loss) < 1e-5


@pytest.mark.parametrize("grid,mask_ratio,decode_ratio", [((8, 14, 14), 0.9, 0.5), ((8, 14, 14), 0.9, 0.25), ((4, 7, 7), 0.75, 0.84)])
def test_decoder_subset_generator(bvc, grid, mask_ratio, decode_ratio):
    slots, per = grid[0], grid[1] * grid[2]
    tube = bvc.TubeMaskingGenerator(grid, mask_ratio, rng=np.random.RandomState(3))
    gen = bvc.DecoderSubsetGenerator(grid, decode_ratio, rng=np.random.RandomState(5))
    keep = int(decode_ratio * int(mask_ratio * per))
    rows = []
    for _ in range(3):
        m = tube()
        d = gen(m)
        assert d.shape == (slots * per,) and d.dtype == np.float64 and set(np.unique(d)) <= {0.0, 1.0}
        assert not np.any((d != 0) & (m == 0))                              # a subset of the mask
        per_slot = d.reshape(slots, per).sum(axis=1)
        assert (per_slot == keep).all(), per_slot                           # exactly the stated count in every slot
        rows.append(d)
        by_slot = d.reshape(slots, per)
        assert sum(1 for t in range(1, slots) if not np.array_equal(by_slot[t], by_slot[0])) >= 1      # the draw is fresh per slot
    assert len({int(r.sum()) for r in rows}) == 1                           # every clip decodes the same number
    assert int(rows[0].sum()) == slots * keep


def test_decoder_subset_generator_draws_from_numpy_global_rng_and_rejects_bad_input(bvc):
    grid = (4, 4, 4)
    m = bvc.TubeMaskingGenerator(grid, 0.75, rng=np.random.RandomState(0))()
    np.random.seed(11)
    a = bvc.DecoderSubsetGenerator(grid, 0.5)(m)
    np.random.seed(11)
    b = bvc.DecoderSubsetGenerator(grid, 0.5)(m)
    assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        bvc.DecoderSubsetGenerator(grid, 0.0)
    with pytest.raises(ValueError):
        bvc.DecoderSubsetGenerator(grid, 0.01)(m)          # keeps none of the 12 masked positions of a slot
    ragged = m.copy()
    ragged[np.flatnonzero(ragged)[0]] = 0
    with pytest.raises(ValueError):
        bvc.DecoderSubsetGenerator(grid, 0.5)(ragged)


def test_create_dual_refuses_bad_decode_counts_without_a_gpu(bvc):
    L = bvc._lib.lib()
    kw = {k: v for k, v in vo.TINY.__dict__.items() if k != "decoder_norm_eps"}
    cc = bvc.VideoMAEConfig(**kw).to_c()
    nmask = 4 * int(0.75 * 16) // 2      # TINY: 2 slots of 16 positions, 12 masked each
    assert nmask == 24
    for ndec in (0, -1, nmask + 1):
        h = ctypes.c_void_p()
        assert L.bvc_videomae_create_dual(ctypes.byref(cc), 2, nmask, ndec, ctypes.byref(h)) != 0
        assert h.value is None
        assert b"num_decoded" in L.bvc_last_error()


def test_forward_signature_takes_the_decode_mask_before_output_logits(bvc):
    import inspect
    names = list(inspect.signature(bvc.VideoMAEForPreTraining.forward).parameters)
    assert names[:5] == ["self", "pixel_values", "bool_masked_pos", "bool_decode_pos", "output_logits"]


def test_distributed_data_parallel_passes_the_decode_mask_through(bvc, tmp_path):
    """One gloo rank in this process, a stub module that records what it is called with: the wrapper hands bool_decode_pos (and the
    other arguments) to the module as the very objects it was given, and the backward through it still runs."""
    import torch.distributed as dist

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(()))
            self.seen = None

        def forward(self, pixel_values, bool_masked_pos=None, bool_decode_pos=None, output_logits=False):
            self.seen = (pixel_values, bool_masked_pos, bool_decode_pos, output_logits)
            return self.w * pixel_values.sum()

    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/rendezvous", rank=0, world_size=1)
    try:
        stub = Stub()
        wrapped = bvc.DistributedDataParallel(stub)
        px, mask = torch.ones(2, 3), torch.tensor([[True, True, False], [True, False, True]])
        dec = torch.tensor([[True, False, False], [False, False, True]])
        loss = wrapped(px, bool_masked_pos=mask, bool_decode_pos=dec, output_logits=True)
        assert stub.seen[0] is px and stub.seen[1] is mask and stub.seen[2] is dec and stub.seen[3] is True
        loss.backward()
        assert float(stub.w.grad) == 6.0
        wrapped(px, bool_masked_pos=mask)
        assert stub.seen[2] is None and stub.seen[3] is False
    finally:
        dist.destroy_process_group()
