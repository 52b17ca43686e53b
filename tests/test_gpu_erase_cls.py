"""Fine-tuning with random erasing inside the patch gather: VideoMAEForVideoClassification.forward(..., erase=) on uint8 clips against
the same model on the f32 clip that tests/erase_ref.erase_clips composes from the device's own noise (bvc.erase_noise).

Erasing only selects values - a source pixel, a zero or a noise value - so the erased forward and backward equal the plain ones on the
composed clip bit for bit (deterministic mode), alone and with a CutMix armed as well (erase each clip, then mix the batch).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from tests import erase_ref as E   # noqa: E402
from tests import mixup_ref as R   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402
from tests.test_gpu_videomae_cls import NL, _heads, _model   # noqa: E402

bvc = G.bvc
dev = torch.device("cuda:0")
CFG = vo.TINY
B = 4
S = CFG.image_size
T, C = CFG.num_frames, CFG.num_channels
LABELS = torch.tensor([1, 4, 9, 4])
SEED, OFFSET = 0x51ED270B1A2B3C4D, 11
# clip 0: a box whose edges cut 8-pixel runs and cross patch boundaries; clip 1 untouched; clip 2 two overlapping boxes; clip 3 the border
BOXES = [[(5, 43, 10, 37), (0, 0, 0, 0)], [(0, 0, 0, 0), (0, 0, 0, 0)], [(16, 32, 0, 48), (20, 60, 30, 34)], [(0, S, S - 9, S), (S - 3, S, 0, S)]]


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(31)
    u8 = torch.randint(0, 256, (B, T, C, S, S), generator=g, dtype=torch.uint8)
    f32 = (u8.float() / 255.0 - 0.5) / 0.25
    noise = bvc.erase_noise(SEED, OFFSET, "pixel", B, T, C, S, S, dev).cpu()
    colours = bvc.erase_noise(SEED, OFFSET, "rand", B, T, C, S, S, dev).cpu()
    return dict(u8=u8.to(dev), f32=f32, noise=noise, colours=colours, params=vo.make_params(CFG, seed=1), heads=_heads(CFG))


@pytest.fixture(autouse=True)
def deterministic():
    bvc.use_deterministic_algorithms(True)
    yield
    bvc.use_deterministic_algorithms(False)


def _soft_model(data):
    m = _model(CFG, data["params"], data["heads"])
    m.config.problem_type = "soft_label_classification"
    return m


def _erase(mode="pixel", boxes=BOXES):
    return bvc.ClipErase(boxes, mode, seed=SEED, offset=OFFSET, image_size=(S, S), device=dev)


def _composed(data, er, mix=None):
    x = E.erase_clips(data["f32"], er.boxes, er.modes, data["noise"], data["colours"])
    if mix is not None:
        x = R.mix_clips(x, mix.partner, mix.lam, mix.box)
    return x.to(dev)


def _cutmix():
    mix = bvc.ClipMix([3, 2, 1, 0], [1.0] * B, [(8, 50, 20, 45)] * B, image_size=(S, S), device=dev)      # intersects the partners' boxes
    return mix, R.soft_targets(LABELS, mix.partner, mix.target_lam, NL, 0.1)


def _step(m, px, soft, mix=None, erase=None):
    out = m(pixel_values=px, labels=soft.to(dev), mix=mix, erase=erase)
    out.loss.backward()
    torch.cuda.synchronize()
    return out.loss.detach().cpu(), out.logits.detach().cpu(), {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


def _same_step(a, b):
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    assert set(a[2]) == set(b[2]) and len(a[2]) > 4
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_pixel_erasing_on_uint8_equals_the_composed_clip_bitwise(data):
    assert S % 16 == 0 and S >= 64
    er = _erase()
    soft = R.smooth(LABELS, NL, 0.1)
    erased = _step(_soft_model(data), data["u8"], soft, erase=er)
    _same_step(erased, _step(_soft_model(data), _composed(data, er), soft))
    # and it did erase: the plain clips give other logits
    assert not torch.equal(erased[1], _step(_soft_model(data), data["u8"], soft)[1])


def test_erasing_then_cutmix_equals_the_composed_clip_bitwise(data):
    er = bvc.ClipErase(BOXES, [[2, 2], [2, 2], [1, 2], [0, 1]], seed=SEED, offset=OFFSET, image_size=(S, S), device=dev)
    mix, soft = _cutmix()
    both = _step(_soft_model(data), data["u8"], soft, mix=mix, erase=er)
    _same_step(both, _step(_soft_model(data), _composed(data, er, mix), soft))
    only_mix = _step(_soft_model(data), data["u8"], soft, mix=mix)
    assert not torch.equal(both[1], only_mix[1])


def test_encoder_context_gives_the_same_embeddings(data):
    er = _erase()
    mix, _ = _cutmix()
    for mx in (None, mix):
        ref = _soft_model(data)(pixel_values=_composed(data, er, mx), output_last_hidden_state=True)
        m = _soft_model(data)
        with torch.no_grad():                                          # train mode without a graph: the forward-only context
            out = m(pixel_values=data["u8"], mix=mx, erase=er, output_last_hidden_state=True)
        assert m._train.h is None
        assert torch.equal(out.logits, ref.logits.detach()) and torch.equal(out.last_hidden_state, ref.last_hidden_state)
        frozen = _soft_model(data)
        for p in frozen.videomae.parameters():
            p.requires_grad = False
        probe = frozen(pixel_values=data["u8"], mix=mx, erase=er)     # the linear probe's path
        assert frozen._train.h is None and probe.logits.requires_grad
        assert torch.equal(probe.logits.detach(), ref.logits.detach())


def test_erase_is_consumed_not_sticky(data):
    er = _erase()
    m = _soft_model(data)
    erased = m(pixel_values=data["u8"], erase=er).logits.detach().cpu()
    after = m(pixel_values=data["u8"]).logits.detach().cpu()
    never = _soft_model(data)(pixel_values=data["u8"]).logits.detach().cpu()
    assert torch.equal(after, never) and not torch.equal(erased, never)
    # the two states are independent: a mix alone after an erase alone is the mix alone
    mix, _ = _cutmix()
    assert torch.equal(m(pixel_values=data["u8"], mix=mix).logits.detach().cpu(), _soft_model(data)(pixel_values=data["u8"], mix=mix).logits.detach().cpu())


def test_bad_entry_gives_nan_logits_and_the_next_forward_is_finite(data):
    m = _soft_model(data)
    outside = [[(0, S + 1, 0, 8)]] + [[(0, 8, 0, 8)]] * 3
    for bad in (_erase(boxes=outside), _erase(mode=[[2], [2], [2], [3]], boxes=[[(0, 8, 0, 8)]] * B)):
        out = m(pixel_values=data["u8"], erase=bad, output_last_hidden_state=True)
        assert torch.isnan(out.logits).all() and torch.isnan(out.last_hidden_state).all()
        assert torch.isfinite(m(pixel_values=data["u8"], erase=_erase()).logits).all()
        assert torch.isfinite(m(pixel_values=data["u8"]).logits).all()
    # a bad erase entry under a whole-image CutMix, where no pixel of the bad clip's own is read
    whole = bvc.ClipMix([3, 2, 1, 0], [1.0] * B, [(0, S, 0, S)] * B, image_size=(S, S), device=dev)
    assert torch.isnan(m(pixel_values=data["u8"], mix=whole, erase=_erase(boxes=outside)).logits).all()
    assert torch.isfinite(m(pixel_values=data["u8"], mix=whole, erase=_erase()).logits).all()


def test_eval_mode_and_wrong_batch_raise(data):
    er = _erase()
    m = _soft_model(data)
    m.eval()
    with pytest.raises(ValueError, match="eval mode"):
        m(pixel_values=data["u8"], erase=er)
    m.train()
    with pytest.raises(ValueError, match="batch of 4"):
        m(pixel_values=data["u8"][:3], erase=er)
    with pytest.raises(ValueError, match="device table"):
        m(pixel_values=data["u8"], erase=bvc.ClipErase(BOXES, "pixel"))
    # the library refuses the mismatch too: armed for 4, the forward has 3; more than 4 boxes per clip; and a refusal disarms
    m(pixel_values=data["u8"])
    h = m._get_train_ctx(B)
    L = bvc._lib
    L.check(L.lib().bvc_videomae_cls_set_erase(h, er.table.data_ptr(), B, er.num_boxes, SEED, OFFSET, L.current_stream_ptr()), "set_erase")
    with pytest.raises(L.BvcError, match="erase was set for 4"):
        m(pixel_values=data["u8"][:3])
    assert L.lib().bvc_videomae_cls_set_erase(h, er.table.data_ptr(), B, 5, SEED, OFFSET, L.current_stream_ptr()) != 0
    assert L.lib().bvc_videomae_cls_set_erase(h, er.table.data_ptr(), B + 1, 2, SEED, OFFSET, L.current_stream_ptr()) != 0
    plain = _soft_model(data)(pixel_values=data["u8"][:3]).logits
    assert torch.equal(m(pixel_values=data["u8"][:3]).logits, plain)
    L.check(L.lib().bvc_videomae_cls_set_erase(h, er.table.data_ptr(), 3, er.num_boxes, SEED, OFFSET, L.current_stream_ptr()), "set_erase")
    L.check(L.lib().bvc_videomae_cls_set_erase(h, None, 0, 0, 0, 0, L.current_stream_ptr()), "set_erase")       # NULL disarms
    assert torch.equal(m(pixel_values=data["u8"][:3]).logits, plain)
