"""Fine-tuning with Mixup / CutMix inside the patch gather: VideoMAEForVideoClassification.forward(..., mix=) against the same model
on the clips tests/mixup_ref.mix_clips composes, and against the fp32 CPU oracle.

CutMix only selects pixels, so the mixed forward and backward equal the unmixed ones on the composed clip bit for bit (deterministic
mode).  Mixup blends in f32 with a multiply-add the compiler may contract, so it is held to the bars of tests/test_gpu_videomae_cls.py
against the oracle fed the composed clip and the soft targets: loss 1e-3 relative, logits 2e-2, encoder gradients 5e-2 relative L2
with its floor, heads 2e-2.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from tests import mixup_ref as R   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402
from tests.test_gpu_videomae_cls import NL, _grad_errs, _heads, _model, _oracle   # noqa: E402
from tests.test_gpu_videomae import _log   # noqa: E402

bvc = G.bvc
dev = torch.device("cuda:0")
CFG = vo.TINY
B = 4
S = CFG.image_size
LABELS = torch.tensor([1, 4, 9, 4])


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(31)
    u8 = torch.randint(0, 256, (B, CFG.num_frames, CFG.num_channels, S, S), generator=g, dtype=torch.uint8)
    f32 = (u8.float() / 255.0 - 0.5) / 0.25
    return dict(u8=u8.to(dev), f32=f32, params=vo.make_params(CFG, seed=1), heads=_heads(CFG))


@pytest.fixture(autouse=True)
def deterministic():
    bvc.use_deterministic_algorithms(True)
    yield
    bvc.use_deterministic_algorithms(False)


def _soft_model(data):
    m = _model(CFG, data["params"], data["heads"])
    m.config.problem_type = "soft_label_classification"
    return m


def _cutmix():
    """a box whose edges cut 8-pixel runs and cross patch boundaries; the batch flipped"""
    box = (5, 43, 10, 37)
    mix = bvc.ClipMix([3, 2, 1, 0], [1.0] * B, [box] * B, image_size=(S, S), device=dev)
    soft = R.soft_targets(LABELS, mix.partner, mix.target_lam, NL, 0.1)
    return mix, soft


def _step(m, px, soft, mix):
    out = m(pixel_values=px, labels=soft.to(dev), mix=mix)
    out.loss.backward()
    torch.cuda.synchronize()
    return out.loss.detach().cpu(), out.logits.detach().cpu(), {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


def test_cutmix_on_uint8_equals_the_composed_clip_bitwise(data):
    mix, soft = _cutmix()
    assert mix.target_lam.tolist() == [1.0 - (38 * 27) / float(S * S)] * B
    composed = R.mix_clips(data["f32"], mix.partner, mix.lam, mix.box).to(dev)
    loss_a, logits_a, grads_a = _step(_soft_model(data), data["u8"], soft, mix)
    loss_b, logits_b, grads_b = _step(_soft_model(data), composed, soft, None)
    assert torch.equal(logits_a, logits_b) and torch.equal(loss_a, loss_b)
    assert set(grads_a) == set(grads_b) and len(grads_a) > 4
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k
    # and it did mix: the unmixed clips give other logits
    assert not torch.equal(logits_a, _step(_soft_model(data), data["u8"], soft, None)[1])


def test_mixup_step_matches_the_oracle_on_the_composed_clip(data):
    lam = 0.7310586
    mix = bvc.ClipMix([3, 2, 1, 0], [lam] * B, [(0, 0, 0, 0)] * B, image_size=(S, S), device=dev)
    soft = R.soft_targets(LABELS, mix.partner, mix.target_lam, NL, 0.1)
    composed = R.mix_clips(data["f32"], mix.partner, mix.lam, mix.box)
    ref_loss, ref_logits, ref_grads = _oracle(CFG, data["params"], data["heads"], composed,
                                              lambda z: torch.sum(-soft * torch.log_softmax(z, -1), -1).mean())
    m = _soft_model(data)
    loss, logits, _ = _step(m, data["u8"], soft, mix)
    rel = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    el = G.rel_err(logits, ref_logits)
    _log(f"[cls_mixup] loss hip {float(loss):.7f} oracle {float(ref_loss):.7f} rel {rel:.2e}; logits rel {el:.2e}")
    assert rel < 1e-3 and el < 2e-2
    _grad_errs(m, ref_grads, "cls_mixup")


def test_mix_is_consumed_not_sticky(data):
    mix, soft = _cutmix()
    m = _soft_model(data)
    mixed = m(pixel_values=data["u8"], mix=mix).logits.detach().cpu()
    after = m(pixel_values=data["u8"]).logits.detach().cpu()
    never = _soft_model(data)(pixel_values=data["u8"]).logits.detach().cpu()
    assert torch.equal(after, never) and not torch.equal(mixed, never)


def test_linear_probe_and_no_grad_paths_honour_the_mix(data):
    mix, soft = _cutmix()
    train = _soft_model(data)(pixel_values=data["u8"], mix=mix).logits.detach().cpu()
    m = _soft_model(data)
    for p in m.videomae.parameters():
        p.requires_grad = False
    out = m(pixel_values=data["u8"], labels=soft.to(dev), mix=mix)          # frozen encoder, train mode: the forward-only context
    assert m._train.h is None and out.logits.requires_grad
    out.loss.backward()
    assert m.classifier.weight.grad is not None and m.fc_norm.weight.grad is not None
    assert torch.equal(out.logits.detach().cpu(), train)
    m2 = _soft_model(data)
    with torch.no_grad():
        assert torch.equal(m2(pixel_values=data["u8"], mix=mix).logits.cpu(), train)
    assert m2._train.h is None


def test_mixup_object_end_to_end(data):
    """bvc.Mixup's own output drives a step: finite loss, soft targets on the device, host-readable spec"""
    mixup = bvc.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", label_smoothing=0.1, num_classes=NL, generator=np.random.default_rng(0))
    mix, soft = mixup(B, LABELS.to(dev), image_size=(S, S), device=dev)
    assert soft.is_cuda and soft.shape == (B, NL) and mix.table.is_cuda and mix.table.shape == (B, 6)
    assert mix.table.cpu()[:, 0].tolist() == mix.partner.tolist() and mix.table.cpu()[:, 2:].tolist() == mix.box.tolist()
    assert torch.equal(mix.table.cpu()[:, 1].contiguous().view(torch.float32), torch.from_numpy(mix.lam))
    m = _soft_model(data)
    loss, logits, grads = _step(m, data["u8"], soft, mix)
    composed = R.mix_clips(data["f32"], mix.partner, mix.lam, mix.box).to(dev)
    ref = _step(_soft_model(data), composed, soft, None)
    assert torch.isfinite(loss) and G.rel_err(logits, ref[1]) < 2e-2


def test_eval_mode_and_wrong_batch_raise(data):
    mix, soft = _cutmix()
    m = _soft_model(data)
    m.eval()
    with pytest.raises(ValueError, match="eval mode"):
        m(pixel_values=data["u8"], mix=mix)
    m.train()
    with pytest.raises(ValueError, match="batch of 4"):
        m(pixel_values=data["u8"][:3], mix=mix)
    with pytest.raises(ValueError, match="device table"):
        m(pixel_values=data["u8"], mix=bvc.ClipMix([3, 2, 1, 0], [1.0] * B, [(0, 0, 0, 0)] * B))
    # the library refuses the mismatch too: armed for 4, the forward has 3
    m(pixel_values=data["u8"])                     # the fine-tuning context exists, sized for 4 clips
    h = m._get_train_ctx(B)
    L = bvc._lib
    L.check(L.lib().bvc_videomae_cls_set_mix(h, mix.table.data_ptr(), B, L.current_stream_ptr()), "set_mix")
    with pytest.raises(L.BvcError, match="mix was set for 4"):
        m(pixel_values=data["u8"][:3])
    assert torch.isfinite(m(pixel_values=data["u8"][:3]).logits).all()       # and the refusal disarmed it
