"""Mixup / CutMix on the host: the plan ``bvc.Mixup`` draws (partners, boxes, weights, soft targets) and the soft-target loss.
No GPU: ``device="cpu"`` yields host tensors and no library call."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mixup_ref as R

H, W, K = 64, 48, 10


def _labels(B):
    return (torch.arange(B) * 3) % K


def _mixup(bvc, seed=0, **kw):
    args = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1, num_classes=K,
                generator=np.random.default_rng(seed))
    args.update(kw)
    return bvc.Mixup(**args)


@pytest.mark.parametrize("B", [4, 5])
def test_partner_is_the_flipped_batch(bvc, B):
    mix, soft = _mixup(bvc, cutmix_alpha=0.0)(B, _labels(B), image_size=(H, W), device="cpu")
    assert mix.table is None and soft.device.type == "cpu" and soft.dtype == torch.float32 and soft.shape == (B, K)
    assert mix.partner.tolist() == [B - 1 - b for b in range(B)]
    assert mix.batch_size == B and mix.lam.dtype == np.float32 and mix.box.shape == (B, 4)
    assert (mix.box == 0).all() and (mix.lam < 1).all() and len(set(mix.lam.tolist())) == 1      # Mixup, one weight per batch
    assert torch.allclose(soft, R.soft_targets(_labels(B), mix.partner, mix.lam, K, 0.1), atol=1e-7)


def test_cutmix_boxes_lie_in_the_image_and_lam_is_the_clipped_area(bvc):
    m = _mixup(bvc, seed=3, mixup_alpha=0.0, mode="elem")
    clipped = 0
    for _ in range(20):
        mix, soft = m(6, _labels(6), image_size=(H, W), device="cpu")
        y0, y1, x0, x1 = mix.box.T
        assert (0 <= y0).all() and (y0 <= y1).all() and (y1 <= H).all() and (0 <= x0).all() and (x0 <= x1).all() and (x1 <= W).all()
        assert (mix.lam == 1.0).all()                       # the table's blend weight: selection only
        area = (y1 - y0).astype(np.int64) * (x1 - x0)
        assert np.array_equal(mix.target_lam, 1.0 - area / float(H * W))          # exactly
        clipped += int(((y0 == 0) | (y1 == H) | (x0 == 0) | (x1 == W)).sum())
        assert torch.allclose(soft, R.soft_targets(_labels(6), mix.partner, mix.target_lam, K, 0.1), atol=1e-6)
    assert clipped > 0      # the draws did reach the image border, so the correction was exercised


def test_cutmix_box_follows_the_recipe(bvc):
    from bvc_amd.mixup import cutmix_box
    (y0, y1, x0, x1), lam = cutmix_box(0.75, 10, 40, H, W)       # r = 0.5: ch = 32, cw = 24
    assert (y0, y1, x0, x1) == (0, 26, 28, 48) and lam == 1.0 - (26 * 20) / float(H * W)
    # the same draws by hand
    g = np.random.default_rng(11)
    m = _mixup(bvc, seed=11, mixup_alpha=0.0)
    mix, _ = m(2, _labels(2), image_size=(H, W), device="cpu")
    assert g.random() < 1.0
    lam0 = g.beta(1.0, 1.0)
    cy, cx = int(g.integers(0, H)), int(g.integers(0, W))
    box, lam = cutmix_box(lam0, cy, cx, H, W)
    assert mix.box.tolist() == [list(box)] * 2 and mix.target_lam.tolist() == [lam] * 2


def test_prob_zero_is_the_identity_and_plain_smoothed_labels(bvc):
    for mode in ("batch", "elem"):
        mix, soft = _mixup(bvc, prob=0.0, mode=mode)(5, _labels(5), image_size=(H, W), device="cpu")
        assert mix.partner.tolist() == list(range(5)) and (mix.lam == 1.0).all() and (mix.box == 0).all()
        assert torch.equal(soft, R.smooth(_labels(5), K, 0.1))


def test_elem_mode_draws_per_clip(bvc):
    mix, soft = _mixup(bvc, seed=5, mode="elem")(8, _labels(8), image_size=(H, W), device="cpu")
    specs = {(float(l), tuple(b)) for l, b in zip(mix.lam.tolist(), mix.box.tolist())}
    assert len(specs) > 1
    assert (mix.lam < 1).any() and (mix.box != 0).any()          # both kinds occur under switch_prob = 0.5 with this seed
    assert mix.partner.tolist() == [7 - b for b in range(8)]
    # batch mode: one spec
    mix, _ = _mixup(bvc, seed=5)(8, _labels(8), image_size=(H, W), device="cpu")
    assert len({(float(l), tuple(b)) for l, b in zip(mix.lam.tolist(), mix.box.tolist())}) == 1


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_soft_target_rows_sum_to_one(bvc, mode):
    m = _mixup(bvc, seed=9, mode=mode)
    for B in (1, 4, 7):
        _, soft = m(B, _labels(B), image_size=(H, W), device="cpu")
        assert torch.allclose(soft.sum(1), torch.ones(B), atol=1e-6) and (soft >= 0).all()


def test_bad_arguments(bvc):
    with pytest.raises(ValueError):
        _mixup(bvc, mode="pair")
    with pytest.raises(ValueError):
        _mixup(bvc, mixup_alpha=0.0, cutmix_alpha=0.0)
    with pytest.raises(ValueError):
        _mixup(bvc)(4, _labels(3), image_size=(H, W), device="cpu")
    with pytest.raises(ValueError):
        bvc.ClipMix([0, 1], [1.0], [[0, 0, 0, 0]] * 2)


def test_clipmix_built_by_hand(bvc):
    mix = bvc.ClipMix([1, 0], [1.0, 0.25], [[0, 32, 0, 24], [0, 0, 0, 0]], image_size=(H, W))
    assert mix.table is None and mix.batch_size == 2
    assert mix.target_lam.tolist() == [1.0 - (32 * 24) / float(H * W), 0.25]


def test_mix_clips_reference():
    g = torch.Generator().manual_seed(0)
    px = torch.randn(3, 2, 3, 8, 8, generator=g)
    out = R.mix_clips(px, [2, 1, 0], [1.0, 1.0, 0.25], [(2, 6, 1, 5), (0, 0, 0, 0), (0, 8, 0, 4)])
    assert torch.equal(out[0, :, :, 2:6, 1:5], px[2, :, :, 2:6, 1:5]) and torch.equal(out[0, :, :, :2], px[0, :, :, :2])
    assert torch.equal(out[1], px[1])
    assert torch.equal(out[2, :, :, :, :4], px[0, :, :, :, :4])
    assert torch.equal(out[2, :, :, :, 4:], 0.25 * px[2, :, :, :, 4:] + 0.75 * px[0, :, :, :, 4:])


def test_soft_target_cross_entropy_is_torchs_probability_target_form(bvc):
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(6, K, generator=g) * 3
    _, soft = _mixup(bvc, seed=2, mode="elem")(6, _labels(6), image_size=(H, W), device="cpu")
    assert abs(float(bvc.soft_target_cross_entropy(logits, soft)) - float(F.cross_entropy(logits, soft))) < 1e-6
    onehot = F.one_hot(_labels(6), K).float()
    assert abs(float(bvc.soft_target_cross_entropy(logits, onehot)) - float(F.cross_entropy(logits, _labels(6)))) < 1e-6
    with pytest.raises(ValueError):
        bvc.soft_target_cross_entropy(logits, soft[:, :5])


def test_classification_loss_soft_labels_are_never_inferred(bvc):
    from types import SimpleNamespace
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(4, K, generator=g)
    _, soft = _mixup(bvc, seed=6)(4, _labels(4), image_size=(H, W), device="cpu")
    cfg = SimpleNamespace(num_labels=K, problem_type=None)
    loss = bvc.videomae.classification_loss(cfg, logits, soft)          # float labels, nothing said: BCE, as in transformers
    assert cfg.problem_type == "multi_label_classification"
    assert torch.equal(loss, F.binary_cross_entropy_with_logits(logits, soft))
    assert bvc.videomae.infer_problem_type(K, soft) == "multi_label_classification"
    cfg = SimpleNamespace(num_labels=K, problem_type="soft_label_classification")
    loss = bvc.videomae.classification_loss(cfg, logits, soft)
    assert cfg.problem_type == "soft_label_classification"
    assert abs(float(loss) - float(F.cross_entropy(logits, soft))) < 1e-6


def test_eval_mode_refuses_a_mix(bvc):
    m = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(image_size=32, num_frames=2, hidden_size=64, num_hidden_layers=1,
                                                             num_attention_heads=1, intermediate_size=64, num_labels=K)).eval()
    mix = bvc.ClipMix([1, 0], [1.0, 1.0], [[0, 8, 0, 8]] * 2, image_size=(32, 32))
    with pytest.raises(ValueError, match="eval mode"):
        m(pixel_values=torch.zeros(2, 2, 3, 32, 32), mix=mix)
