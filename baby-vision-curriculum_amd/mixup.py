"""Mixup / CutMix with label smoothing for fine-tuning: the host side of the mix inside the patch gather (include/bvc.h, bvc_clip_mix).

``Mixup`` draws, per batch, what the published VideoMAE fine-tuning recipe draws - a Mixup weight or a CutMix box per batch or per
clip - and hands back two things: a ``ClipMix`` (one table entry per clip: partner, weight, box) that
``VideoMAEForVideoClassification.forward(..., mix=)`` gives to the library, where the patch gather composes the two clips while it
reads them (uint8 or f32; the mixed clip is never written), and the soft targets for ``problem_type="soft_label_classification"``.
The draws are host-side (a ``numpy.random.Generator``), like the mask generators': no device sync.
"""
import numpy as np
import torch


def smooth_one_hot(labels, num_classes, smoothing):
    """[B] integer labels -> [B, K] f32: 1 - s + s / K on the class, s / K elsewhere."""
    labels = labels.long().view(-1, 1)
    out = torch.full((labels.shape[0], int(num_classes)), float(smoothing) / int(num_classes), dtype=torch.float32, device=labels.device)
    return out.scatter_(1, labels, 1.0 - float(smoothing) + float(smoothing) / int(num_classes))


def soft_targets(labels, partner, lam, num_classes, smoothing):
    """soft[b] = lam[b] * smooth(y[b]) + (1 - lam[b]) * smooth(y[partner[b]]) in f32; ``partner`` (int64) and ``lam`` (f32) on
    ``labels``' device."""
    y = smooth_one_hot(labels, num_classes, smoothing)
    w = lam.to(torch.float32).view(-1, 1)
    return w * y + (1.0 - w) * y[partner.long()]


def cutmix_box(lam0, cy, cx, H, W):
    """The recipe's box for a drawn weight and centre, clipped to the image: (y0, y1, x0, x1) and the weight corrected to the area
    that survived clipping, 1 - box_area / (H * W)."""
    r = np.sqrt(1.0 - lam0)
    ch, cw = int(H * r), int(W * r)
    y0, y1 = int(np.clip(cy - ch // 2, 0, H)), int(np.clip(cy + ch // 2, 0, H))
    x0, x1 = int(np.clip(cx - cw // 2, 0, W)), int(np.clip(cx + cw // 2, 0, W))
    return (y0, y1, x0, x1), 1.0 - ((y1 - y0) * (x1 - x0)) / float(H * W)


class ClipMix:
    """The mix of one batch: per clip ``partner`` (int32 [B]), ``lam`` (f32 [B], the blend weight outside the box: 1 for CutMix
    and for an unmixed clip) and ``box`` (int32 [B, 4]: rows [y0, y1) x columns [x0, x1) of every frame that come from the partner) -
    numpy arrays on the host, readable without a sync - and ``table``, the same as the library's device table ([B, 6] int32, the
    weight's bits in column 1), or None when built for the CPU.  ``target_lam`` (f64 [B]) is the weight of the clip's own label in the
    soft target: ``lam`` for Mixup, 1 - box_area / (H * W) for CutMix; ``partner_dev`` / ``target_lam_dev`` are its device copies (views of
    the allocation ``table`` lives in: one asynchronous upload from pinned memory for all three)."""

    def __init__(self, partner, lam, box, image_size=None, device=None, target_lam=None):
        self.partner = np.ascontiguousarray(partner, dtype=np.int32).reshape(-1)
        B = self.partner.shape[0]
        self.lam = np.ascontiguousarray(lam, dtype=np.float32).reshape(-1)
        self.box = np.ascontiguousarray(box, dtype=np.int32).reshape(-1, 4)
        if self.lam.shape[0] != B or self.box.shape[0] != B:
            raise ValueError(f"ClipMix: partner, lam and box must have one entry per clip ({B}, {self.lam.shape[0]}, {self.box.shape[0]})")
        self.image_size = tuple(int(v) for v in image_size) if image_size is not None else None
        if target_lam is None:
            target_lam = self.lam.astype(np.float64)
            if self.image_size is not None:
                area = (self.box[:, 1] - self.box[:, 0]).clip(min=0) * (self.box[:, 3] - self.box[:, 2]).clip(min=0)
                target_lam = target_lam * (1.0 - area / float(self.image_size[0] * self.image_size[1]))
        self.target_lam = np.asarray(target_lam, dtype=np.float64).reshape(-1)
        self.table = self.partner_dev = self.target_lam_dev = None
        device = torch.device(device) if device is not None else None
        if device is not None and device.type != "cpu":
            # one pinned staging block and one asynchronous copy for everything the device needs (a pageable copy would make the
            # host wait for the stream to drain, every step): [table 6 B | target_lam as f32 B | partner B] int32
            host = torch.empty(8 * B, dtype=torch.int32, pin_memory=True)
            h = host.numpy()
            t = h[:6 * B].reshape(B, 6)
            t[:, 0] = self.partner
            t[:, 1] = self.lam.view(np.int32)
            t[:, 2:] = self.box
            h[6 * B:7 * B] = self.target_lam.astype(np.float32).view(np.int32)
            h[7 * B:] = self.partner
            d = host.to(device, non_blocking=True)
            self.table = d[:6 * B].view(B, 6)
            self.target_lam_dev = d[6 * B:7 * B].view(torch.float32)
            self.partner_dev = d[7 * B:]

    @property
    def batch_size(self):
        return int(self.partner.shape[0])

    def __repr__(self):
        return f"ClipMix(batch_size={self.batch_size}, device={self.table.device if self.table is not None else 'cpu'})"


class Mixup:
    """Mixup / CutMix of a batch of clips with label smoothing, with the interface of the published recipe:

        mixup = bvc.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1,
                          num_classes=K, generator=np.random.default_rng(seed))
        mix, soft = mixup(B, labels, image_size=(H, W), device=pixels.device)
        out = model(pixel_values=pixels, labels=soft, mix=mix)      # config.problem_type = "soft_label_classification"

    Rules:
      * the partner of clip b is B - 1 - b (the batch flipped); with an odd B the middle clip is its own partner;
      * mode "batch": with probability ``prob`` the batch is mixed at all, otherwise every entry is the identity (partner b, lam 1,
        empty box); when both alphas are positive CutMix is chosen with probability ``switch_prob`` (with one positive alpha, that
        one); one weight / box serves the whole batch.  mode "elem" draws all of this per clip.  Draw order per decision:
        ``random()`` against ``prob``, ``random()`` against ``switch_prob`` (only when both alphas are positive), ``beta(a, a)``, and for
        CutMix ``integers(0, H)``, ``integers(0, W)``;
      * Mixup: lam ~ Beta(a, a), a = ``mixup_alpha``; table entry (partner, lam, empty box);
      * CutMix: lam0 ~ Beta(a, a), a = ``cutmix_alpha``; r = sqrt(1 - lam0), ch = int(H r), cw = int(W r), cy ~ integers(0, H),
        cx ~ integers(0, W); the box is [clip(cy - ch // 2), clip(cy + ch // 2)) x [clip(cx - cw // 2), clip(cx + cw // 2)), clipped
        to the image, the same in every frame; the target weight is corrected to the box that survived clipping,
        lam = 1 - box_area / (H W); the table's lam field is 1.0;
      * soft target: soft[b] = lam_b * smooth(y[b]) + (1 - lam_b) * smooth(y[partner]), where smooth puts 1 - s + s / K on the
        class and s / K elsewhere (s = ``label_smoothing``);
      * data parallel: each rank mixes within its own local batch (partners never cross ranks); give every rank its own generator
        seed, as for the mask generators.

    ``device="cpu"`` (or None) yields host tensors and a ``ClipMix`` without a device table: no library call, no GPU needed."""

    def __init__(self, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1,
                 num_classes=1000, generator=None):
        if mode not in ("batch", "elem"):
            raise ValueError(f"mode {mode!r} must be 'batch' or 'elem'")
        if mixup_alpha < 0 or cutmix_alpha < 0 or (mixup_alpha == 0 and cutmix_alpha == 0 and prob > 0):
            raise ValueError("mixup_alpha / cutmix_alpha must be >= 0, one of them positive (or prob = 0)")
        if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0 and 0.0 <= label_smoothing < 1.0):
            raise ValueError("prob and switch_prob must lie in [0, 1], label_smoothing in [0, 1)")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.mode = float(prob), float(switch_prob), mode
        self.label_smoothing, self.num_classes = float(label_smoothing), int(num_classes)
        self.generator = generator if generator is not None else np.random.default_rng()

    def _draw(self, H, W):
        """One decision: (lam for the table, box, weight of the own label)."""
        g = self.generator
        if not g.random() < self.prob:
            return 1.0, (0, 0, 0, 0), 1.0
        both = self.mixup_alpha > 0 and self.cutmix_alpha > 0
        cut = (g.random() < self.switch_prob) if both else self.cutmix_alpha > 0
        if not cut:
            lam = float(g.beta(self.mixup_alpha, self.mixup_alpha))
            return lam, (0, 0, 0, 0), lam
        lam0 = float(g.beta(self.cutmix_alpha, self.cutmix_alpha))
        cy, cx = int(g.integers(0, H)), int(g.integers(0, W))
        box, lam = cutmix_box(lam0, cy, cx, H, W)
        return 1.0, box, lam

    def __call__(self, batch_size, labels, image_size, device=None):
        B = int(batch_size)
        H, W = (int(v) for v in image_size)
        if labels.shape[0] != B:
            raise ValueError(f"Mixup: {labels.shape[0]} labels for a batch of {B}")
        draws = [self._draw(H, W)] * B if self.mode == "batch" else [self._draw(H, W) for _ in range(B)]
        lam = np.array([d[0] for d in draws], dtype=np.float32)
        box = np.array([d[1] for d in draws], dtype=np.int32).reshape(B, 4)
        tlam = np.array([d[2] for d in draws], dtype=np.float64)
        mixed = np.array([d[0] != 1.0 or d[1] != (0, 0, 0, 0) for d in draws])
        partner = np.where(mixed, B - 1 - np.arange(B), np.arange(B)).astype(np.int32)
        device = torch.device(device) if device is not None else torch.device("cpu")
        mix = ClipMix(partner, lam, box, image_size=(H, W), device=device, target_lam=tlam)
        if mix.table is not None:
            soft = soft_targets(labels.to(device), mix.partner_dev, mix.target_lam_dev, self.num_classes, self.label_smoothing)
        else:
            soft = soft_targets(labels, torch.from_numpy(partner.astype(np.int64)), torch.from_numpy(tlam.astype(np.float32)),
                                self.num_classes, self.label_smoothing)
        return mix, soft
