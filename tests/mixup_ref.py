"""Plain-torch restatement of Mixup / CutMix on clips and of the soft targets (the reference of the mix inside the patch gather)."""
import torch


def mix_clips(pixels_f32, partner, lam, box):
    """pixels_f32 [B, T, C, H, W] normalised f32; per clip b: partner[b], lam[b], box[b] = (y0, y1, x0, x1).  Inside the box (rows
    [y0, y1) x columns [x0, x1) of every frame) the partner's pixel; outside it the clip's own pixel when lam == 1, otherwise
    lam * own + (1 - lam) * partner in f32 (two roundings of the products, one of the sum: no fused multiply-add)."""
    px = pixels_f32.to(torch.float32)
    out = torch.empty_like(px)
    for b in range(px.shape[0]):
        own, oth = px[b], px[int(partner[b])]
        w = torch.tensor(float(lam[b]), dtype=torch.float32)
        blend = own.clone() if float(w) == 1.0 else w * own + (torch.tensor(1.0, dtype=torch.float32) - w) * oth
        y0, y1, x0, x1 = (int(v) for v in box[b])
        if y1 > y0 and x1 > x0:
            blend[:, :, y0:y1, x0:x1] = oth[:, :, y0:y1, x0:x1]
        out[b] = blend
    return out


def smooth(labels, num_classes, s):
    y = torch.full((labels.shape[0], num_classes), s / num_classes, dtype=torch.float32)
    y[torch.arange(labels.shape[0]), labels.long()] = 1.0 - s + s / num_classes
    return y


def soft_targets(labels, partner, lam, num_classes, s):
    """soft[b] = lam_b * smooth(y[b]) + (1 - lam_b) * smooth(y[partner[b]])"""
    y = smooth(labels, num_classes, s)
    w = torch.as_tensor(lam, dtype=torch.float32).view(-1, 1)
    return w * y + (1.0 - w) * y[torch.as_tensor(partner).long()]


def tokens_to_rows(pixels_f32, cfg_T, C, H, W, ts, ps):
    """[B, T, C, H, W] -> [B, L, K] rows in Conv3d weight order (c, dt, dy, dx), token-major: the unfold the plain gather equals."""
    B = pixels_f32.shape[0]
    v = pixels_f32.permute(0, 2, 1, 3, 4).reshape(B, C, cfg_T // ts, ts, H // ps, ps, W // ps, ps)
    return v.permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, (cfg_T // ts) * (H // ps) * (W // ps), C * ts * ps * ps)
