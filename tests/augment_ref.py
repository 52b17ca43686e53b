"""Oracle of the clip transforms (include/bvc.h, bvc_frame_aug) for tests/test_augment_host.py and tests/test_gpu_augment.py.

Geometry: torch's own ``F.interpolate(uint8, mode="bilinear", antialias=True, align_corners=False)`` on the CPU - the very call
torchvision's ``resize`` makes for tensors - on the entry's region, then the window slice and the mirror.

Colour: torchvision is not installed where these tests run, so its code cannot be the oracle.  This file is a stage-by-stage
RESTATEMENT of the arithmetic of torchvision's tensor functions for uint8 images (``adjust_brightness`` / ``adjust_contrast`` /
``adjust_saturation`` / ``adjust_hue`` / ``rgb_to_grayscale`` in transforms/_functional_tensor.py), evaluated in fp64 with the same
per-stage rounding: every stage takes the previous stage's uint8 values and truncates its own result to uint8.  It is not
torchvision, and it shares no code with the library.  Every stage also marks the elements whose fp64 value before truncation sits within TIE of
an integer, where an f32 evaluation may legitimately truncate the other way.

The table is read through its numpy fields only (bvc.augment.FRAME_AUG); factors are the table's f32 values, widened.
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
TIE = 2e-3          # |fp64 value - nearest integer| up to which an f32 evaluation (error < 1e-4 at these magnitudes) may differ


def resize_window(frames, e, Ho, Wo, flip=True):
    """uint8 [3, Ho, Wo]: entry ``e``'s geometry of ``frames`` [F, 3, Hs, Ws] through torch's antialiased bilinear resize."""
    region = frames[int(e["src"]), :, int(e["y0"]):int(e["y0"]) + int(e["h"]), int(e["x0"]):int(e["x0"]) + int(e["w"])]
    r = F.interpolate(region[None], size=(int(e["Hr"]), int(e["Wr"])), mode="bilinear", antialias=True, align_corners=False)[0]
    r = r[:, int(e["oy"]):int(e["oy"]) + Ho, int(e["ox"]):int(e["ox"]) + Wo]
    return r.flip(-1) if flip and int(e["flip"]) else r


def _finish(pre, safe):
    """(uint8 result as int64, near) of a stage whose fp64 value before rounding is ``pre``: clamp to [0, 255], truncate.  ``near``
    marks the elements within TIE of an integer, except those in ``safe``: elements whose value is an exact integer that an f32
    evaluation reproduces exactly as well (a single product, a blend with ratio 1 or 0 on integers, an all-zero sum)."""
    near = ((pre - pre.round()).abs() <= TIE) & ~safe
    return pre.clamp(0.0, 255.0).floor().to(torch.int64), near


def gray_stage(img):
    """[3, H, W] int64 -> ([H, W] int64, near): trunc(0.2989 r + 0.587 g + 0.114 b)"""
    v = img.double()
    pre = 0.2989 * v[0] + 0.587 * v[1] + 0.114 * v[2]
    return _finish(pre, pre == 0.0)


def brightness(img, f):
    pre = f * img.double()          # the product of an f32 factor and an 8-bit integer is exact in fp64; an integer result is exact in f32 too
    return _finish(pre, pre == pre.round())


def contrast(img, f):
    g, _ = gray_stage(img)
    pre = f * img.double() + (1.0 - f) * g.double().mean()
    return _finish(pre, torch.full(pre.shape, f == 1.0))


def saturation(img, f):
    g, gnear = gray_stage(img)
    pre = f * img.double() + (1.0 - f) * g.double()[None]
    out, near = _finish(pre, torch.full(pre.shape, f in (0.0, 1.0)))
    return out, near | (gnear[None] if f != 1.0 else False)


def hue(img, f):
    x = img.double() / 255.0
    r, g, b = x[0], x[1], x[2]
    maxc, minc = x.max(0).values, x.min(0).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = torch.remainder(h + f, 1.0)
    v = maxc
    i = torch.floor(h * 6.0)
    fr = h * 6.0 - i
    i = i.to(torch.int64) % 6
    p = (v * (1.0 - s)).clamp(0.0, 1.0)
    q = (v * (1.0 - s * fr)).clamp(0.0, 1.0)
    t = (v * (1.0 - s * (1.0 - fr))).clamp(0.0, 1.0)
    a1 = torch.stack((v, q, p, p, t, v))
    a2 = torch.stack((t, v, v, q, p, p))
    a3 = torch.stack((p, p, t, v, v, q))
    pick = i[None]
    out = torch.stack((a1.gather(0, pick)[0], a2.gather(0, pick)[0], a3.gather(0, pick)[0]))
    pre = out * (255.0 + 1.0 - 1e-3)
    return _finish(pre, pre == 0.0)


def to_gray(img):
    g, near = gray_stage(img)
    return g[None].expand(3, -1, -1).contiguous(), near[None].expand(3, -1, -1)


STAGE = {BRIGHTNESS: brightness, CONTRAST: contrast, SATURATION: saturation, HUE: hue}


def ops_of(e):
    return [(int(e["order"]) >> (4 * i)) & 15 for i in range(int(e["nops"]))]


def colour_chain(img_u8, e):
    """The entry's jitter stages and gray stage on a uint8 [3, H, W] frame.  Returns (uint8 result, near) where ``near`` marks the
    elements at which ANY stage's fp64 value before truncation lay within TIE of an integer (channel-wise; a gray tie inside a
    saturation or grayscale stage marks all three channels of the pixel)."""
    img = img_u8.to(torch.int64)
    near = torch.zeros(img.shape, dtype=torch.bool)
    for op in ops_of(e):
        img, n = STAGE[op](img, float(np.float32(e["factor"][op])))
        near = near | n
    if int(e["gray"]):
        img, n = to_gray(img)
        near = near | n
    return img.to(torch.uint8), near


def transform(frames, table, Ho, Wo):
    """The whole transform per table entry: uint8 [F_out, 3, Ho, Wo] and the near-tie mask of the colour stages."""
    outs, nears = [], []
    for e in table:
        r = resize_window(frames, e, Ho, Wo, flip=False)
        o, n = colour_chain(r, e)
        if int(e["flip"]):
            o, n = o.flip(-1), n.flip(-1)
        outs.append(o)
        nears.append(n)
    return torch.stack(outs), torch.stack(nears)


def lsb_response(img_u8, e):
    """The chain's own largest response to moving its input by one LSB: max over the 26 non-zero shifts d in {-1, 0, 1}^3 (one per
    channel, applied to the whole frame and clamped) of max |chain(img + d) - chain(img)|."""
    base, _ = colour_chain(img_u8, e)
    worst = 0
    for d in itertools.product((-1, 0, 1), repeat=3):
        if d == (0, 0, 0):
            continue
        moved = (img_u8.to(torch.int64) + torch.tensor(d).view(3, 1, 1)).clamp(0, 255).to(torch.uint8)
        out, _ = colour_chain(moved, e)
        worst = max(worst, int((out.to(torch.int64) - base.to(torch.int64)).abs().max()))
    return worst
