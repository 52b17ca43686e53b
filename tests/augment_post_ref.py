"""The post stage of the clip transforms (include/bvc.h, bvc_frame_post) restated in numpy: Pillow's GaussianBlur and Image.rotate
as integer arithmetic, and the gray of the stage before.  tests/test_augment_post_host.py checks this restatement against PIL itself
(where PIL imports) and the library's host twin against it; tests/test_gpu_augment_post.py checks the kernels against the twin.
Everything is integer arithmetic, so every comparison is for equality.
"""
import math

import numpy as np
import torch

f32 = np.float32

BLUR_SHAPES = [(1, 9), (2, 5), (3, 3), (17, 40), (33, 65)]
BLUR_RADII = [0.0, 0.1, 0.3, 1.0, 2.0, 4.0]
ROT_SHAPES = [(24, 24), (17, 40), (33, 65)]
ROT_ANGLES = [0.0, 90.0, -90.0, 45.0, -45.0, 1e-3, 180.0]


def drawn_radii(n=20):
    return [float(v) for v in np.random.default_rng(101).uniform(0.1, 4.0, n)]


def drawn_angles(n=20):
    return [float(v) for v in np.random.default_rng(102).uniform(-90.0, 90.0, n)]


def frames(n, H, W, seed):
    """[n, 3, H, W] uint8: smooth structure + noise, with the extremes 0 and 255 present"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = 127.5 + 100.0 * torch.sin(xx / 3.0 + torch.arange(3).view(3, 1, 1)) * torch.cos(yy / 4.0)
    x = base[None] + 60.0 * torch.randn(n, 3, H, W, generator=g)
    return x.clamp(0, 255).to(torch.uint8).contiguous()


def blur_weights(radius):
    """(r, ww, fw) of Pillow's box approximation: _gaussian_blur_radius in f32 (its square root and floor in f64), the box weight by an
    f32 division"""
    radius = f32(radius)
    sigma2 = radius * radius / f32(3)
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = (f32(2) * l + f32(1)) * (l * (l + f32(1)) - f32(3) * sigma2)
    a = a / (f32(6) * (sigma2 - (l + f32(1)) * (l + f32(1))))
    fr = l + a
    assert type(fr) is np.float32
    r = int(fr)
    ww = int(f32(1 << 24) / (fr * f32(2) + f32(1)))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def box_pass(x, axis, r, ww, fw):
    """one box pass along ``axis`` of a uint8 array, taps beyond the ends reading the end values"""
    n = x.shape[axis]
    pad = [(0, 0)] * x.ndim
    pad[axis] = (r + 1, r + 1)
    p = np.pad(x.astype(np.int64), pad, mode="edge")

    def at(k):                                      # the samples at offset k - (r + 1) from every position
        return np.take(p, np.arange(k, k + n), axis=axis)

    inner = sum(at(k) for k in range(1, 2 * r + 2))
    acc = ww * inner + fw * (at(0) + at(2 * r + 2)) + (1 << 23)
    assert int(acc.max()) < (1 << 32)
    return (acc >> 24).astype(np.uint8)


def blur(x, weights):
    """[..., H, W] uint8 -> three passes along the rows, then three along the columns"""
    r, ww, fw = weights
    x = np.asarray(x)
    for axis in (-1, -2):
        for _ in range(3):
            x = box_pass(x, x.ndim + axis, r, ww, fw)
    return x


def gray(x):
    """[3, H, W] uint8 -> the truncated f32 gray of csrc/augment.h on all three channels"""
    r, g, b = (np.asarray(x[c]).astype(f32) for c in range(3))
    v = ((f32(0.2989) * r + f32(0.587) * g) + f32(0.114) * b).astype(np.int64).astype(np.uint8)
    return np.stack([v, v, v])


def rotation_coeffs(angle, H, W):
    """a0 .. a5: the matrix of Image.rotate(angle) about (W / 2, H / 2), fixed to 16.16 as ImagingTransform's affine_fixed does"""
    t = -math.radians(angle % 360.0)
    m0, m1, m3, m4 = round(math.cos(t), 15), round(math.sin(t), 15), round(-math.sin(t), 15), round(math.cos(t), 15)
    cx, cy = W / 2.0, H / 2.0
    m2 = m0 * -cx + m1 * -cy + 0.0
    m5 = m3 * -cx + m4 * -cy + 0.0
    m2 += cx
    m5 += cy

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))

    return [fix(m0), fix(m1), fix(m2 + m0 * 0.5 + m1 * 0.5), fix(m3), fix(m4), fix(m5 + m3 * 0.5 + m4 * 0.5)]


def rotate(x, a):
    """[3, H, W] uint8 gathered through the 16.16 map; 0 outside"""
    x = np.asarray(x)
    H, W = x.shape[-2:]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    xin = (a[2] + a[1] * yy + a[0] * xx) >> 16
    yin = (a[5] + a[4] * yy + a[3] * xx) >> 16
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = x[:, np.clip(yin, 0, H - 1), np.clip(xin, 0, W - 1)]
    return np.where(inside[None], out, 0).astype(np.uint8)


def apply(x, radius=None, to_gray=False, angle=None):
    """one frame [3, H, W] through blur -> gray -> rotation, as a torch tensor"""
    x = np.asarray(x)
    if radius is not None:
        x = blur(x, blur_weights(radius))
    if to_gray:
        x = gray(x)
    if angle is not None:
        x = rotate(x, rotation_coeffs(angle, x.shape[-2], x.shape[-1]))
    return torch.from_numpy(np.ascontiguousarray(x))


def entry(A, e, H, W, radius=None, to_gray=False, angle=None):
    """fill one FRAME_POST entry through the library's own helpers"""
    if radius is not None:
        e["blur_r"], e["blur_ww"], e["blur_fw"] = A.blur_weights(radius)
    e["gray"] = int(to_gray)
    if angle is not None:
        e["rotate"], e["rot"] = 1, A.rotation_coeffs(angle, (H, W))


def table(A, H, W, cases):
    """cases: a list of dicts (radius / to_gray / angle) -> the post table"""
    t = A.empty_post_table(len(cases))
    for e, kw in zip(t, cases):
        entry(A, e, H, W, **kw)
    return t


def pil_blur(x, radius):
    from PIL import Image, ImageFilter
    im = Image.fromarray(np.ascontiguousarray(np.asarray(x).transpose(1, 2, 0))).filter(ImageFilter.GaussianBlur(radius))
    return np.asarray(im).transpose(2, 0, 1)


def pil_rotate(x, angle):
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(np.asarray(x).transpose(1, 2, 0)))
    return np.asarray(im.rotate(angle, resample=Image.NEAREST, expand=False, fillcolor=0)).transpose(2, 0, 1)
