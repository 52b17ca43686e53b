"""RandAugment (include/bvc.h, bvc_frame_randaug) restated in numpy: the 15 PIL operations on one RGB uint8 frame [3, H, W], and a
whole table entry (a chain of them).  tests/test_randaug_host.py checks this restatement against PIL itself (where PIL imports) and the
library's host twin against it; tests/test_gpu_randaug.py checks the kernels against the twin.  Every comparison is for equality of
bytes: the integer parts are integer arithmetic, the float parts single IEEE operations in a fixed order.
"""
import math

import numpy as np
import torch

from tests import augment_post_ref as P

f32 = np.float32

OPS = ["AutoContrast", "Equalize", "Invert", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness", "Sharpness",
       "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"]
ID = {name: i for i, name in enumerate(OPS)}
SHAPES = [(1, 9), (2, 5), (3, 3), (17, 40), (33, 65)]
FILL = (124, 116, 104)

frames = P.frames       # [n, 3, H, W] uint8: smooth structure + noise, with 0 and 255 present


# ---------------------------------------------------------------- edge frames
def constant_frame(H, W, value=77):
    """AutoContrast has hi <= lo, Equalize has len(nz) <= 1"""
    return torch.full((3, H, W), value, dtype=torch.uint8)


def two_level_frame(H, W, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.where(torch.rand(3, H, W, generator=g) < 0.5, 40, 199).to(torch.uint8)


def noise_frame(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)


def _equalize_facts(x):
    """per channel: (step, the largest LUT value before the clamp)"""
    out = []
    for c in range(3):
        h = np.bincount(np.asarray(x[c]).reshape(-1), minlength=256)
        nz = h[h > 0]
        step = (int(nz.sum()) - int(nz[-1])) // 255 if len(nz) > 1 else 0
        top = 0
        if step:
            n = step // 2
            for i in range(256):
                top = max(top, n // step)
                n += int(h[i])
        out.append((step, top))
    return out


def step_zero_frame():
    """3 x 3 noise: fewer than 255 pixels below the last level, so Equalize's step is 0 and its LUT the identity"""
    x = noise_frame(3, 3, seed=11)
    facts = _equalize_facts(x)
    assert all(len(np.unique(np.asarray(x[c]))) > 1 and facts[c][0] == 0 for c in range(3)), facts
    return x


def over_255_frame():
    """uniform noise at 17 x 40: Equalize's n // step passes 255 before the clamp"""
    x = noise_frame(17, 40, seed=12)
    facts = _equalize_facts(x)
    assert any(step > 0 and top > 255 for step, top in facts), facts
    return x


def edge_frames(H, W):
    """the edge frames that exist at every shape, as [n, 3, H, W]"""
    return torch.stack([constant_frame(H, W), two_level_frame(H, W), noise_frame(H, W, seed=H * 7 + W)])


# ---------------------------------------------------------------- the operations
def _lut(x, lut):
    return np.stack([np.asarray(lut[c], dtype=np.uint8)[x[c]] for c in range(3)])


def autocontrast(x):
    luts = []
    for c in range(3):
        h = np.bincount(x[c].reshape(-1), minlength=256)
        nzi = np.nonzero(h)[0]
        lo, hi = int(nzi[0]), int(nzi[-1])
        if hi <= lo:
            luts.append(list(range(256)))
            continue
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        luts.append([min(255, max(0, int(i * scale + offset))) for i in range(256)])
    return _lut(x, luts)


def equalize(x):
    luts = []
    for c in range(3):
        h = [int(v) for v in np.bincount(x[c].reshape(-1), minlength=256)]
        nz = [v for v in h if v]
        step = (sum(nz) - nz[-1]) // 255 if len(nz) > 1 else 0
        if step == 0:
            luts.append(list(range(256)))
            continue
        n, lut = step // 2, []
        for i in range(256):
            lut.append(min(255, n // step))
            n += h[i]
        luts.append(lut)
    return _lut(x, luts)


def luma(x):
    r, g, b = (x[c].astype(np.int64) for c in range(3))
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16


def blend(d, v, f):
    """t = d + f (v - d) in f32, one operation at a time; clamp; truncate"""
    d, v, f = np.asarray(d).astype(f32), np.asarray(v).astype(f32), f32(f)
    t = d + f * (v - d)
    assert t.dtype == f32
    return np.minimum(np.maximum(t, f32(0)), f32(255)).astype(np.int64).astype(np.uint8)


def smooth(x):
    """ImageFilter.SMOOTH: the frame's outermost rows and columns copied; inside, 0.5 plus the three kernel rows of the 3 x 3 window in
    turn, each row's three products summed left to right first, all in f32; truncated"""
    H, W = x.shape[-2:]
    out = x.copy()
    if H < 3 or W < 3:
        return out
    k1, k5 = f32(1) / f32(13), f32(5) / f32(13)
    v = x.astype(f32)
    ss = np.full((3, H - 2, W - 2), f32(0.5))
    for dy, kr in ((2, (k1, k1, k1)), (1, (k1, k5, k1)), (0, (k1, k1, k1))):      # Pillow starts with the row below
        row = v[:, dy:H - 2 + dy]
        ss = ss + ((row[:, :, 0:W - 2] * kr[0] + row[:, :, 1:W - 1] * kr[1]) + row[:, :, 2:W] * kr[2])
    assert ss.dtype == f32
    out[:, 1:-1, 1:-1] = np.minimum(np.maximum(ss, f32(0)), f32(255)).astype(np.int64).astype(np.uint8)
    return out


def fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def affine_coeffs(m):
    """a0 .. a5 of Image.transform(AFFINE, m), as ImagingTransform's affine_fixed fixes them"""
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def gather(x, a, fill):
    H, W = x.shape[-2:]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    xin = (a[2] + a[1] * yy + a[0] * xx) >> 16
    yin = (a[5] + a[4] * yy + a[3] * xx) >> 16
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = x[:, np.clip(yin, 0, H - 1), np.clip(xin, 0, W - 1)]
    return np.where(inside[None], out, np.asarray(fill[:3], dtype=np.uint8).reshape(3, 1, 1)).astype(np.uint8)


def coeffs(op, param, H, W):
    """the six coefficients of a geometric op"""
    name = OPS[op] if not isinstance(op, str) else op
    p = float(param)
    if name == "ShearX":
        return affine_coeffs((1.0, p, 0.0, 0.0, 1.0, 0.0))
    if name == "ShearY":
        return affine_coeffs((1.0, 0.0, 0.0, p, 1.0, 0.0))
    if name == "TranslateX":
        return affine_coeffs((1.0, 0.0, p, 0.0, 1.0, 0.0))
    if name == "TranslateY":
        return affine_coeffs((1.0, 0.0, 0.0, 0.0, 1.0, p))
    assert name == "Rotate"
    return P.rotation_coeffs(p, H, W)


def apply_op(x, op, param=None, fill=FILL):
    """one op on one frame [3, H, W] uint8 (numpy)"""
    x = np.asarray(x)
    name = OPS[op] if not isinstance(op, str) else op
    if name == "AutoContrast":
        return autocontrast(x)
    if name == "Equalize":
        return equalize(x)
    if name == "Invert":
        return (255 - x).astype(np.uint8)
    if name == "Posterize":
        return (x & (~((1 << (8 - int(param))) - 1) & 255)).astype(np.uint8)
    if name == "Solarize":
        return np.where(x < int(param), x, 255 - x).astype(np.uint8)
    if name == "SolarizeAdd":
        return np.where(x < 128, np.minimum(255, x.astype(np.int64) + int(param)), x).astype(np.uint8)
    if name == "Color":
        return blend(luma(x)[None], x, param)
    if name == "Contrast":
        L = luma(x)
        m = int(int(L.sum()) / L.size + 0.5)
        return blend(m, x, param)
    if name == "Brightness":
        return blend(0, x, param)
    if name == "Sharpness":
        return blend(smooth(x), x, param)
    return gather(x, coeffs(name, param, x.shape[-2], x.shape[-1]), fill)


def apply_chain(x, stages, fill=FILL):
    """stages: a list of (op, param) -> the frame after all of them, as a torch tensor"""
    x = np.asarray(x)
    for op, param in stages:
        x = apply_op(x, op, param, fill)
    return torch.from_numpy(np.ascontiguousarray(x))


def table(A, H, W, chains, fill=FILL):
    """chains: one list of (op, param) per frame -> the table, through the library's own helper"""
    t = A.empty_randaug_table(len(chains))
    for i, stages in enumerate(chains):
        t[i] = A.randaug_entry(stages, (H, W), fill=fill)
    return t


# ---------------------------------------------------------------- parameters: the ends of each range and 20 drawn values
def op_params(name, H, W, n=20):
    g = np.random.default_rng(200 + ID[name])
    if name in ("AutoContrast", "Equalize", "Invert"):
        return [None]
    if name == "Posterize":
        return list(range(0, 9))
    if name == "Solarize":
        return [0, 256, 1, 255, 128] + [int(v) for v in g.integers(0, 257, n)]
    if name == "SolarizeAdd":
        return [0, 110, 1] + [int(v) for v in g.integers(0, 111, n)]
    if name in ("Color", "Contrast", "Brightness", "Sharpness"):
        return [0.1, 1.9, 1.0, 0.0] + [float(v) for v in g.uniform(0.1, 1.9, n)]
    if name in ("ShearX", "ShearY"):
        return [-0.3, 0.3, 0.0] + [float(v) for v in g.uniform(-0.3, 0.3, n)]
    if name in ("TranslateX", "TranslateY"):
        edge = W if name == "TranslateX" else H
        return [-0.45 * edge, 0.45 * edge, 0.0, float(edge), float(-edge) - 1.0] + [float(v) for v in g.uniform(-0.45 * edge, 0.45 * edge, n)]
    return [-30.0, 30.0, 0.0] + [float(v) for v in g.uniform(-30.0, 30.0, n)]


def random_chain(g, n, H, W):
    """n stages, ops drawn with replacement (repeats happen), parameters from op_params"""
    out = []
    for _ in range(n):
        name = OPS[int(g.integers(0, 15))]
        ps = op_params(name, H, W)
        out.append((name, ps[int(g.integers(0, len(ps)))]))
    return out


# ---------------------------------------------------------------- PIL
def pil_op(x, name, param=None, fill=FILL):
    from PIL import Image, ImageEnhance, ImageOps
    im = Image.fromarray(np.ascontiguousarray(np.asarray(x).transpose(1, 2, 0)), "RGB")
    fill = tuple(int(v) for v in fill[:3])
    if name == "AutoContrast":
        r = ImageOps.autocontrast(im)
    elif name == "Equalize":
        r = ImageOps.equalize(im)
    elif name == "Invert":
        r = ImageOps.invert(im)
    elif name == "Posterize":
        r = ImageOps.posterize(im, int(param))
    elif name == "Solarize":
        r = ImageOps.solarize(im, int(param))
    elif name == "SolarizeAdd":
        r = im.point([min(255, i + int(param)) if i < 128 else i for i in range(256)] * 3)
    elif name in ("Color", "Contrast", "Brightness", "Sharpness"):
        r = getattr(ImageEnhance, name)(im).enhance(param)
    elif name == "Rotate":
        r = im.rotate(param, resample=Image.NEAREST, fillcolor=fill)
    else:
        p = float(param)
        m = {"ShearX": (1, p, 0, 0, 1, 0), "ShearY": (1, 0, 0, p, 1, 0), "TranslateX": (1, 0, p, 0, 1, 0), "TranslateY": (1, 0, 0, 0, 1, p)}[name]
        r = im.transform(im.size, Image.AFFINE, m, resample=Image.NEAREST, fillcolor=fill)
    return np.asarray(r).transpose(2, 0, 1)
