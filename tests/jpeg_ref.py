"""JPEG decode (include/bvc.h "JPEG decode", csrc/jpeg.h): the fixtures of tests/golden/jpeg_*.json, an independent marker scan, and
a short numpy restatement of the three arithmetic stages - ISLOW IDCT, fancy upsampling, YCbCr -> RGB.  The restatement is NOT a
second oracle (the recorded PIL / libjpeg-turbo bytes are the oracle); it is there to say which stage a mismatch comes from."""
import base64
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _load(fname):
    with open(os.path.join(GOLDEN, fname)) as fh:
        cases = json.load(fh)["cases"]
    for c in cases:
        c["jpeg"] = base64.b64decode(c["jpeg_b64"])
        if "rgb_b64" in c:
            c["rgb"] = np.frombuffer(base64.b64decode(c["rgb_b64"]), np.uint8).reshape(3, c["height"], c["width"])
    return cases


def decode_cases():
    return _load("jpeg_decode.json")


def refuse_cases():
    return _load("jpeg_refuse.json")


def case(name):
    return next(c for c in decode_cases() + refuse_cases() if c["name"] == name)


def find_marker(data, marker):
    """offset of the FF of the first header segment with this marker"""
    pos = 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF
        if data[pos + 1] == marker:
            return pos
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    raise ValueError(f"no marker {marker:#x}")


def scan_segments(data):
    """[(first byte, end byte)] of the restart segments of the first scan, found by a plain walk over the bytes"""
    sos = find_marker(data, 0xDA)
    pos = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
    out, begin = [], pos
    while pos + 1 < len(data):
        if data[pos] == 0xFF and data[pos + 1] != 0:
            out.append((begin, pos))
            if not 0xD0 <= data[pos + 1] <= 0xD7:
                return out
            begin = pos + 2
            pos += 2
        else:
            pos += 2 if data[pos] == 0xFF else 1
    out.append((begin, len(data)))
    return out


def picture(W, H, seed, gray=False, sigma=40):
    """a gradient plus noise as a PIL image (the caller has imported PIL)"""
    from PIL import Image
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    a = np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y) * 255 // max(W + H - 2, 1)], -1).astype(np.float64)
    im = Image.fromarray(np.clip(a + g.normal(0, sigma, a.shape), 0, 255).astype(np.uint8))
    return im.convert("L") if gray else im


def encode(im, **kw):
    import io
    opts = dict(quality=90)
    opts.update(kw)
    bio = io.BytesIO()
    im.save(bio, "JPEG", **opts)
    return bio.getvalue()


def pil_planar(data, mode="RGB"):
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    if mode == "YCbCr":
        im.draft("YCbCr", im.size)      # libjpeg's own YCbCr output: upsampled, not colour-converted
        assert im.mode == "YCbCr"
    else:
        im = im.convert("RGB")
    return np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1))


# ---------------------------------------------------------------- the restatement
def _idct8(v):
    """one 8-point pass of jidctint along the last axis, before the descale (int64: no wrap to think about)"""
    v = v.astype(np.int64)
    z1 = (v[..., 2] + v[..., 6]) * 4433
    tmp2, tmp3 = z1 - v[..., 6] * 15137, z1 + v[..., 2] * 6270
    tmp0, tmp1 = (v[..., 0] + v[..., 4]) << 13, (v[..., 0] - v[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = v[..., 7], v[..., 5], v[..., 3], v[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return np.stack([tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3], -1)


def idct_islow(block):
    """dequantised coefficients [8, 8] (row-major) -> samples [8, 8] uint8: columns (descale 11), rows (descale 18), range limit"""
    ws = (_idct8(np.asarray(block).T) + (1 << 10)) >> 11      # [column][row]
    v = ((_idct8(ws.T) + (1 << 17)) >> 18) & 1023
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896))).astype(np.uint8)


def upsample_h2v1(c, W):
    """a chroma plane [rows, >= cw] to [rows, W]; cw = ceil(W / 2) real samples per row"""
    cw = (W + 1) // 2
    c = c[:, :cw].astype(np.int32)
    if cw <= 2:
        return np.repeat(c, 2, axis=1)[:, :W].astype(np.uint8)
    prev, nxt = np.concatenate([c[:, :1], c[:, :-1]], 1), np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * cw), np.int32)
    out[:, 0::2] = (3 * c + prev + 1) >> 2
    out[:, 1::2] = (3 * c + nxt + 2) >> 2
    out[:, 0], out[:, -1] = c[:, 0], c[:, -1]
    return out[:, :W].astype(np.uint8)


def upsample_h2v2(c, W, H):
    cw, ch = (W + 1) // 2, (H + 1) // 2
    c = c[:ch, :cw].astype(np.int32)
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:H, :W].astype(np.uint8)
    above, below = np.concatenate([c[:1], c[:-1]], 0), np.concatenate([c[1:], c[-1:]], 0)
    sums = np.empty((2 * ch, cw), np.int32)
    sums[0::2], sums[1::2] = 3 * c + above, 3 * c + below
    prev, nxt = np.concatenate([sums[:, :1], sums[:, :-1]], 1), np.concatenate([sums[:, 1:], sums[:, -1:]], 1)
    out = np.empty((2 * ch, 2 * cw), np.int32)
    out[:, 0::2] = (3 * sums + prev + 8) >> 4
    out[:, 1::2] = (3 * sums + nxt + 7) >> 4
    out[:, 0], out[:, -1] = (4 * sums[:, 0] + 8) >> 4, (4 * sums[:, -1] + 7) >> 4
    return out[:H, :W].astype(np.uint8)


def ycc_to_rgb(ycc):
    """[3, H, W] uint8 YCbCr -> RGB with libjpeg's 16-bit tables"""
    y, cb, cr = (ycc[i].astype(np.int64) for i in range(3))
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b]), 0, 255).astype(np.uint8)
