#!/usr/bin/env python3
"""Writes tests/golden/jpeg_decode.json and jpeg_refuse.json: tiny JPEG files (a gradient plus noise, so that AC coefficients and long
codes occur) with the SHA-256 of what PIL / libjpeg-turbo decodes them to.

    python tools/make_jpeg_golden.py                 # needs PIL; rewrites the two fixture files
    python tools/make_jpeg_golden.py --extract DIR   # no PIL: the fixtures' files as DIR/<name>.jpg (for tools/jpeg_host_check)

Per case: name, the file's bytes (base64), width, height, what made it, and for decodable files sha256 of
``PIL.Image.open(f).convert("RGB")`` in planar [3, H, W] order; the three smallest also carry those bytes (rgb_b64).  Parse-only cases
carry ``refuse`` (the reason parse must give) or ``flags`` (the status bits parse must pre-set): a progressive file, and header-patched
copies made here - a 4:4:4 file whose SOF says 4:1:1, a segment length that lies, a missing EOI, a DHT with over-subscribed counts.
"""
import base64
import hashlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "..", "tests", "golden")
FILES = ("jpeg_decode.json", "jpeg_refuse.json")

# name, (W, H), mode, save options, noise sigma
CASES = [
    ("444_16x16", (16, 16), "RGB", dict(subsampling=0), 40),
    ("444_47x33", (47, 33), "RGB", dict(subsampling=0), 40),
    ("422_47x33", (47, 33), "RGB", dict(subsampling=1), 40),
    ("420_47x33", (47, 33), "RGB", dict(subsampling=2), 40),
    ("420_33x47_optimize", (33, 47), "RGB", dict(subsampling=2, optimize=True), 40),
    ("420_47x33_rst2", (47, 33), "RGB", dict(subsampling=2, restart_marker_blocks=2), 40),
    ("422_40x24_rstrow", (40, 24), "RGB", dict(subsampling=1, restart_marker_rows=1), 40),
    ("420_65x17_rst1", (65, 17), "RGB", dict(subsampling=2, restart_marker_blocks=1), 40),
    ("gray_23x19", (23, 19), "L", dict(), 40),
    ("gray_8x8", (8, 8), "L", dict(), 40),
    ("420_1x1", (1, 1), "RGB", dict(subsampling=2), 40),
    ("420_7x5", (7, 5), "RGB", dict(subsampling=2), 40),
    ("444_17x9_q100", (17, 9), "RGB", dict(subsampling=0, quality=100), 400),
    ("420_17x9_q5", (17, 9), "RGB", dict(subsampling=2, quality=5), 40),
]
WITH_BYTES = ("420_1x1", "420_7x5", "gray_8x8")


def picture(W, H, mode, sigma, seed):
    from PIL import Image
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    a = np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y) * 255 // max(W + H - 2, 1)], -1).astype(np.float64)
    a = np.clip(a + g.normal(0, sigma, a.shape), 0, 255).astype(np.uint8)
    im = Image.fromarray(a)
    return im.convert("L") if mode == "L" else im


def encode(im, **kw):
    opts = dict(quality=90)
    opts.update(kw)
    bio = io.BytesIO()
    im.save(bio, "JPEG", **opts)
    return bio.getvalue()


def pil_planar(data):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).transpose(2, 0, 1))


def find_marker(data, marker):
    """offset of the FF of the first header segment with this marker"""
    pos = 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF
        if data[pos + 1] == marker:
            return pos
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    raise ValueError(f"no marker {marker:#x}")


def patched(base):
    d = bytearray(base)
    sof = find_marker(d, 0xC0)
    d[sof + 11] = 0x41                     # the first component's sampling byte: 4 x 1
    yield "patch_sof_411", bytes(d), dict(refuse="sampling")
    d = bytearray(base)
    dqt = find_marker(d, 0xDB)
    d[dqt + 2], d[dqt + 3] = 0xFF, 0xF0    # a segment longer than the file
    yield "patch_length", bytes(d), dict(refuse="bad_length")
    assert base[-2:] == b"\xff\xd9"
    yield "patch_no_eoi", base[:-2], dict(flags=8)
    d = bytearray(base)
    dht = find_marker(d, 0xC4)
    assert d[dht + 4] == 0x00 and d[dht + 5] == 0 and d[dht + 7] >= 2      # DC table 0 of the standard tables: 0, 1, 5, ...
    d[dht + 5] += 2                        # two codes of one bit: the all-ones code in use
    d[dht + 7] -= 2                        # ... and the table's total unchanged
    yield "patch_dht_oversubscribed", bytes(d), dict(refuse="huffman")


def make():
    import PIL
    from PIL import features
    decode, refuse = [], []
    by_name = {}
    for seed, (name, (W, H), mode, kw, sigma) in enumerate(CASES):
        data = encode(picture(W, H, mode, sigma, seed), **kw)
        by_name[name] = data
        rgb = pil_planar(data)
        assert rgb.shape == (3, H, W)
        case = dict(name=name, width=W, height=H, options={k: v for k, v in kw.items()}, jpeg_b64=base64.b64encode(data).decode(),
                    sha256=hashlib.sha256(rgb.tobytes()).hexdigest())
        if name in WITH_BYTES:
            case["rgb_b64"] = base64.b64encode(rgb.tobytes()).decode()
        decode.append(case)
    prog = encode(picture(47, 33, "RGB", 40, 100), subsampling=2, progressive=True)
    refuse.append(dict(name="420_47x33_progressive", width=47, height=33, jpeg_b64=base64.b64encode(prog).decode(), refuse="progressive"))
    for name, data, expect in patched(by_name["444_47x33"]):
        refuse.append(dict(name=name, width=47, height=33, jpeg_b64=base64.b64encode(data).decode(), **expect))
    head = dict(writer="tools/make_jpeg_golden.py", pil=PIL.__version__, libjpeg_turbo=features.version("libjpeg_turbo"))
    for fname, cases in zip(FILES, (decode, refuse)):
        path = os.path.join(GOLDEN, fname)
        with open(path, "w") as fh:
            json.dump(dict(head, cases=cases), fh, indent=1)
            fh.write("\n")
        print(f"{fname}: {len(cases)} cases, {os.path.getsize(path)} bytes")


def extract(dst):
    os.makedirs(dst, exist_ok=True)
    for fname in FILES:
        with open(os.path.join(GOLDEN, fname)) as fh:
            for case in json.load(fh)["cases"]:
                with open(os.path.join(dst, case["name"] + ".jpg"), "wb") as out:
                    out.write(base64.b64decode(case["jpeg_b64"]))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--extract":
        extract(sys.argv[2])
    else:
        make()
