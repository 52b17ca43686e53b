#!/usr/bin/env python3
"""Writes tests/golden/jpeg_split.json: JPEG files whose scans are long enough to be cut into tens of chunks by the split path of
bvc.jpeg (include/bvc.h, bvc_op_jpeg_decode_split), with the SHA-256 of what PIL / libjpeg-turbo decodes them to.

    python tools/make_jpeg_split_golden.py      # needs PIL; rewrites the fixture file

Same pictures as tools/make_jpeg_golden.py (a gradient plus noise), same record per case; the head also lists the chunk sizes the tests
run at.  No file has a restart interval unless its case says so.  The writer checks what the tests rely on and fails when a picture
does not have it (change the seed or the sigma then, not the check): the quality-100 file must put at least three chunk boundaries of
the smallest chunk on the 00 of an FF 00 pair and three directly behind one."""
import base64
import hashlib
import json
import os

import make_jpeg_golden as G

OUT = os.path.join(G.GOLDEN, "jpeg_split.json")
MIN_CHUNK, THREADS = 16, 512      # BVC_JPEG_SPLIT_MIN_CHUNK, BVC_JPEG_SPLIT_THREADS
CHUNKS = [MIN_CHUNK, 32, 64, 0]

# name, (W, H), mode, save options, noise sigma, seed
CASES = [
    ("420_160x120", (160, 120), "RGB", dict(subsampling=2, quality=90), 10, 1),
    ("422_96x64", (96, 64), "RGB", dict(subsampling=1), 25, 2),
    ("444_64x48_q100", (64, 48), "RGB", dict(subsampling=0, quality=100), 120, 6),
    ("gray_120x90", (120, 90), "L", dict(), 20, 4),
    ("420_128x128_flat_q10", (128, 128), "RGB", dict(subsampling=2, quality=10), 0, 5),
    ("420_56x40_optimize", (56, 40), "RGB", dict(subsampling=2, optimize=True), 60, 6),
    ("420_96x96_rstrows2", (96, 96), "RGB", dict(subsampling=2, restart_marker_rows=2), 25, 7),
    ("420_17x9_tiny", (17, 9), "RGB", dict(subsampling=2, quality=5), 0, 8),
]


def scan_range(data):
    sos = G.find_marker(data, 0xDA)
    begin = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
    return begin, len(data) - 2


def chunk_of(nbytes, chunk):
    return max(chunk, (-(-nbytes // THREADS) + 3) // 4 * 4)


def stuffing_at_boundaries(data, chunk):
    begin, end = scan_range(data)
    c = chunk_of(end - begin, chunk)
    on = sum(1 for at in range(begin + c, end, c) if data[at] == 0 and data[at - 1] == 0xFF)
    behind = sum(1 for at in range(begin + c, end, c) if data[at - 1] == 0 and data[at - 2] == 0xFF)
    return on, behind


def make():
    import PIL
    from PIL import features
    cases = []
    for name, (W, H), mode, kw, sigma, seed in CASES:
        data = G.encode(G.picture(W, H, mode, sigma, seed), **kw)
        rgb = G.pil_planar(data)
        assert rgb.shape == (3, H, W)
        begin, end = scan_range(data)
        assert (b"\xff\xdd" in data[:begin]) == ("restart_marker_rows" in kw), name
        note = ""
        if name == "444_64x48_q100":
            on, behind = stuffing_at_boundaries(data, MIN_CHUNK)
            assert on >= 3 and behind >= 3, (on, behind)
            note = f", {data[begin:end].count(bytes([255, 0]))} FF 00 pairs, {on} / {behind} boundaries on / behind a stuffed 00"
        if name == "420_17x9_tiny":
            assert end - begin < 2 * MIN_CHUNK, end - begin
        print(f"{name}: {len(data)} bytes, scan {end - begin}{note}")
        cases.append(dict(name=name, width=W, height=H, options=dict(kw), sigma=sigma, seed=seed, jpeg_b64=base64.b64encode(data).decode(),
                          sha256=hashlib.sha256(rgb.tobytes()).hexdigest()))
    head = dict(writer="tools/make_jpeg_split_golden.py", pil=PIL.__version__, libjpeg_turbo=features.version("libjpeg_turbo"), chunks=CHUNKS)
    with open(OUT, "w") as fh:
        json.dump(dict(head, cases=cases), fh, indent=1)
        fh.write("\n")
    print(f"jpeg_split.json: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    make()
