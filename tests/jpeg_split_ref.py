"""The split path of bvc.jpeg (include/bvc.h, bvc_op_jpeg_decode_split): the fixtures of tests/golden/jpeg_split.json and a plain walk
over a scan, symbol by symbol, that says where symbols start and blocks end - so that a test can prove that its input has a chunk
boundary inside a symbol, on a stuffed 00, or a chunk holding many blocks.  The walk is no decoder: it keeps no coefficient."""
import json
import os

from tests import jpeg_ref as R

with open(os.path.join(R.GOLDEN, "jpeg_split.json")) as _fh:
    HEAD = {k: v for k, v in json.load(_fh).items() if k != "cases"}
CHUNKS = HEAD["chunks"]      # the chunk sizes the tests run at: the smallest, 32, 64 and 0 (the default)


def split_cases():
    return R._load("jpeg_split.json")


def split_case(name):
    return next(c for c in split_cases() if c["name"] == name)


def stuffing_at(data, boundaries):
    """how many of the byte offsets lie on the 00 of an FF 00 pair, and how many directly behind one"""
    on = sum(1 for at in boundaries if data[at] == 0 and data[at - 1] == 0xFF)
    behind = sum(1 for at in boundaries if data[at - 1] == 0 and data[at - 2] == 0xFF)
    return on, behind


def walk(info, s=0):
    """Segment s of a parsed file: (starts, ends) - the bit position, in the raw file, of every symbol's first bit, and of the first
    bit behind every block.  A stuffed 00 belongs to its FF: no position lies inside one."""
    data, rec = info.data, info.record
    begin, end, _, mcus = (int(v) for v in info.segments[s])
    raw, val, i = [], [], begin      # the de-stuffed bytes and where each lies in the file
    while i < end:
        raw.append(i)
        val.append(int(data[i]))
        i += 2 if data[i] == 0xFF else 1
    raw.append(end)
    nbits = 8 * len(val)
    huff = rec["huff"][0]
    hs, vs, ncomp = (int(rec[k][0]) for k in ("hs", "vs", "ncomp"))
    hv = hs * vs
    nblk = 1 if ncomp == 1 else hv + 2
    at = 0

    def pos():
        return 8 * raw[at >> 3] + (at & 7)

    def bits(n):
        nonlocal at
        v = 0
        for _ in range(n):
            v = (v << 1) | ((val[at >> 3] >> (7 - (at & 7))) & 1)
            at += 1
        return v

    def symbol(h):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | bits(1)
            if code <= int(h["maxcode"][length]):
                return int(h["huffval"][(code + int(h["valoff"][length])) & 255])
        raise ValueError("no such code")

    starts, ends = [], []
    for _ in range(mcus):
        for bi in range(nblk):
            comp = 0 if bi < hv else bi - hv + 1
            dc, ac = huff[int(rec["td"][0][comp])], huff[2 + int(rec["ta"][0][comp])]
            starts.append(pos())
            bits(symbol(dc))
            k = 1
            while k < 64:
                starts.append(pos())
                rs = symbol(ac)
                r, size = rs >> 4, rs & 15
                bits(size)
                if size:
                    k += r + 1
                elif r == 15:
                    k += 16
                else:
                    break
            assert at <= nbits
            ends.append(pos())
    return starts, ends
