"""JPEG decode on the CPU (bvc_jpeg_parse, bvc_jpeg_decode_host, bvc.jpeg).  No GPU.

The oracle is libjpeg-turbo through PIL: the recorded SHA-256 (and, for the three smallest cases, bytes) of
``Image.open(f).convert("RGB")`` in tests/golden/jpeg_decode.json, and where PIL imports a live decode of the same files and of a sweep
of sizes encoded on the spot (the only tests here that are skipped without it).  Integer arithmetic end to end: the bar is ZERO
differing bytes.  Then what parse refuses and why, truncation at every byte of a scan, and the segment table against an independent walk
over the markers."""
import hashlib

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import jpeg_ref as R


@pytest.fixture(scope="module")
def bvc():
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def J(bvc):
    return bvc.jpeg


NAMES = [c["name"] for c in R.decode_cases()]


def _differing(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


def test_struct_layouts(bvc, J):
    assert J.INFO.itemsize == bvc._lib.lib().bvc_jpeg_info_bytes() == 4248 and J.HUFF.itemsize == 912
    assert J.INFO.fields["blob_offset"][1] == 56 and J.INFO.fields["qt"][1] == 88 and J.INFO.fields["huff"][1] == 600
    for name in ("bvc_jpeg_parse", "bvc_jpeg_decode_host", "bvc_op_jpeg_decode_workspace", "bvc_op_jpeg_decode"):
        assert name in bvc._lib.SYMBOLS and getattr(bvc._lib.lib(), name) is not None
    assert bvc.JpegClipRing is J.JpegClipRing and bvc.JpegUnsupported is J.JpegUnsupported


def test_fixture_table_is_the_one_asked_for():
    assert len(NAMES) == 14 and {(c["width"], c["height"]) for c in R.decode_cases()} >= {(16, 16), (47, 33), (33, 47), (40, 24), (65, 17),
                                                                                             (23, 19), (8, 8), (1, 1), (7, 5), (17, 9)}
    assert sorted(c["name"] for c in R.decode_cases() if "rgb" in c) == ["420_1x1", "420_7x5", "gray_8x8"]


# ---------------------------------------------------------------- the twin against the recorded and the live decode
@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_recorded_pil(J, name):
    c = R.case(name)
    got = J.decode_host([c["jpeg"]])
    assert got.status == [0] and tuple(got[0].shape) == (3, c["height"], c["width"])
    assert hashlib.sha256(got[0].numpy().tobytes()).hexdigest() == c["sha256"], name
    if "rgb" in c:
        assert _differing(got[0], c["rgb"]) == 0


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_equals_live_pil(J, name):
    pytest.importorskip("PIL")
    c = R.case(name)
    want = R.pil_planar(c["jpeg"])
    assert hashlib.sha256(want.tobytes()).hexdigest() == c["sha256"], "this PIL decodes the fixture to other bytes than the recorded ones"
    assert _differing(J.decode_host([c["jpeg"]])[0], want) == 0


SWEEP = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (4, 4), (5, 3), (3, 5), (8, 8), (9, 9), (15, 16), (16, 15), (16, 17), (17, 16), (17, 17),
         (24, 8), (8, 24), (25, 31), (31, 25), (32, 32), (33, 33), (33, 1), (1, 33), (41, 7), (7, 41), (48, 48), (49, 49), (50, 1), (47, 50),
         (50, 50)]


@pytest.mark.parametrize("subsampling", [0, 1, 2])
def test_host_twin_equals_pil_on_a_sweep_of_sizes(J, subsampling):
    pytest.importorskip("PIL")
    assert len(SWEEP) == 30
    for i, (W, H) in enumerate(SWEEP):
        kw = dict(subsampling=subsampling)
        if i % 3 == 1:
            kw["restart_marker_blocks"] = 1 + i % 4
        if i % 5 == 2:
            kw["optimize"] = True
        data = R.encode(R.picture(W, H, seed=1000 * subsampling + i), **kw)
        got = J.decode_host([data])
        assert got.status == [0] and _differing(got[0], R.pil_planar(data)) == 0, f"{W}x{H} subsampling {subsampling} {kw}"


# ---------------------------------------------------------------- the restatement (localises a mismatch; not an oracle)
def test_restated_colour_conversion_equals_pil():
    pytest.importorskip("PIL")
    for name in ("444_47x33", "420_47x33", "444_17x9_q100"):
        data = R.case(name)["jpeg"]
        assert _differing(R.ycc_to_rgb(R.pil_planar(data, "YCbCr")), R.pil_planar(data)) == 0, name


def test_restated_idct_and_upsampling():
    # a DC-only block is flat at 128 + DC / 8; any block is within 1 of the exact inverse DCT (the accuracy class of the ISLOW IDCT)
    for dc in (-1024, -300, 0, 8, 13, 1016):
        b = np.zeros((8, 8), np.int64)
        b[0, 0] = dc
        assert (R.idct_islow(b) == np.clip(128 + ((dc + 4) >> 3), 0, 255)).all()
    g = np.random.default_rng(3)
    k = np.arange(8)
    basis = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k[:, None] == 0, np.sqrt(1 / 8), np.sqrt(2 / 8))
    for _ in range(50):
        b = g.integers(-60, 60, (8, 8))
        exact = basis.T @ b @ basis + 128
        assert np.abs(R.idct_islow(b).astype(np.float64) - np.clip(exact, 0, 255)).max() <= 1.0 + 1e-9
    flat = np.full((9, 12), 77, np.uint8)
    assert (R.upsample_h2v1(flat, 23) == 77).all() and R.upsample_h2v1(flat, 23).shape == (9, 23)
    assert (R.upsample_h2v2(flat, 23, 17) == 77).all() and R.upsample_h2v2(flat, 23, 17).shape == (17, 23)
    c = np.array([[10, 50, 90]], np.uint8)
    assert R.upsample_h2v1(c, 6).tolist() == [[10, 20, 40, 60, 80, 90]] and R.upsample_h2v1(c, 4).tolist() == [[10, 10, 50, 50]]


# ---------------------------------------------------------------- parse
def test_decodable_fixtures_parse_with_their_layout(J):
    for c in R.decode_cases():
        info = J.parse(c["jpeg"])
        assert (info.width, info.height, info.flags) == (c["width"], c["height"], 0)
        want = (1, 1) if c["name"].startswith(("gray", "444")) else ((2, 1) if c["name"].startswith("422") else (2, 2))
        assert info.sampling == want and info.ncomp == (1 if c["name"].startswith("gray") else 3)
        assert int(info.segments[:, 3].sum()) == int(info.record["mcus_x"][0]) * int(info.record["mcus_y"][0])
        assert (info.restart_interval > 0) == ("rst" in c["name"]) and (info.nseg > 1) == ("rst" in c["name"])
    assert J.parse(R.case("420_65x17_rst1")["jpeg"]).nseg == 10      # the RSTn counter wraps


def test_recorded_refusals_and_flags(J):
    seen = {}
    for c in R.refuse_cases():
        r = J.try_parse(c["jpeg"])
        if "refuse" in c:
            assert isinstance(r, J.JpegUnsupported) and r.reason == c["refuse"], c["name"]
            with pytest.raises(J.JpegUnsupported, match=c["refuse"]):
                J.parse(c["jpeg"])
        else:
            assert isinstance(r, J.JpegInfo) and r.flags == c["flags"] == J.ST_NO_EOI, c["name"]
        seen[c["name"]] = c.get("refuse", "flags")
    assert seen == {"420_47x33_progressive": "progressive", "patch_sof_411": "sampling", "patch_length": "bad_length",
                    "patch_no_eoi": "flags", "patch_dht_oversubscribed": "huffman"}
    # without its EOI the file still decodes to the same bytes, with the status bit raised
    got = J.decode_host([R.case("patch_no_eoi")["jpeg"]])
    assert got.status == [J.ST_NO_EOI] and _differing(got[0], J.decode_host([R.case("444_47x33")["jpeg"]])[0]) == 0


def test_header_patches_are_refused_by_reason(J):
    base = R.case("444_47x33")["jpeg"]
    sof, sos = R.find_marker(base, 0xC0), R.find_marker(base, 0xDA)

    def patched(at, value):
        d = bytearray(base)
        d[at:at + len(value)] = value
        return bytes(d)

    app14 = lambda t: b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([t])      # noqa: E731
    cases = {
        "not_jpeg": b"\x89PNG" + base[4:],
        "arithmetic": patched(sof + 1, b"\xc9"),
        "lossless": patched(sof + 1, b"\xc3"),
        "progressive": patched(sof + 1, b"\xc2"),
        "precision": patched(sof + 4, b"\x0c"),
        "size": patched(sof + 5, b"\x00\x00"),
        "components": patched(sof + 9, b"\x04"),
        "sampling": patched(sof + 11, b"\x12"),                       # 1 x 2 luma (4:4:0)
        "quant": patched(sof + 12, b"\x03"),                          # a table no DQT defined
        "rgb": base[:2] + app14(0) + base[2:],
        "multi_scan": base[:sos] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + base[sos + 14:],
        "scan_header": patched(sos + 12, b"\x3e"),                    # Se = 62
        "huffman": patched(sos + 6, b"\x22"),                         # tables 2 / 2
        "restart": base[:sos + 14 + 20] + b"\xff\xd0" + base[sos + 14 + 20:],      # RST0 in a file without DRI
        "bad_length": base[:sof + 6],
        "header": base[:2] + b"\x00\x00" + base[2:],
    }
    assert set(cases) == set(J.REASONS.values())
    for reason, data in cases.items():
        r = J.try_parse(data)
        assert isinstance(r, J.JpegUnsupported) and r.reason == reason, (reason, getattr(r, "reason", "accepted"))
    assert isinstance(J.try_parse(base[:2] + app14(1) + base[2:]), J.JpegInfo)      # Adobe, transform 1: YCbCr
    big = patched(sof + 5, b"\x10\x01")      # 4097 rows
    assert J.try_parse(big).reason == "size" and isinstance(J.try_parse(patched(sof + 5, b"\x10\x00")), J.JpegInfo)
    with pytest.raises(ValueError):
        J.parse(np.zeros((2, 2), np.uint8))


def test_segment_table_matches_the_markers(J):
    for name in ("420_47x33_rst2", "422_40x24_rstrow", "420_65x17_rst1", "420_47x33", "gray_8x8"):
        data = R.case(name)["jpeg"]
        info = J.parse(data)
        want = R.scan_segments(data)
        assert [tuple(s) for s in info.segments[:, :2].tolist()] == want, name
        ri, total = info.restart_interval, int(info.record["mcus_x"][0]) * int(info.record["mcus_y"][0])
        firsts = [i * ri for i in range(len(want))]
        assert info.segments[:, 2].tolist() == firsts and info.segments[:, 3].tolist() == [min(ri, total - f) if ri else total for f in firsts]
        for i, (b, e) in enumerate(want[:-1]):
            assert data[e] == 0xFF and data[e + 1] == 0xD0 + i % 8
    info = J.parse(R.case("422_40x24_rstrow")["jpeg"])
    assert info.restart_interval == int(info.record["mcus_x"][0]) and info.nseg == int(info.record["mcus_y"][0])


# ---------------------------------------------------------------- damaged scans
@pytest.mark.parametrize("name", ["444_16x16", "420_47x33_rst2", "gray_8x8", "420_33x47_optimize"])
def test_truncation_at_every_byte_of_the_scan(J, name):
    c = R.case(name)
    data = c["jpeg"]
    begin = int(J.parse(data).record["scan_begin"][0])
    whole = J.decode_host([data])[0]
    for cut in range(begin, len(data)):
        got = J.decode_host([data[:cut]])
        assert got.status[0] != 0 and got.status[0] & J.ST_NO_EOI, cut
        assert tuple(got[0].shape) == (3, c["height"], c["width"])
    assert _differing(J.decode_host([data[:-2]])[0], whole) == 0
    assert J.decode_host([data[:begin]]).status[0] & J.ST_TRUNCATED


def test_a_short_restart_segment_raises_its_status_and_spares_the_others(J):
    data = R.case("420_47x33_rst2")["jpeg"]
    info = J.parse(data)
    b, e = (int(v) for v in info.segments[2, :2])
    cut = data[:b + (e - b) // 2] + data[e:]
    got, whole = J.decode_host([cut]), J.decode_host([data])[0]
    assert got.status == [J.ST_TRUNCATED]
    # MCUs 4 and 5 of nine 16 x 16 MCUs in three columns: the first MCU row is untouched above its last luma row (which chroma of the
    # second row reaches through the upsampling filter)
    assert _differing(got[0][:, :15], whole[:, :15]) == 0 and _differing(got[0], whole) > 0
    assert J.decode_host([cut])[0].equal(got[0])
