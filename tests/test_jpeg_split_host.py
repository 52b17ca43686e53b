"""The split path of the JPEG decode on the CPU (bvc_jpeg_decode_host_split, bvc.jpeg.decode_host_split): jpeg_split_kernel's chunk loop,
rounds and placement in plain C++, its lanes run one after another.  No GPU.

The bar is the module's: ZERO differing bytes and equal status bits against the one-lane host twin (decode_host) on every input,
damaged ones included, and the recorded SHA-256 of libjpeg-turbo's decode.  An undamaged file never falls back; a damaged one falls
back exactly where the twin reports TRUNCATED, BAD_CODE or BAD_RUN.  The input-property tests prove, with split_chunks and a plain walk
over the bytes (tests/jpeg_split_ref.py), that the fixtures put chunk boundaries where the path can go wrong."""
import hashlib

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import jpeg_ref as R
from tests import jpeg_split_ref as S


@pytest.fixture(scope="module")
def J():
    ge.build()
    return ge.load_package().jpeg


CASES = R.decode_cases() + S.split_cases()
NAMES = [c["name"] for c in CASES]
ERR = 7      # ST_TRUNCATED | ST_BAD_CODE | ST_BAD_RUN


def _case(name):
    return next(c for c in CASES if c["name"] == name)


def _differing(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


def _split_all(J):
    return 2 * J.SPLIT_MIN_CHUNK      # low enough to split everything splittable


def test_the_interface_and_the_fixture_table(J):
    assert (J.SPLIT_MIN_CHUNK, J.SPLIT_THREADS) == (16, 512) and 16 <= J.SPLIT_MIN_CHUNK <= 32 and J.SPLIT_THREADS <= 1024
    assert S.CHUNKS == [J.SPLIT_MIN_CHUNK, 32, 64, 0] and J.SPLIT_AUTO_BYTES >= 2 * J.SPLIT_MIN_CHUNK
    assert [(c["name"], c["width"], c["height"]) for c in S.split_cases()] == [
        ("420_160x120", 160, 120), ("422_96x64", 96, 64), ("444_64x48_q100", 64, 48), ("gray_120x90", 120, 90),
        ("420_128x128_flat_q10", 128, 128), ("420_56x40_optimize", 56, 40), ("420_96x96_rstrows2", 96, 96), ("420_17x9_tiny", 17, 9)]
    for c in S.split_cases():
        info = J.parse(c["jpeg"])
        assert (info.restart_interval > 0) == ("rst" in c["name"]), c["name"]
        n = len(J.split_chunks(info, J.SPLIT_MIN_CHUNK))
        assert n == 0 if c["name"] == "420_17x9_tiny" else n >= 19, (c["name"], n)
    rst = J.parse(S.split_case("420_96x96_rstrows2")["jpeg"])
    assert rst.nseg == 3 and all(J.is_split(int(e - b), _split_all(J)) for b, e in rst.segments[:, :2])
    with pytest.raises(ValueError):
        J.decode_host_split([CASES[0]["jpeg"]], 32, 8)
    with pytest.raises(ValueError):
        J.decode_host_split([CASES[0]["jpeg"]], -1)


def test_chunks_follow_the_documented_rule(J):
    for c in CASES:
        info = J.parse(c["jpeg"])
        for chunk in S.CHUNKS:
            want = []
            for b, e in info.segments[:, :2].tolist():
                if e - b >= 2 * J.SPLIT_MIN_CHUNK:
                    size = max(chunk or J.SPLIT_DEFAULT_CHUNK, (-(-(e - b) // J.SPLIT_THREADS) + 3) // 4 * 4)
                    want += [(at, min(at + size, e)) for at in range(b, e, size)]
            assert J.split_chunks(info, chunk) == want, (c["name"], chunk)
            assert J.split_chunks(info, chunk, split=1 << 20) == []
    big = J.parse(S.split_case("444_64x48_q100")["jpeg"])      # 12998 bytes on 512 lanes: 28 bytes a lane
    assert {e - b for b, e in J.split_chunks(big, 16)[:-1]} == {28} and len(J.split_chunks(big, 16)) <= J.SPLIT_THREADS


@pytest.mark.parametrize("name", NAMES)
def test_split_twin_equals_the_twin_and_the_recorded_decode(J, name):
    c = _case(name)
    info = J.parse(c["jpeg"])
    want = J.decode_host([info])
    assert want.status == [0]
    for chunk in S.CHUNKS:
        got = J.decode_host_split([info], _split_all(J), chunk)
        assert got.status == [0] and got.fallback == [0], (name, chunk)
        assert _differing(got[0], want[0]) == 0, (name, chunk)
        assert hashlib.sha256(got[0].numpy().tobytes()).hexdigest() == c["sha256"], (name, chunk)
        chunks = len(J.split_chunks(info, chunk))
        assert got.rounds[0] <= max(chunks - 1, 0) and (chunks > 0 or got.rounds[0] == 0), (name, chunk, got.rounds, chunks)


def test_segments_below_split_stay_on_the_old_path(J):
    tiny = S.split_case("420_17x9_tiny")["jpeg"]
    info = J.parse(tiny)
    assert int(info.segments[0, 1] - info.segments[0, 0]) < 2 * J.SPLIT_MIN_CHUNK and J.split_chunks(info, J.SPLIT_MIN_CHUNK) == []
    assert J.decode_host_split([info], 1, J.SPLIT_MIN_CHUNK).rounds == [0]
    big = S.split_case("420_160x120")["jpeg"]
    for split in (0, len(big)):      # no segment reaches them
        got = J.decode_host_split([big], split, J.SPLIT_MIN_CHUNK)
        assert got.rounds == [0] and got.fallback == [0] and _differing(got[0], J.decode_host([big])[0]) == 0
    q100 = S.split_case("444_64x48_q100")["jpeg"]      # a scan of 12 998 bytes
    assert 6482 < J.SPLIT_AUTO_BYTES <= 12998 and J.is_split(12998, "auto") and not J.is_split(6482, "auto")
    assert J.decode_host_split([big], "auto").rounds == [0] and J.decode_host_split([q100], "auto").rounds[0] >= 2
    assert J.decode_host_split([q100], "auto").rounds == J.decode_host_split([q100], J.SPLIT_AUTO_BYTES).rounds


# ---------------------------------------------------------------- what the inputs hit
def test_q100_file_has_chunk_boundaries_on_and_behind_stuffed_bytes(J):
    data = S.split_case("444_64x48_q100")["jpeg"]
    bounds = [b for b, _ in J.split_chunks(J.parse(data), J.SPLIT_MIN_CHUNK)[1:]]
    on, behind = S.stuffing_at(data, bounds)
    print(f"{len(bounds)} chunk boundaries: {on} on the 00 of an FF 00 pair, {behind} directly behind one")
    assert on >= 3 and behind >= 3


def test_flat_file_has_a_chunk_with_many_blocks_and_symbols_straddle_boundaries(J):
    info = J.parse(S.split_case("420_128x128_flat_q10")["jpeg"])
    _, ends = S.walk(info)
    assert len(ends) == 64 * 6
    most = max(sum(1 for p in ends if 8 * b < p <= 8 * e) for b, e in J.split_chunks(info, J.SPLIT_MIN_CHUNK))
    print(f"flat file: up to {most} block ends in one {J.SPLIT_MIN_CHUNK}-byte chunk")
    assert most >= 8
    straddled = total = 0
    for name in ("420_160x120", "420_56x40_optimize", "gray_120x90"):
        info = J.parse(S.split_case(name)["jpeg"])
        starts = set(S.walk(info)[0])
        bounds = [8 * b for b, _ in J.split_chunks(info, J.SPLIT_MIN_CHUNK)[1:]]
        straddled += sum(1 for p in bounds if p not in starts)
        total += len(bounds)
    print(f"{straddled} of {total} chunk boundaries lie inside a symbol")
    assert straddled >= total // 2 and straddled >= 100


def test_the_hand_over_loop_iterates(J):
    rounds = {c["name"]: J.decode_host_split([c["jpeg"]], _split_all(J), J.SPLIT_MIN_CHUNK).rounds[0] for c in S.split_cases()}
    print(rounds)
    assert max(rounds.values()) >= 2 and rounds["420_17x9_tiny"] == 0
    # ... and does not crawl: a lane that synchronised by itself keeps its state when a dead one is handed to it
    info = J.parse(S.split_case("420_160x120")["jpeg"])
    assert rounds["420_160x120"] < len(J.split_chunks(info, J.SPLIT_MIN_CHUNK)) // 4


# ---------------------------------------------------------------- damaged scans
def _check_damaged(J, data, chunk, what):
    """bytes and status of the split twin equal the twin's; it falls back exactly where a split segment is damaged"""
    info = J.try_parse(data)
    if isinstance(info, J.JpegUnsupported):
        return None
    want, got = J.decode_host([info]), J.decode_host_split([info], _split_all(J), chunk)
    assert got.status == want.status and _differing(got[0], want[0]) == 0, what
    sizes = [int(e - b) for b, e in info.segments[:, :2]]
    if not (want.status[0] & ERR):
        assert got.fallback == [0], what
    elif all(J.is_split(s, _split_all(J)) for s in sizes):
        assert got.fallback[0] >= 1, what
    assert got.fallback[0] <= sum(J.is_split(s, _split_all(J)) for s in sizes)
    assert got.rounds[0] <= max([len(J.split_chunks(info, chunk)) - 1, 0])
    return want.status[0], got.fallback[0]


@pytest.mark.parametrize("name", ["420_160x120", "422_96x64", "gray_120x90", "420_56x40_optimize"])
def test_truncation_at_every_7th_byte_of_the_scan(J, name):
    data = _case(name)["jpeg"]
    begin = int(J.parse(data).record["scan_begin"][0])
    fell = 0
    for i, cut in enumerate(range(begin, len(data), 7)):
        st, fb = _check_damaged(J, data[:cut], (J.SPLIT_MIN_CHUNK, 64)[i & 1], (name, cut))
        assert st & J.ST_NO_EOI
        fell += fb
    assert fell >= (len(data) - begin) // 7 - 6      # all but the cuts that leave fewer than two chunks, or only the padding off


@pytest.mark.parametrize("name", [c["name"] for c in S.split_cases()] + ["420_47x33_rst2", "444_17x9_q100", "420_33x47_optimize"])
def test_one_flipped_bit_at_200_positions(J, name):
    data = _case(name)["jpeg"]
    g = np.random.default_rng(sum(name.encode()))
    decoded = damaged = 0
    for i in range(200):
        d = bytearray(data)
        d[int(g.integers(len(d)))] ^= 1 << int(g.integers(8))
        r = _check_damaged(J, bytes(d), (J.SPLIT_MIN_CHUNK, 32, 64, 0)[i & 3], (name, i))
        decoded += r is not None
        damaged += r is not None and bool(r[0] & ERR)
    print(f"{name}: {decoded} of 200 decoded, {damaged} with a damaged scan")
    assert decoded >= 100


def test_a_restart_segment_cut_in_half(J):
    data = S.split_case("420_96x96_rstrows2")["jpeg"]
    info = J.parse(data)
    whole = J.decode_host([data])[0]
    for k in range(info.nseg):
        b, e = (int(v) for v in info.segments[k, :2])
        cut = data[:b + (e - b) // 2] + data[e:]
        for chunk in (J.SPLIT_MIN_CHUNK, 64):
            st, fb = _check_damaged(J, cut, chunk, ("rst", k, chunk))
            assert st == J.ST_TRUNCATED and fb == 1
        assert _differing(J.decode_host_split([cut], _split_all(J), 0)[0], whole) > 0
