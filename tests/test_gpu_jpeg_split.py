"""The split path of the JPEG decode on the GPU (bvc_op_jpeg_decode_split, csrc/jpeg.hip: jpeg_split_kernel, jpeg_idct_kernel and the
flagged fall-back) against the host twins: decode_host for bytes and status, decode_host_split for the round counts - the algorithm is
deterministic, so the device must take exactly the twin's rounds.  tests/test_jpeg_split_host.py ties the split twin to the one-lane
twin and to libjpeg-turbo, and proves what the fixtures hit.

Zero differing bytes, equal status bits, `.fallback` zero on undamaged files and one on damaged ones.  Damaged inputs are only of kinds
that tools/jpeg_split_host_check.cpp takes through the same jpeg.h functions under the sanitizers: files cut at a length and a restart
segment cut to half."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G          # noqa: E402
from tests import jpeg_ref as R          # noqa: E402
from tests import jpeg_split_ref as S    # noqa: E402

bvc = G.bvc
J = bvc.jpeg
dev = torch.device("cuda:0")

CASES = R.decode_cases() + S.split_cases()
NAMES = [c["name"] for c in CASES]
FILES = [c["jpeg"] for c in CASES]
INFOS = [J.parse(f) for f in FILES]
TWIN = J.decode_host(INFOS)      # computed once, never changed
assert TWIN.status == [0] * len(FILES)
MIN = J.SPLIT_MIN_CHUNK
ALL = 2 * MIN          # splits everything splittable
MIXED = 1780           # the files with restart intervals, the tiny ones and the flat one stay on the one-lane path
SAME_SIZE = ["444_47x33", "422_47x33", "420_47x33", "420_47x33_rst2"]      # four frames of 33 rows x 47 columns


@pytest.fixture(scope="module")
def twin_rounds():
    cache = {}

    def get(split, chunk):
        if (split, chunk) not in cache:
            got = J.decode_host_split(INFOS, split, chunk)
            assert got.fallback == [0] * len(FILES) and got.status == TWIN.status
            cache[split, chunk] = got.rounds
        return cache[split, chunk]
    return get


def _same(got, want, what):
    got = [g.cpu() for g in got]
    n = sum(int((g != w).sum()) for g, w in zip(got, want))
    shapes = [tuple(g.shape) for g in got] == [tuple(w.shape) for w in want]
    print(f"{what}: {n} bytes differ from the host twin in {len(want)} images")
    assert shapes and n == 0 and len(got) == len(want), what


def test_the_mixed_call_mixes():
    split = {n: sum(J.is_split(int(e - b), MIXED) for b, e in i.segments[:, :2]) for n, i in zip(NAMES, INFOS)}
    assert all(split[n] == 0 for n in NAMES if "rst" in n or "tiny" in n or n in ("420_1x1", "420_7x5", "gray_8x8", "420_17x9_q5"))
    assert sum(split.values()) == 6 and split["420_56x40_optimize"] == split["444_64x48_q100"] == split["444_47x33"] == 1


@pytest.mark.parametrize("lanes", [0, 64])
@pytest.mark.parametrize("chunk", [MIN, 64, 0])
def test_all_fixtures_in_one_mixed_call_equal_the_twins(twin_rounds, chunk, lanes):
    got = J.decode(FILES, dev, lanes=lanes, split=MIXED, chunk=chunk)
    assert isinstance(got, list) and got.refused == [] and got.status.dtype == got.fallback.dtype == got.rounds.dtype == torch.int32
    assert got.fallback.device.type == "cuda" and tuple(got.fallback.shape) == tuple(got.rounds.shape) == (len(FILES),)
    _same(got, TWIN, f"{len(FILES)} files, 6 of them split, chunk {chunk}, lanes {lanes}")
    assert got.status.cpu().tolist() == [0] * len(FILES) and got.fallback.cpu().tolist() == [0] * len(FILES)
    rounds = got.rounds.cpu().tolist()
    print("rounds", dict(zip(NAMES, rounds)))
    assert rounds == twin_rounds(MIXED, chunk) and max(rounds) >= 2


@pytest.mark.parametrize("chunk", [MIN, 32])
def test_every_splittable_segment_split(twin_rounds, chunk):
    got = J.decode(None, dev, infos=INFOS, split=ALL, chunk=chunk)
    _same(got, TWIN, f"every segment of {ALL} bytes or more split, chunk {chunk}")
    assert not bool(got.status.any()) and not bool(got.fallback.any())
    assert got.rounds.cpu().tolist() == twin_rounds(ALL, chunk)


def test_130_files_make_more_workgroups_than_a_wave_of_launches_places():
    rst = [NAMES.index(n) for n in ("420_65x17_rst1", "420_47x33_rst2", "420_96x96_rstrows2", "422_40x24_rstrow")]
    idx = [(7 * i) % len(FILES) for i in range(100)] + [rst[i % 4] for i in range(30)]      # the last 30 with several segments each
    infos = [INFOS[i] for i in idx]
    split = sum(J.is_split(int(e - b), ALL) for i in infos for b, e in i.segments[:, :2])
    print(f"130 files, {sum(i.nseg for i in infos)} segments, {split} of them split")
    assert len(idx) == 130 and split > 256      # one workgroup per split segment, 256 CUs
    want = J.decode_host_split(infos, ALL, MIN)
    for lanes in (0, 64):
        got = J.decode(None, dev, infos=infos, lanes=lanes, split=ALL, chunk=MIN)
        _same(got, [TWIN[i] for i in idx], f"130 files, lanes {lanes}")
        assert not bool(got.status.any()) and not bool(got.fallback.any()) and got.rounds.cpu().tolist() == want.rounds


def test_out_and_infos_given_by_the_caller():
    total = sum(t.numel() for t in TWIN)
    buf = torch.full((total + 7,), 201, dtype=torch.uint8, device=dev)
    got = J.decode(None, dev, out=buf, infos=INFOS, lanes=64, split=ALL, chunk=MIN)
    _same(got, TWIN, "out= and infos=")
    assert got[0].data_ptr() == buf.data_ptr() and bool((buf[total:] == 201).all())
    files = [R.case(n)["jpeg"] for n in SAME_SIZE]
    out = torch.empty(4, 3, 33, 47, dtype=torch.uint8, device=dev)
    got = J.decode(files, dev, out=out, check=True, split="auto", chunk=MIN)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (4, 3, 33, 47) and tuple(got.rounds.shape) == (4,)
    _same(list(got), J.decode_host(files), "uniform batch into out=")
    with pytest.raises(ValueError):
        J.decode(files, dev, split=ALL, chunk=MIN - 1)
    with pytest.raises(ValueError):
        J.decode(files, dev, split=-5)


def test_a_refused_file_leaves_zeros_and_its_neighbours_alone():
    prog = R.case("420_47x33_progressive")["jpeg"]
    files = [R.case(n)["jpeg"] for n in SAME_SIZE]
    mixed = files[:2] + [prog] + files[2:]
    want = J.decode_host_split(files, ALL, MIN)
    for out in (None, torch.full((5, 3, 33, 47), 9, dtype=torch.uint8, device=dev)):
        got = J.decode(mixed, dev, out=out, lanes=64, split=ALL, chunk=MIN)
        assert tuple(got.shape) == (5, 3, 33, 47) and got.refused == [(2, "progressive")]
        assert not bool(got[2].any()) and got.status.cpu().tolist() == [0] * 5 and got.fallback.cpu().tolist() == [0] * 5
        assert got.rounds.cpu().tolist() == want.rounds[:2] + [0] + want.rounds[2:]
        _same([got[i] for i in (0, 1, 3, 4)], J.decode_host(files), "neighbours of a refused file")


def test_damaged_files_fall_back_and_equal_the_twin():
    whole = S.split_case("420_160x120")["jpeg"]
    begin = int(J.parse(whole).record["scan_begin"][0])
    cut_mid = whole[:begin + (len(whole) - begin) // 2]
    other = S.split_case("422_96x64")["jpeg"]
    cut_third = other[:int(J.parse(other).record["scan_begin"][0]) + 1500]
    rst = S.split_case("420_96x96_rstrows2")["jpeg"]
    b, e = (int(v) for v in J.parse(rst).segments[1, :2])
    cut_seg = rst[:b + (e - b) // 2] + rst[e:]
    files = [whole, cut_mid, rst, cut_seg, other, cut_third, whole]
    want = J.decode_host(files)
    assert want.status == [0, J.ST_TRUNCATED | J.ST_NO_EOI, 0, J.ST_TRUNCATED, 0, J.ST_TRUNCATED | J.ST_NO_EOI, 0]
    assert J.decode_host_split(files, ALL, MIN).fallback == [0, 1, 0, 1, 0, 1, 0]
    for lanes, chunk in ((0, MIN), (64, 64)):
        got = J.decode(files, dev, lanes=lanes, split=ALL, chunk=chunk)
        assert got.status.cpu().tolist() == want.status
        assert got.fallback.cpu().tolist() == [0, 1, 0, 1, 0, 1, 0]
        _same(list(got), want, f"three damaged files among good ones, lanes {lanes}, chunk {chunk}")
        assert got.rounds.cpu().tolist() == J.decode_host_split(files, ALL, chunk).rounds
    with pytest.raises(J.JpegDecodeError) as err:
        J.decode(files, dev, check=True, split=ALL)
    assert err.value.status.tolist() == want.status


def test_clip_ring_with_split_decodes_what_decode_does_and_feeds_clip_transform():
    files = [R.case(n)["jpeg"] for n in SAME_SIZE]
    batches = [files, files[::-1], files[2:] + files[:2]]
    ring = J.JpegClipRing((2, 2, 33, 47), dev, depth=2, max_bytes=1 << 16, split=ALL, chunk=MIN)
    plain = J.JpegClipRing((2, 2, 33, 47), dev, depth=2, max_bytes=1 << 16)
    assert ring.work.numel() > 3 * plain.work.numel() and (ring.split, ring.chunk, plain.split) == (ALL, MIN, 0)
    tf = bvc.ClipTransform(16, augs="n")
    assert ring.stage(batches[0]) and ring.stage([batches[1][:2], batches[1][2:]]) and not ring.stage(batches[2])
    for i, batch in enumerate(batches):
        clips = ring.get()
        assert tuple(clips.shape) == (2, 2, 3, 33, 47) and clips.dtype == torch.uint8
        direct = J.decode(batch, dev, split=ALL, chunk=MIN)
        twin = torch.stack(list(J.decode_host(batch))).view(2, 2, 3, 33, 47)
        assert torch.equal(clips, direct.view_as(clips)) and torch.equal(clips.cpu(), twin)
        assert not bool(clips.status.any()) and not bool(clips.fallback.any())
        assert clips.rounds.cpu().tolist() == J.decode_host_split(batch, ALL, MIN).rounds == direct.rounds.cpu().tolist()
        assert torch.equal(tf(clips), tf(twin.to(dev)))
        ring.release()
        if i == 0:
            assert ring.stage(batches[2])


def test_decoding_twice_and_deterministic_mode_change_nothing():
    a = J.decode(None, dev, infos=INFOS, lanes=64, split=ALL, chunk=MIN)
    b = J.decode(None, dev, infos=INFOS, lanes=64, split=ALL, chunk=MIN)
    bvc.use_deterministic_algorithms(True)
    try:
        c = J.decode(None, dev, infos=INFOS, lanes=64, split=ALL, chunk=MIN)
    finally:
        bvc.use_deterministic_algorithms(False)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    for name in ("status", "fallback", "rounds"):
        assert torch.equal(getattr(a, name), getattr(b, name)) and torch.equal(getattr(a, name), getattr(c, name))


def test_split_0_is_the_one_lane_path_and_gives_the_same_tensor():
    one = J.decode(None, dev, infos=INFOS)
    two = J.decode(None, dev, infos=INFOS, split=ALL, chunk=MIN)
    assert all(torch.equal(x, y) for x, y in zip(one, two)) and torch.equal(one.status, two.status)
    assert not bool(one.rounds.any()) and not bool(one.fallback.any()) and bool(two.rounds.any())
