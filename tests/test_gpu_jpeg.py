"""JPEG decode on the GPU (bvc_op_jpeg_decode, csrc/jpeg.hip) against the host twin (the same csrc/jpeg.h arithmetic compiled for the
host; tests/test_jpeg_host.py ties the twin to the recorded and the live libjpeg-turbo bytes), and JpegClipRing end to end.

Integer arithmetic and no atomics: the bar is ZERO differing bytes and equal status bits everywhere.  The work item of the entropy kernel
is one segment on one lane, so every call here mixes sizes, samplings and restart layouts, and runs at several `lanes`: 0 (the call's
choice - one segment per wave for so few), 64 (a wave's lanes hold different images and finish at different times) and 7 (a wave that
is neither full nor a power of two).  Damaged inputs are only ones that tools/jpeg_host_check.cpp takes through the same reader under
the sanitizers: files cut at a length, and files with one restart segment cut to half."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from tests import jpeg_ref as R   # noqa: E402

bvc = G.bvc
J = bvc.jpeg
dev = torch.device("cuda:0")

FILES = [c["jpeg"] for c in R.decode_cases()]
TWIN = J.decode_host(FILES)      # computed once, never changed
assert TWIN.status == [0] * len(FILES)
SAME_SIZE = ["444_47x33", "422_47x33", "420_47x33", "420_47x33_rst2"]      # four frames of 33 rows x 47 columns


def _same(got, want, what):
    got = [g.cpu() for g in got]
    n = sum(int((g != w).sum()) for g, w in zip(got, want))
    shapes = [tuple(g.shape) for g in got] == [tuple(w.shape) for w in want]
    print(f"{what}: {n} bytes differ from the host twin in {len(want)} images")
    assert shapes and n == 0 and len(got) == len(want), what


@pytest.mark.parametrize("lanes", [0, 64, 7])
def test_all_fixtures_in_one_call_equal_host_twin(lanes):
    got = J.decode(FILES, dev, lanes=lanes)
    assert isinstance(got, list) and got.refused == [] and got.status.dtype == torch.int32
    _same(got, TWIN, f"{len(FILES)} mixed files, lanes {lanes}")
    assert got.status.cpu().tolist() == [0] * len(FILES)


@pytest.mark.parametrize("lanes", [0, 64])
def test_130_files_fill_more_than_two_waves(lanes):
    idx = [(7 * i) % len(FILES) for i in range(130)]
    files = [FILES[i] for i in idx]
    assert sum(J.parse(f).nseg for f in files) > 128
    got = J.decode(files, dev, lanes=lanes)
    _same(got, [TWIN[i] for i in idx], f"130 files, lanes {lanes}")
    assert not bool(got.status.any())


def test_out_and_infos_given_by_the_caller():
    infos = [J.try_parse(f) for f in FILES]
    total = sum(t.numel() for t in TWIN)
    buf = torch.full((total + 7,), 201, dtype=torch.uint8, device=dev)
    got = J.decode(None, dev, out=buf, infos=infos, lanes=64)
    _same(got, TWIN, "out= and infos=")
    assert got[0].data_ptr() == buf.data_ptr() and bool((buf[total:] == 201).all())
    files = [R.case(n)["jpeg"] for n in SAME_SIZE]
    out = torch.empty(4, 3, 33, 47, dtype=torch.uint8, device=dev)
    got = J.decode(files, dev, out=out, check=True)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (4, 3, 33, 47)
    _same(list(got), J.decode_host(files), "uniform batch into out=")
    with pytest.raises(ValueError):
        J.decode(files, dev, out=torch.empty(4, 3, 33, 48, dtype=torch.uint8, device=dev))


def test_a_refused_file_leaves_zeros_and_its_neighbours_alone():
    prog = R.case("420_47x33_progressive")["jpeg"]
    files = [R.case(n)["jpeg"] for n in SAME_SIZE]
    mixed = files[:2] + [prog] + files[2:]
    for out in (None, torch.full((5, 3, 33, 47), 9, dtype=torch.uint8, device=dev)):
        got = J.decode(mixed, dev, out=out, lanes=64)
        assert tuple(got.shape) == (5, 3, 33, 47) and got.refused == [(2, "progressive")]
        assert not bool(got[2].any()) and got.status.cpu().tolist() == [0] * 5
        _same([got[i] for i in (0, 1, 3, 4)], J.decode_host(files), "neighbours of a refused file")
    got = J.decode([FILES[0], prog, FILES[1]], dev)      # mixed sizes: a list, the refused one of zero size
    assert got.refused == [(1, "progressive")] and got[1].numel() == 0
    _same([got[0], got[2]], TWIN[:2], "neighbours of a refused file, mixed sizes")


def test_truncated_files_raise_their_status_and_equal_the_twin():
    whole = R.case("420_47x33")["jpeg"]
    begin = int(J.parse(whole).record["scan_begin"][0])
    cut_mid = whole[:begin + (len(whole) - begin) // 2]
    rst = R.case("420_47x33_rst2")["jpeg"]
    b, e = (int(v) for v in J.parse(rst).segments[2, :2])
    cut_seg = rst[:b + (e - b) // 2] + rst[e:]
    files = [whole, cut_mid, rst, cut_seg]
    want = J.decode_host(files)
    assert want.status == [0, J.ST_TRUNCATED | J.ST_NO_EOI, 0, J.ST_TRUNCATED]
    for lanes in (0, 64):
        got = J.decode(files, dev, lanes=lanes)
        assert got.status.cpu().tolist() == want.status
        _same(list(got), want, f"two truncated files, lanes {lanes}")
    with pytest.raises(J.JpegDecodeError) as err:
        J.decode(files, dev, check=True)
    assert err.value.status.tolist() == want.status


def test_clip_ring_decodes_what_decode_does_and_feeds_clip_transform():
    files = [R.case(n)["jpeg"] for n in SAME_SIZE]
    batches = [files, files[::-1], files[2:] + files[:2]]
    ring = J.JpegClipRing((2, 2, 33, 47), dev, depth=2, max_bytes=1 << 16)
    tf = bvc.ClipTransform(16, augs="n")
    assert ring.stage(batches[0]) and ring.stage([batches[1][:2], batches[1][2:]]) and not ring.stage(batches[2])
    for i, batch in enumerate(batches):
        clips = ring.get()
        assert tuple(clips.shape) == (2, 2, 3, 33, 47) and clips.dtype == torch.uint8
        direct = J.decode(batch, dev)
        twin = torch.stack(list(J.decode_host(batch))).view(2, 2, 3, 33, 47)
        assert torch.equal(clips, direct.view_as(clips)) and torch.equal(clips.cpu(), twin)
        assert not bool(clips.status.any())
        assert torch.equal(tf(clips), tf(twin.to(dev)))
        ring.release()
        if i == 0:
            assert ring.stage(batches[2])
    with pytest.raises(RuntimeError):
        ring.get()
    with pytest.raises(ValueError, match="33 x 47"):
        ring.stage([FILES[0]] + files[1:])
    with pytest.raises(J.JpegUnsupported):
        ring.stage([R.case("420_47x33_progressive")["jpeg"]] + files[1:])


def test_decoding_twice_and_deterministic_mode_change_nothing():
    a = J.decode(FILES, dev, lanes=64)
    b = J.decode(FILES, dev, lanes=64)
    bvc.use_deterministic_algorithms(True)
    try:
        c = J.decode(FILES, dev, lanes=64)
    finally:
        bvc.use_deterministic_algorithms(False)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.equal(a.status, b.status) and torch.equal(a.status, c.status)
