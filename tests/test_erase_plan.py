"""Random erasing on the host: the counter function of tests/erase_ref.py against known answers, the plan ``bvc.RandomErasing`` draws
(share erased, box geometry, reproducibility, the call offset) and the table a ``ClipErase`` holds.  No GPU: ``device="cpu"`` yields
no device table and no library call."""
import math

import numpy as np
import pytest
import torch

from tests import erase_ref as E

H, W = 64, 48


def _re(bvc, seed=0, **kw):
    args = dict(probability=0.25, mode="pixel", generator=np.random.default_rng(seed))
    args.update(kw)
    return bvc.RandomErasing(**args)


# ---------------------------------------------------------------- counter function
def test_philox_known_answers():
    """the Random123 known-answer vectors of philox4x32-10: all-zero counter and key, all-ones, and the digits of pi"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = E.philox4x32_10(*[np.array([c], dtype=np.uint64) for c in ctr], *key)
        assert tuple(int(g[0]) for g in got) == want


def test_philox_equals_the_librarys_host_generator(bvc):
    """bvc_dropout_mask_host drops element e when draw e & 3 of counter {e >> 2, (2 layer + branch) << 8, offset} is below p 2^32:
    the numpy function reproduces its keep bytes, at two thresholds"""
    seed, offset, layer, branch, M, N = 0x1234567887654321, 0x0000000500000007, 3, 1, 8, 64
    q = np.arange(M * N // 4, dtype=np.uint64)
    r = np.stack(E.philox4x32_10(q, np.uint64((2 * layer + branch) << 8), offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32), axis=-1)
    for p in (0.5, 0.1):
        keep = bvc.dropgate.dropout_mask_host(seed, offset, layer, branch, M, N, p).numpy().reshape(-1)
        thr = int(np.float64(np.float32(p)) * 4294967296.0)
        assert np.array_equal(keep, (r.reshape(-1) >= thr).astype(np.uint8))


def test_normals_follow_the_rule():
    """lane layout and the uniforms' ranges: u1 in (0, 1], u2 in [0, 1), |z| <= sqrt(-2 ln 2^-24) = 5.77; f32 evaluation close to f64"""
    r = E.draws(7, 3, np.arange(4096, dtype=np.uint64), E.TAG_PIXEL)
    z = E.normals(r)
    u1 = ((r[0] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (r[1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1) and np.array_equal(u2.astype(np.float32).astype(np.float64), u2)
    assert np.allclose(z[:, 0], np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2), rtol=0, atol=1e-12)
    assert np.allclose(z[:, 1], np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2), rtol=0, atol=1e-12)
    assert np.abs(z).max() <= math.sqrt(-2 * math.log(2.0 ** -24)) + 1e-12
    assert np.abs(E.normals(r, np.float32).astype(np.float64) - z).max() < 1e-5
    # the two tags and two offsets are different streams; pixel_noise / colours lay the lanes out in element order
    assert not np.array_equal(r[0], E.draws(7, 3, np.arange(4096, dtype=np.uint64), E.TAG_COLOUR)[0])
    assert not np.array_equal(r[0], E.draws(7, 4, np.arange(4096, dtype=np.uint64), E.TAG_PIXEL)[0])
    assert np.array_equal(E.pixel_noise(7, 3, 2, 2, 4, 16, 16).reshape(-1, 4), z[:1024])
    assert np.array_equal(E.colours(7, 3, 2, 2).reshape(-1, 4), E.normals(E.draws(7, 3, np.arange(16, dtype=np.uint64), E.TAG_COLOUR)))


# ---------------------------------------------------------------- draws
def test_share_erased_is_binomial(bvc):
    n, p = 4000, 0.25
    er = _re(bvc, seed=1)(n, image_size=(H, W), device="cpu")
    assert er.table is None and er.batch_size == n and er.num_boxes == 1
    k = int(er.erased.sum())
    assert abs(k - n * p) <= 5 * math.sqrt(n * p * (1 - p))
    assert (er.modes == 2).all()
    assert int(_re(bvc, probability=0.0)(50, image_size=(H, W)).erased.sum()) == 0
    assert int(_re(bvc, probability=1.0)(50, image_size=(H, W)).erased.sum()) == 50


@pytest.mark.parametrize("counts", [(1, None), (1, 4), (2, 3)])
def test_boxes_follow_the_rule(bvc, counts):
    """the draws by hand, in the documented order, on a generator with the same seed: every box equal, inside the image, h < H, w < W,
    and |h w - area| <= 0.5 (h + w) + 0.25 (h and w are sqrt(area aspect) and sqrt(area / aspect) rounded, each off by at most 0.5)"""
    lo, hi = counts
    re = _re(bvc, seed=5, probability=0.6, min_count=lo, max_count=hi)
    g = np.random.default_rng(5)
    assert re.seed == int(g.integers(0, 2 ** 63))
    er = re(300, image_size=(H, W), device="cpu")
    nmax = hi if hi is not None else lo
    assert er.boxes.shape == (300, nmax, 4)
    seen = set()
    for b in range(300):
        want = []
        if g.random() < 0.6:
            count = int(g.integers(lo, hi + 1)) if hi is not None else lo
            for _ in range(count):
                for _ in range(10):
                    area = float(g.uniform(0.02, 1 / 3)) * H * W / count
                    aspect = math.exp(float(g.uniform(math.log(0.3), math.log(1 / 0.3))))
                    h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
                    if h < H and w < W:
                        top, left = int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1))
                        assert abs(h * w - area) <= 0.5 * (h + w) + 0.25
                        want.append([top, top + h, left, left + w])
                        break
            seen.add(len(want))
        got = [list(v) for v in er.boxes[b].tolist()]
        assert got[:len(want)] == want and all(v == [0, 0, 0, 0] for v in got[len(want):])
        for y0, y1, x0, x1 in want:
            assert 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W and y1 - y0 < H and x1 - x0 < W
    assert seen >= set(range(lo, nmax + 1))          # every count occurred


def test_fixed_seed_reproduces_and_offset_advances(bvc):
    a, b = _re(bvc, seed=9, probability=0.5), _re(bvc, seed=9, probability=0.5)
    for call in range(3):
        ea, eb = a(16, image_size=(H, W)), b(16, image_size=(H, W))
        assert np.array_equal(ea.boxes, eb.boxes) and ea.seed == eb.seed == a.seed
        assert ea.offset == eb.offset == call
    assert a.offset == 3
    assert _re(bvc, seed=10).seed != a.seed
    assert not np.array_equal(_re(bvc, seed=10, probability=0.5)(16, image_size=(H, W)).boxes, _re(bvc, seed=9, probability=0.5)(16, image_size=(H, W)).boxes)


def test_bad_arguments(bvc):
    with pytest.raises(ValueError):
        _re(bvc, max_count=5)
    with pytest.raises(ValueError):
        _re(bvc, min_count=0)
    with pytest.raises(ValueError):
        _re(bvc, min_count=3, max_count=2)
    with pytest.raises(ValueError):
        _re(bvc, mode="noise")
    with pytest.raises(ValueError):
        _re(bvc, probability=1.5)
    with pytest.raises(ValueError):
        bvc.ClipErase(np.zeros((2, 5, 4)), "pixel")
    with pytest.raises(ValueError):
        bvc.ClipErase(np.zeros((2, 2, 4)), ["pixel", "const", "rand"])


# ---------------------------------------------------------------- tables
def test_clip_erase_layout(bvc):
    er = bvc.ClipErase([[(1, 5, 2, 6), (0, 0, 0, 0)], [(3, 4, 5, 6), (7, 8, 9, 10)]], [["const", "pixel"], ["rand", 2]], seed=2 ** 63 + 5, offset=7,
                       image_size=(H, W))
    assert er.table is None and er.batch_size == 2 and er.num_boxes == 2 and er.image_size == (H, W)
    assert er.boxes.dtype == np.int32 and er.modes.dtype == np.int32
    assert er.modes.tolist() == [[0, 2], [1, 2]] and er.erased.tolist() == [True, True]
    assert er.seed == 2 ** 63 + 5 and er.offset == 7
    one = bvc.ClipErase([(1, 5, 2, 6), (0, 0, 0, 0)], "rand")          # [B, 4]: one box per clip, one mode for all
    assert one.boxes.shape == (2, 1, 4) and one.modes.tolist() == [[1], [1]] and one.erased.tolist() == [True, False]
    assert bvc.erase.MODES == {"const": 0, "rand": 1, "pixel": 2} and bvc.erase.MAX_BOXES == 4


def test_new_symbols_are_in_the_library_table(bvc):
    import ctypes
    S = bvc._lib.SYMBOLS
    for name in ("bvc_videomae_cls_set_erase", "bvc_videomae_encoder_set_erase"):
        assert S[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p])
    assert len(S["bvc_op_gather_patches_aug"][1]) == 18 and S["bvc_op_gather_patches_aug"][1][7:9] == [ctypes.c_uint64] * 2
    assert len(S["bvc_op_erase_noise"][1]) == 10


def test_erase_clips_reference():
    g = torch.Generator().manual_seed(0)
    px = torch.randn(2, 2, 3, 8, 8, generator=g)
    noise, col = torch.randn(2, 2, 3, 8, 8, generator=g), torch.randn(2, 2, 4, 4, generator=g)
    out = E.erase_clips(px, [[(2, 6, 1, 5), (4, 8, 3, 7)], [(0, 0, 0, 0), (0, 8, 0, 4)]], [[2, 0], [2, 1]], noise, col)
    assert torch.equal(out[0, :, :, 2:4, 1:5], noise[0, :, :, 2:4, 1:5]) and torch.equal(out[0, :, :, 4:6, 1:3], noise[0, :, :, 4:6, 1:3])
    assert (out[0, :, :, 4:8, 3:7] == 0).all()                             # the later box wins where they overlap
    assert torch.equal(out[0, :, :, :2], px[0, :, :, :2])
    for t in range(2):
        for c in range(3):
            assert (out[1, t, c, :, :4] == col[1, t, 1, c]).all()
    assert torch.equal(out[1, :, :, :, 4:], px[1, :, :, :, 4:])


def test_eval_mode_and_batch_mismatch_raise(bvc):
    m = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(image_size=32, num_frames=2, hidden_size=64, num_hidden_layers=1,
                                                             num_attention_heads=1, intermediate_size=64, num_labels=10))
    er = bvc.ClipErase([(0, 8, 0, 8)] * 2, "pixel", image_size=(32, 32))
    with pytest.raises(ValueError, match="eval mode"):
        m.eval()(pixel_values=torch.zeros(2, 2, 3, 32, 32), erase=er)
    with pytest.raises(ValueError, match="batch of 2"):
        m.train()(pixel_values=torch.zeros(3, 2, 3, 32, 32), erase=er)
