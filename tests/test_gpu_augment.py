"""Clip transforms on the GPU (bvc_op_clip_transform, csrc/augment.hip) against the host twin (the same csrc/augment.h arithmetic
compiled for the host) and against the oracle of tests/augment_ref.py, with the cases and bars of tests/test_augment_host.py.

Against the host twin: max |diff| <= 1 LSB and a differing share of at most the case's share of oracle near-tie elements (for pure
geometry that share is zero: the kernels must reproduce the twin bit for bit).  Against the oracle: the CPU bars.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import videomae_oracle as vo   # noqa: E402
from tests import augment_ref as R   # noqa: E402
from tests import gpu_util as G   # noqa: E402
from tests import test_augment_host as H   # noqa: E402

bvc = G.bvc
A = bvc.augment
dev = torch.device("cuda:0")


def _gpu(x, t, size):
    out = A.clip_transform(x.to(dev), t, size)
    torch.cuda.synchronize()
    return out.cpu()


def _check_twin(got, host, near_share, what):
    d = (got.int() - host.int()).abs()
    share = float((d > 0).float().mean())
    print(f"{what}: GPU vs host twin: max |diff| {int(d.max())}, differing share {share:.4%} (near-tie share {near_share:.4%})")
    assert int(d.max()) <= 1, what
    assert share <= near_share, f"{what}: {share:.4%} of the elements differ from the host twin"


@pytest.mark.parametrize("Hs,Ws,Ho,Wo", H.RESIZE_SHAPES + [(16, 16, 16, 16)])
def test_resize_shapes(Hs, Ws, Ho, Wo):
    x = H._frames(2, Hs, Ws, seed=Hs * 1000 + Ws)
    t = H._whole(A, 2, Hs, Ws, Ho, Wo)
    t["flip"][1] = 1
    got = _gpu(x, t, (Ho, Wo))
    _check_twin(got, A.clip_transform_host(x, t, (Ho, Wo)), 0.0, f"{Hs}x{Ws}->{Ho}x{Wo}")
    H._check_resize(got, torch.stack([R.resize_window(x, e, Ho, Wo) for e in t]), f"{Hs}x{Ws}->{Ho}x{Wo}")
    if (Hs, Ws) == (Ho, Wo):
        assert torch.equal(got[0], x[0]) and torch.equal(got[1], x[1].flip(-1))


def test_center_crop_border_boxes_and_exact_crops():
    for Hs, Ws, S in [(48, 64, 32), (64, 48, 32), (37, 53, 16)]:
        x = H._frames(2, Hs, Ws, seed=3)
        t = A.center_crop_params(2, (Hs, Ws), S)
        got = _gpu(x, t, S)
        _check_twin(got, A.clip_transform_host(x, t, S), 0.0, f"centre crop {Hs}x{Ws}")
        H._check_resize(got, torch.stack([R.resize_window(x, e, S, S) for e in t]), f"centre crop {Hs}x{Ws}")
    Hs, Ws, S = 45, 61, 16
    x = H._frames(1, Hs, Ws, seed=4)
    boxes = [(0, 0, 30, 25), (Ws - 33, 0, 33, 20), (0, Hs - 27, 22, 27), (Ws - 40, Hs - 31, 40, 31), (0, 0, Ws, Hs), (0, 10, Ws, 9),
             (20, 0, 7, Hs), (Ws - 16, Hs - 16, 16, 16), (3, 5, 16, 16)]
    t = A.empty_table(len(boxes))
    for e, (x0, y0, w, h) in zip(t, boxes):
        e["x0"], e["y0"], e["w"], e["h"], e["Hr"], e["Wr"] = x0, y0, w, h, S, S
    got = _gpu(x, t, S)
    _check_twin(got, A.clip_transform_host(x, t, S), 0.0, "border boxes")
    for i, e in enumerate(t):
        H._check_resize(got[i], R.resize_window(x, e, S, S), f"box {boxes[i]}")
    assert torch.equal(got[7], x[0, :, Hs - 16:, Ws - 16:]) and torch.equal(got[8], x[0, :, 5:21, 3:19])


def test_each_colour_stage_alone():
    x = H._colour_frame()
    t = np.concatenate([H._stage_table(A, op, f) for op, f in H.STAGE_CASES])
    got = _gpu(x, t, 32)
    host = A.clip_transform_host(x, t, 32)
    want, near = R.transform(x, t, 32, 32)
    for i, (op, f) in enumerate(H.STAGE_CASES):
        _check_twin(got[i], host[i], float(near[i].float().mean()), f"op {op} factor {f}")
        H.check_against_colour_oracle(got[i], want[i], near[i], f"op {op} factor {f}")
        if op != "gray" and f == (0.0 if op == R.HUE else 1.0):
            assert torch.equal(got[i], x[0])


def test_full_chains_after_a_real_resize():
    x = H._frames(24, 40, 52, seed=6).view(2, 12, 3, 40, 52)
    t = H.chain_table(A, 40, 52, 24, seed=7)
    got = _gpu(x, t, 24)
    host = A.clip_transform_host(x, t, 24)
    _, near = R.transform(x.view(24, 3, 40, 52), t, 24, 24)
    for i in range(48):
        _check_twin(got[i], host[i], float(near[i].float().mean()), f"chain {i}")
    H.check_chains(got, x.view(24, 3, 40, 52), t, 24, "GPU")


@pytest.fixture(scope="module")
def tile_case():
    """2 frames of 256 x 340 -> 224 x 224 (Resize(224) + CenterCrop(224): 49 tiles per frame) with the full chain, contrast first in
    one frame and last in the other, one mirrored, one grayscale"""
    x = H._frames(2, 256, 340, seed=10)
    t = A.center_crop_params(2, (256, 340), 224)
    t["nops"] = 4
    t["order"] = [A.pack_order([1, 0, 3, 2]), A.pack_order([2, 3, 0, 1])]
    t["factor"] = [(1.3, 0.7, 1.6, 0.07), (0.8, 1.5, 0.4, -0.15)]
    t["flip"], t["gray"] = [0, 1], [0, 1]
    return x, t


def test_real_tile_geometry(tile_case):
    x, t = tile_case
    got = _gpu(x, t, 224)
    host = A.clip_transform_host(x, t, 224)
    _, near = R.transform(x, t, 224, 224)
    for i in range(2):
        _check_twin(got[i], host[i], float(near[i].float().mean()), f"256x340->224x224 frame {i}")
    H.check_chains(got, x, t, 224, "GPU 224")


def test_output_size_that_is_no_multiple_of_the_tile():
    x = H._frames(3, 57, 71, seed=11)
    t = H.chain_table(A, 57, 71, 40, seed=12)[[0, 13, 47]]
    t["src"] = [0, 1, 2]
    got = _gpu(x, t, 40)
    host = A.clip_transform_host(x, t, 40)
    _, near = R.transform(x, t, 40, 40)
    for i in range(3):
        _check_twin(got[i], host[i], float(near[i].float().mean()), f"40x40 frame {i}")
    H.check_chains(got, x, t, 40, "GPU 40")


def test_a_tile_whose_rows_need_more_source_rows_than_one_group_holds():
    """a 6-fold vertical shrink: 32 output rows read about 200 source rows, more than the 80 the kernel holds at a time"""
    x = H._frames(1, 400, 70, seed=13)
    t = H._whole(A, 1, 400, 70, 64, 48)
    got = _gpu(x, t, (64, 48))
    _check_twin(got, A.clip_transform_host(x, t, (64, 48)), 0.0, "400x70->64x48")
    H._check_resize(got, torch.stack([R.resize_window(x, e, 64, 48) for e in t]), "400x70->64x48")


def test_repeatable_deterministic_mode_and_guard_band(tile_case):
    x, t = tile_case
    xd = x.to(dev)
    n = 2 * 3 * 224 * 224
    guard = 4096
    runs = []
    for det in (False, False, True):
        bvc.use_deterministic_algorithms(det)
        try:
            buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device=dev)
            A.clip_transform(xd, t, 224, out=buf[guard:guard + n])
            torch.cuda.synchronize()
        finally:
            bvc.use_deterministic_algorithms(False)
        assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + n:] == 0xA5).all()), "bytes outside the output were written"
        runs.append(buf[guard:guard + n].cpu())
    assert torch.equal(runs[0], runs[1]), "two runs of one call differ"
    assert torch.equal(runs[0], runs[2]), "deterministic mode changes the result"
    # an odd-sized output at an odd byte offset: the unaligned path of the second pass
    x2 = H._frames(1, 30, 33, seed=14)
    t2 = H.chain_table(A, 30, 33, 21, seed=15)[[5]]
    t2["src"] = 0
    n2 = 3 * 21 * 21
    buf = torch.full((guard + 1 + n2 + guard,), 0xA5, dtype=torch.uint8, device=dev)
    A.clip_transform(x2.to(dev), t2, 21, out=buf[guard + 1:guard + 1 + n2])
    torch.cuda.synchronize()
    assert bool((buf[:guard + 1] == 0xA5).all()) and bool((buf[guard + 1 + n2:] == 0xA5).all())
    assert torch.equal(buf[guard + 1:guard + 1 + n2].cpu().view(1, 3, 21, 21), A.clip_transform_host(x2, t2, 21))


def test_device_refusals():
    Err = bvc._lib.BvcError
    x = torch.zeros(1, 3, 32, 32, dtype=torch.uint8, device=dev)
    good = H._whole(A, 1, 32, 32, 16, 16)
    for field, value, msg in [("w", 0, "empty region"), ("x0", 1, "outside"), ("ox", 1, "window")]:
        bad = good.copy()
        bad[field] = value
        with pytest.raises(Err, match=msg):
            A.clip_transform(x, bad, 16)
    with pytest.raises(Err, match="channels"):
        A.clip_transform(torch.zeros(1, 1, 32, 32, dtype=torch.uint8, device=dev), good, 16)


def test_transformed_clips_feed_the_models_like_the_host_twins():
    """ClipTransform's output is an ordinary uint8 clip: VideoMAE pre-training and the JEPA ViT-Tiny encoder give, bit for bit, what
    they give on the host twin's tensor for the same table"""
    cfg = vo.TINY
    g = torch.Generator().manual_seed(16)
    src = torch.randint(0, 256, (2, cfg.num_frames, 3, 80, 100), generator=g, dtype=torch.uint8)
    tf = A.ClipTransform(cfg.image_size, augs="cjg", crop_scale=(0.3, 1.0), flip=0.5, consistent=False, generator=np.random.default_rng(17))
    clips = tf(src.to(dev))
    assert clips.dtype == torch.uint8 and tuple(clips.shape) == (2, cfg.num_frames, 3, cfg.image_size, cfg.image_size)
    twin = A.clip_transform_host(src, tf.last_table, cfg.image_size).view_as(clips).to(dev)
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    model = bvc.VideoMAEForPreTraining(bvc.VideoMAEConfig(**kw))
    model.load_state_dict(vo.make_params(cfg, seed=0))
    model.to(dev).train()
    _, mask = vo.synthetic_batch(cfg, 2, 0, 0.75)
    losses = [model(px, bool_masked_pos=mask.to(dev)).loss.detach().cpu() for px in (clips, twin)]
    assert torch.isfinite(losses[0]) and torch.equal(losses[0], losses[1])

    tf2 = A.ClipTransform(64, augs="cj", views=2, generator=np.random.default_rng(18))
    src2 = torch.randint(0, 256, (2, 2, 3, 80, 72), generator=g, dtype=torch.uint8)
    views = tf2(src2.to(dev))
    assert tuple(views.shape) == (4, 2, 3, 64, 64)
    twin2 = A.clip_transform_host(src2, tf2.last_table, 64).view_as(views).to(dev)
    enc = bvc.jepa.vit_tiny(img_size=[64], num_frames=2, tubelet_size=1).to(dev)
    with torch.no_grad():
        a, b = enc(views), enc(twin2)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
