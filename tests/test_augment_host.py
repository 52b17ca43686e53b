"""Clip transforms on the CPU: the host twin of the kernels (bvc_clip_transform_host, the same csrc/augment.h arithmetic compiled for
the host) against the oracle of tests/augment_ref.py, and the sampler of bvc.augment.  No GPU.

Bars
  * resize against torch's F.interpolate(antialias=True): max |diff| <= 1 LSB and at most 3 % of the elements different, per case.
    Both compute a horizontal pass rounded to uint8 and a vertical pass rounded to uint8.  The bar leaves room for an f32 evaluation
    of the weights (measured: up to 3.3 % different at 17 -> 16, which is rich in ties); the library holds its weights in torch's own
    fixed point and the measured difference is zero in every case (figures printed by the tests).
  * a colour stage alone against the fp64 oracle: equal wherever the oracle's value before truncation is farther than 2e-3 from an
    integer (f32 evaluation error at these magnitudes is below 1e-4), within 1 LSB elsewhere; such near-tie elements are at most 2 %
    of each case (asserted: a condition on the inputs).
  * full chains after a real resize: per frame max |diff| <= 1 + the oracle's own largest response to a 1-LSB move of its post-resize
    input (augment_ref.lsb_response), because the chain may start 1 LSB off and contrast / saturation amplify.
The sampler follows torchvision's get_params RULES; parity with torchvision's random stream is not claimed and not tested.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from tests import augment_ref as R


@pytest.fixture(scope="module")
def bvc():
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def A(bvc):
    return bvc.augment


def _frames(n, Hs, Ws, seed):
    """smooth structure + noise: neither flat (where every filter agrees) nor white noise alone"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(Hs, dtype=torch.float32), torch.arange(Ws, dtype=torch.float32), indexing="ij")
    base = 127.5 + 90.0 * torch.sin(xx / 5.0 + torch.arange(3).view(3, 1, 1)) * torch.cos(yy / 7.0)
    x = base[None] + 50.0 * torch.randn(n, 3, Hs, Ws, generator=g)
    return x.clamp(0, 255).to(torch.uint8).contiguous()


def _whole(A, n, Hs, Ws, Ho, Wo):
    t = A.empty_table(n)
    t["src"] = np.arange(n)
    t["w"], t["h"], t["Hr"], t["Wr"] = Ws, Hs, Ho, Wo
    return t


def _check_resize(got, want, what):
    d = (got.int() - want.int()).abs()
    share = float((d > 0).float().mean())
    print(f"{what}: max |diff| {int(d.max())}, differing share {share:.4%}")
    assert int(d.max()) <= 1, what
    assert share <= 0.03, f"{what}: {share:.4%} of the elements differ"


RESIZE_SHAPES = [(37, 53, 16, 16), (9, 12, 16, 16), (64, 48, 16, 24), (53, 37, 32, 16), (17, 16, 16, 16), (240, 320, 32, 32)]


@pytest.mark.parametrize("Hs,Ws,Ho,Wo", RESIZE_SHAPES)
def test_resize_matches_torch(A, Hs, Ws, Ho, Wo):
    x = _frames(2, Hs, Ws, seed=Hs * 1000 + Ws)
    t = _whole(A, 2, Hs, Ws, Ho, Wo)
    got = A.clip_transform_host(x, t, (Ho, Wo))
    want = torch.stack([R.resize_window(x, e, Ho, Wo) for e in t])
    _check_resize(got, want, f"{Hs}x{Ws}->{Ho}x{Wo}")


def test_exact_copy_crop_and_flip(A):
    x = _frames(2, 16, 16, seed=1)
    t = _whole(A, 2, 16, 16, 16, 16)
    assert torch.equal(A.clip_transform_host(x, t, 16), x)                     # a region of the output size is a copy
    big = _frames(1, 40, 52, seed=2)
    t = A.empty_table(3)
    t["x0"], t["y0"], t["w"], t["h"], t["Hr"], t["Wr"] = [5, 36, 0], [7, 24, 0], 16, 16, 16, 16       # inside, bottom-right corner, top-left
    got = A.clip_transform_host(big, t, 16)
    for i, (x0, y0) in enumerate([(5, 7), (36, 24), (0, 0)]):
        assert torch.equal(got[i], big[0, :, y0:y0 + 16, x0:x0 + 16])
    t = _whole(A, 1, 40, 52, 16, 24)                                          # the mirror of a real resize
    plain = A.clip_transform_host(big, t, (16, 24))
    t["flip"] = 1
    assert torch.equal(A.clip_transform_host(big, t, (16, 24)), plain.flip(-1))


@pytest.mark.parametrize("Hs,Ws,S", [(48, 64, 32), (64, 48, 32), (37, 53, 16), (40, 40, 24)])
def test_resize_center_crop_geometry(A, Hs, Ws, S):
    x = _frames(2, Hs, Ws, seed=3)
    t = A.center_crop_params(2, (Hs, Ws), S)
    short, long_ = min(Hs, Ws), max(Hs, Ws)
    assert {int(t["Hr"][0]), int(t["Wr"][0])} == {S, int(S * long_ / short)}
    got = A.clip_transform_host(x, t, S)
    full = torch.nn.functional.interpolate(x, size=(int(t["Hr"][0]), int(t["Wr"][0])), mode="bilinear", antialias=True, align_corners=False)
    oy, ox = int(round((full.shape[2] - S) / 2.0)), int(round((full.shape[3] - S) / 2.0))
    _check_resize(got, full[:, :, oy:oy + S, ox:ox + S], f"Resize({S}) + CenterCrop({S}) of {Hs}x{Ws}")


def test_crop_boxes_touching_the_borders(A):
    Hs, Ws, S = 45, 61, 16
    x = _frames(1, Hs, Ws, seed=4)
    boxes = [(0, 0, 30, 25), (Ws - 33, 0, 33, 20), (0, Hs - 27, 22, 27), (Ws - 40, Hs - 31, 40, 31), (0, 0, Ws, Hs), (0, 10, Ws, 9),
             (20, 0, 7, Hs)]
    t = A.empty_table(len(boxes))
    for e, (x0, y0, w, h) in zip(t, boxes):
        e["x0"], e["y0"], e["w"], e["h"], e["Hr"], e["Wr"] = x0, y0, w, h, S, S
    got = A.clip_transform_host(x, t, S)
    for i, e in enumerate(t):
        _check_resize(got[i], R.resize_window(x, e, S, S), f"box {boxes[i]}")


# ---------------------------------------------------------------- colour
SPECIAL = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (37, 37, 37), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255),
           (255, 0, 255), (1, 1, 1), (254, 255, 0)]


@functools.lru_cache(maxsize=None)
def _colour_frame():
    """32 x 32 random colours, with pure grays, saturated primaries and secondaries, 0 and 255 at the head of the first row.

    The range ends are fifths (0.6 = 3/5, 1.4, 0.2, 1.8), so f * v lands on an integer for every v that is a multiple of 5, and
    f * v + (1 - f) * gray for every v = gray (mod 5): a fifth of all uniformly drawn values would be near-tie elements, where the fp64
    oracle and an f32 evaluation may truncate either way and the comparison says little.  The random pixels are therefore drawn from
    those at which no brightness, saturation, hue or gray case of STAGE_CASES comes within augment_ref.TIE of an integer (a contrast
    case depends on the frame's mean and is left to chance); the special pixels stay as they are and are the near-tie elements that
    the 2 % condition counts.  Built once; nobody writes to it."""
    g = torch.Generator().manual_seed(5)
    cand = torch.randint(0, 256, (1, 3, 1, 20000), generator=g, dtype=torch.uint8)
    ok = torch.ones(20000, dtype=torch.bool)
    for op, f in STAGE_CASES:
        if op != R.CONTRAST:
            _, near = R.transform(cand, _stage_table_for(op, f, 1, 20000), 1, 20000)
            ok &= ~near[0].any(0)[0]
    keep = cand[0, :, 0, ok][:, :32 * 32]
    assert keep.shape[1] == 32 * 32
    x = keep.reshape(1, 3, 32, 32).clone()
    for i, c in enumerate(SPECIAL):
        x[0, :, 0, i] = torch.tensor(c, dtype=torch.uint8)
    return x.contiguous()


# both ends of the reference's ranges (s = 0.5: [0.6, 1.4] and +-0.1; the nominal ColorJitter(0.8, 0.8, 0.8, 0.2): [0.2, 1.8] and +-0.2)
BLEND_FACTORS = [0.6, 1.4, 0.2, 1.8, 1.0]
HUE_FACTORS = [-0.1, 0.1, -0.2, 0.2, 0.0]
STAGE_CASES = [(op, f) for op in (R.BRIGHTNESS, R.CONTRAST, R.SATURATION) for f in BLEND_FACTORS] + [(R.HUE, f) for f in HUE_FACTORS] + \
              [("gray", 0.0)]


def _stage_table_for(op, f, H_, W_):
    """one identity-geometry entry over an H_ x W_ frame with the single stage (op, f)"""
    A = ge.load_package().augment
    t = _whole(A, 1, H_, W_, H_, W_)
    if op == "gray":
        t["gray"] = 1
    else:
        t["nops"], t["order"] = 1, A.pack_order([op])
        t["factor"][0, op] = f
    return t


def _stage_table(A, op, f):
    return _stage_table_for(op, f, 32, 32)


def check_against_colour_oracle(got, want, near, what, tie_cap=0.02):
    """equal off the oracle's near-tie elements, within 1 LSB on them; near-tie share bounded (a condition on the inputs)"""
    d = (got.int() - want.int()).abs()
    share = float(near.float().mean())
    print(f"{what}: max |diff| {int(d.max())}, differing {int((d > 0).sum())}, near-tie share {share:.4%}")
    assert tie_cap is None or share <= tie_cap, f"{what}: {share:.4%} near-tie elements: the inputs do not test the stage"
    assert int(d[~near].max()) == 0 if (~near).any() else True, f"{what}: differs off the near-tie elements"
    assert int(d.max()) <= 1, what


@pytest.mark.parametrize("op,f", STAGE_CASES)
def test_each_colour_stage_alone(A, op, f):
    x = _colour_frame()
    t = _stage_table(A, op, f)
    got = A.clip_transform_host(x, t, 32)
    want, near = R.transform(x, t, 32, 32)
    check_against_colour_oracle(got, want, near, f"op {op} factor {f}")
    if op != "gray" and f == (0.0 if op == R.HUE else 1.0):
        assert torch.equal(got, x), "the stage must be the identity at this factor"


def chain_table(A, Hs, Ws, S, seed):
    """all 24 stage orders x {no gray, gray} = 48 entries over the 24 source frames of a 2 x 12 batch, each after a real resize of its
    own region, some mirrored; factors uniform in the nominal ColorJitter(0.8, 0.8, 0.8, 0.2) ranges"""
    rng = np.random.default_rng(seed)
    t = A.empty_table(48)
    for i, (perm, gray) in enumerate(itertools.product(itertools.permutations(range(4)), (0, 1))):
        e = t[i]
        w, h = int(rng.integers(S // 2, Ws + 1)), int(rng.integers(S // 2, Hs + 1))
        e["src"], e["w"], e["h"] = i % 24, w, h
        e["x0"], e["y0"] = int(rng.integers(0, Ws - w + 1)), int(rng.integers(0, Hs - h + 1))
        e["Hr"], e["Wr"], e["flip"], e["gray"] = S, S, int(rng.integers(0, 2)), gray
        e["nops"], e["order"] = 4, A.pack_order(perm)
        e["factor"] = (rng.uniform(0.2, 1.8), rng.uniform(0.2, 1.8), rng.uniform(0.2, 1.8), rng.uniform(-0.2, 0.2))
    return t


def check_chains(got, x, t, S, what):
    for i, e in enumerate(t):
        start = R.resize_window(x, e, S, S, flip=False)
        want, _ = R.colour_chain(start, e)
        if int(e["flip"]):
            want = want.flip(-1)
        bar = 1 + R.lsb_response(start, e)
        d = int((got[i].int() - want.int()).abs().max())
        print(f"{what} frame {i} order {R.ops_of(e)} gray {int(e['gray'])}: max |diff| {d}, bar {bar}")
        assert d <= bar, f"{what}: frame {i}: max |diff| {d} > {bar}"


def test_full_chains_after_a_real_resize(A):
    x = _frames(24, 40, 52, seed=6).view(2, 12, 3, 40, 52)
    t = chain_table(A, 40, 52, 24, seed=7)
    got = A.clip_transform_host(x, t, 24)
    check_chains(got, x.view(24, 3, 40, 52), t, 24, "host")


def test_chains_on_identity_geometry_meet_the_stage_bars(A):
    """the same 48 chains with no resize in front: the input is known exactly, so the chain must equal the oracle at every pixel
    where no stage came near a tie.  Nothing is asserted at the other pixels (an early stage's 1 LSB feeds the later stages; the
    lsb_response bar of the test above covers that); their share is printed."""
    x = _colour_frame().expand(24, -1, -1, -1).contiguous()
    t = chain_table(A, 32, 32, 32, seed=8)
    t["x0"], t["y0"], t["w"], t["h"] = 0, 0, 32, 32
    got = A.clip_transform_host(x, t, 32)
    want, near = R.transform(x, t, 32, 32)
    for i in range(48):
        px_near = near[i].any(0, keepdim=True).expand_as(near[i])          # a tie in one channel reaches the others through gray and hue
        d = (got[i].int() - want[i].int()).abs()
        print(f"chain {i}: differing {int((d > 0).sum())}, near-tie pixels {float(px_near.float().mean()):.2%}")
        assert int(d[~px_near].max()) == 0, f"chain {i} differs off the near-tie pixels"


# ---------------------------------------------------------------- sampler
def _within(mean, expect, std, n, what):
    se = std / np.sqrt(n)
    assert abs(mean - expect) <= 4 * se, f"{what}: mean {mean:.5f}, expected {expect:.5f} +- {4 * se:.5f}"


def test_sampler_follows_get_params_rules(A):
    N, S = 20000, 256
    g = np.random.default_rng(2024)
    # crop_scale (0.2, 0.5) on a square frame: no attempt can fail (w, h <= sqrt(0.5 * 4 / 3) S), so area and ratio are the plain draws
    t, info = A.sample_params(N, 1, (S, S), 224, augs="cjg", crop_scale=(0.2, 0.5), jitter_strength=0.5, flip=0.5, generator=g,
                              return_info=True)
    assert t.shape == (N,) and not info["fallback"].any()
    w, h = t["w"].astype(np.float64), t["h"].astype(np.float64)
    assert (t["x0"] >= 0).all() and (t["y0"] >= 0).all() and (t["x0"] + t["w"] <= S).all() and (t["y0"] + t["h"] <= S).all()
    assert (t["Hr"] == 224).all() and (t["Wr"] == 224).all() and (t["ox"] == 0).all() and (t["oy"] == 0).all()
    area = w * h / (S * S)
    slack = (w + h + 1) / (S * S)                                   # w and h are rounded to integers
    assert (area >= 0.2 - slack).all() and (area <= 0.5 + slack).all()
    _within(area.mean(), 0.35, 0.3 / np.sqrt(12), N, "crop area")
    logr = np.log(w / h)
    rslack = 0.5 / w + 0.5 / h + 1e-9
    assert (logr >= np.log(3 / 4) - 2 * rslack).all() and (logr <= np.log(4 / 3) + 2 * rslack).all()
    _within(logr.mean(), 0.0, 2 * np.log(4 / 3) / np.sqrt(12), N, "log aspect ratio")
    _within(((t["x0"] + w / 2) / S).mean(), 0.5, 0.2, N, "crop centre x")      # std of the centre is below 0.2 for these sizes

    applied = t["nops"] == 4
    assert ((t["nops"] == 0) | applied).all()
    _within(applied.mean(), 0.8, np.sqrt(0.8 * 0.2), N, "jitter apply probability")
    n = int(applied.sum())
    f = t["factor"][applied].astype(np.float64)
    assert (f[:, :3] >= 0.6 - 1e-6).all() and (f[:, :3] <= 1.4 + 1e-6).all() and (np.abs(f[:, 3]) <= 0.1 + 1e-6).all()
    for k, name in enumerate(("brightness", "contrast", "saturation")):
        _within(f[:, k].mean(), 1.0, 0.8 / np.sqrt(12), n, name)
    _within(f[:, 3].mean(), 0.0, 0.2 / np.sqrt(12), n, "hue")
    assert (t["factor"][~applied] == np.array([1, 1, 1, 0], dtype=np.float32)).all()
    orders = t["order"][applied]
    stages = np.stack([(orders >> (4 * i)) & 15 for i in range(4)], axis=1)
    assert (np.sort(stages, axis=1) == np.arange(4)).all()                     # every order is a permutation
    assert len(set(orders.tolist())) == 24
    for op in range(4):
        _within((stages[:, 0] == op).mean(), 0.25, np.sqrt(0.25 * 0.75), n, f"op {op} first")
    _within((t["gray"] != 0).mean(), 1 - 0.8 * 0.5, np.sqrt(0.6 * 0.4), N, "gray probability ('j' 0.2 or 'g' 0.5)")
    _within((t["flip"] != 0).mean(), 0.5, 0.5, N, "flip probability")
    # the nominal strength: factors in [max(0, 1 - 0.8 s), 1 + 0.8 s] with s = 1.5 -> [0, 2.2]
    t2 = A.sample_params(2000, 1, (S, S), 224, augs="j", jitter_strength=1.5, jitter_p=1.0, generator=g)
    f2 = t2["factor"]
    assert (f2[:, :3] >= 0).all() and (f2[:, :3] <= 2.2 + 1e-6).all() and f2[:, :3].min() < 0.05 and (np.abs(f2[:, 3]) <= 0.3 + 1e-6).all()
    assert (t2["w"] == S).all() and (t2["Hr"] == 224).all()                    # no 'c': Resize + CenterCrop of the whole frame


def test_sampler_fallback_consistency_and_views(A):
    g = np.random.default_rng(9)
    t, info = A.sample_params(3, 4, (256, 340), 224, augs="c", crop_scale=(2.0, 3.0), generator=g, return_info=True)
    assert info["fallback"].all()                                              # an impossible area: the centre-crop fallback, here the whole frame
    assert (t["w"] == 340).all() and (t["h"] == 256).all() and (t["x0"] == 0).all() and (t["y0"] == 0).all()
    t, info = A.sample_params(2, 1, (100, 400), 64, augs="c", crop_scale=(2.0, 3.0), generator=g, return_info=True)
    assert info["fallback"].all() and (t["h"] == 100).all() and (t["w"] == round(100 * 4 / 3)).all() and (t["x0"] == (400 - 133) // 2).all()

    B, T = 5, 6
    geo = ["x0", "y0", "w", "h", "Hr", "Wr", "oy", "ox", "flip", "nops", "order", "factor", "gray"]
    t = A.sample_params(B, T, (64, 80), 32, augs="cjg", flip=0.5, consistent=True, generator=g).reshape(B, T)
    for k in geo:
        assert (t[k] == t[k][:, :1]).all(), k                                  # one draw per clip
    assert (t["src"] == np.arange(B * T).reshape(B, T)).all()
    assert len({tuple(r) for r in t[["x0", "y0", "w", "h"]][:, 0].tolist()}) > 1     # but not one draw per batch
    t = A.sample_params(B, T, (64, 80), 32, augs="cjg", flip=0.5, consistent=False, generator=g).reshape(B, T)
    assert any(len({tuple(r) for r in t[["x0", "y0", "w", "h"]][b].tolist()}) > 1 for b in range(B))      # one draw per frame

    t = A.sample_params(B, T, (64, 80), 32, augs="cj", views=2, generator=g).reshape(2, B, T)
    assert (t["src"][0] == t["src"][1]).all() and (t["src"][0] == np.arange(B * T).reshape(B, T)).all()
    assert not (t["x0"][0] == t["x0"][1]).all() or not (t["w"][0] == t["w"][1]).all()      # the views are drawn independently


# ---------------------------------------------------------------- refusals
def test_refusals(bvc, A):
    with pytest.raises(ValueError, match="'b'"):
        A.ClipTransform(32, augs="cjb")
    with pytest.raises(ValueError, match="'b'"):
        A.sample_params(1, 1, (32, 32), 16, augs="b")
    with pytest.raises(ValueError, match="rotation"):
        A.ClipTransform(32, augs="c", rotation=15)
    with pytest.raises(ValueError, match="channels"):
        A.ClipTransform(16)(torch.zeros(1, 2, 1, 32, 32, dtype=torch.uint8))
    Err = bvc._lib.BvcError
    good = _whole(A, 1, 32, 32, 16, 16)
    with pytest.raises(Err, match="channels"):
        A.clip_transform_host(torch.zeros(1, 1, 32, 32, dtype=torch.uint8), good, 16)
    x = torch.zeros(1, 3, 32, 32, dtype=torch.uint8)
    A.clip_transform_host(x, good, 16)
    for field, value, msg in [("w", 0, "empty region"), ("h", -3, "empty region"), ("x0", 1, "outside"), ("y0", -1, "outside"),
                              ("w", 33, "outside"), ("src", 1, "source frame"), ("ox", 1, "window"), ("oy", -1, "window"),
                              ("Hr", 15, "window"), ("Wr", 1, "window"), ("nops", 5, "colour stages")]:
        bad = good.copy()
        bad[field] = value
        with pytest.raises(Err, match=msg):
            A.clip_transform_host(x, bad, 16)
    bad = good.copy()
    bad["nops"], bad["order"] = 2, A.pack_order([1, 1])
    with pytest.raises(Err, match="twice"):
        A.clip_transform_host(x, bad, 16)
    bad = _whole(A, 1, 320, 320, 16, 16)                                      # a 20-fold shrink: above BVC_AUG_MAX_SCALE
    with pytest.raises(Err, match="supported factor"):
        A.clip_transform_host(torch.zeros(1, 3, 320, 320, dtype=torch.uint8), bad, 16)
    with pytest.raises(Err):                                                   # the device path never falls back to the host
        A.clip_transform(x, good, 16)
