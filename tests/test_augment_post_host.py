"""The post stage of the clip transforms on the CPU (bvc_clip_post_host, bvc_aug_blur_weights, bvc.augment.ClipAugment's sampler).
No GPU.

Three links, each for EQUALITY (the whole stage is integer arithmetic; the gray is the f32 expression of the stage before, evaluated
in the same order on both sides):
  * tests/augment_post_ref.py, a numpy restatement of Pillow's GaussianBlur and Image.rotate(NEAREST), against PIL itself, where PIL
    imports (the only tests here that are skipped without it);
  * the library's host twin against the restatement, on the same cases plus blur -> gray -> rotation combined;
  * the host twin against tests/golden/augment_post_pil.json, PIL's own output recorded by tools/make_augment_post_golden.py.
"""
import base64
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from tests import augment_post_ref as P


@pytest.fixture(scope="module")
def bvc():
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def A(bvc):
    return bvc.augment


def _differing(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


# ---------------------------------------------------------------- the restatement against PIL
@pytest.mark.parametrize("H,W", P.BLUR_SHAPES)
def test_restated_blur_equals_pil(H, W):
    pytest.importorskip("PIL")
    x = P.frames(1, H, W, seed=H * 100 + W)[0].numpy()
    for radius in P.BLUR_RADII + P.drawn_radii():
        assert _differing(P.blur(x, P.blur_weights(radius)), P.pil_blur(x, radius)) == 0, f"{H}x{W} radius {radius}"


@pytest.mark.parametrize("H,W", P.ROT_SHAPES)
def test_restated_rotation_equals_pil(H, W):
    pytest.importorskip("PIL")
    x = P.frames(1, H, W, seed=H * 100 + W + 1)[0].numpy()
    for angle in P.ROT_ANGLES + P.drawn_angles():
        assert _differing(P.rotate(x, P.rotation_coeffs(angle, H, W)), P.pil_rotate(x, angle)) == 0, f"{H}x{W} angle {angle}"


# ---------------------------------------------------------------- the host twin against the restatement
@pytest.mark.parametrize("H,W", P.BLUR_SHAPES)
def test_host_blur_equals_restatement(A, H, W):
    radii = P.BLUR_RADII + P.drawn_radii()
    x = P.frames(len(radii) + 1, H, W, seed=H * 100 + W)
    t = P.table(A, H, W, [dict(radius=r) for r in radii] + [dict()])        # the last frame is not blurred
    got = A.clip_post_host(x, t)
    for i, r in enumerate(radii):
        assert _differing(got[i], P.apply(x[i], radius=r)) == 0, f"{H}x{W} radius {r}"
    assert torch.equal(got[-1], x[-1])
    assert torch.equal(got[0], x[0])                                           # radius 0 is the identity, as in PIL


@pytest.mark.parametrize("H,W", P.ROT_SHAPES)
def test_host_rotation_equals_restatement(A, H, W):
    angles = P.ROT_ANGLES + P.drawn_angles()
    x = P.frames(len(angles) + 1, H, W, seed=H * 100 + W + 1)
    t = P.table(A, H, W, [dict(angle=a) for a in angles] + [dict()])
    got = A.clip_post_host(x, t)
    for i, a in enumerate(angles):
        assert list(t["rot"][i]) == P.rotation_coeffs(a, H, W)
        assert _differing(got[i], P.apply(x[i], angle=a)) == 0, f"{H}x{W} angle {a}"
    assert torch.equal(got[-1], x[-1])
    assert torch.equal(got[0], x[0])                                           # angle 0
    if H == W:
        assert torch.equal(got[1], torch.rot90(x[1], 1, (-2, -1))) and torch.equal(got[2], torch.rot90(x[2], -1, (-2, -1)))


COMBINED = [dict(radius=1.3, to_gray=True, angle=30.0), dict(radius=2.0, to_gray=True), dict(to_gray=True, angle=-61.0),
            dict(radius=0.3, angle=90.0), dict(to_gray=True), dict(radius=4.0, to_gray=True, angle=-12.5), dict()]


def test_host_blur_gray_rotate_combined(A):
    H, W = 33, 65
    x = P.frames(len(COMBINED), H, W, seed=5)
    got = A.clip_post_host(x, P.table(A, H, W, COMBINED))
    for i, kw in enumerate(COMBINED):
        assert _differing(got[i], P.apply(x[i], **kw)) == 0, kw
    assert torch.equal(got[4][0], got[4][1]) and torch.equal(got[4][0], got[4][2])


def load_golden(golden_dir):
    fx = json.load(open(os.path.join(golden_dir, "augment_post_pil.json")))
    shape = tuple(fx["shape"])

    def arr(s):
        return torch.from_numpy(np.frombuffer(base64.b64decode(s), dtype=np.uint8).reshape(shape).copy())

    frames = [arr(s) for s in fx["frames"]]
    cases = [(frames[c["frame"]], dict(radius=c["radius"], angle=c["angle"]), arr(c["out"])) for c in fx["cases"]]
    return fx, shape, cases


def test_host_twin_equals_the_pil_fixture(A, golden_dir):
    fx, (_, H, W), cases = load_golden(golden_dir)
    assert fx["pil_version"] and len(cases) == 19
    x = torch.stack([c[0] for c in cases])
    got = A.clip_post_host(x, P.table(A, H, W, [c[1] for c in cases]))
    for i, (_, kw, want) in enumerate(cases):
        assert _differing(got[i], want) == 0, kw


# ---------------------------------------------------------------- weights, validation, identity
def test_blur_weights_match_pillows_types(bvc, A):
    for radius in P.BLUR_RADII + P.drawn_radii():
        assert A.blur_weights(radius) == P.blur_weights(radius), radius
    # an f64 division for ww gives other weights at these two radii: the f32 one is Pillow's
    assert A.blur_weights(1.0) == (0, 11184811, 2796202) and A.blur_weights(0.3) == (0, 16273900, 251658)
    assert A.blur_weights(0.0) == (0, 1 << 24, 0) and A.blur_weights(4.0)[0] == 3
    for bad in (-0.5, float("nan"), 4.0001, float("inf")):
        with pytest.raises(bvc._lib.BvcError, match="radius"):
            A.blur_weights(bad)


def test_each_validation_rule_has_a_named_message(bvc, A):
    Err = bvc._lib.BvcError
    x = torch.zeros(1, 3, 16, 16, dtype=torch.uint8)
    good = P.table(A, 16, 16, [dict(radius=1.0, angle=10.0)])
    A.clip_post_host(x, good)
    for field, value, msg in [("blur_r", 4, "blur_r"), ("blur_r", -2, "blur_r"), ("blur_ww", (1 << 24) + 1, "exceed 2\\^24"),
                              ("blur_fw", 1 << 23, "exceed 2\\^24")]:
        bad = good.copy()
        bad[field] = value
        with pytest.raises(Err, match=msg):
            A.clip_post_host(x, bad)
    for i, value in [(0, 65538), (1, -65538), (3, 65538), (4, -65538), (2, (1 << 30) + 1), (5, -(1 << 30) - 1)]:
        bad = good.copy()
        bad["rot"][0, i] = value
        with pytest.raises(Err, match=f"rot\\[{i}\\]"):
            A.clip_post_host(x, bad)
        bad["rotate"] = 0                                        # coefficients of a frame that does not rotate are not read
        A.clip_post_host(x, bad)
    wide = torch.zeros(1, 3, 1, 4097, dtype=torch.uint8)
    A.clip_post_host(wide, A.empty_post_table(1))
    with pytest.raises(Err, match="4096"):
        A.clip_post_host(wide, P.table(A, 1, 4097, [dict(angle=10.0)]))
    # in and out that overlap: through the C entry point, the Python front end always allocates
    buf = torch.zeros(2 * 3 * 16 * 16 + 8, dtype=torch.uint8)
    rc = bvc._lib.lib().bvc_clip_post_host(buf.data_ptr(), good.ctypes.data, 1, 16, 16, buf.data_ptr() + 3 * 16 * 16 - 1)
    assert rc != 0 and b"overlap" in bvc._lib.lib().bvc_last_error()
    assert bvc._lib.lib().bvc_clip_post_host(buf.data_ptr(), good.ctypes.data, 1, 16, 16, buf.data_ptr() + 3 * 16 * 16) == 0
    with pytest.raises(ValueError, match="one per frame"):
        A.clip_post_host(x, A.empty_post_table(2))
    with pytest.raises(ValueError, match="channels"):
        A.clip_post_host(torch.zeros(1, 1, 16, 16, dtype=torch.uint8), A.empty_post_table(1))
    with pytest.raises(Err):                                     # the device path never falls back to the host
        A.clip_post(x, good)


def test_identity_table_returns_its_input(A):
    x = P.frames(3, 17, 40, seed=6)
    t = A.empty_post_table(3)
    assert not A.post_needed(t)
    got = A.clip_post_host(x, t)
    assert torch.equal(got, x) and got.data_ptr() != x.data_ptr()


# ---------------------------------------------------------------- the sampler
def test_sampler_rules(A):
    g = np.random.default_rng(0)
    t = A.sample_post_params(40, 1, 32, "cjo", generator=g)
    assert t.dtype == A.FRAME_POST and t.shape == (40,)
    assert bool((t["rotate"] == 1).all()) and bool((t["blur_r"] == -1).all()) and bool((t["gray"] == 0).all())
    # every angle lies in `degrees`: a0 = FIX(cos) >= 0 for |angle| <= 90, and with degrees = (20, 30) sin and cos are pinned down
    assert bool((t["rot"][:, 0] >= 0).all()) and len({tuple(r) for r in t["rot"]}) == 40
    t = A.sample_post_params(200, 1, 32, "o", degrees=(20.0, 30.0), generator=g)
    ang = np.degrees(np.arctan2(t["rot"][:, 3].astype(np.float64), t["rot"][:, 0].astype(np.float64)))   # a3 = FIX(-sin(-angle))
    assert bool((ang >= 20.0 - 1e-3).all()) and bool((ang <= 30.0 + 1e-3).all())
    t = A.sample_post_params(4000, 1, 32, "b", generator=g)
    share = float((t["blur_r"] >= 0).mean())
    print(f"blur share over 4000 draws at p = 0.5: {share:.4f}")
    assert 0.45 <= share <= 0.55
    assert bool((t["rotate"] == 0).all()) and bool((t["gray"] == 0).all())
    blurred = t[t["blur_r"] >= 0]
    lo, hi = A.blur_weights(0.1), A.blur_weights(2.0)
    assert bool((blurred["blur_r"] <= hi[0]).all()) and bool((blurred["blur_ww"] <= lo[1]).all()) and bool((blurred["blur_ww"] >= hi[1]).all())
    # 'g' is drawn here only together with 'b'
    assert bool((A.sample_post_params(64, 1, 32, "cjg", generator=g)["gray"] == 0).all())
    tg = A.sample_post_params(400, 1, 32, "bg", generator=g)
    assert 0.4 <= float(tg["gray"].mean()) <= 0.6
    # the draw order b, g, o: the same stream read by hand gives the same entries
    t = A.sample_post_params(8, 1, (24, 40), "bgo", generator=np.random.default_rng(3))
    h = np.random.default_rng(3)
    for e in t:
        want = A.empty_post_table(1)[0]
        if h.random() < 0.5:
            want["blur_r"], want["blur_ww"], want["blur_fw"] = A.blur_weights(h.uniform(0.1, 2.0))
        want["gray"] = int(h.random() < 0.5)
        want["rotate"], want["rot"] = 1, A.rotation_coeffs(h.uniform(-90.0, 90.0), (24, 40))
        assert e.tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="unknown"):
        A.sample_post_params(1, 1, 32, "x")
    with pytest.raises(ValueError, match="blur_radius"):
        A.sample_post_params(1, 1, 32, "b", blur_radius=(0.1, 5.0))


def test_sampler_draws_per_clip_or_per_frame(A):
    B, T, V = 3, 4, 2
    t = A.sample_post_params(B, T, 32, "bo", blur_p=1.0, views=V, generator=np.random.default_rng(1)).reshape(V * B, T)
    for clip in t:
        assert all(e.tobytes() == clip[0].tobytes() for e in clip)
    assert len({clip[0].tobytes() for clip in t}) == V * B
    t = A.sample_post_params(B, T, 32, "bo", blur_p=1.0, views=V, consistent=False, generator=np.random.default_rng(1))
    assert len({e.tobytes() for e in t}) == V * B * T


def test_clip_augment_equals_clip_transform_on_the_shared_letters(bvc, A):
    assert bvc.ClipAugment is A.ClipAugment
    a = A.ClipAugment(16, augs="cjg", generator=np.random.default_rng(9), views=2)
    b = A.ClipTransform(16, augs="cjg", generator=np.random.default_rng(9), views=2)
    ta, pa = a.sample(3, 2, (32, 40))
    tb = b.sample(3, 2, (32, 40))
    assert ta.tobytes() == tb.tobytes() and not A.post_needed(pa)
    x = P.frames(6, 32, 40, seed=8)
    assert torch.equal(A.clip_post_host(A.clip_transform_host(x, ta, 16), pa), A.clip_transform_host(x, tb, 16))
    assert a.sample(3, 2, (32, 40))[0].tobytes() == b.sample(3, 2, (32, 40)).tobytes()        # the streams stay in step
    # 'o' brings its flip, 'b' moves the extra gray behind the blur
    o = A.ClipAugment(16, augs="cjo", generator=np.random.default_rng(10))
    t1, p1 = o.sample(64, 1, (32, 40))
    assert 0 < int(t1["flip"].sum()) < 64 and bool((p1["rotate"] == 1).all())
    bg = A.ClipAugment(16, augs="cbg", generator=np.random.default_rng(11))
    t2, p2 = bg.sample(64, 1, (32, 40))
    assert int(t2["gray"].sum()) == 0 and 0 < int(p2["gray"].sum()) < 64 and int(t2["flip"].sum()) == 0
    with pytest.raises(ValueError, match="unknown"):
        A.ClipAugment(16, augs="cjx")


def test_new_symbols_are_in_the_table(bvc):
    for name in ("bvc_aug_blur_weights", "bvc_op_clip_post_workspace", "bvc_op_clip_post", "bvc_clip_post_host"):
        assert name in bvc._lib.SYMBOLS and getattr(bvc._lib.lib(), name) is not None
    assert bvc._lib.lib().bvc_op_clip_post_workspace(4, 16, 24) == 4 * 3 * 16 * 24
