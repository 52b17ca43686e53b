"""RandAugment on the CPU (bvc_clip_randaug_host, bvc.augment's sampler and parser).  No GPU.

Three links, each for EQUALITY of bytes:
  * tests/randaug_ref.py, a numpy restatement of the fifteen PIL operations, against PIL itself, where PIL imports (the only tests
    here that are skipped without it);
  * the library's host twin against the restatement, per op and for chains of 1 to 8 stages with repeats;
  * validation, the sampler's rules, the config parser, and ClipAugment's unchanged draws.
"""
import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from tests import randaug_ref as R


@pytest.fixture(scope="module")
def bvc():
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def A(bvc):
    return bvc.augment


def _differing(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


def frames_of(H, W):
    """ordinary and edge frames of one shape, and the two frames with a fixed shape where it is theirs"""
    xs = [R.frames(1, H, W, seed=H * 100 + W)[0]] + list(R.edge_frames(H, W))
    if (H, W) == (3, 3):
        xs.append(R.step_zero_frame())
    if (H, W) == (17, 40):
        xs.append(R.over_255_frame())
    return torch.stack(xs)


# ---------------------------------------------------------------- the restatement against PIL
@pytest.mark.parametrize("H,W", R.SHAPES)
@pytest.mark.parametrize("name", R.OPS)
def test_restatement_equals_pil(name, H, W):
    pytest.importorskip("PIL")
    for x in frames_of(H, W).numpy():
        for p in R.op_params(name, H, W):
            if name == "Posterize" and p == 0:
                assert not R.apply_op(x, name, p).any()        # PIL refuses 0 bits; the restatement gives 0
                continue
            assert _differing(R.apply_op(x, name, p), R.pil_op(x, name, p)) == 0, f"{name}({p}) {H}x{W}"


def test_edge_frames_reach_their_branches():
    R.step_zero_frame()
    x = R.over_255_frame().numpy()
    assert int(R.equalize(x).max()) == 255
    c = R.constant_frame(5, 7).numpy()
    assert _differing(R.autocontrast(c), c) == 0 and _differing(R.equalize(c), c) == 0


# ---------------------------------------------------------------- the host twin against the restatement
@pytest.mark.parametrize("H,W", R.SHAPES)
@pytest.mark.parametrize("name", R.OPS)
def test_host_twin_equals_restatement_per_op(A, name, H, W):
    xs = frames_of(H, W)
    for p in R.op_params(name, H, W):
        t = R.table(A, H, W, [[(name, p)]] * len(xs))
        got = A.rand_augment_host(xs, t)
        for i in range(len(xs)):
            assert _differing(got[i], R.apply_chain(xs[i], [(name, p)])) == 0, f"{name}({p}) {H}x{W} frame {i}"


@pytest.mark.parametrize("H,W", [(3, 3), (17, 40), (33, 65)])
def test_host_twin_equals_restatement_on_chains(A, H, W):
    g = np.random.default_rng(H * 10 + W)
    chains = [R.random_chain(g, n, H, W) for n in range(1, 9) for _ in range(3)]
    chains.append([("Equalize", None), ("Equalize", None), ("AutoContrast", None), ("Contrast", 1.4), ("Contrast", 1.4), ("Rotate", 20.0)])
    chains.append([])
    x = R.frames(len(chains), H, W, seed=H + W)
    got = A.rand_augment_host(x, R.table(A, H, W, chains))
    for i, chain in enumerate(chains):
        assert _differing(got[i], R.apply_chain(x[i], chain)) == 0, chain
    assert torch.equal(got[-1], x[-1])


def test_fill_colour_and_identity(A):
    x = R.frames(2, 9, 11, seed=1)
    t = R.table(A, 9, 11, [[("TranslateX", 11.0)], []], fill=(1, 2, 3))
    got = A.rand_augment_host(x, t)
    assert all(bool((got[0, c] == c + 1).all()) for c in range(3)) and torch.equal(got[1], x[1])
    t = A.empty_randaug_table(2)
    got = A.rand_augment_host(x, t)
    assert torch.equal(got, x) and got.data_ptr() != x.data_ptr()


# ---------------------------------------------------------------- validation
def test_each_malformed_field_is_refused_by_name(bvc, A):
    Err = bvc._lib.BvcError
    assert A.FRAME_RANDAUG.itemsize == bvc._lib.lib().bvc_frame_randaug_bytes() == 296
    x = torch.zeros(1, 3, 16, 16, dtype=torch.uint8)
    good = R.table(A, 16, 16, [[("Posterize", 3), ("Solarize", 100), ("SolarizeAdd", 50), ("Color", 1.5), ("Rotate", 10.0)]])
    A.rand_augment_host(x, good)

    def refused(msg, edit):
        bad = good.copy()
        edit(bad)
        with pytest.raises(Err, match=msg):
            A.rand_augment_host(x, bad)

    def setter(stage, field, value):
        def edit(t):
            t["stage"][0, stage][field] = value
        return edit

    def set_nops(value):
        def edit(t):
            t["nops"] = value
        return edit

    refused("nops", set_nops(9))
    refused("nops", set_nops(-1))
    refused("unknown op", setter(0, "op", 15))
    refused("unknown op", setter(4, "op", -1))
    refused("ival", setter(0, "ival", 9))
    refused("ival", setter(0, "ival", -1))
    refused("ival", setter(1, "ival", 257))
    refused("ival", setter(2, "ival", 111))
    for v in (float("nan"), float("inf"), -0.5):
        refused("fval", setter(3, "fval", v))
    for i, value in [(0, 65538), (1, -65538), (3, 65538), (4, -65538), (2, (1 << 30) + 1), (5, -(1 << 30) - 1)]:
        def edit(t, i=i, value=value):
            t["stage"]["aff"][0, 4, i] = value
        refused(f"aff\\[{i}\\]", edit)
    # fields of stages beyond nops, and fields an op does not read, are not looked at
    ok = good.copy()
    ok["stage"][0, 6]["op"] = 99
    ok["stage"][0, 3]["ival"] = 1000
    ok["stage"]["aff"][0, 0, 2] = 1 << 31 - 1
    A.rand_augment_host(x, ok)
    wide = torch.zeros(1, 3, 1, 4097, dtype=torch.uint8)
    A.rand_augment_host(wide, R.table(A, 1, 4097, [[("Invert", None)]]))
    with pytest.raises(Err, match="4096"):
        A.rand_augment_host(wide, R.table(A, 1, 4097, [[("ShearX", 0.1)]]))
    # in and out that overlap: through the C entry point, the Python front end always allocates
    buf = torch.zeros(2 * 3 * 16 * 16 + 8, dtype=torch.uint8)
    L = bvc._lib.lib()
    assert L.bvc_clip_randaug_host(buf.data_ptr(), good.ctypes.data, 1, 16, 16, buf.data_ptr() + 3 * 16 * 16 - 1) != 0
    assert b"overlap" in L.bvc_last_error()
    assert L.bvc_clip_randaug_host(buf.data_ptr(), good.ctypes.data, 1, 16, 16, buf.data_ptr() + 3 * 16 * 16) == 0
    with pytest.raises(ValueError, match="one per frame"):
        A.rand_augment_host(x, A.empty_randaug_table(2))
    with pytest.raises(ValueError, match="channels"):
        A.rand_augment_host(torch.zeros(1, 1, 16, 16, dtype=torch.uint8), A.empty_randaug_table(1))
    with pytest.raises(Err):                                     # the device path never falls back to the host
        A.rand_augment(x, good)
    with pytest.raises(ValueError, match="ival"):
        A.randaug_stage("Posterize", 9, 16)
    with pytest.raises(ValueError, match="fval"):
        A.randaug_stage("Color", -1.0, 16)
    with pytest.raises(ValueError, match="unknown"):
        A.randaug_stage("Blur", 1.0, 16)
    with pytest.raises(ValueError, match="at most 8"):
        A.randaug_entry([("Invert", None)] * 9, 16)


# ---------------------------------------------------------------- the sampler
def _stages(t):
    return [(int(s["op"]), s) for e in t for s in e["stage"][:int(e["nops"])]]


def test_sampler_is_reproducible_and_shares_entries_within_a_clip(bvc, A):
    assert bvc.sample_randaug_params is A.sample_randaug_params and tuple(bvc.RANDAUG_OPS) == tuple(R.OPS)
    B, T, V = 3, 4, 2
    a = A.sample_randaug_params(B, T, 32, views=V, generator=np.random.default_rng(5))
    b = A.sample_randaug_params(B, T, 32, views=V, generator=np.random.default_rng(5))
    assert a.dtype == A.FRAME_RANDAUG and a.shape == (V * B * T,) and a.tobytes() == b.tobytes()
    assert a.tobytes() != A.sample_randaug_params(B, T, 32, views=V, generator=np.random.default_rng(6)).tobytes()
    for clip in a.reshape(V * B, T):
        assert all(e.tobytes() == clip[0].tobytes() for e in clip)
    assert bool((a["fill"][:, :3] == np.array([124, 116, 104])).all())
    per_frame = A.sample_randaug_params(B, T, 32, views=V, prob=1.0, consistent=False, generator=np.random.default_rng(5))
    assert len({e.tobytes() for e in per_frame}) == V * B * T


def test_sampler_prob_and_ranges(A):
    g = np.random.default_rng(7)
    assert bool((A.sample_randaug_params(50, 1, 32, prob=0.0, generator=g)["nops"] == 0).all())
    for k in (0, 1, 4, 8):
        assert bool((A.sample_randaug_params(50, 1, 32, num_ops=k, prob=1.0, generator=g)["nops"] == k).all())
    half = A.sample_randaug_params(2000, 1, 32, prob=0.5, generator=g)["nops"]
    assert 1.8 <= float(half.mean()) <= 2.2 and int(half.min()) == 0 and int(half.max()) == 4
    H, W = 24, 40
    zero = A.sample_randaug_params(400, 1, (H, W), magnitude=0.0, magnitude_std=0.0, prob=1.0, generator=g)
    ident = np.array(A.affine_coeffs((1, 0, 0, 0, 1, 0)))
    for op, s in _stages(zero):
        name = R.OPS[op]
        if name in ("Color", "Contrast", "Brightness", "Sharpness"):
            assert float(s["fval"]) == 1.0
        elif name in ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"):
            assert (s["aff"] == ident).all()
        elif name in ("Posterize", "Solarize", "SolarizeAdd"):
            assert int(s["ival"]) == {"Posterize": 4, "Solarize": 256, "SolarizeAdd": 0}[name]
    top = A.sample_randaug_params(400, 1, (H, W), magnitude=10.0, magnitude_std=0.0, prob=1.0, generator=g)
    seen = set()
    for op, s in _stages(top):
        name = R.OPS[op]
        seen.add(name)
        if name in ("Color", "Contrast", "Brightness", "Sharpness"):
            assert float(s["fval"]) in (float(np.float32(0.1)), float(np.float32(1.9)))
        elif name in ("Posterize", "Solarize", "SolarizeAdd"):
            assert int(s["ival"]) == {"Posterize": 0, "Solarize": 0, "SolarizeAdd": 110}[name]
        elif name == "Rotate":
            assert list(s["aff"]) in [list(A.rotation_coeffs(a, (H, W))) for a in (-30.0, 30.0)]
        elif name != "AutoContrast" and name != "Equalize" and name != "Invert":
            v = {"ShearX": 0.3, "ShearY": 0.3, "TranslateX": 0.45 * W, "TranslateY": 0.45 * H}[name]
            assert list(s["aff"]) in [R.coeffs(name, sgn * v, H, W) for sgn in (-1.0, 1.0)]
    assert seen == set(R.OPS)
    # with a spread, every parameter stays inside its range and every table is accepted by the library
    wild = A.sample_randaug_params(300, 1, (H, W), magnitude=9.0, magnitude_std=5.0, prob=1.0, num_ops=8, generator=g)
    for op, s in _stages(wild):
        assert 0 <= int(s["ival"]) <= 256 and (float(s["fval"]) == 0.0 or 0.1 <= float(s["fval"]) <= 1.9 + 1e-6)
    A.rand_augment_host(torch.zeros(300, 3, H, W, dtype=torch.uint8), wild)
    only = A.sample_randaug_params(100, 1, 32, ops=["Invert", 14], prob=1.0, generator=g)
    assert {op for op, _ in _stages(only)} == {2, 14}
    for kw, msg in [(dict(num_ops=9), "num_ops"), (dict(prob=1.5), "prob"), (dict(magnitude=11.0), "magnitude"), (dict(ops=["Blur"]), "unknown"),
                    (dict(ops=[]), "ops"), (dict(fill=(1, 2)), "fill")]:
        with pytest.raises(ValueError, match=msg):
            A.sample_randaug_params(1, 1, 32, **kw)


def test_sampler_draws_ops_uniformly(A):
    n = 20000
    t = A.sample_randaug_params(n // 4, 1, 32, num_ops=4, prob=1.0, generator=np.random.default_rng(8))
    counts = np.bincount([op for op, _ in _stages(t)], minlength=15)
    assert int(counts.sum()) == n
    p = 1.0 / 15.0
    sd = (n * p * (1.0 - p)) ** 0.5
    dev = np.abs(counts - n * p) / sd
    print(f"op counts over {n} draws: {counts.tolist()}; largest deviation {float(dev.max()):.2f} sd")
    assert float(dev.max()) <= 5.0
    signs = np.array([s["aff"][1] for op, s in _stages(t) if op == 10])          # ShearX: a1 carries the sign
    assert abs(float((signs < 0).mean()) - 0.5) <= 5.0 * 0.5 / len(signs) ** 0.5


def test_sampler_reads_its_stream_in_the_documented_order(A):
    H, W = 24, 40
    t = A.sample_randaug_params(6, 1, (H, W), num_ops=3, magnitude=6.0, magnitude_std=1.0, prob=0.7, generator=np.random.default_rng(9))
    h = np.random.default_rng(9)
    signed = {"Color", "Contrast", "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"}
    for e in t:
        names = []
        for _ in range(3):
            name = R.OPS[int(h.integers(0, 15))]
            if not h.random() < 0.7:
                continue
            h.normal(6.0, 1.0)
            if name in signed:
                h.random()
            names.append(name)
        assert [R.OPS[int(s["op"])] for s in e["stage"][:int(e["nops"])]] == names


# ---------------------------------------------------------------- the parser
def test_parse_randaug(bvc, A):
    assert bvc.parse_randaug is A.parse_randaug
    assert A.parse_randaug("rand-m7-n4-mstd0.5-inc1") == dict(magnitude=7.0, num_ops=4, magnitude_std=0.5)
    assert A.parse_randaug("rand") == {}
    assert A.parse_randaug("rand-m9.5-p0.25") == dict(magnitude=9.5, prob=0.25)
    for kw in (dict(num_ops=4, magnitude=7.0, magnitude_std=0.5, prob=0.5), dict(num_ops=2, magnitude=9.0, magnitude_std=0.0, prob=1.0),
               dict(num_ops=8, magnitude=0.0, magnitude_std=2.5, prob=0.125)):
        assert A.parse_randaug(A.format_randaug(**kw)) == kw
    for bad, field in [("rand-m7-inc0", "inc0"), ("rand-m7-w0", "w0"), ("rand-mmax5", "mmax5"), ("rand-m", "'m'"), ("rand-n4-foo", "foo"),
                       ("rand-m7-mstd0.5.1", "mstd0.5.1")]:
        with pytest.raises(ValueError, match=field):
            A.parse_randaug(bad)
    with pytest.raises(ValueError, match="rand"):
        A.parse_randaug("augmix-m7")
    ra = A.RandAugment("rand-m3-n2-mstd0-p1", generator=np.random.default_rng(1))
    assert ra.kw["magnitude"] == 3.0 and ra.kw["num_ops"] == 2 and ra.kw["magnitude_std"] == 0.0 and ra.kw["prob"] == 1.0
    assert bool((ra.sample(5, 2, 32)["nops"] == 2).all())
    with pytest.raises(ValueError, match="inc0"):
        A.RandAugment("rand-m7-inc0")


# ---------------------------------------------------------------- ClipAugment
def test_clip_augment_without_randaug_draws_what_it_drew(bvc, A):
    assert bvc.RandAugment is A.RandAugment
    kw = dict(augs="cjbo", views=2)
    plain = A.ClipAugment(16, generator=np.random.default_rng(12), **kw)
    assert plain.randaug is None
    # the two tables, drawn by hand from the same seed in the documented order
    h = np.random.default_rng(12)
    want_t = A.sample_params(3, 2, (32, 40), (16, 16), views=2, generator=h, **plain.kw)
    want_p = A.sample_post_params(3, 2, (16, 16), views=2, generator=h, **plain.post_kw)
    tables = plain.sample(3, 2, (32, 40))
    assert len(tables) == 2 and tables[0].tobytes() == want_t.tobytes() and tables[1].tobytes() == want_p.tobytes()
    # with randaug the first two tables are the same and the third follows them in the stream
    for spec in ("rand-m7-n4-mstd0.5-inc1", A.RandAugment("rand-m7-n4-mstd0.5-inc1")):
        with_ra = A.ClipAugment(16, generator=np.random.default_rng(12), randaug=spec, **kw)
        t, p, r = with_ra.sample(3, 2, (32, 40))
        assert t.tobytes() == want_t.tobytes() and p.tobytes() == want_p.tobytes()
        assert r.tobytes() == A.sample_randaug_params(3, 2, (16, 16), views=2, generator=h, **with_ra.randaug.kw).tobytes()
        assert r.shape == (12,)
        h = np.random.default_rng(12)
        A.sample_params(3, 2, (32, 40), (16, 16), views=2, generator=h, **plain.kw)
        A.sample_post_params(3, 2, (16, 16), views=2, generator=h, **plain.post_kw)


def test_new_symbols_are_in_the_table(bvc):
    for name in ("bvc_frame_randaug_bytes", "bvc_op_clip_randaug_workspace", "bvc_op_clip_randaug", "bvc_clip_randaug_host"):
        assert name in bvc._lib.SYMBOLS and getattr(bvc._lib.lib(), name) is not None
    assert bvc._lib.lib().bvc_op_clip_randaug_workspace(4, 16, 24) == 4 * (3 * 256 * 4 + 3 * 256) + 4 * 3 * 16 * 24
    assert bvc._lib.lib().bvc_op_clip_randaug_workspace(0, 16, 24) == 0
