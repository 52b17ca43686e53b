"""RandAugment on the GPU (bvc_op_clip_randaug, csrc/randaug.hip) against the host twin (the same csrc/randaug.h arithmetic compiled
for the host; tests/test_randaug_host.py ties the twin to a numpy restatement and that to PIL), and RandAugment / ClipAugment end to end.

Integer histograms and single f32 / f64 operations in a fixed order: the bar is ZERO differing bytes everywhere.  Shapes: a thread of
the apply kernel owns 16 consecutive pixels of a plane and a workgroup 4096, a workgroup of the histogram kernel 16384, and the loads
are 16 bytes, 4 bytes or single bytes wide by what the plane's size and the buffers' alignment allow.  So the frames run from planes
smaller than one thread's run with odd sizes (1 x 9, 2 x 5, 3 x 3: bytes), over 17 x 40 (words, a last run of 8) and 33 x 65 (bytes,
runs that wrap rows, a tail) to 224 x 224 (16-byte loads, 13 workgroups per frame, 4 histogram workgroups per frame).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from tests import randaug_ref as R   # noqa: E402
from tests import test_randaug_host as HT   # noqa: E402

bvc = G.bvc
A = bvc.augment
dev = torch.device("cuda:0")


def _gpu(x, t, **kw):
    out = A.rand_augment(x.to(dev), t, **kw)
    torch.cuda.synchronize()
    return out.cpu()


def _same(got, want, what):
    n = int((got != want).sum())
    print(f"{what}: {n} of {got.numel()} bytes differ from the host twin")
    assert n == 0, what


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_every_op_equals_host_twin(H, W):
    """every op alone, at the ends of its range and at 20 drawn parameters, on the ordinary and the edge frames: one frame per case"""
    xs, chains = [], []
    for name in R.OPS:
        for p in R.op_params(name, H, W):
            for x in HT.frames_of(H, W):
                xs.append(x)
                chains.append([(name, p)])
    x = torch.stack(xs)
    t = R.table(A, H, W, chains)
    _same(_gpu(x, t), A.rand_augment_host(x, t), f"15 ops, {len(chains)} cases, {H}x{W}")


def test_every_op_equals_host_twin_at_224():
    H = W = 224
    base = R.frames(1, H, W, seed=224)[0]
    xs, chains = [], []
    for name in R.OPS:
        for p in R.op_params(name, H, W, n=1)[:3] + R.op_params(name, H, W, n=1)[-1:]:
            xs.append(base)
            chains.append([(name, p)])
    for name in ("AutoContrast", "Equalize", "Contrast", "Sharpness"):
        for x in (R.constant_frame(H, W), R.two_level_frame(H, W), R.noise_frame(H, W, seed=5)):
            xs.append(x)
            chains.append([(name, 1.7)])
    x = torch.stack(xs)
    t = R.table(A, H, W, chains)
    _same(_gpu(x, t), A.rand_augment_host(x, t), f"15 ops, {len(chains)} cases, 224x224")


@pytest.mark.parametrize("F", [1, 5, 37])
@pytest.mark.parametrize("H,W", [(33, 65), (17, 40), (32, 48)])
def test_frames_with_different_ops_and_stage_counts(F, H, W):
    """at one stage index the frames run different ops, and some have no such stage: nops cycles through 0 .. 8"""
    g = np.random.default_rng(F * 1000 + H)
    chains = [R.random_chain(g, (f + 3) % 9, H, W) for f in range(F)]
    x = R.frames(F, H, W, seed=F + H)
    t = R.table(A, H, W, chains)
    assert F == 1 or len({int(n) for n in t["nops"]}) > 1
    got = _gpu(x, t)
    _same(got, A.rand_augment_host(x, t), f"F {F}, {H}x{W}")
    for f in range(F):
        if not chains[f]:
            assert torch.equal(got[f], x[f])


def test_chains_of_statistics_ops():
    """two statistics ops in a row, then Contrast, then a gather: every histogram is of the frame as the stage before left it"""
    H, W = 70, 132
    chains = [[("Equalize", None), ("AutoContrast", None), ("Contrast", 1.6), ("Rotate", 17.0)],
              [("Contrast", 0.3), ("Contrast", 1.8), ("Equalize", None), ("ShearX", -0.2)],
              [("AutoContrast", None)] * 8,
              [("Equalize", None), ("Invert", None), ("Equalize", None), ("Color", 1.9), ("AutoContrast", None), ("Sharpness", 1.9),
               ("Contrast", 0.1), ("TranslateY", -9.5)],
              [("Invert", None)]]
    x = torch.cat([R.frames(4, H, W, seed=40), (R.frames(1, H, W, seed=41) // 3 + 60)])       # the last one: values 60 .. 145
    t = R.table(A, H, W, chains)
    got = _gpu(x, t)
    _same(got, A.rand_augment_host(x, t), "statistics chains 70x132")
    for f, chain in enumerate(chains):
        assert torch.equal(got[f], R.apply_chain(x[f], chain)), chain      # and the restatement, directly


@pytest.mark.parametrize("H,W", [(1, 9), (2, 5), (5, 2), (2, 40), (40, 1)])
def test_sharpness_on_frames_without_an_interior(H, W):
    x = R.frames(3, H, W, seed=H * 10 + W)
    t = R.table(A, H, W, [[("Sharpness", 1.9)], [("Sharpness", 0.1), ("Sharpness", 1.5)], [("Sharpness", 0.0)]])
    got = _gpu(x, t)
    _same(got, A.rand_augment_host(x, t), f"Sharpness {H}x{W}")
    assert torch.equal(got, x)             # SMOOTH copies such a frame, and a blend of a frame with itself is that frame


def test_range_ends():
    H, W = 33, 65
    fill = (9, 200, 77)
    chains = [[("TranslateX", float(W))], [("TranslateX", -float(W) - 3.0)], [("TranslateY", float(H))], [("TranslateY", -1000.0)],
              [("TranslateX", 0.0)], [("TranslateY", 0.0)], [("ShearX", 0.0)], [("ShearY", 0.0)], [("Rotate", 0.0)],
              [("Posterize", 0)], [("Posterize", 8)], [("Solarize", 0)], [("Solarize", 256)], [("SolarizeAdd", 0)], [("Brightness", 0.0)]]
    x = R.frames(len(chains), H, W, seed=50)
    t = R.table(A, H, W, chains, fill=fill)
    got = _gpu(x, t)
    _same(got, A.rand_augment_host(x, t), "range ends 33x65")
    want_fill = torch.tensor(fill, dtype=torch.uint8).view(3, 1, 1).expand(3, H, W)
    for f in range(4):
        assert torch.equal(got[f], want_fill), chains[f]
    for f in (4, 5, 6, 7, 8, 10, 12, 13):
        assert torch.equal(got[f], x[f]), chains[f]
    assert not got[9].any() and not got[14].any() and torch.equal(got[11], 255 - x[11])


def _guarded(n, offset, guard=64):
    buf = torch.full((guard + offset + n + guard,), 0xA5, dtype=torch.uint8, device=dev)
    return buf, buf[guard + offset:guard + offset + n]


def _guards_intact(buf, n, offset, guard=64):
    return bool((buf[:guard + offset] == 0xA5).all()) and bool((buf[guard + offset + n:] == 0xA5).all())


@pytest.mark.parametrize("H,W,offset", [(32, 48, 0), (33, 65, 1), (17, 40, 4)])
def test_deterministic_and_writes_exactly_its_bytes(H, W, offset):
    """two runs agree; a larger workspace full of 0xFF gives what an exact one gives; nothing is written outside `out` (64 guard bytes
    on each side) or to `in`; at an aligned start, at an odd one and at one that allows words only"""
    g = np.random.default_rng(H)
    F = 9
    chains = [R.random_chain(g, f % 9, H, W) for f in range(F)]
    chains[3] = [("Equalize", None), ("Contrast", 1.3), ("AutoContrast", None)]
    x = R.frames(F, H, W, seed=60)
    t = R.table(A, H, W, chains)
    n = x.numel()
    want = A.rand_augment_host(x, t)
    in_buf, xin = _guarded(n, offset)
    xin.copy_(x.view(-1).to(dev))
    xin = xin.view(F, 3, H, W)
    need = int(bvc._lib.lib().bvc_op_clip_randaug_workspace(F, H, W))
    results = []
    for work in (None, None, torch.full((need,), 0xFF, dtype=torch.uint8, device=dev),
                 torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device=dev)):
        out_buf, out = _guarded(n, offset)
        assert A.rand_augment(xin, t, out=out, workspace=work) is out
        torch.cuda.synchronize()
        assert _guards_intact(out_buf, n, offset), "bytes outside out were written"
        results.append(out.cpu().view_as(x))
    assert _guards_intact(in_buf, n, offset) and torch.equal(xin.cpu(), x), "the input was written"
    for r in results:
        _same(r, want, f"out= {H}x{W} offset {offset}")


@pytest.mark.parametrize("H,W", [(6, 40), (32, 48), (5, 20), (9, 36), (7, 19)])
@pytest.mark.parametrize("offset", [0, 4, 1])
def test_sharpness_window_loads(H, W, offset):
    """the 3 x 3 window arrives as 16-byte loads (16 | W, aligned), as words (4 | W; 5 x 20 has runs that end with their row, so
    without a word to the right, and runs that start at column 4) or as bytes (odd widths, odd starts): the same bytes every way"""
    x = R.frames(4, H, W, seed=H + W)
    t = R.table(A, H, W, [[("Sharpness", 1.9)], [("Sharpness", 0.1)], [("Sharpness", 1.3), ("Sharpness", 1.3), ("Sharpness", 0.6)],
                          [("Rotate", 10.0), ("Sharpness", 1.9)]])
    n = x.numel()
    in_buf, xin = _guarded(n, offset)
    xin.copy_(x.view(-1).to(dev))
    out_buf, out = _guarded(n, offset)
    A.rand_augment(xin.view(4, 3, H, W), t, out=out)
    torch.cuda.synchronize()
    assert _guards_intact(out_buf, n, offset) and _guards_intact(in_buf, n, offset)
    _same(out.cpu().view_as(x), A.rand_augment_host(x, t), f"Sharpness {H}x{W} offset {offset}")


def test_refusals_write_nothing():
    H, W = 16, 24
    x = R.frames(2, H, W, seed=70).to(dev)
    good = R.table(A, H, W, [[("Equalize", None), ("Rotate", 5.0)], [("Color", 0.5)]])
    n = x.numel()
    L = bvc._lib.lib()
    need = int(L.bvc_op_clip_randaug_workspace(2, H, W))
    work = torch.zeros(need, dtype=torch.uint8, device=dev)
    table_dev = torch.from_numpy(good.view(np.uint8).copy()).to(dev)
    # out inside in
    both = torch.zeros(2 * n, dtype=torch.uint8, device=dev)
    rc = L.bvc_op_clip_randaug(both.data_ptr(), good.ctypes.data, table_dev.data_ptr(), 2, H, W, both.data_ptr() + n - 1, work.data_ptr(), G.stream())
    assert rc != 0 and b"overlap" in L.bvc_last_error()
    rc = L.bvc_op_clip_randaug(x.data_ptr(), good.ctypes.data, table_dev.data_ptr(), 2, H, W, x.data_ptr(), work.data_ptr(), G.stream())
    assert rc != 0 and b"overlap" in L.bvc_last_error()
    torch.cuda.synchronize()
    assert not both.any()
    # a malformed table, whichever frame and stage holds the fault
    for edit, msg in [(lambda t: t["nops"].__setitem__(1, 9), "nops"), (lambda t: t["stage"]["op"].__setitem__((0, 1), 15), "unknown op"),
                      (lambda t: t["stage"]["fval"].__setitem__((1, 0), float("nan")), "fval"),
                      (lambda t: t["stage"]["aff"].__setitem__((0, 1, 2), (1 << 30) + 1), "aff\\[2\\]")]:
        bad = good.copy()
        edit(bad)
        out = torch.full((n,), 0x5A, dtype=torch.uint8, device=dev)
        with pytest.raises(bvc._lib.BvcError, match=msg):
            A.rand_augment(x, bad, out=out)
        torch.cuda.synchronize()
        assert bool((out == 0x5A).all()), f"{msg}: refused, but out was written"
    with pytest.raises(ValueError, match="workspace"):
        A.rand_augment(x, good, workspace=work[:need - 1])


def test_the_call_does_not_synchronise():
    """a table with statistics stages, table stages and a gather, under torch's synchronisation trap (the first call, outside it,
    loads the code objects)"""
    H, W = 33, 65
    x = R.frames(3, H, W, seed=75)
    t = R.table(A, H, W, [[("Equalize", None), ("Contrast", 1.2), ("Rotate", 9.0)], [("Solarize", 99), ("Sharpness", 1.5)], []])
    xd = x.to(dev)
    A.rand_augment(xd, t)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = A.rand_augment(xd, t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _same(out.cpu(), A.rand_augment_host(x, t), "no synchronisation 33x65")


def test_identity_table_returns_the_input():
    x = R.frames(3, 17, 40, seed=80)
    got = _gpu(x, A.empty_randaug_table(3))
    assert torch.equal(got, x)


def test_rand_augment_callable_and_clip_augment_hook():
    g = torch.Generator().manual_seed(90)
    clips = torch.randint(0, 256, (2, 4, 3, 40, 40), generator=g, dtype=torch.uint8)
    ra = bvc.RandAugment("rand-m9-n4-mstd0.5-p1-inc1", generator=np.random.default_rng(91))
    out = ra(clips.to(dev))
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 4, 3, 40, 40)
    t = ra.last_table
    assert t.shape == (8,) and bool((t["nops"] == 4).all())
    _same(out.cpu(), A.rand_augment_host(clips, t), "RandAugment on [2, 4, 3, 40, 40]")
    per_frame = bvc.RandAugment("rand-m9-n4-mstd0.5-p1-inc1", consistent=False, generator=np.random.default_rng(92))
    out = per_frame(clips.to(dev))
    torch.cuda.synchronize()
    _same(out.cpu(), A.rand_augment_host(clips, per_frame.last_table), "RandAugment per frame")

    # as ClipAugment's last stage ('c', 'b', 'o' only: the stages before are exact too), two views
    aug = A.ClipAugment(40, augs="cbo", views=2, randaug="rand-m9-n3-p1", generator=np.random.default_rng(93))
    src = torch.randint(0, 256, (2, 4, 3, 48, 56), generator=g, dtype=torch.uint8)
    out = aug(src.to(dev))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (4, 4, 3, 40, 40) and aug.last_randaug_table.shape == (16,)
    before = A.clip_post_host(A.clip_transform_host(src, aug.last_table, 40), aug.last_post_table)
    _same(out.cpu(), A.rand_augment_host(before, aug.last_randaug_table).view_as(out), "ClipAugment(randaug=...)")

    # without randaug: the same seed, the same two tables, the bytes of the two stages alone
    plain = A.ClipAugment(40, augs="cbo", views=2, generator=np.random.default_rng(93))
    out_plain = plain(src.to(dev))
    torch.cuda.synchronize()
    assert plain.last_randaug_table is None
    assert plain.last_table.tobytes() == aug.last_table.tobytes() and plain.last_post_table.tobytes() == aug.last_post_table.tobytes()
    _same(out_plain.cpu(), before.view_as(out_plain), "ClipAugment without randaug")
