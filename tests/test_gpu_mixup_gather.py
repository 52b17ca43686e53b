"""Mixup / CutMix inside the patch gather, at op level (bvc_op_gather_patches_mix) against the plain gather of the clip that
tests/mixup_ref.mix_clips composes in torch.

Selection (identity, CutMix) is exact: bitwise equality.  Mixup computes lam * own + (1 - lam) * partner in f32 and may contract the
multiply-add, which moves the f32 value by a few f32 ulps and so the bf16 rounding by at most one step: every element within 1 bf16
ulp, and fewer than 1 % of the elements different at all.  On the CPU, for this file's inputs (36 864 pixels, lam 0.25 and 0.7310586,
empty and mixed box), the reference computed with either product fused into the sum differed from the unfused one in up to 21 % of the
f32 values and in none of the bf16 values, so the 1 % bar leaves room for nothing but such boundary cases.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from tests import mixup_ref as R   # noqa: E402

L = G.L
bvc = G.bvc
dev = torch.device("cuda:0")
B, T, C, H, W, TS, PS = 3, 4, 3, 32, 32, 2, 16
NTOK = (T // TS) * (H // PS) * (W // PS)
K = C * TS * PS * PS
FLIP = [2, 1, 0]                  # the odd batch makes clip 1 its own partner
EMPTY = (0, 0, 0, 0)
IDX = {"all": [list(range(NTOK))] * B,
       "subset": [[0, 2, 3, 5, 7], [1, 2, 4, 6, 7], [0, 1, 3, 4, 6]]}      # ascending per clip, as the visible-token lists are


@pytest.fixture(scope="module")
def clips():
    g = torch.Generator().manual_seed(20)
    u8 = torch.randint(0, 256, (B, T, C, H, W), generator=g, dtype=torch.uint8)
    f32 = (u8.float() / 255.0 - 0.5) / 0.25            # ToTensor + Normalize, the arithmetic of the uint8 path
    return {"u8": u8.to(dev), "f32": f32.to(dev), "host": f32}


def _fmt(src):
    return L.pixel_format(src, 0.5, 0.25, C)


def _idx(which):
    return torch.tensor(IDX[which], dtype=torch.int32, device=dev).contiguous()


def _plain(f32_dev, idx):
    n = idx.shape[1]
    A = torch.zeros(B * n, K, device=dev, dtype=torch.bfloat16)
    L.check(L.lib().bvc_op_gather_patches(G.ptr(f32_dev), G.ptr(idx), G.ptr(A), B, n, T, C, H, W, TS, PS, G.stream()), "gather")
    return A


def _mixed(src, idx, partner, lam, box):
    mix = bvc.ClipMix(partner, lam, box, image_size=(H, W), device=dev)
    n = idx.shape[1]
    A = torch.full((B * n, K), float("nan"), device=dev, dtype=torch.bfloat16)
    f = _fmt(src)
    L.check(L.lib().bvc_op_gather_patches_mix(G.ptr(src), ctypes.byref(f) if f is not None else None, G.ptr(idx), G.ptr(A),
                                              G.ptr(mix.table), B, n, T, C, H, W, TS, PS, G.stream()), "gather_mix")
    torch.cuda.synchronize()
    return A


def _ref(clips, idx, partner, lam, box):
    """the plain gather of the clip composed in torch"""
    A = _plain(R.mix_clips(clips["host"], partner, lam, box).to(dev), idx)
    torch.cuda.synchronize()
    return A


def test_plain_gather_is_the_unfold(clips):
    """the yardstick itself: the plain gather equals the unfold of the clip, for the token subset too"""
    rows = R.tokens_to_rows(clips["host"], T, C, H, W, TS, PS).to(torch.bfloat16)
    for which in IDX:
        idx = _idx(which)
        ref = torch.stack([rows[b, IDX[which][b]] for b in range(B)]).reshape(-1, K)
        assert torch.equal(_plain(clips["f32"], idx).cpu(), ref)


@pytest.mark.parametrize("which", ["all", "subset"])
@pytest.mark.parametrize("src", ["f32", "u8"])
def test_identity_specs_are_the_plain_gather(clips, src, which):
    idx = _idx(which)
    A = _mixed(clips[src], idx, list(range(B)), [1.0] * B, [EMPTY] * B)
    assert torch.equal(A, _plain(clips["f32"], idx))


@pytest.mark.parametrize("which", ["all", "subset"])
@pytest.mark.parametrize("src", ["f32", "u8"])
@pytest.mark.parametrize("box", [(0, 32, 0, 32), EMPTY, (3, 29, 5, 23), (16, 32, 0, 16)])
def test_cutmix_selects_exactly(clips, src, which, box):
    """whole image, empty, a box whose edges cut 4- and 8-pixel runs and cross the patch boundary at 16, exactly one patch"""
    idx = _idx(which)
    A = _mixed(clips[src], idx, FLIP, [1.0] * B, [box] * B)
    ref = _ref(clips, idx, FLIP, [1.0] * B, [box] * B)
    assert torch.equal(A, ref)
    if box == (0, 32, 0, 32):
        rows = _plain(clips["f32"], idx).view(B, -1, K)
        if which == "all":
            assert torch.equal(A.view(B, -1, K), rows[FLIP])      # every clip became its partner


def _ordinal(x):
    """bf16 -> integers in value order (adjacent representable values differ by 1; +0 and -0 coincide)"""
    bits = x.view(torch.int16).int()
    return torch.where(bits >= 0, bits, -(bits & 0x7FFF))


@pytest.mark.parametrize("which", ["all", "subset"])
@pytest.mark.parametrize("src", ["f32", "u8"])
@pytest.mark.parametrize("lam,box", [(0.25, EMPTY), (0.7310586, EMPTY), (0.25, (3, 29, 5, 23))])
def test_mixup_blends_within_one_bf16_ulp(clips, src, which, lam, box):
    idx = _idx(which)
    A = _mixed(clips[src], idx, FLIP, [lam] * B, [box] * B)
    ref = _ref(clips, idx, FLIP, [lam] * B, [box] * B)
    assert torch.isfinite(A.float()).all()
    d = (_ordinal(A) - _ordinal(ref)).abs()
    share = float((d != 0).float().mean())
    print(f"mixup lam {lam} box {box} {src} {which}: max bf16 ulp {int(d.max())}, share differing {share:.2e}")
    assert int(d.max()) <= 1
    assert share < 0.01
    assert not torch.equal(A, _plain(clips["f32"], idx))          # it did mix


def test_per_clip_specs_in_one_table(clips):
    """one table, three kinds: CutMix for clip 0, untouched clip 1, Mixup with a box for clip 2"""
    idx = _idx("all")
    partner, lam, box = [2, 1, 0], [1.0, 1.0, 0.5], [(3, 29, 5, 23), EMPTY, (16, 32, 0, 16)]
    for src in ("f32", "u8"):
        A = _mixed(clips[src], idx, partner, lam, box).view(B, -1, K)
        ref = _ref(clips, idx, partner, lam, box).view(B, -1, K)
        assert torch.equal(A[:2], ref[:2])
        assert int((_ordinal(A[2]) - _ordinal(ref[2])).abs().max()) <= 1


def test_null_arguments_are_refused(clips):
    idx = _idx("all")
    A = torch.zeros(B * NTOK, K, device=dev, dtype=torch.bfloat16)
    assert L.lib().bvc_op_gather_patches_mix(G.ptr(clips["f32"]), None, G.ptr(idx), G.ptr(A), None, B, NTOK, T, C, H, W, TS, PS, G.stream()) != 0
    assert b"null" in L.lib().bvc_last_error()
    mix = bvc.ClipMix(list(range(B)), [1.0] * B, [EMPTY] * B, device=dev)
    assert L.lib().bvc_op_gather_patches_mix(G.ptr(clips["f32"]), None, G.ptr(idx), G.ptr(A), G.ptr(mix.table), 0, NTOK, T, C, H, W, TS, PS,
                                             G.stream()) != 0


def test_out_of_range_entry_is_clamped_and_poisons_the_forward(clips):
    """The kernel clamps the partner into [0, B) and the box into the image before it forms an address (rowops.hip,
    gather_patches_mix_kernel: `partner`, `y0` ... `x1`), so an entry out of range reads clip B - 1 / clip 0 instead: at op level the
    result is that of the clamped table; at model level the context's status word turns the logits NaN, and the next forward is
    clean again."""
    idx = _idx("all")
    A = _mixed(clips["u8"], idx, [7, 1, -3], [1.0] * B, [(-5, 40, 8, 99)] * B)
    ref = _ref(clips, idx, [2, 1, 0], [1.0] * B, [(0, 32, 8, 32)] * B)
    assert torch.equal(A, ref)

    from oracle import videomae_oracle as vo
    from tests.test_gpu_videomae_cls import _heads, _model
    cfg = vo.TINY
    m = _model(cfg, vo.make_params(cfg, seed=0), _heads(cfg))
    px = vo.synthetic_batch(cfg, 4, 0, 0.9)[0].to(dev)
    S = cfg.image_size
    good = bvc.ClipMix([3, 2, 1, 0], [1.0] * 4, [(0, S // 2, 0, S // 2)] * 4, image_size=(S, S), device=dev)
    bad = bvc.ClipMix([3, 2, 9, 0], [1.0] * 4, [(0, S // 2, 0, S // 2)] * 4, image_size=(S, S), device=dev)
    out = m(pixel_values=px, mix=bad, output_last_hidden_state=True)
    assert torch.isnan(out.logits).all() and torch.isnan(out.last_hidden_state).all()
    assert torch.isfinite(m(pixel_values=px, mix=good).logits).all()
    with torch.no_grad():                                  # the forward-only context has the same guard
        assert torch.isnan(m(pixel_values=px, mix=bad).logits).all()
        assert torch.isfinite(m(pixel_values=px, mix=good).logits).all()


def test_rows_shorter_than_a_wave(clips):
    """One channel, tubelet 1: K / 8 = 32 threads per row of A, so a wave spans two rows and the kernel runs its per-lane instantiation
    (the reference's shapes have K / 8 = 192 and run the wave-uniform one).  Same bars."""
    t, c, ts = 2, 1, 1
    ntok, k = (t // ts) * (H // PS) * (W // PS), c * ts * PS * PS
    g = torch.Generator().manual_seed(21)
    u8 = torch.randint(0, 256, (B, t, c, H, W), generator=g, dtype=torch.uint8)
    f32 = (u8.float() / 255.0 - 0.5) / 0.25
    idx = torch.tensor([[0, 3, 4, 6, 7], [1, 2, 3, 5, 6], [0, 1, 2, 5, 7]], dtype=torch.int32, device=dev)
    n = idx.shape[1]

    def plain(x):
        A = torch.zeros(B * n, k, device=dev, dtype=torch.bfloat16)
        L.check(L.lib().bvc_op_gather_patches(G.ptr(x), G.ptr(idx), G.ptr(A), B, n, t, c, H, W, ts, PS, G.stream()), "gather")
        torch.cuda.synchronize()
        return A

    for lam, box in ((1.0, (3, 29, 5, 23)), (0.25, (3, 29, 5, 23)), (1.0, EMPTY)):
        partner = FLIP if (lam, box) != (1.0, EMPTY) else list(range(B))
        mix = bvc.ClipMix(partner, [lam] * B, [box] * B, image_size=(H, W), device=dev)
        ref = plain(R.mix_clips(f32, partner, [lam] * B, [box] * B).to(dev))
        for src in (f32.to(dev), u8.to(dev)):
            f = L.pixel_format(src, 0.5, 0.25, c)
            A = torch.full((B * n, k), float("nan"), device=dev, dtype=torch.bfloat16)
            L.check(L.lib().bvc_op_gather_patches_mix(G.ptr(src), ctypes.byref(f) if f is not None else None, G.ptr(idx), G.ptr(A),
                                                      G.ptr(mix.table), B, n, t, c, H, W, ts, PS, G.stream()), "gather_mix")
            torch.cuda.synchronize()
            if lam == 1.0:
                assert torch.equal(A, ref)
            else:
                d = (_ordinal(A) - _ordinal(ref)).abs()
                assert int(d.max()) <= 1 and float((d != 0).float().mean()) < 0.01
