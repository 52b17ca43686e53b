"""Random erasing inside the patch gather, at op level: bvc_op_erase_noise against the float64 Box-Muller of tests/erase_ref.py, and
bvc_op_gather_patches_aug against the plain gather of the clip that erase_ref.erase_clips (and mixup_ref.mix_clips) compose in torch
from the DEVICE noise - erasing only selects values, so that comparison is bitwise.

Noise accuracy.  The bar A is not a constant: the test evaluates the kernel's formula in numpy float32 on the very draws it checks and
takes 4 x the largest deviation of that from float64; the factor is room for the device math library's last-ulp differences in logf /
sqrtf / sincosf.  For this file's seed and offset numpy gives a largest f32 deviation of 1.26e-6 over the 36 864 pixel values and
8.35e-7 over the 192 colours, so A = 5.04e-6 and 3.34e-6; the device deviated by 1.14e-6 and 8.64e-7 (the test prints all three).

Composed with Mixup the blend lam * own + (1 - lam) * partner may be contracted into a multiply-add, as in the mix kernel: within
1 bf16 ulp and fewer than 1 % of the elements different, the bar and the argument of tests/test_gpu_mixup_gather.py - erased values
are blended with the partner's values like any other, never with themselves.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from tests import erase_ref as E   # noqa: E402
from tests import mixup_ref as R   # noqa: E402

L = G.L
bvc = G.bvc
dev = torch.device("cuda:0")
B, T, C, H, W, TS = 3, 4, 3, 32, 32, 2
SEED, OFFSET = 0x9E3779B97F4A7C15, (3 << 32) | 5          # both halves of both words are in use
FLIP = [2, 1, 0]
EMPTY = (0, 0, 0, 0)
WHOLE, CUT, PATCH = (0, 32, 0, 32), (3, 29, 5, 23), (16, 32, 0, 16)
# token lists per patch size: K / 8 = 192 at PS 16 (a wave lies in one row of A), 48 at PS 8 (it does not)
IDX = {16: {"all": [list(range(8))] * B, "subset": [[0, 2, 3, 5, 7], [1, 2, 4, 6, 7], [0, 1, 3, 4, 6]]},
       8: {"all": [list(range(32))] * B, "subset": [[0, 5, 9, 14, 18, 27, 31], [1, 2, 10, 13, 21, 22, 30], [3, 4, 11, 12, 17, 25, 29]]}}
GEOMS = [(16, "all"), (16, "subset"), (8, "all"), (8, "subset")]


@pytest.fixture(scope="module")
def clips():
    g = torch.Generator().manual_seed(20)
    u8 = torch.randint(0, 256, (B, T, C, H, W), generator=g, dtype=torch.uint8)
    f32 = (u8.float() / 255.0 - 0.5) / 0.25            # ToTensor + Normalize, the arithmetic of the uint8 path
    noise = bvc.erase_noise(SEED, OFFSET, 0, B, T, C, H, W, dev)
    colours = bvc.erase_noise(SEED, OFFSET, 1, B, T, C, H, W, dev)
    torch.cuda.synchronize()
    return {"u8": u8.to(dev), "f32": f32.to(dev), "host": f32, "noise": noise.cpu(), "colours": colours.cpu()}


def _idx(ps, which):
    return torch.tensor(IDX[ps][which], dtype=torch.int32, device=dev).contiguous()


def _plain(f32_dev, idx, ps):
    n = idx.shape[1]
    A = torch.zeros(B * n, C * TS * ps * ps, device=dev, dtype=torch.bfloat16)
    L.check(L.lib().bvc_op_gather_patches(G.ptr(f32_dev), G.ptr(idx), G.ptr(A), B, n, T, C, H, W, TS, ps, G.stream()), "gather")
    torch.cuda.synchronize()
    return A


def _aug(src, idx, ps, boxes, modes, mix=None, seed=SEED, offset=OFFSET):
    er = bvc.ClipErase(boxes, modes, seed=seed, offset=offset, image_size=(H, W), device=dev)
    n = idx.shape[1]
    A = torch.full((B * n, C * TS * ps * ps), float("nan"), device=dev, dtype=torch.bfloat16)
    f = L.pixel_format(src, 0.5, 0.25, C)
    L.check(L.lib().bvc_op_gather_patches_aug(G.ptr(src), ctypes.byref(f) if f is not None else None, G.ptr(idx), G.ptr(A),
                                              G.ptr(mix.table) if mix is not None else None, G.ptr(er.table), er.num_boxes, seed, offset,
                                              B, n, T, C, H, W, TS, ps, G.stream()), "gather_aug")
    torch.cuda.synchronize()
    return A


def _mix_kernel(src, idx, ps, mix):
    n = idx.shape[1]
    A = torch.full((B * n, C * TS * ps * ps), float("nan"), device=dev, dtype=torch.bfloat16)
    f = L.pixel_format(src, 0.5, 0.25, C)
    L.check(L.lib().bvc_op_gather_patches_mix(G.ptr(src), ctypes.byref(f) if f is not None else None, G.ptr(idx), G.ptr(A),
                                              G.ptr(mix.table), B, n, T, C, H, W, TS, ps, G.stream()), "gather_mix")
    torch.cuda.synchronize()
    return A


def _ref(clips, idx, ps, boxes, modes, mix=None):
    """the plain gather of the clip erased, then mixed, in torch"""
    x = E.erase_clips(clips["host"], boxes, modes, clips["noise"], clips["colours"])
    if mix is not None:
        x = R.mix_clips(x, mix.partner, mix.lam, mix.box)
    return _plain(x.to(dev), idx, ps)


def _ordinal(x):
    """bf16 -> integers in value order (adjacent representable values differ by 1; +0 and -0 coincide)"""
    bits = x.view(torch.int16).int()
    return torch.where(bits >= 0, bits, -(bits & 0x7FFF))


# ---------------------------------------------------------------- the noise
@pytest.mark.parametrize("kind", [0, 1])
def test_noise_matches_the_float64_rule(clips, kind):
    got = (clips["noise"] if kind == 0 else clips["colours"]).numpy().astype(np.float64)
    ref = E.pixel_noise(SEED, OFFSET, B, T, C, H, W) if kind == 0 else E.colours(SEED, OFFSET, B, T)
    f32 = E.pixel_noise(SEED, OFFSET, B, T, C, H, W, np.float32) if kind == 0 else E.colours(SEED, OFFSET, B, T, np.float32)
    own = float(np.abs(f32.astype(np.float64) - ref).max())
    A = 4.0 * own
    err = float(np.abs(got - ref).max())
    print(f"erase noise kind {kind}: numpy f32 deviates {own:.2e} from f64, bar A = {A:.2e}, device deviates {err:.2e} (n = {ref.size})")
    assert got.shape == ref.shape
    assert err <= A
    assert np.abs(got).max() <= 5.78


def test_noise_moments(clips):
    z = clips["noise"].numpy().astype(np.float64).reshape(-1)
    n = z.size
    assert n == 36864
    print(f"erase noise: mean {z.mean():+.4f} (bar {5 / np.sqrt(n):.4f}), var {z.var():.4f} (bar 1 +- {5 * np.sqrt(2 / n):.4f})")
    assert abs(z.mean()) <= 5 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / n)


def test_noise_differs_by_frame_clip_and_offset_and_repeats_bitwise(clips):
    z, col = clips["noise"], clips["colours"]
    assert not torch.equal(z[0, 0], z[0, 1]) and not torch.equal(z[0], z[1])
    assert not torch.equal(col[0, 0], col[0, 1]) and not torch.equal(col[0], col[1]) and not torch.equal(col[0, 0, 0], col[0, 0, 1])
    for kind, ref in ((0, z), (1, col)):
        again = bvc.erase_noise(SEED, OFFSET, kind, B, T, C, H, W, dev).cpu()
        assert torch.equal(again, ref)
        assert not torch.equal(bvc.erase_noise(SEED, OFFSET + 1, kind, B, T, C, H, W, dev).cpu(), ref)
        assert not torch.equal(bvc.erase_noise(SEED, OFFSET + (1 << 32), kind, B, T, C, H, W, dev).cpu(), ref)
        assert not torch.equal(bvc.erase_noise(SEED + 1, OFFSET, kind, B, T, C, H, W, dev).cpu(), ref)
    assert L.lib().bvc_op_erase_noise(SEED, OFFSET, 2, B, T, C, H, W, G.ptr(z.to(dev)), G.stream()) != 0
    assert L.lib().bvc_op_erase_noise(SEED, OFFSET, 0, B, T, C, H, W, None, G.stream()) != 0


# ---------------------------------------------------------------- erasing alone: bitwise
@pytest.mark.parametrize("ps,which", GEOMS)
@pytest.mark.parametrize("src", ["f32", "u8"])
@pytest.mark.parametrize("mode", ["const", "rand", "pixel"])
def test_one_box_per_clip_is_exact(clips, src, ps, which, mode):
    """whole image, empty, a box whose edges cut 4- and 8-pixel runs and cross the patch boundary at 16, exactly one 16 x 16 patch"""
    idx = _idx(ps, which)
    plain = _plain(clips["f32"], idx, ps)
    for box in (WHOLE, EMPTY, CUT, PATCH):
        boxes, modes = [[box]] * B, [[bvc.erase.MODES[mode]]] * B
        A = _aug(clips[src], idx, ps, boxes, modes)
        assert torch.equal(A, _ref(clips, idx, ps, boxes, modes)), box
        assert torch.equal(A, plain) == (box == EMPTY), box
    if mode == "const":
        assert (_aug(clips[src], idx, ps, [[WHOLE]] * B, [[0]] * B).float() == 0).all()


@pytest.mark.parametrize("ps,which", GEOMS)
@pytest.mark.parametrize("src", ["f32", "u8"])
def test_later_box_wins_and_per_clip_tables(clips, src, ps, which):
    idx = _idx(ps, which)
    # two overlapping boxes of different modes, in each of the six orders of two modes
    for m0 in range(3):
        for m1 in range(3):
            if m0 == m1:
                continue
            boxes, modes = [[CUT, (10, 32, 12, 31)]] * B, [[m0, m1]] * B
            A = _aug(clips[src], idx, ps, boxes, modes)
            assert torch.equal(A, _ref(clips, idx, ps, boxes, modes)), (m0, m1)
            swapped = _aug(clips[src], idx, ps, [[(10, 32, 12, 31), CUT]] * B, [[m1, m0]] * B)
            assert not torch.equal(A, swapped)                           # the order matters in the overlap
    # one table: clip 0 no box, clip 1 one box, clip 2 four boxes of all modes, the last one inside the third
    boxes = [[EMPTY] * 4, [CUT, EMPTY, EMPTY, EMPTY], [(0, 9, 0, 32), PATCH, (2, 30, 20, 28), (4, 12, 22, 26)]]
    modes = [[2, 2, 2, 2], [1, 0, 0, 0], [1, 2, 0, 1]]
    A = _aug(clips[src], idx, ps, boxes, modes)
    assert torch.equal(A, _ref(clips, idx, ps, boxes, modes))
    n = idx.shape[1]
    assert torch.equal(A[:n], _plain(clips["f32"], idx, ps)[:n])


@pytest.mark.parametrize("ps,which", GEOMS)
@pytest.mark.parametrize("src", ["f32", "u8"])
def test_no_boxes_is_the_plain_gather_and_the_mix_kernel(clips, src, ps, which):
    idx = _idx(ps, which)
    for nb in (1, 4):
        boxes, modes = [[EMPTY] * nb] * B, [[2] * nb] * B
        assert torch.equal(_aug(clips[src], idx, ps, boxes, modes), _plain(clips["f32"], idx, ps))
        for lam, box in ((1.0, CUT), (0.25, EMPTY), (0.7310586, PATCH)):
            mix = bvc.ClipMix(FLIP, [lam] * B, [box] * B, image_size=(H, W), device=dev)
            assert torch.equal(_aug(clips[src], idx, ps, boxes, modes, mix), _mix_kernel(clips[src], idx, ps, mix)), (lam, box)


# ---------------------------------------------------------------- composed with the mix
@pytest.mark.parametrize("ps,which", GEOMS)
@pytest.mark.parametrize("src", ["f32", "u8"])
def test_cutmix_over_erased_partners_is_exact(clips, src, ps, which):
    """the CutMix box intersects the partner's erase box: inside it the partner's ERASED content shows, outside it the clip's own"""
    idx = _idx(ps, which)
    boxes = [[(3, 29, 5, 23), EMPTY], [(0, 20, 14, 32), (12, 18, 0, 32)], [(8, 32, 0, 12), (0, 32, 9, 10)]]
    modes = [[2, 2], [1, 0], [2, 1]]
    for cut in ((10, 26, 2, 19), WHOLE, PATCH):
        mix = bvc.ClipMix(FLIP, [1.0] * B, [cut] * B, image_size=(H, W), device=dev)
        A = _aug(clips[src], idx, ps, boxes, modes, mix)
        assert torch.equal(A, _ref(clips, idx, ps, boxes, modes, mix)), cut
    if which == "all":       # every clip became its erased partner
        n = idx.shape[1]
        whole = bvc.ClipMix(FLIP, [1.0] * B, [WHOLE] * B, image_size=(H, W), device=dev)
        assert torch.equal(_aug(clips[src], idx, ps, boxes, modes, whole).view(B, n, -1), _aug(clips[src], idx, ps, boxes, modes).view(B, n, -1)[FLIP])


@pytest.mark.parametrize("ps,which", GEOMS)
@pytest.mark.parametrize("src", ["f32", "u8"])
def test_mixup_over_erased_clips_within_one_bf16_ulp(clips, src, ps, which):
    idx = _idx(ps, which)
    boxes, modes = [[CUT], [(0, 20, 14, 32)], [PATCH]], [[2], [1], [2]]
    for lam, box in ((0.25, EMPTY), (0.25, (10, 26, 2, 19))):
        mix = bvc.ClipMix(FLIP, [lam] * B, [box] * B, image_size=(H, W), device=dev)
        A = _aug(clips[src], idx, ps, boxes, modes, mix)
        ref = _ref(clips, idx, ps, boxes, modes, mix)
        assert torch.isfinite(A.float()).all()
        d = (_ordinal(A) - _ordinal(ref)).abs()
        share = float((d != 0).float().mean())
        print(f"mixup {lam} box {box} over erased clips, {src} ps {ps} {which}: max bf16 ulp {int(d.max())}, share differing {share:.2e}")
        assert int(d.max()) <= 1
        assert share < 0.01
        assert not torch.equal(A, _aug(clips[src], idx, ps, boxes, modes))          # it did mix


# ---------------------------------------------------------------- bad entries
def test_null_table_and_box_counts_are_refused(clips):
    idx = _idx(16, "all")
    A = torch.zeros(B * 8, C * TS * 256, device=dev, dtype=torch.bfloat16)
    er = bvc.ClipErase([[CUT] * 4] * B, 2, device=dev)

    def call(tab, nb):
        return L.lib().bvc_op_gather_patches_aug(G.ptr(clips["f32"]), None, G.ptr(idx), G.ptr(A), None, tab, nb, SEED, OFFSET, B, 8, T, C, H, W,
                                                 TS, 16, G.stream())
    assert call(None, 1) != 0 and b"null" in L.lib().bvc_last_error()
    assert call(G.ptr(er.table), 5) != 0 and b"boxes" in L.lib().bvc_last_error()
    assert call(G.ptr(er.table), 0) != 0
    assert call(G.ptr(er.table), 4) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("ps", [16, 8])
def test_out_of_range_entry_is_clamped_and_poisons_the_forward(clips, ps):
    """The kernel clamps a box into the image and a mode into 0 .. 2 before it forms an address or a counter (rowops.hip, erase_run:
    `y0` ... `x1`, `mode`), so at op level the result is that of the clamped table; at model level the context's status word turns
    the logits NaN, and the next forward is clean again."""
    idx = _idx(ps, "all")
    for src in ("u8", "f32"):
        A = _aug(clips[src], idx, ps, [[(-1, 33, 5, 23)], [(3, 29, -1, 33)], [CUT]], [[2], [1], [3]])
        assert torch.equal(A, _ref(clips, idx, ps, [[(0, 32, 5, 23)], [(3, 29, 0, 32)], [CUT]], [[2], [1], [2]]))
        A = _aug(clips[src], idx, ps, [[(-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1)], [CUT], [CUT]], [[0], [-1], [2 ** 31 - 1]])
        assert torch.equal(A, _ref(clips, idx, ps, [[WHOLE], [CUT], [CUT]], [[0], [0], [2]]))
    if ps != 16:
        return
    from oracle import videomae_oracle as vo
    from tests.test_gpu_videomae_cls import _heads, _model
    cfg = vo.TINY
    m = _model(cfg, vo.make_params(cfg, seed=0), _heads(cfg))
    px = vo.synthetic_batch(cfg, 4, 0, 0.9)[0].to(dev)
    S = cfg.image_size
    good = bvc.ClipErase([[(0, S // 2, 0, S // 2)]] * 4, 2, seed=1, image_size=(S, S), device=dev)
    for bad in (bvc.ClipErase([[(0, S // 2, 0, S // 2)]] * 3 + [[(0, S + 1, 0, S // 2)]], 2, seed=1, image_size=(S, S), device=dev),
                bvc.ClipErase([[(0, S // 2, 0, S // 2)]] * 4, [[2], [2], [3], [2]], seed=1, image_size=(S, S), device=dev)):
        out = m(pixel_values=px, erase=bad, output_last_hidden_state=True)
        assert torch.isnan(out.logits).all() and torch.isnan(out.last_hidden_state).all()
        assert torch.isfinite(m(pixel_values=px, erase=good).logits).all()
        with torch.no_grad():                                  # the forward-only context has the same guard
            assert torch.isnan(m(pixel_values=px, erase=bad).logits).all()
            assert torch.isfinite(m(pixel_values=px, erase=good).logits).all()
