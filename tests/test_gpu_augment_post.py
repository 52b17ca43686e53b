"""The post stage of the clip transforms on the GPU (bvc_op_clip_post, csrc/augment.hip: blur, gray, rotation) against the host twin
(the same csrc/augment.h arithmetic compiled for the host), against PIL's recorded output, and ClipAugment end to end.

The stage is integer arithmetic: the bar is ZERO differing elements everywhere.  Only ClipAugment with colour jitter inherits the bar of
the stage before it (tests/test_gpu_augment.py, _check_twin).  Shapes: the blur kernel works on 32 x 64 tiles with a halo of 3 (r + 1)
pixels in words of four pixels, so the frames run from smaller than one box window (1 x 9, 3 x 3) over widths that are no multiple of
4 (the byte paths) and one tile with every halo beyond the frame (17 x 40) to several tiles with halos inside the frame on some sides
and a last tile narrower than a word (33 x 65, 64 x 48, 70 x 132).  No test feeds the kernels a table the call would refuse.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import augment_post_ref as P   # noqa: E402
from tests import augment_ref as R   # noqa: E402
from tests import gpu_util as G   # noqa: E402
from tests import test_augment_post_host as H   # noqa: E402

bvc = G.bvc
A = bvc.augment
dev = torch.device("cuda:0")


def _gpu(x, t):
    out = A.clip_post(x.to(dev), t)
    torch.cuda.synchronize()
    return out.cpu()


def _same(got, want, what):
    n = int((got != want).sum())
    print(f"{what}: {n} of {got.numel()} elements differ from the host twin")
    assert n == 0, what


BLUR_RADII = [0.0, 0.3, 1.0, 2.0, 4.0]


@pytest.mark.parametrize("Hh,W", [(1, 9), (3, 3), (17, 40), (33, 65), (64, 48), (70, 132)])
def test_blur_equals_host_twin(Hh, W):
    cases = [dict(radius=r) for r in BLUR_RADII] + [dict(), dict(radius=1.3, to_gray=True), dict(to_gray=True)]     # mixed: one frame untouched
    x = P.frames(len(cases), Hh, W, seed=Hh * 100 + W)
    t = P.table(A, Hh, W, cases)
    got = _gpu(x, t)
    _same(got, A.clip_post_host(x, t), f"blur {Hh}x{W}")
    assert torch.equal(got[0], x[0]) and torch.equal(got[5], x[5])


ROT_ANGLES = [0.0, 90.0, -90.0, 45.0, 1e-3, -37.5]


@pytest.mark.parametrize("Hh,W", [(24, 24), (17, 40), (33, 65)])
def test_rotation_equals_host_twin(Hh, W):
    cases = [dict(angle=a) for a in ROT_ANGLES] + [dict()]
    x = P.frames(len(cases), Hh, W, seed=Hh * 100 + W + 1)
    t = P.table(A, Hh, W, cases)
    got = _gpu(x, t)
    _same(got, A.clip_post_host(x, t), f"rotation {Hh}x{W}")
    assert torch.equal(got[0], x[0]) and torch.equal(got[6], x[6])


def test_blur_gray_rotate_combined():
    x = P.frames(len(H.COMBINED), 33, 65, seed=5)
    t = P.table(A, 33, 65, H.COMBINED)
    _same(_gpu(x, t), A.clip_post_host(x, t), "blur + gray + rotate 33x65")


def test_gpu_equals_the_pil_fixture(golden_dir):
    _, (_, Hh, W), cases = H.load_golden(golden_dir)
    x = torch.stack([c[0] for c in cases])
    got = _gpu(x, P.table(A, Hh, W, [c[1] for c in cases]))
    for i, (_, kw, want) in enumerate(cases):
        assert torch.equal(got[i], want), kw


@pytest.mark.parametrize("Hh,W,offset", [(32, 40, 0), (33, 65, 1)])
def test_out_path_writes_exactly_its_bytes(Hh, W, offset):
    """`out=` with 64 guard bytes on each side, for each launch plan: blur only, rotation only, both (through the workspace) and the
    identity (one copy); at an aligned start with whole-word rows and at an odd start with odd rows"""
    guard = 64
    plans = {"blur": [dict(radius=2.0), dict(to_gray=True)], "rotate": [dict(angle=33.0), dict()],
             "both": [dict(radius=1.0, angle=-70.0), dict(radius=4.0)], "identity": [dict(), dict()]}
    x = P.frames(2, Hh, W, seed=21)
    n = x.numel()
    for name, cases in plans.items():
        t = P.table(A, Hh, W, cases)
        buf = torch.full((guard + offset + n + guard,), 0xA5, dtype=torch.uint8, device=dev)
        out = buf[guard + offset:guard + offset + n]
        assert A.clip_post(x.to(dev), t, out=out) is out
        torch.cuda.synchronize()
        assert bool((buf[:guard + offset] == 0xA5).all()) and bool((buf[guard + offset + n:] == 0xA5).all()), f"{name}: bytes outside out were written"
        _same(out.cpu().view_as(x), A.clip_post_host(x, t), f"out= {name} {Hh}x{W}")


def _check_stage_one_bar(got, host, near_share, what):
    """tests/test_gpu_augment.py::_check_twin: at most 1 LSB apart, and a differing share of at most the share of elements at which the
    colour chains' fp64 oracle (tests/augment_ref.py) sits near a truncation tie"""
    d = (got.int() - host.int()).abs()
    share = float((d > 0).float().mean())
    print(f"{what}: GPU vs host twins: max |diff| {int(d.max())}, differing share {share:.4%} (near-tie share {near_share:.4%})")
    assert int(d.max()) <= 1, what
    assert share <= near_share, f"{what}: {share:.4%} of the elements differ from the host twins"


def test_clip_augment_end_to_end():
    g = torch.Generator().manual_seed(30)
    src = torch.randint(0, 256, (2, 2, 3, 32, 40), generator=g, dtype=torch.uint8)
    for augs, exact in (("cbo", True), ("cjbo", False)):
        aug = A.ClipAugment(16, augs=augs, views=2, generator=np.random.default_rng(31))
        out = aug(src.to(dev))
        torch.cuda.synchronize()
        assert out.dtype == torch.uint8 and tuple(out.shape) == (4, 2, 3, 16, 16)
        post = aug.last_post_table
        assert bool((post["rotate"] == 1).all()) and 0 < int((post["blur_r"] >= 0).sum())
        twin = A.clip_post_host(A.clip_transform_host(src, aug.last_table, 16), post).view_as(out)
        if exact:
            _same(out.cpu(), twin, f"ClipAugment({augs!r})")
        else:
            _, near = R.transform(src.view(-1, 3, 32, 40), aug.last_table, 16, 16)
            _check_stage_one_bar(out.cpu(), twin, float(near.float().mean()), f"ClipAugment({augs!r})")


def test_clip_augment_equals_clip_transform_on_the_shared_letters():
    g = torch.Generator().manual_seed(32)
    src = torch.randint(0, 256, (2, 2, 3, 32, 40), generator=g, dtype=torch.uint8).to(dev)
    a = A.ClipAugment(16, augs="cjg", views=2, generator=np.random.default_rng(33))(src)
    b = A.ClipTransform(16, augs="cjg", views=2, generator=np.random.default_rng(33))(src)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
