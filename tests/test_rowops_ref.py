"""Pins tests/rowops_ref.py on the CPU, so that the bars of tests/test_gpu_rowops.py are bars against the operations themselves: every
float64 reference is compared with torch's own double-precision op (F.layer_norm with autograd, F.smooth_l1_loss, F.normalize-style
cosine normalisation, mean(1), Tensor.unfold), the pixel targets with the oracle at the TINY geometry, and the condition under which
the integer cases are exact in float32 is checked for every shape the GPU tests use."""
import dataclasses
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import videomae_oracle as vo
from tests import rowops_ref as R

F64 = torch.float64


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_row_map():
    assert R.row_map(0, 12, 20, 8) == 8 and R.row_map(11, 12, 20, 8) == 19 and R.row_map(12, 12, 20, 8) == 28
    assert R.row_map(35, 12, 20, 8) == 59 and R.row_map(7, 0, 0, 0) == 7
    assert R.mapped_rows(36, (12, 20, 8)).tolist() == [c * 20 + 8 + j for c in range(3) for j in range(12)]
    assert R.physical_rows(36, (12, 20, 8)) == 60 and R.physical_rows(37, (12, 20, 8)) == 80 and R.physical_rows(9, None) == 9
    # the map used for the column sums leaves room after the last mapped row of a clip
    assert int(R.mapped_rows(1000, (5, 9, 3)).max()) < R.physical_rows(1000, (5, 9, 3))


@pytest.mark.parametrize("M,D,rmap", [(7, 4, None), (5, 132, None), (36, 192, (12, 20, 8))])
def test_layernorm_is_torch_layer_norm(M, D, rmap):
    g = torch.Generator().manual_seed(1)
    P = R.physical_rows(M, rmap)
    x = torch.randn(P, D, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(M, D, generator=g).to(torch.bfloat16)
    eps = 1e-6
    y, mean, rstd = R.layernorm_fwd(x, gamma, beta, eps, M, rmap)
    dx, dg, db = R.layernorm_bwd(dy, x, gamma, eps, M, rmap)
    assert all(t.dtype == F64 for t in (y, mean, rstd, dx, dg, db))
    rows = R.mapped_rows(M, rmap)
    xr = x[rows].double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = F.layer_norm(xr, (D,), gr, br, R.f32_value(eps))
    ref.backward(dy.double())
    assert _close(y, ref.detach()) and _close(mean, xr.detach().mean(1))
    assert _close(rstd, 1 / torch.sqrt(xr.detach().var(1, unbiased=False) + R.f32_value(eps)))
    assert _close(dx, xr.grad, 1e-11) and _close(dg, gr.grad, 1e-11) and _close(db, br.grad, 1e-11)
    # statistics handed in are used as given
    dx2, _, _ = R.layernorm_bwd(dy, x, gamma, eps, M, rmap, mean=mean.float(), rstd=rstd.float())
    assert not torch.equal(dx2, dx) and _close(dx2, dx, 1e-5)
    # eps sits inside the square root, and the variance is the biased one
    c = torch.full((2, D), 3.0)
    _, m0, r0 = R.layernorm_fwd(c, None, None, 1e-6)
    assert torch.equal(m0, torch.full((2,), 3.0, dtype=F64)) and _close(r0, torch.full((2,), 1 / math.sqrt(R.f32_value(1e-6)), dtype=F64))


def test_colsum_and_token_mean():
    g = torch.Generator().manual_seed(2)
    X = torch.randn(27, 24, generator=g).to(torch.bfloat16)
    assert _close(R.colsum(X, 27, 16, 0.25), 0.25 * X.double()[:, :16].sum(0))
    rows = R.mapped_rows(13, (5, 9, 3))
    assert _close(R.colsum(X.float(), 13, 24, 1.0, (5, 9, 3)), X.double()[rows].sum(0))
    assert _close(R.colsum_abs(X, 27, 16, 0.25), 0.25 * X.double()[:, :16].abs().sum(0))
    x = torch.randn(3, 17, 68, generator=g)
    xd = x.double().requires_grad_(True)
    dm = torch.randn(3, 68, generator=g)
    xd.mean(1).backward(dm.double())
    assert _close(R.token_mean(x), xd.detach().mean(1)) and _close(R.token_mean_bwd(dm, 17), xd.grad)


@pytest.mark.parametrize("eps", [1e-8, 1e-3])
def test_row_normalize_is_cosine_normalisation(eps):
    g = torch.Generator().manual_seed(3)
    f = torch.randn(6, 128, generator=g)
    f[1] = 0
    f[4] = f[4] / f[4].norm() * (0.25 * eps)           # a row the clamp decides
    dfn = torch.randn(6, 128, generator=g)
    fn, inv = R.row_normalize(f, eps)
    e = R.f32_value(eps)
    fd = f.double().requires_grad_(True)
    ref = fd / fd.norm(dim=1, keepdim=True).clamp_min(e)
    safe = [0, 2, 3, 4, 5]                              # (torch's norm has no gradient at the zero row itself)
    assert _close(fn, ref.detach()) and _close(fn, F.normalize(f.double(), dim=1, eps=e))
    assert torch.equal(fn[1], torch.zeros(128, dtype=F64)) and float(inv[1]) == 1 / e and float(inv[4]) == 1 / e
    (ref[safe] * dfn.double()[safe]).sum().backward()
    df = R.row_normalize_bwd(f, dfn, eps)
    assert _close(df[safe], fd.grad[safe], 1e-11)
    assert _close(df[1], dfn.double()[1] / e) and bool(torch.isfinite(df).all())
    # two normalised rows give F.cosine_similarity
    cos = (fn[0] * fn[2]).sum()
    assert abs(float(cos) - float(F.cosine_similarity(f[0].double(), f[2].double(), dim=0, eps=e))) < 1e-12


def test_smooth_l1_and_ema():
    g = torch.Generator().manual_seed(4)
    z, h = torch.randn(1025, generator=g) * 2, torch.randn(1025, generator=g)
    one = torch.tensor(1.0)
    for i, d in enumerate((0.0, 1.0, -1.0, float(torch.nextafter(one, one * 2)), float(torch.nextafter(one, one * 0)),
                           -float(torch.nextafter(one, one * 2)), -float(torch.nextafter(one, one * 0)))):
        z[i], h[i] = d, 0.0
    zd = z.double().requires_grad_(True)
    loss = F.smooth_l1_loss(zd, h.double(), beta=1.0)
    (loss * 1024.0).backward()
    assert abs(float(R.smooth_l1(z, h)) - float(loss.detach())) < 1e-13
    assert _close(R.smooth_l1_grad(z, h, 1024.0), zd.grad)
    gr = R.smooth_l1_grad(z, h, 1024.0)
    assert float(gr[1]) == 1024.0 / 1025 and float(gr[2]) == -1024.0 / 1025 and float(gr[3]) == 1024.0 / 1025 and float(gr[0]) == 0.0
    assert 0 < float(gr[4]) < 1024.0 / 1025
    k, q = torch.randn(9, generator=g), torch.randn(9, generator=g)
    assert torch.equal(R.ema(k, q, 1.0), k.double()) and torch.equal(R.ema(k, q, 0.0), q.double())
    m = R.f32_value(0.996)
    assert _close(R.ema(k, q, 0.996), torch.lerp(q.double(), k.double(), m))


def test_target_select_and_nce():
    g = torch.Generator().manual_seed(5)
    nsets, B, Np, L, D = 4, 3, 5, 49, 12
    h = torch.randn(B * L, D, generator=g)
    idx = torch.randint(0, L, (nsets * B * Np,), generator=g).to(torch.int32)
    out = R.target_select(h, idx, nsets, B, Np, L, 1e-6)
    ln = F.layer_norm(h.double(), (D,), eps=R.f32_value(1e-6)).view(B, L, D)
    for i in range(nsets):
        for b in range(B):
            for j in range(Np):
                m = (i * B + b) * Np + j
                assert _close(out[m], ln[b, int(idx[m])])
    p = torch.rand(2 * 257, generator=g) + 0.1
    loss, lse, s1 = R.nce_finalize(p, 257, 10.0, 514)
    neg, pos = p.double()[0::2], p.double()[1::2]
    assert abs(lse - (10.0 + float(torch.log(neg.sum())))) < 1e-12 and abs(loss - (lse - float(pos.sum()) / 514)) < 1e-12
    assert s1 == -1.0 / 514


def test_patches_are_an_unfold_in_conv3d_weight_order():
    g = torch.Generator().manual_seed(6)
    B, T, C, H, W, ts, ps = 2, 4, 3, 16, 24, 2, 8
    clip = torch.randn(B, T, C, H, W, generator=g)
    L = (T // ts) * (H // ps) * (W // ps)
    idx = torch.stack([torch.randperm(L, generator=g)[:5] for _ in range(B)]).to(torch.int32)
    A = R.gather_patches(clip, idx, ts, ps)
    assert A.dtype == clip.dtype and A.shape == (B * 5, C * ts * ps * ps)
    # a Conv3d with one-hot filters over (c, dt, dy, dx) reads the same element
    K = C * ts * ps * ps
    w = torch.eye(K).view(K, C, ts, ps, ps)
    conv = F.conv3d(clip.permute(0, 2, 1, 3, 4), w, stride=(ts, ps, ps)).flatten(2).transpose(1, 2)      # [B][L][K]
    for b in range(B):
        for j in range(5):
            assert torch.equal(A[b * 5 + j], conv[b, int(idx[b, j])])
    # element by element against the index formula of the kernel header
    tok = int(idx[1, 3])
    wp, hp = W // ps, H // ps
    tp, yp, xp = tok // (hp * wp), (tok // wp) % hp, tok % wp
    for k in (0, 7, ps * ps + 3, K - 1):
        dx, dy, dt, c = k % ps, (k // ps) % ps, (k // (ps * ps)) % ts, k // (ps * ps * ts)
        assert float(A[5 + 3, k]) == float(clip[1, tp * ts + dt, c, yp * ps + dy, xp * ps + dx])


@pytest.mark.parametrize("norm_pix", [0, 1])
def test_pixel_labels_match_the_oracle(norm_pix):
    cfg = dataclasses.replace(vo.TINY, norm_pix_loss=bool(norm_pix))
    B = 3
    pixels, mask = vo.synthetic_batch(cfg, B, seed=3, mask_ratio=0.75)
    nmask = int(mask[0].sum())
    idx = torch.stack([torch.nonzero(mask[b]).flatten() for b in range(B)]).to(torch.int32)
    ref = vo.pixel_labels(cfg, pixels, mask).reshape(B * nmask, -1)
    got = R.pixel_labels(pixels, idx, cfg.tubelet_size, cfg.patch_size, norm_pix)
    assert got.dtype == F64 and got.shape == ref.shape
    assert float((got - ref.double()).abs().max()) < 2e-5          # the oracle computes in float32
    # one channel: no un-normalisation
    one = pixels[:, :, :1].contiguous()
    raw = R.pixel_labels(one, idx, cfg.tubelet_size, cfg.patch_size, 0)
    assert torch.equal(raw, R.gather_patches(one, idx, cfg.tubelet_size, cfg.patch_size).double())


def test_pixel_labels_statistics():
    g = torch.Generator().manual_seed(7)
    clip = torch.randn(1, 2, 3, 16, 32, generator=g)
    idx = torch.tensor([[1, 0]], dtype=torch.int32)
    out = R.pixel_labels(clip, idx, 2, 16, 1).view(2, 512, 3)
    un = clip.double() * torch.tensor([R.f32_value(s) for s in R.IMAGENET_STD], dtype=F64)[None, None, :, None, None] \
        + torch.tensor([R.f32_value(s) for s in R.IMAGENET_MEAN], dtype=F64)[None, None, :, None, None]
    for j, tok in enumerate((1, 0)):
        for c in range(3):
            v = un[0, :, c, :, tok * 16:(tok + 1) * 16].reshape(-1)
            ref = (v - v.mean()) / (v.std(unbiased=True) + R.f32_value(1e-6))
            assert _close(out[j, :, c], ref)


def test_integer_cases_are_exact_in_float32():
    """rows * 8 < 2^24 for every shape of the bit-exact GPU cases, and the helper says no where it should."""
    assert R.sums_are_exact((1 << 21) - 1) and not R.sums_are_exact(1 << 21)
    for M in R.LN_ROWS + R.LN_WIDTH_ROWS:
        assert R.sums_are_exact(M, start_abs=1024)                     # dbeta onto integers of magnitude <= 1024
    for M in R.COLSUM_BF16_M:
        assert R.sums_are_exact(M, R.INT_RANGE * 4, start_abs=4096)    # quarter-integers after alpha = 0.25 (x 2): scaled by 4
    for M in R.COLSUM_F32_M:
        assert R.sums_are_exact(M, start_abs=1024)
    for N in R.TOKEN_MEAN_N:
        assert R.sums_are_exact(N)
    # and float32 really is exact there, in any order: the worst case is the largest magnitude the condition admits
    n = (1 << 21) - 1
    v = torch.full((n,), 8.0)
    assert float(v.sum()) == 8.0 * n and float(v.flip(0).cumsum(0)[-1]) == 8.0 * n
    # ulp32: spacing of float32
    u = R.ulp32(torch.tensor([1.0, 1.5, 2.0, 1024.0, 0.75], dtype=F64))
    assert u.tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -13, 2.0 ** -24]
