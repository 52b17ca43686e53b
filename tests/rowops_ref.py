"""float64 references, case lists and bar helpers for the row / element kernels of csrc/rowops.hip  --  TEST INFRASTRUCTURE ONLY.

Imported by tests/test_rowops_ref.py (CPU: pins what is defined here against torch's own double-precision ops) and by
tests/test_gpu_rowops.py (the kernels through the C ABI).  Nothing here touches the library; every function is plain torch, takes the
tensors the kernel sees (f32 or bf16, on any device), widens them to float64 and returns float64 on the same device.

Layouts are those of include/bvc.h: rows are dense [M][D] unless a row map (rin, rout, roff) is given, in which case logical row m
lives at physical row (m / rin) * rout + roff + m % rin of the tensor passed in (rin <= 0: dense).
"""
import math

import torch

F64 = torch.float64

# ---------------------------------------------------------------------------------------------- shapes the GPU tests run
LN_WIDTHS = (4, 132, 192, 260, 384, 512, 516, 1024, 1028, 1280, 1408, 1536)
LN_WIDTH_ROWS = (5, 16385)
LN_ROWS = (1, 3, 5, 7, 8, 9, 8203, 16383, 16384, 16385, 40001, 131089)
LN_ROW_WIDTHS = (128, 192)
COLSUM_BF16_N = (8, 520, 1032)
COLSUM_BF16_M = (1, 63, 64, 65, 16383, 16384, 16385)
COLSUM_F32_D = (4, 260, 384)
COLSUM_F32_M = (1, 255, 256, 257, 1000)
TOKEN_MEAN_B = (1, 3)
TOKEN_MEAN_N = (1, 15, 16, 17, 197, 1568)
TOKEN_MEAN_D = (4, 68, 192, 1280)
FLAT_SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025, (1 << 20) + 3)
INT_RANGE = 8            # the exact cases draw integers from [-8, 8]


def f32_value(v):
    """The float32 a C `float` argument carries, as a Python float (what the kernel is handed for eps, alpha, momentum)."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def sums_are_exact(rows, max_abs=INT_RANGE, start_abs=0):
    """True when every partial sum of `rows` integers of magnitude <= max_abs (onto a start value of magnitude <= start_abs) is an
    integer below 2^24, hence exact in float32 whatever the order of the additions; scaling by a power of two keeps it exact."""
    return rows * max_abs + start_abs < (1 << 24)


def ulp32(v):
    """Spacing of float32 at |v| (float64 tensor in, float64 out): the gap to the next float32 above float32(|v|)."""
    a = v.abs().to(torch.float32)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).to(F64)


# ---------------------------------------------------------------------------------------------- row map
def row_map(m, rin=0, rout=0, roff=0):
    """Physical row of logical row m (int or integer tensor)."""
    if rin <= 0:
        return m
    return (m // rin) * rout + roff + m % rin


def mapped_rows(M, rmap=None, device=None):
    """int64 tensor [M]: the physical row of each logical row."""
    m = torch.arange(M, dtype=torch.int64, device=device)
    return m if rmap is None else row_map(m, *rmap)


def physical_rows(M, rmap=None):
    """Rows a tensor must have to hold logical rows 0 .. M-1 under the map, whole clips of `rout` rows."""
    if rmap is None or rmap[0] <= 0:
        return M
    rin, rout, _ = rmap
    return ((M + rin - 1) // rin) * rout


def _rows(x, M, rmap):
    M = x.shape[0] if M is None else M
    return x[mapped_rows(M, rmap, x.device)].to(F64)


# ---------------------------------------------------------------------------------------------- LayerNorm
def layernorm_fwd(x, gamma, beta, eps, M=None, rmap=None):
    """(y [M][D], mean [M], rstd [M]): biased variance, eps inside the square root (torch.nn.LayerNorm).  gamma / beta None = no affine."""
    xr = _rows(x, M, rmap)
    mean = xr.mean(1)
    var = ((xr - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + f32_value(eps))
    y = (xr - mean[:, None]) * rstd[:, None]
    if gamma is not None:
        y = y * gamma.to(F64) + beta.to(F64)
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, eps, M=None, rmap=None, mean=None, rstd=None):
    """(dx [M][D] by logical row, dgamma [D], dbeta [D]) for upstream dy [M][D]; the statistics are recomputed in float64 unless given."""
    xr = _rows(x, M, rmap)
    if mean is None:
        _, mean, rstd = layernorm_fwd(x, None, None, eps, M, rmap)
    mean, rstd = mean.to(F64), rstd.to(F64)
    xh = (xr - mean[:, None]) * rstd[:, None]
    dyd = dy.to(F64)
    g = dyd * gamma.to(F64)
    dx = rstd[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dx, (dyd * xh).sum(0), dyd.sum(0)


# ---------------------------------------------------------------------------------------------- column sums, token mean
def colsum(X, M, N, alpha=1.0, rmap=None):
    """alpha * sum over the M (mapped) rows of X[:, :N]; X may be wider than N (its leading dimension)."""
    return f32_value(alpha) * _rows(X, M, rmap)[:, :N].sum(0)


def colsum_abs(X, M, N, alpha=1.0, rmap=None):
    """|alpha| * sum |X|: the magnitude the rounding errors of a column sum scale with (its condition, not its value)."""
    return abs(f32_value(alpha)) * _rows(X, M, rmap)[:, :N].abs().sum(0)


def token_mean(x):
    """x [B][N][D] -> [B][D]."""
    return x.to(F64).mean(1)


def token_mean_bwd(dmean, N):
    """dmean [B][D] -> dx [B][N][D] = dmean / N for every token."""
    return (dmean.to(F64) / N)[:, None, :].expand(-1, N, -1)


# ---------------------------------------------------------------------------------------------- row normalisation
def row_normalize(f, eps, dtype=F64):
    """(fn [n][p], inv [n]): fn = f / max(||f||, eps), inv = 1 / max(||f||, eps)  (the two norms of F.cosine_similarity).
    dtype = torch.float32: the same expression as torch evaluates it in single precision (a yardstick, not a reference)."""
    fd = f.to(dtype)
    inv = 1.0 / fd.norm(dim=1).clamp_min(f32_value(eps))
    return fd * inv[:, None], inv


def row_normalize_bwd(f, dfn, eps, dtype=F64):
    """df of fn = f / max(||f||, eps): inv * (dfn - fhat (fhat . dfn)) where the norm decides, dfn / eps where eps does."""
    fd, gd = f.to(dtype), dfn.to(dtype)
    e = f32_value(eps)
    nrm = fd.norm(dim=1)
    inv = 1.0 / nrm.clamp_min(e)
    fh = fd * inv[:, None]
    free = inv[:, None] * (gd - fh * (fh * gd).sum(1, keepdim=True))
    return torch.where((nrm > e)[:, None], free, gd * inv[:, None])


# ---------------------------------------------------------------------------------------------- smooth-L1, EMA
def smooth_l1(z, h):
    """mean over all elements of 0.5 d^2 (|d| < 1) or |d| - 0.5, d = z - h  (beta = 1)."""
    a = (z.to(F64) - h.to(F64)).abs()
    return torch.where(a < 1.0, 0.5 * a * a, a - 0.5).mean()


def smooth_l1_grad(z, h, gout):
    """gout / n * clamp(z - h, -1, 1), elementwise, in the shape of z."""
    d = z.to(F64) - h.to(F64)
    return float(gout) / d.numel() * d.clamp(-1.0, 1.0)


def ema(target, online, m):
    """m * target + (1 - m) * online with m the float32 the kernel is handed (1 - m is then exact in float32 for m in [0.5, 1] and 0)."""
    m = f32_value(m)
    return target.to(F64) * m + online.to(F64) * (1.0 - m)


# ---------------------------------------------------------------------------------------------- JEPA target selection, InfoNCE
def target_select(h, idx, nsets, B, Np, L, eps):
    """LayerNorm without affine over h [B*L][D], then out[(i*B + b)*Np + j] = LN(h[b*L + idx[(i*B + b)*Np + j]])."""
    y, _, _ = layernorm_fwd(h, None, None, eps)
    m = torch.arange(nsets * B * Np, device=h.device)
    b = (m // Np) % B
    return y[b * L + idx.to(torch.int64)]


def nce_finalize(partial, ntiles, inv_t, npos):
    """(loss, lse, -1/npos) from partial[2t] = sum exp(s - 1/T) over negatives and partial[2t + 1] = sum s over positives of tile t."""
    p = partial.to(F64)[:2 * ntiles].view(ntiles, 2)
    lse = f32_value(inv_t) + math.log(float(p[:, 0].sum()))
    return lse - float(p[:, 1].sum()) / npos, lse, -1.0 / npos


# ---------------------------------------------------------------------------------------------- pixel targets, tube patches
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _tubes(v, ts, ps):
    """[B][T][C][H][W] -> [B][L][C][ts][ps][ps] through Tensor.unfold: token = (t', y', x') row-major."""
    B, T, C, H, W = v.shape
    u = v.unfold(1, ts, ts).unfold(3, ps, ps).unfold(4, ps, ps)       # [B][T'][C][H'][W'][ts][ps][ps]
    return u.permute(0, 1, 3, 4, 2, 5, 6, 7).reshape(B, (T // ts) * (H // ps) * (W // ps), C, ts, ps, ps)


def gather_patches(clip, idx, ts, ps):
    """Rows of the patch-embedding product: A[b*n + j][(c, dt, dy, dx)] = the tube of token idx[b][j] of clip b in Conv3d weight
    order.  A pure gather: the dtype of `clip` is kept."""
    B, n = idx.shape
    t = _tubes(clip, ts, ps)
    rows = t[torch.arange(B, device=clip.device)[:, None], idx.to(torch.int64)]
    return rows.reshape(B * n, -1)


def pixel_labels(clip, idx, ts, ps, norm_pix, dtype=F64):
    """Targets of tokens idx [B][n]: with three channels the clip is un-normalised (v * std + mean, the ImageNet constants as the
    float32 values the kernel holds); per token and channel, over the ts*ps*ps values: (f - mean) / (sqrt(unbiased var) + 1e-6) when
    norm_pix; laid out [(dt, dy, dx)][c].  -> [B*n][ts*ps*ps*C].  dtype = torch.float32 gives the same formula as torch evaluates
    it in single precision (the yardstick of the GPU test's budget), not a reference."""
    B, T, C, H, W = clip.shape
    v = clip.to(dtype)
    if C == 3:
        sd = torch.tensor([f32_value(s) for s in IMAGENET_STD], dtype=dtype, device=clip.device)[None, None, :, None, None]
        mu = torch.tensor([f32_value(s) for s in IMAGENET_MEAN], dtype=dtype, device=clip.device)[None, None, :, None, None]
        v = v * sd + mu
    n = idx.shape[1]
    t = gather_patches(v, idx, ts, ps).view(B * n, C, ts * ps * ps)
    if norm_pix:
        t = (t - t.mean(2, keepdim=True)) / (t.var(2, unbiased=True, keepdim=True).sqrt() + f32_value(1e-6))
    return t.transpose(1, 2).reshape(B * n, -1)
