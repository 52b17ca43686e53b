"""float64 references, guarded buffers and per-element bars for the GEMM kernels (csrc/gemm.hip, gemm_persist.hip, gemm8.hip,
gemm_as.hip)  --  TEST INFRASTRUCTURE ONLY.

Imported by tests/test_gemm_ref.py (CPU: pins what is defined here against float64 autograd and the SimCLR oracle, proves the
exactness bound of the integer cases and plants faults for the checkers to catch) and by tests/test_gpu_gemm.py (the kernels through
the C ABI).  Nothing here touches the library; everything is plain torch on whatever device the tensors live on.

Operands are taken AS STORED (include/bvc.h): 2-D bf16 tensors [rows][ld] whose rows may be wider than what the product uses,
  NT: A [M][lda] (k contiguous), B [N][ldb] (k contiguous)      NN: A [M][lda], B [K][ldb] (n contiguous)
  TN: A [K][lda] (m contiguous), B [K][ldb] (n contiguous)
and every epilogue function takes `acc`, the float64 sum_k A(m,k) B(k,n) of `product`, and returns float64.
"""
import math

import torch

F64 = torch.float64
BF16 = torch.bfloat16
NT, NN, TN = 0, 1, 2
INT_RANGE = 8                          # the exact cases draw integers from [-8, 8]
ERF_ABS_ERROR = 1.5e-7                 # csrc/common.h: Abramowitz-Stegun 7.1.26
PAT32, PAT16 = 0x00A5A5A5, 0x5AA5      # guard patterns: a tiny normal float (any add to it shows), a bf16 no kernel here produces
TILES = {0: (128, 128), 1: (128, 64), 2: (64, 64), 6: (128, 128), 7: (128, 64), 9: (128, 128), 10: (256, 256), 11: (256, 128),
         12: (128, 384), 13: (256, 256), 15: (128, 128), 16: (128, 128), 17: (128, 128), 18: (128, 128)}

# ---------------------------------------------------------------------------------------------- shapes the GPU tests run
# (M, N, K) of the exact (integer) cases of tests/test_gpu_gemm.py; test_gemm_ref.py proves 64 K < 2^24 (plus the addends) for each
SWEEP_SHAPES = ((8, 8, 64), (136, 72, 192), (264, 200, 64), (264, 200, 128), (264, 200, 640))
TN_RAGGED_K = (1, 63, 65, 200)
PERSIST_SHAPES = ((4104, 4040, 128), (4104, 2056, 192))
GEMM8_SHAPES = ((200, 192, 256), (520, 384, 384), (4360, 1032, 128))
AS_SHAPES = tuple((M, N, 384) for M in (8, 136, 424) for N in (128, 384))
GATE_SHAPE = (333, 200, 192)
LARGE_NT = (1100, 72, 128)
LARGE_TN = (72, 136, 2010)
EXACT_SHAPES = (SWEEP_SHAPES + tuple((264, 200, K) for K in TN_RAGGED_K) + PERSIST_SHAPES + GEMM8_SHAPES + AS_SHAPES +
                (GATE_SHAPE, LARGE_NT, (1100, 128, 384), LARGE_TN, (136, 8200, 64)))
EXACT_ADDEND = 1024                    # integer bias / residual / positional / label / start values are drawn from [-1024, 1024]


def f32_value(v):
    """The float32 a C `float` argument carries, as a Python float."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def product_is_exact(K, alpha=1.0, addends=0):
    """True when every partial sum of K products of integers in [-8, 8] (64 K), scaled by a power of two and joined by `addends`
    integer addends of magnitude <= EXACT_ADDEND, is an integer multiple of the scale below 2^24 of it: exact in float32 in any
    order of the additions, atomics included."""
    m, e = math.frexp(abs(alpha))
    return m == 0.5 and INT_RANGE * INT_RANGE * K + addends * EXACT_ADDEND / abs(alpha) < (1 << 24)


def ulp32(v):
    """Spacing of float32 at |v| (float64 tensor in, float64 out)."""
    a = v.abs().to(torch.float32)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).to(F64)


def rne_bf16(ref):
    """round-to-nearest-even bf16 of a float64 tensor whose values are float32 numbers (the exact cases)."""
    f = ref.to(torch.float32)
    assert torch.equal(f.to(F64), ref), "rne_bf16: the reference is not a float32 number"
    return f.to(BF16)


# ---------------------------------------------------------------------------------------------- the product
def storage_shapes(layout, M, N, K):
    """(rows, used width) of A and of B as stored."""
    if layout == NT:
        return (M, K), (N, K)
    if layout == NN:
        return (M, K), (K, N)
    return (K, M), (K, N)


def operands(A, B, layout, M, N, K):
    """float64 A [M][K] and B [K][N] from the stored arrays (columns past the used width are dropped)."""
    a, b = A.to(F64), B.to(F64)
    if layout == NT:
        return a[:M, :K], b[:N, :K].t()
    if layout == NN:
        return a[:M, :K], b[:K, :N]
    return a[:K, :M].t(), b[:K, :N]


def product(A, B, layout, M, N, K):
    """(sum_k A(m,k) B(k,n), sum_k |A(m,k)| |B(k,n)|), float64 [M][N]."""
    a, b = operands(A, B, layout, M, N, K)
    return a @ b, a.abs() @ b.abs()


def product_f32(A, B, layout, M, N, K):
    """torch's own float32 product of the same operands (what the bars are measured with); TF32 off while it runs."""
    a, b = operands(A, B, layout, M, N, K)
    was = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        return a.to(torch.float32) @ b.to(torch.float32)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = was


def scaled(acc, alpha=1.0, alpha_dev=None, bias=None):
    """v = alpha * alpha_dev * acc + bias[n]: what every epilogue starts from (acc float64 or float32: the dtype is kept)."""
    a = f32_value(alpha) * (float(alpha_dev) if alpha_dev is not None else 1.0)
    v = acc * a
    return v + bias.to(acc.dtype)[None, :] if bias is not None else v


def rowsum(A, M, K, alpha=1.0, alpha_dev=None):
    """TN only: alpha * sum_k A(m,k) over the stored [K][lda] array, and the sum of magnitudes."""
    a = A.to(F64)[:K, :M] * (f32_value(alpha) * (float(alpha_dev) if alpha_dev is not None else 1.0))
    return a.sum(0), a.abs().sum(0)


# ---------------------------------------------------------------------------------------------- epilogues
def epi_resid(v, resid):
    return v + resid.to(v.dtype)


def epi_pos(v, pos, rowtok):
    return v + pos.to(v.dtype)[rowtok.long()]


def epi_relu(v):
    return v.clamp_min(0)


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def epi_gelu(v):
    """(C = gelu'(v), C2 = gelu(v)), exact erf."""
    return gelu_grad(v), gelu(v)


def gelu_erf_room(v):
    """absolute error the kernel's erf approximation (|error| <= 1.5e-7) puts into (gelu', gelu) at pre-activation v:
    gelu' = 0.5 (1 + erf) + ...  ->  0.5 x 1.5e-7;   gelu = 0.5 x (1 + erf)  ->  0.5 |x| x 1.5e-7."""
    return torch.full_like(v, 0.5 * ERF_ABS_ERROR), 0.5 * v.abs() * ERF_ABS_ERROR


def e2d_rows(M, rin, rout):
    """int64 [M]: output row of product row m, (m / rin) * rout + m % rin."""
    m = torch.arange(M, dtype=torch.int64)
    return (m // rin) * rout + m % rin


def e2d_untouched(M, rin, rout, P):
    """bool [P]: the rows of a P-row output that EPI_E2D must leave as they were."""
    keep = torch.ones(P, dtype=torch.bool)
    keep[e2d_rows(M, rin, rout)] = False
    return keep


def tile_sums(x, bm, bn):
    """[tiles_m * tiles_n] float64: the sum of x over each bm x bn tile, tile id = tm * tiles_n + tn (ragged tiles hold what there is)."""
    M, N = x.shape
    tm, tn = (M + bm - 1) // bm, (N + bn - 1) // bn
    pad = torch.zeros(tm * bm, tn * bn, dtype=x.dtype, device=x.device)
    pad[:M, :N] = x
    return pad.view(tm, bm, tn, bn).sum((1, 3)).reshape(-1)


def epi_loss(v, labels, bm, bn):
    """(difference d = v - labels, logits v, per-tile partials sum d^2)."""
    d = v - labels.to(v.dtype)
    return d, v, tile_sums(d * d, bm, bn)


def epi_dgelu(v, aux):
    return v * aux.to(v.dtype)


def drelu_gate(aux):
    """bool: aux > 0 decided on the bf16 bits - sign clear and any other bit set (so +0.0 and -0.0 close the gate, the smallest
    positive subnormal opens it)."""
    bits = aux.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return ((bits & 0x8000) == 0) & ((bits & 0x7FFF) != 0)


def epi_drelu(v, aux):
    return v * drelu_gate(aux).to(v.dtype)


def nce_masks(M, N, device=None):
    """(positives |n - m| == 1, negatives |n - m| > 1) of an M x N block of the similarity matrix."""
    d = (torch.arange(N, device=device)[None, :] - torch.arange(M, device=device)[:, None]).abs()
    return d == 1, d > 1


def epi_nce(v, inv_t, bm, bn):
    """[2 tiles]: partial[2 t] = sum over the negatives of tile t of exp(v - 1/T), partial[2 t + 1] = sum over its positives of v
    (the comment of EPI_NCE in csrc/gemm_kernel_body.inc; v = cos / T)."""
    pos, neg = nce_masks(*v.shape, device=v.device)
    a = tile_sums(torch.exp(v - inv_t) * neg, bm, bn)
    b = tile_sums(v * pos, bm, bn)
    return torch.stack([a, b], 1).reshape(-1)


def nce_finalize(partial, inv_t, npos):
    """(loss, lse, -1 / npos) from the partials, as bvc_op_nce_finalize folds them."""
    p = partial.view(-1, 2).sum(0)
    lse = inv_t + torch.log(p[0])
    return lse - p[1] / npos, lse, -1.0 / npos


def epi_nce_bwd(v, lse, pc):
    """d loss / d v: exp(v - lse) on the negatives, pc on the positives, 0 on the diagonal."""
    pos, neg = nce_masks(*v.shape, device=v.device)
    return torch.exp(v - lse) * neg + pc * pos.to(v.dtype)


def seg_rows(M, seg_rows_, seg_stride, seg_off):
    """int64 [M]: row of the longer array that compact row m stands for (seg_rows_ == 0: dense)."""
    m = torch.arange(M, dtype=torch.int64)
    if seg_rows_ == 0:
        return m
    return (m // seg_rows_) * seg_stride + seg_off + m % seg_rows_


def epi_resid_ln(v, resid, gamma, beta, eps, seg=None):
    """(C = v + resid, C2 = LayerNorm(C), mean, rstd); `resid` is addressed through the segment map."""
    rows = seg_rows(v.shape[0], *(seg or (0, 0, 0))).to(v.device)
    c = v + resid.to(v.dtype)[rows]
    mean = c.mean(1)
    rstd = 1 / torch.sqrt(c.var(1, unbiased=False) + f32_value(eps))
    return c, (c - mean[:, None]) * rstd[:, None] * gamma.to(v.dtype) + beta.to(v.dtype), mean, rstd


def epi_dln(g, x, gamma, mean, rstd):
    """LayerNorm backward on complete rows, g = d / d(LayerNorm output): (dx, dgamma, dbeta) with the statistics as handed in."""
    x, gamma, mean, rstd = x.to(g.dtype), gamma.to(g.dtype), mean.to(g.dtype), rstd.to(g.dtype)
    xh = (x - mean[:, None]) * rstd[:, None]
    gg = g * gamma
    dx = rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    return dx, (g * xh).sum(0), g.sum(0)


def epi_resid_gate(v, resid, keep, p, path_scale, rows_per_sample):
    """C = resid + gate .* v with gate = path_scale[m / rows_per_sample] * keep / (1 - p) (keep: the 0 / 1 bytes of bvc_dropout_mask_host)."""
    M = v.shape[0]
    g = torch.ones(M, 1, dtype=v.dtype, device=v.device)
    if path_scale is not None:
        g = path_scale.to(v.dtype)[torch.arange(M, device=v.device) // rows_per_sample][:, None]
    if keep is not None:
        g = g * keep.to(v.dtype) * f32_value(1.0 / (1.0 - p))
    return resid.to(v.dtype) + g * v


# ---------------------------------------------------------------------------------------------- guarded, strided memory
def strided(data, ld, fill=float("nan")):
    """The rows of a 2-D tensor laid out ld apart in a buffer that covers exactly first to last element used; the gaps hold `fill`.
    Returns (view [rows][width] of the buffer, bytes)."""
    rows, w = data.shape
    assert ld >= w
    buf = torch.full(((rows - 1) * ld + w,), fill, dtype=data.dtype, device=data.device)
    view = buf.as_strided((rows, w), (ld, 1))
    view.copy_(data)
    return view, buf.numel() * buf.element_size()


class Guarded:
    """[guard | rows x ld payload | guard]: `t` is the [rows][N] view the kernel may write; the columns [N, ld) of every row and
    both guards hold a fixed bit pattern and must hold it after the call.  fill: "nan", a number or a [rows][N] tensor."""

    def __init__(self, rows, N, ld=None, dtype=torch.float32, fill="nan", device="cuda"):
        ld = N if ld is None else ld
        wide = torch.empty(0, dtype=dtype).element_size() == 4
        self.pat = PAT32 if wide else PAT16
        self.g = g = max(64, (ld + 63) // 64 * 64)
        self.rows, self.N, self.ld = rows, N, ld
        self.buf = torch.empty(2 * g + rows * ld, dtype=dtype, device=device)
        self.ibuf = self.buf.view(torch.int32 if wide else torch.int16)
        self.ibuf.fill_(self.pat)
        self.full = self.buf[g:g + rows * ld].view(rows, ld)
        self.t = self.full[:, :N]
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill.reshape(rows, N))
        else:
            self.t.fill_(float("nan") if fill == "nan" else fill)
        assert self.t.data_ptr() % 16 == 0

    def bits(self):
        """int copy of the [rows][N] payload"""
        return self.ibuf[self.g:self.g + self.rows * self.ld].view(self.rows, self.ld)[:, :self.N].clone()

    def check(self, what):
        front = self.ibuf[:self.g] != self.pat
        back = self.ibuf[self.g + self.rows * self.ld:] != self.pat
        assert not bool(front.any()), f"{what}: {int(front.sum())} elements written BEFORE the buffer"
        assert not bool(back.any()), f"{what}: {int(back.sum())} elements written PAST the end (first at +{int(back.nonzero()[0])})"
        if self.ld > self.N:
            gap = self.ibuf[self.g:self.g + self.rows * self.ld].view(self.rows, self.ld)[:, self.N:] != self.pat
            assert not bool(gap.any()), (f"{what}: {int(gap.sum())} elements written into the row gap [N, ldc) "
                                         f"(first at row {int(gap.nonzero()[0][0])}, column {self.N + int(gap.nonzero()[0][1])})")


def same_bits(a, b):
    w = torch.int32 if a.element_size() == 4 else torch.int16
    return torch.equal(a.contiguous().view(w), b.contiguous().view(w))


def rows_unchanged(before_bits, after_bits, rows_mask, what):
    """the rows of an output that the call must not touch (EPI_E2D's rin .. rout band) are bit-identical"""
    m = rows_mask.to(before_bits.device)
    bad = (before_bits[m] != after_bits[m]).any(1)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} untouched rows were written (first: row {int(m.nonzero()[int(bad.nonzero()[0])])})"


# ---------------------------------------------------------------------------------------------- bars, per element
def f32_room(ref, t32, scale):
    """(room [same shape], worst torch-f32 error relative to the element's scale): 4 x that error x scale, at least 4 ulp of the scale."""
    scale = scale.to(F64)
    nz = scale > 0
    et = (t32.to(F64) - ref).abs()
    wt = float((et[nz] / scale[nz]).max()) if bool(nz.any()) else 0.0
    return torch.maximum(4 * wt * scale, 4 * ulp32(scale)), wt


def _worst(err, scale):
    nz = scale > 0
    return float((err[nz] / scale[nz]).max()) if bool(nz.any()) else float(err.max())


def _first(bad):
    return tuple(bad.nonzero()[0].tolist())


def check_f32(log, key, got, ref, t32, scale, extra=None):
    """f32 output against float64 `ref`, per element: |got - ref| <= max(4 x worst torch-f32 error x scale, 4 ulp of the scale)
    (+ `extra`, an absolute allowance with a stated source)."""
    ref, scale = ref.to(F64), scale.to(F64)
    got = got.to(F64).reshape(ref.shape)
    room, wt = f32_room(ref, t32.reshape(ref.shape), scale)
    if extra is not None:
        room = room + extra
    err = (got - ref).abs()
    if log is not None:
        log.add(key, _worst(err, scale), wt)
    bad = ~(err <= room)
    if bool(bad.any()):
        i = _first(bad)
        raise AssertionError(f"{key}: {int(bad.sum())} of {bad.numel()} elements over the bar; first {i}: got {float(got[i])!r}, ref "
                             f"{float(ref[i])!r}, bar {float(room[i]):.3e} (torch-f32 worst {wt:.3e} x scale {float(scale[i]):.3e})")


def check_bf16(log, key, got, ref, t32, scale, extra=None):
    """bf16 output per element: |got - ref| <= 2^-8 |ref| + the f32 room of that element (+ `extra`)."""
    ref, scale = ref.to(F64), scale.to(F64)
    got = got.to(F64).reshape(ref.shape)
    room, wt = f32_room(ref, t32.reshape(ref.shape), scale)
    if extra is not None:
        room = room + extra
    err = (got - ref).abs()
    if log is not None:
        log.add(key, _worst(err, scale), wt)
    bad = ~(err <= 2.0 ** -8 * ref.abs() + room)
    if bool(bad.any()):
        i = _first(bad)
        raise AssertionError(f"{key}: {int(bad.sum())} of {bad.numel()} elements over the bf16 bar; first {i}: got {float(got[i])!r}, "
                             f"ref {float(ref[i])!r}")


def check_exact(key, got, ref, bf16=False):
    """the integer cases: an f32 output equals the reference bit for bit, a bf16 output its round-to-nearest-even."""
    if bf16:
        want = rne_bf16(ref.to(F64))
        bad = got.reshape(want.shape).view(torch.int16) != want.view(torch.int16)
        # (+0.0 and -0.0 are one value: an integer sum that cancels may come out with either sign)
        bad &= ~((got.reshape(want.shape) == 0) & (want == 0))
    else:
        want = ref.to(F64)
        bad = got.to(F64).reshape(want.shape) != want
    if bool(bad.any()):
        i = _first(bad)
        raise AssertionError(f"{key}: {int(bad.sum())} of {bad.numel()} elements of an exact case differ; first {i}: got "
                             f"{float(got.reshape(want.shape)[i])!r}, want {float(want[i])!r}")


class CaseLog:
    """Worst kernel and torch-f32 error per output of one case; one line of the parity report."""

    def __init__(self, name):
        self.name, self.items = name, {}

    def add(self, key, k, t):
        a, b = self.items.get(key, (0.0, 0.0))
        self.items[key] = (k if not k <= a else a, t if not t <= b else b)      # (a NaN sticks)

    def note(self, key, text):
        self.items[key] = text

    def line(self):
        parts = [f"{k} {v}" if isinstance(v, str) else f"{k} {v[0]:.2e}/{v[1]:.2e}" for k, v in self.items.items()]
        return f"gemm {self.name}: " + "  ".join(parts) + "   (kernel/torch-f32, relative to the element scale)"
