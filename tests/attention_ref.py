"""Reference, rounding model, per-row metric, inputs and guarded memory for the attention tests  --  TEST INFRASTRUCTURE ONLY.

Imported by tests/test_attention_ref.py (CPU: pins what is defined here) and tests/test_gpu_attention_edges.py (the kernels of
csrc/attention.hip through the C ABI).  Nothing here touches the library.

Layouts are those of the kernels and of `_ref_attention` in tests/test_gpu_ops.py: qkv bf16 [B*N][3*D] with q | k | v column blocks
(head h at column h * HD of its block, D = H * HD), ctx / dctx [B*N][D], lse f32 [B*H][N] in log2 units.  `heads()` turns a
[B*N][D] array into the [B][H][N][HD] view `row_err` takes.
"""
import math

import torch

from oracle import videomae_oracle_bf16 as vb

KINDS = ("gauss", "sharp", "shift", "headscale")


def heads(t, B, N, H, HD):
    """[B*N][H*HD] -> [B][H][N][HD] (a view)."""
    return t.reshape(B, N, H, HD).permute(0, 2, 1, 3)


def _split(qkv, B, N, H, HD, dtype):
    x = qkv.to(dtype).view(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def _formula(qkv, dctx, B, N, H, HD, scale, dtype):
    """softmax(q k^T scale) v and its gradients by autograd, every operation in `dtype`, from the bf16-rounded operands."""
    D = H * HD
    scale = HD ** -0.5 if scale is None else float(scale)
    x = qkv.to(torch.bfloat16).to(dtype).detach().clone().requires_grad_(True)
    q, k, v = _split(x, B, N, H, HD, dtype)
    s = (q @ k.transpose(-1, -2)) * scale
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * N, D)
    lse2 = (torch.logsumexp(s, dim=-1) * math.log2(math.e)).reshape(B * H, N)
    (o * dctx.to(torch.bfloat16).to(dtype)).sum().backward()
    g = x.grad
    return o.detach(), lse2.detach(), g[:, :D], g[:, D:2 * D], g[:, 2 * D:]


def reference(qkv, dctx, B, N, H, HD, scale=None):
    """(ctx, lse, dq, dk, dv) in float64 on the device of `qkv`: ctx / dq / dk / dv [B*N][D], lse [B*H][N] in log2 units."""
    return _formula(qkv, dctx, B, N, H, HD, scale, torch.float64)


def model(qkv, dctx, B, N, H, HD, scale=None):
    """The same five quantities (float32) from the project's rounding model of its own kernels, `oracle.videomae_oracle_bf16._Attention`
    under `vb.BUILD`: bf16 P, bf16 dS, bf16 outputs, f32 accumulation.  Its distance from `reference` is the error that correct
    arithmetic at the kernels' precision produces, which is what the per-row bars of the GPU tests are multiples of.  (The model has
    no separate lse rounding: lse is the f32 logsumexp.)"""
    if scale is not None and float(scale) != HD ** -0.5:
        raise ValueError("model(): the oracle's attention has the 1/sqrt(head_dim) scale built in")
    D = H * HD
    x = qkv.to(torch.bfloat16).float().detach().clone().requires_grad_(True)
    q, k, v = _split(x, B, N, H, HD, torch.float32)
    o = vb._Attention.apply(q, k, v, vb.BUILD).transpose(1, 2).reshape(B * N, D)
    (o * dctx.to(torch.bfloat16).float()).sum().backward()
    with torch.no_grad():
        s = (q @ k.transpose(-1, -2)) * HD ** -0.5
        lse2 = (torch.logsumexp(s, dim=-1) * math.log2(math.e)).reshape(B * H, N)
    g = x.grad
    return o.detach(), lse2, g[:, :D], g[:, D:2 * D], g[:, 2 * D:]


def row_err(got, ref):
    """Worst row of `got` against `ref`, both [B][H][N][HD]:  max over rows of |got - ref| / max(|ref|, rms over the head's rows of
    |ref|)  (Euclidean norms over HD).  The floor is the head's typical row norm, so a row whose true value is tiny is measured
    against its neighbours' size instead of dominating; no row is left out.  Where a whole head of `ref` is exactly zero the
    quotient of a non-zero error is inf (0 for an exact zero).  Returns (worst, (clip, head, row))."""
    g, r = got.double(), ref.double()
    assert g.shape == r.shape and g.dim() == 4, (g.shape, r.shape)
    num = (g - r).norm(dim=-1)                                   # [B][H][N]
    rn = r.norm(dim=-1)
    floor = rn.pow(2).mean(dim=-1, keepdim=True).sqrt()          # [B][H][1]
    den = torch.maximum(rn, floor)
    e = torch.where(num == 0, torch.zeros_like(num), num / den)  # 0 / 0 -> 0, x / 0 -> inf, NaN stays NaN
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    i = int(e.argmax())
    n_ = e.shape[2]
    return float(e.flatten()[i]), (i // (e.shape[1] * n_), (i // n_) % e.shape[1], i % n_)


def whole_err(got, ref):
    """|got - ref| / |ref| over the whole tensor (the metric of tests/gpu_util.rel_err)."""
    g, r = got.double(), ref.double()
    return float((g - r).norm() / (r.norm() + 1e-30))


def inputs(kind, B, N, H, HD, seed):
    """(qkv [B*N][3*D], dctx [B*N][D]), bf16, on the CPU, from a seeded generator.
      gauss      unit normal
      sharp      q and k x 4: a few keys carry each row's softmax
      shift      k + 3.0: a common offset on every key, which cancels in dQ = dS K only as far as the rounded dS sums to zero
      headscale  v of head h x 2^(h % 3 - 1): taking another head's values changes magnitudes instead of hiding in noise"""
    assert kind in KINDS, kind
    D = H * HD
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * N, 3, H, HD, generator=g)
    dctx = torch.randn(B * N, D, generator=g)
    if kind == "sharp":
        x[:, 0:2] *= 4.0
    elif kind == "shift":
        x[:, 1] += 3.0
    elif kind == "headscale":
        x[:, 2] *= torch.tensor([2.0 ** (h % 3 - 1) for h in range(H)]).view(1, H, 1)
    return x.reshape(B * N, 3 * D).to(torch.bfloat16), dctx.to(torch.bfloat16)


class Arena:
    """ONE allocation out of which a test carves its operands and outputs, each at a 256-byte-aligned address with a guard band of
    its own before it and another after it.  The bands hold a fixed byte pattern that reads as NaN both as bf16 and as f32 (at any
    2-byte phase), so a kernel that READS past an operand poisons its result, and a kernel that WRITES past an output changes a band,
    which `check()` reports by tensor and side.  Every band lies inside the arena's own allocation - the allocation ends with the
    last tensor's `after` band, never with a tensor - so a stray access within GUARD bytes of a tensor (64 KiB, or `guard` bytes
    where a test asks for more) faults nothing.

        A = Arena("cuda", qkv=((B * N, 3 * D), torch.bfloat16), lse=((B * H, N), torch.float32))
        A["qkv"].copy_(...); ...; A.check()
    """
    GUARD = 64 * 1024
    ALIGN = 256
    PATTERN = (0xA5, 0xFF, 0xC3, 0x7F)      # bf16 0xFFA5 / 0x7FC3, f32 0x7FC3FFA5 / 0xFFA57FC3: all NaN

    def __init__(self, device, guard=0, **spec):
        self.GUARD = max(self.GUARD, (int(guard) + self.ALIGN - 1) // self.ALIGN * self.ALIGN)      # wider bands on request
        A, G = self.ALIGN, self.GUARD
        sizes = {}
        for name, (shape, dtype) in spec.items():
            n = 1
            for d in shape:
                n *= int(d)
            sizes[name] = n * torch.empty((), dtype=dtype).element_size()
        total = A + sum(2 * G + (nb + A - 1) // A * A for nb in sizes.values())
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self._pat = torch.tensor(self.PATTERN, dtype=torch.uint8, device=device)
        self.buf.copy_(self._expected(0, total))
        self.tensors, self.spans = {}, {}
        cur = (-base) % A                     # first byte at an aligned address
        for name, (shape, dtype) in spec.items():
            off = cur + G                      # G is a multiple of ALIGN
            nb = sizes[name]
            self.tensors[name] = self.buf[off:off + nb].view(dtype).view(*shape)
            self.spans[name] = (off, off + nb)
            assert self.tensors[name].data_ptr() % A == 0
            cur = off + (nb + A - 1) // A * A + G
        assert cur <= total
        self.total = total

    def _expected(self, a, b):
        return self._pat[torch.arange(a, b, device=self.buf.device) % 4]

    def __getitem__(self, name):
        return self.tensors[name]

    def bands(self):
        """(tensor name, side, first byte, end byte) of every guard band, in address order."""
        for name, (a, b) in self.spans.items():
            yield name, "before", a - self.GUARD, a
            yield name, "after", b, b + self.GUARD

    def check(self):
        for name, side, a, b in self.bands():
            assert 0 <= a and b <= self.total
            got, want = self.buf[a:b], self._expected(a, b)
            if not torch.equal(got, want):
                bad = torch.nonzero(got != want).flatten()
                where = (self.GUARD - int(bad[-1])) if side == "before" else int(bad[0]) + 1
                raise AssertionError(f"guard band {side} {name!r} was written: {bad.numel()} byte(s) changed, the nearest "
                                     f"{where} byte(s) {'before its first' if side == 'before' else 'past its last'} byte")
