"""bvc_op_attention_probs (csrc/attention_probs.hip, through the C ABI): P = exp2(q.k scale log2 e - lse) as a dense f32
[B][H][N][N] array from a qkv and the lse bvc_op_attention_fwd wrote for it.

Reference and model: tests/introspection_ref.py (probs_reference: float64 softmax of the bf16 operands; probs_model: float32
exp2(s2 - lse2) in torch), metric: tests/attention_ref.row_err on [B][H][N][N].  Operands and outputs are carved from an
attention_ref.Arena (NaN-reading guard bands on both sides of each, outputs pre-filled with NaN); every case ends with
Arena.check() and a no-NaN check of probs, so a row or column past N that was stored, or an element that was not, fails.

Bars, per case: worst row <= ROW_BAR x the model's worst row of the same input; no row above 1e-4 (the model alone stays below
1e-5 on every input here; a wrong key, head, clip or lse row gives 0.1 ... 1); |rowsum - 1| <= 1e-4 for every row.
ROW_BAR = 2.5, the project's ratio (tests/test_gpu_attention_edges.py).  The kernel differs from the model by v_exp_f32 and by
the round-off of the forward kernel's lse (a running maximum and a row sum kept per 32-key tile); every figure is printed and
logged (gpu_util.log_parity) before anything is asserted.  Measured on an MI355X over the 132 grid cases with N > 1 (six widths
x 22: 13 lengths, three of them in all four kinds): kernel / model between 0.51 and 1.31, median 0.95 (worst: width 80, N = 65,
gauss), so 2.5 holds with room and is kept.  N = 1 is the one shape where the model is exact (P = 1): there the kernel is held to
the float32 round-off bound worked out in _hold (measured: 0 at five widths, 1.19e-7 at width 96).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():   # collected on the CPU box, run on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import attention_ref as R   # noqa: E402
from tests import gpu_util as G   # noqa: E402
from tests import introspection_ref as IR   # noqa: E402

L = G.L
dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32

WIDTHS = [32, 64, 80, 88, 96, 128]
NS = [1, 7, 31, 32, 33, 64, 65, 97, 128, 129, 160, 161, 200, 257]
ALL_KINDS_AT = [33, 160, 257]
CASES = [(N, kind) for N in NS for kind in (R.KINDS if N in ALL_KINDS_AT else R.KINDS[:1])]
ROW_BAR = 2.5      # x the model's worst row of the same case
ROW_CAP = 1e-4
B_, H_ = 2, 3


def _arena(B, N, H, HD):
    D = H * HD
    # bands as wide as 192 rows of qkv, as tests/test_gpu_attention_edges.py gives the forward kernel
    return R.Arena(dev, guard=192 * 3 * D * 2, qkv=((B * N, 3 * D), BF), ctx=((B * N, D), BF), lse=((B * H, N), F32), probs=((B, H, N, N), F32))


def _run(A, B, N, H, HD, scale=None):
    """Outputs to NaN, forward (for lse), probabilities; returns a copy of probs."""
    for n in ("ctx", "lse", "probs"):
        A[n].fill_(float("nan"))
    a = (G.ptr(A["qkv"]), G.ptr(A["ctx"]), G.ptr(A["lse"]), B, N, H, HD)
    if scale is None:
        L.check(L.lib().bvc_op_attention_fwd(*a, G.stream()), "attention_fwd")
    else:
        L.check(L.lib().bvc_op_attention_fwd_scaled(*a, scale, G.stream()), "attention_fwd_scaled")
    L.check(L.lib().bvc_op_attention_probs(G.ptr(A["qkv"]), G.ptr(A["lse"]), G.ptr(A["probs"]), B, N, H, HD,
                                           0.0 if scale is None else scale, G.stream()), "attention_probs")
    torch.cuda.synchronize()
    return A["probs"].clone()


def _hold(got, qkv, B, N, H, HD, label, scale=None):
    """The three bars of the module docstring; every figure printed and logged before anything is asserted."""
    ref = IR.probs_reference(qkv, B, N, H, HD, scale)
    mod = IR.probs_model(qkv, B, N, H, HD, scale)
    k_row, k_at = R.row_err(got, ref)
    m_row, _ = R.row_err(mod, ref)
    ratio = k_row / m_row if m_row > 0 else (0.0 if k_row == 0 else float("inf"))
    rowsum = float((got.double().sum(-1) - 1).abs().max())
    G.log_parity(f"attn_probs d{HD} N{N} B{B} H{H} {label}: row {k_row:.2e} / model {m_row:.2e} = {ratio:.2f} at {k_at}; "
                 f"|rowsum - 1| {rowsum:.1e}")
    fails = []
    if m_row == 0.0:
        # One key: P = 1 and the model gives exactly 1, so there is no model error to take a multiple of.  What correct float32
        # arithmetic may leave: the forward writes lse = the ROUNDED product s * scale_log2 and the kernel subtracts it from the
        # fused, unrounded one - a residue of at most half an ulp of |s2|, i.e. |s2| 2^-24, which exp2 turns into a relative
        # |s2| 2^-24 ln 2 - plus one ulp of the result (2^-23 below 1... 2^-24; v_exp_f32 is good to 1 ulp).
        assert N == 1, "the model is exact for a single key only"
        q, k, _ = R._split(qkv.to(BF), B, N, H, HD, torch.float64)
        s2max = float(((q @ k.transpose(-1, -2)).abs() * (HD ** -0.5 if scale is None else scale) * IR.LOG2E).max())
        bound = 2.0 ** -23 + s2max * 2.0 ** -24
        if not k_row <= bound:
            fails.append(f"one key: |P - 1| = {k_row:.3e} above the float32 round-off bound {bound:.3e}")
    elif not (k_row <= ROW_BAR * m_row or k_row == 0.0):
        fails.append(f"worst row {k_row:.3e} at (clip, head, row) {k_at} is {ratio:.2f} x the model's {m_row:.3e}")
    if not k_row <= ROW_CAP:
        fails.append(f"worst row {k_row:.3e} above {ROW_CAP}")
    if not rowsum <= 1e-4:
        fails.append(f"|rowsum - 1| = {rowsum:.3e}")
    assert not fails, (HD, N, label, fails)


def _finish(A, got):
    A.check()
    assert not torch.isnan(got).any(), "NaN left in probs: an element was not written"


# --------------------------------------------------------------------------- parity grid
@pytest.mark.parametrize("N,kind", CASES, ids=[f"N{n}-{k}" for n, k in CASES])
@pytest.mark.parametrize("HD", WIDTHS)
def test_attention_probs_parity(HD, N, kind):
    B, H = B_, H_
    qkv = R.inputs(kind, B, N, H, HD, seed=6007 * HD + 37 * N + R.KINDS.index(kind))[0].to(dev)
    A = _arena(B, N, H, HD)
    A["qkv"].copy_(qkv)
    first = _run(A, B, N, H, HD)
    second = _run(A, B, N, H, HD)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32)), "probs differ between two launches"
    _hold(first, qkv, B, N, H, HD, kind)
    assert torch.equal(A["qkv"].view(torch.int16), qkv.view(torch.int16))      # operand untouched
    _finish(A, first)


@pytest.mark.parametrize("HD,true_width", [(32, 24), (64, 48)])
def test_attention_probs_explicit_scale(HD, true_width):
    """A stack that zero-pads a head passes the TRUE width's scale (here through the _scaled forward as well); the plain entry
    point's default is another scale, so the result must differ from it."""
    B, H, N = B_, H_, 97
    scale = float(np.float32(1.0) / np.sqrt(np.float32(true_width)))
    qkv = R.inputs("gauss", B, N, H, HD, seed=99 + HD)[0].to(dev)
    A = _arena(B, N, H, HD)
    A["qkv"].copy_(qkv)
    got = _run(A, B, N, H, HD, scale=scale)
    _hold(got, qkv, B, N, H, HD, f"gauss scale 1/sqrt({true_width})", scale=scale)
    plain = _run(A, B, N, H, HD)
    assert not torch.equal(got, plain)
    # scale = 1 / sqrt(head_dim) evaluated in float32, as the launcher does for 0: the same bits
    same = _run(A, B, N, H, HD, scale=float(np.float32(1.0) / np.sqrt(np.float32(HD))))
    assert torch.equal(same.view(torch.int32), plain.view(torch.int32))
    _finish(A, got)


def test_attention_probs_python_wrapper():
    B, H, N, HD = 2, 3, 65, 64
    qkv = R.inputs("gauss", B, N, H, HD, seed=5)[0].to(dev)
    A = _arena(B, N, H, HD)
    A["qkv"].copy_(qkv)
    want = _run(A, B, N, H, HD)
    got = G.bvc.attention_probs(A["qkv"], A["lse"], B, N, H, HD)
    assert got.shape == (B, H, N, N) and got.dtype == F32 and torch.equal(got, want)
    assert torch.equal(G.bvc.attention_probs(A["qkv"], A["lse"], B, N, H, HD, scale=HD ** -0.5), want)
    _finish(A, want)


# --------------------------------------------------------------------------- neighbour invariance
@pytest.mark.parametrize("N", [33, 129, 200])
@pytest.mark.parametrize("HD", WIDTHS)
def test_attention_probs_depend_on_their_own_clip_and_head_only(HD, N):
    """Changing clip 1's qkv leaves clip 0's probs bit-identical; changing head 2's qkv leaves heads 0 / 1 bit-identical (rows
    past a clip's end are clamped inside the clip; the upper half of an 88-wide head's last k-step is zero, not the next head)."""
    B, H = B_, H_
    D = H * HD
    qkv = R.inputs("gauss", B, N, H, HD, seed=31337 + 7919 * HD + N)[0].to(dev)
    A = _arena(B, N, H, HD)
    A["qkv"].copy_(qkv)
    base = _run(A, B, N, H, HD)
    q2 = qkv.clone()
    q2[N:] = (q2[N:].float() * 2.0 + 0.5).to(BF)                       # clip 1, every head
    A["qkv"].copy_(q2)
    other_clip = _run(A, B, N, H, HD)
    assert torch.equal(other_clip[0].view(torch.int32), base[0].view(torch.int32)), "clip 0 changed with clip 1's values"
    assert not torch.equal(other_clip[1], base[1])
    q3 = qkv.clone().view(B * N, 3, H, HD)
    q3[:, :, 2] = (q3[:, :, 2].float() * 2.0 + 0.5).to(BF)              # head 2, every clip
    A["qkv"].copy_(q3.view(B * N, 3 * D))
    other_head = _run(A, B, N, H, HD)
    assert torch.equal(other_head[:, :2].view(torch.int32), base[:, :2].view(torch.int32)), "heads 0 / 1 changed with head 2's values"
    assert not torch.equal(other_head[:, 2], base[:, 2])
    for t in (base, other_clip, other_head):
        _finish(A, t)


# --------------------------------------------------------------------------- past 4 GiB of output
def test_attention_probs_output_past_4_gib():
    """N = 128, width 32, B = 256, H = 257: probs is 4.31 GB (byte offsets past 2^32), qkv 1.6 GB.  The first, the last and 8 seeded
    random heads against the reference; the band after the last head intact.  (Plain tensors, not an Arena: its pattern fill
    needs eight bytes of index per byte.)"""
    B, H, N, HD = 256, 257, 128, 32
    D = H * HD
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 10 ** 9:
        pytest.skip("needs 12 GB of free device memory")
    g = torch.Generator(device=dev).manual_seed(2024)
    qkv = torch.randn(B * N, 3 * D, device=dev, generator=g, dtype=F32).to(BF)
    ctx = torch.empty(B * N, D, device=dev, dtype=BF)
    lse = torch.empty(B * H, N, device=dev, dtype=F32)
    BAND = 1 << 20
    n = B * H * N * N
    assert n * 4 > 2 ** 32
    buf = torch.empty(n + BAND, device=dev, dtype=F32)
    buf[:n].fill_(float("nan"))
    buf[n:].fill_(-7.0)
    L.check(L.lib().bvc_op_attention_fwd(G.ptr(qkv), G.ptr(ctx), G.ptr(lse), B, N, H, HD, G.stream()), "attention_fwd")
    L.check(L.lib().bvc_op_attention_probs(G.ptr(qkv), G.ptr(lse), G.ptr(buf), B, N, H, HD, 0.0, G.stream()), "attention_probs")
    torch.cuda.synchronize()
    assert bool((buf[n:] == -7.0).all()), "the band after the last head was written"
    probs = buf[:n].view(B * H, N, N)
    rng = np.random.RandomState(7)
    picks = [0, B * H - 1] + [int(x) for x in rng.randint(1, B * H - 1, size=8)]
    assert any(bh * N * N * 4 > 2 ** 32 for bh in picks)
    # the ten heads as one 10-clip, one-head problem: one worst row over all of them, held to the grid's bars
    ones, gots = [], []
    for bh in picks:
        b, h = divmod(bh, H)
        ones.append(qkv[b * N:(b + 1) * N].view(N, 3, H, HD)[:, :, h].reshape(N, 3 * HD))
        gots.append(probs[bh])
    got = torch.stack(gots).view(len(picks), 1, N, N)
    assert not torch.isnan(got).any()
    _hold(got, torch.cat(ones).contiguous(), len(picks), N, 1, HD, f"4 GiB case, heads {picks}")
    # no element of the array is left unwritten (a NaN sum would show one), in slices that fit in memory
    for part in probs.view(-1).split(1 << 28):
        assert not bool(torch.isnan(part.sum()))
