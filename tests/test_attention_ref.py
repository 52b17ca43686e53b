"""Pins tests/attention_ref.py on the CPU, so that the bars of tests/test_gpu_attention_edges.py mean what they say: the float64
reference is the formula, the rounding model's error is where it was measured to be, the per-row metric sees what the whole-tensor
norm hides, and the guarded arena reports a stray byte by tensor and side."""
import pytest
import torch

from tests import attention_ref as R

SHAPES = [(2, 129, 2, 64), (2, 125, 2, 128), (1, 500, 2, 96)]
NAMES = (("ctx", 0), ("dq", 2), ("dk", 3), ("dv", 4))


@pytest.mark.parametrize("B,N,H,HD", [(2, 37, 2, 32), (1, 129, 2, 80)])
def test_reference_is_the_formula(B, N, H, HD):
    """float64 against float32 autograd of the same formula: 1e-5 (f32 round-off over sums of <= 129 terms)."""
    qkv, dctx = R.inputs("gauss", B, N, H, HD, seed=1)
    ref = R.reference(qkv, dctx, B, N, H, HD)
    f32 = R._formula(qkv, dctx, B, N, H, HD, None, torch.float32)
    assert all(t.dtype == torch.float64 for t in ref)
    assert ref[0].shape == (B * N, H * HD) and ref[1].shape == (B * H, N) and ref[3].shape == (B * N, H * HD)
    for (name, i) in NAMES:
        assert R.whole_err(f32[i], ref[i]) < 1e-5, name
    assert float((f32[1].double() - ref[1]).abs().max()) < 1e-5
    # an explicit scale is honoured, and the default is 1/sqrt(HD)
    same = R.reference(qkv, dctx, B, N, H, HD, scale=HD ** -0.5)
    other = R.reference(qkv, dctx, B, N, H, HD, scale=0.5 * HD ** -0.5)
    assert torch.equal(same[0], ref[0]) and R.whole_err(other[0], ref[0]) > 1e-2


# (whole-tensor, worst-row) bands of the model's error against the float64 reference, per input kind and tensor.  Measured when
# this file was written (seed 100, the three SHAPES; whole / worst row):
#   gauss, headscale  every tensor 2.33e-3 .. 2.43e-3 / 3.16e-3 .. 3.99e-3
#   sharp             ctx 1.72e-3 .. 1.77e-3 / 3.27e-3 .. 3.40e-3   dv 1.95e-3 .. 2.02e-3 / 3.09e-3 .. 3.61e-3
#                     dq, dk 6.08e-3 .. 8.20e-3 / 2.64e-2 .. 4.78e-2
#   shift             dq 8.82e-3 .. 8.93e-3 / 2.59e-2 .. 3.15e-2   dk 2.35e-3 .. 2.37e-3 / 3.25e-3 .. 4.75e-3   ctx, dv as gauss
# The bands leave the worst-of-rows statistic the room it takes between shapes under identical rounding (x 1.7 observed).
_PLAIN = ((2.2e-3, 2.6e-3), (2.6e-3, 4.4e-3))
BANDS = {
    "gauss": dict(ctx=_PLAIN, dq=_PLAIN, dk=_PLAIN, dv=_PLAIN),
    "headscale": dict(ctx=_PLAIN, dq=_PLAIN, dk=_PLAIN, dv=_PLAIN),
    "sharp": dict(ctx=((1.5e-3, 2.0e-3), (2.6e-3, 4.4e-3)), dv=((1.7e-3, 2.3e-3), (2.6e-3, 4.4e-3)),
                  dq=((5e-3, 1e-2), (2.5e-2, 5.8e-2)), dk=((5e-3, 1e-2), (2.5e-2, 5.8e-2))),
    "shift": dict(ctx=_PLAIN, dv=_PLAIN, dq=((8e-3, 1e-2), (2.3e-2, 3.5e-2)), dk=((2.2e-3, 2.6e-3), (2.6e-3, 5.2e-3))),
}


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B,N,H,HD", SHAPES)
def test_model_error_is_where_it_was_measured(kind, B, N, H, HD):
    qkv, dctx = R.inputs(kind, B, N, H, HD, seed=100)
    assert qkv.dtype == torch.bfloat16 and qkv.shape == (B * N, 3 * H * HD) and dctx.shape == (B * N, H * HD)
    ref = R.reference(qkv, dctx, B, N, H, HD)
    mod = R.model(qkv, dctx, B, N, H, HD)
    assert float((mod[1].double() - ref[1]).abs().max()) < 1e-4       # the model keeps lse in f32
    for name, i in NAMES:
        (wlo, whi), (rlo, rhi) = BANDS[kind][name]
        w = R.whole_err(mod[i], ref[i])
        r, _ = R.row_err(R.heads(mod[i], B, N, H, HD), R.heads(ref[i], B, N, H, HD))
        print(f"model {kind} B{B} N{N} H{H} d{HD} {name}: whole {w:.3e} worst row {r:.3e}")
        assert wlo <= w <= whi, (kind, name, "whole", w)
        assert rlo <= r <= rhi, (kind, name, "row", r)
        assert r >= w                                                   # the worst row is no better than the average one


def test_inputs_are_what_they_say():
    B, N, H, HD = 2, 50, 4, 32
    D = H * HD
    g, _ = R.inputs("gauss", B, N, H, HD, seed=3)
    g = g.float()
    s = R.inputs("sharp", B, N, H, HD, seed=3)[0].float()
    assert torch.equal(s[:, :2 * D], (g[:, :2 * D] * 4)) and torch.equal(s[:, 2 * D:], g[:, 2 * D:])
    k = R.inputs("shift", B, N, H, HD, seed=3)[0].float()
    assert float((k[:, D:2 * D] - g[:, D:2 * D] - 3.0).abs().max()) <= 2 ** -5 and torch.equal(k[:, :D], g[:, :D])    # bf16 below 8
    v = R.inputs("headscale", B, N, H, HD, seed=3)[0].float()
    for h, f in enumerate((0.5, 1.0, 2.0, 0.5)):
        sl = slice(2 * D + h * HD, 2 * D + (h + 1) * HD)
        assert torch.equal(v[:, sl], g[:, sl] * f)
    assert not torch.equal(R.inputs("gauss", B, N, H, HD, seed=4)[0].float(), g)


def test_row_err_definition():
    ref = torch.zeros(1, 2, 4, 8, dtype=torch.float64)
    ref[0, 0, :, 0] = torch.tensor([3.0, 4.0, 0.0, 0.0])        # row norms 3, 4, 0, 0: rms = 2.5
    ref[0, 1, :, 1] = 1.0
    got = ref.clone()
    got[0, 0, 2, 5] = 0.25                                         # a zero row: measured against the head's rms
    assert R.row_err(got, ref) == (0.1, (0, 0, 2))
    got[0, 0, 1, 0] = 5.0                                          # a large row: measured against itself
    assert R.row_err(got, ref) == (0.25, (0, 0, 1))
    got[0, 1, 3, 7] = float("nan")                                # a NaN is the worst there is
    assert R.row_err(got, ref) == (float("inf"), (0, 1, 3))
    z = torch.zeros(1, 1, 2, 4)
    assert R.row_err(z, z)[0] == 0.0                               # exact zero against exact zero
    assert R.row_err(z + 1e-9, z)[0] == float("inf")


def test_one_wrong_row_hides_in_the_whole_tensor_norm_but_not_in_row_err():
    """The gap the per-row bars close: at N = 1568 one key row of dk that is 5 % wrong leaves the whole-tensor error far under
    the 2e-2 bar of tests/test_gpu_ops.py, while row_err rises past 2.5 x the model's own worst row and names the row."""
    B, N, H, HD = 1, 1568, 1, 64
    qkv, dctx = R.inputs("gauss", B, N, H, HD, seed=7)
    ref = R.heads(R.reference(qkv, dctx, B, N, H, HD)[3], B, N, H, HD)
    dk = R.model(qkv, dctx, B, N, H, HD)[3].clone()
    clean, _ = R.row_err(R.heads(dk, B, N, H, HD), ref)
    assert 2.6e-3 <= clean <= 4.4e-3, clean
    dk[1500] *= 1.05
    bad = R.heads(dk, B, N, H, HD)
    assert R.whole_err(bad, ref) < 2e-2
    worst, where = R.row_err(bad, ref)
    assert worst > 2.5 * clean, (worst, clean)
    assert where == (0, 0, 1500)


def _arena():
    return R.Arena("cpu", qkv=((5, 24), torch.bfloat16), lse=((3, 7), torch.float32), odd=((3,), torch.uint8))


def test_arena_layout():
    A = _arena()
    A.check()
    assert A["qkv"].shape == (5, 24) and A["qkv"].dtype == torch.bfloat16 and A["lse"].dtype == torch.float32
    assert torch.isnan(A["qkv"].float()).all() and torch.isnan(A["lse"]).all()      # fresh tensors hold the pattern too
    lo, hi = A.buf.data_ptr(), A.buf.data_ptr() + A.buf.numel()
    n = 0
    for name, side, a, b in A.bands():
        n += 1
        assert b - a >= 64 * 1024 and 0 <= a and b <= A.buf.numel()                   # every band inside the allocation
        a4 = a + (-a) % 4                                                              # readings at the addresses a kernel can use
        for start, dt, size in ((a4, torch.float32, 4), (a4 + 2, torch.float32, 4), (a4, torch.bfloat16, 2)):
            assert torch.isnan(A.buf[start:start + (b - start) // size * size].clone().view(dt).float()).all(), (name, side, dt)
    assert n == 6
    for name, t in A.tensors.items():
        assert t.data_ptr() % 256 == 0
        assert lo + 64 * 1024 <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() + 64 * 1024 <= hi
    # writing every tensor in full leaves every band alone
    A["qkv"].zero_(), A["lse"].zero_(), A["odd"].zero_()
    A.check()


@pytest.mark.parametrize("name,side,at", [("qkv", "after", 0), ("qkv", "before", -1), ("lse", "before", 0), ("odd", "after", 0),
                                          ("lse", "after", -1)])
def test_arena_reports_one_flipped_byte(name, side, at):
    A = _arena()
    band = {(n, s): (a, b) for n, s, a, b in A.bands()}[(name, side)]
    i = band[0] if at == 0 else band[1] - 1
    A.buf[i] ^= 0x01
    with pytest.raises(AssertionError) as e:
        A.check()
    assert f"{side} '{name}'" in str(e.value), str(e.value)
    A.buf[i] ^= 0x01
    A.check()
