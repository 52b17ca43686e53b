"""Pins tests/gemm_ref.py on the CPU, so that the bars of tests/test_gpu_gemm.py are bars against the operations themselves: the
epilogue references against float64 autograd of F.gelu / F.relu / F.layer_norm and against the SimCLR oracle, the index maps against
literal loops, the condition under which the integer cases are exact in float32 for every shape the GPU file runs them at, and the
checkers against faults planted in a copy of a correct result."""
import pytest
import torch
import torch.nn.functional as F

from oracle import simclr_oracle as so
from tests import gemm_ref as R

F64, BF16 = torch.float64, torch.bfloat16


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- product, index maps
@pytest.mark.parametrize("layout", [R.NT, R.NN, R.TN])
def test_product_reads_the_stored_layout(layout):
    M, N, K = 5, 4, 3
    g = _gen(1)
    (ra, wa), (rb, wb) = R.storage_shapes(layout, M, N, K)
    A = torch.randn(ra, wa + 8, generator=g).to(BF16)       # rows wider than used: the extra columns must not matter
    B = torch.randn(rb, wb + 16, generator=g).to(BF16)
    acc, absacc = R.product(A, B, layout, M, N, K)
    for m in range(M):
        for n in range(N):
            s = t = 0.0
            for k in range(K):
                a = float(A[k, m] if layout == R.TN else A[m, k])
                b = float(B[n, k] if layout == R.NT else B[k, n])
                s, t = s + a * b, t + abs(a * b)
            assert abs(float(acc[m, n]) - s) < 1e-12 and abs(float(absacc[m, n]) - t) < 1e-12
    assert _close(R.product_f32(A, B, layout, M, N, K).double(), acc, 1e-6)
    view, nbytes = R.strided(A[:, :wa], wa + 24)
    assert nbytes == ((ra - 1) * (wa + 24) + wa) * 2 and torch.equal(view, A[:, :wa]) and view.stride() == (wa + 24, 1)
    assert bool(torch.isnan(view.as_strided((ra - 1, 24), (wa + 24, 1), wa).float()).all())


def test_scaled_rowsum_and_accumulate():
    g = _gen(2)
    acc = torch.randn(6, 8, generator=g, dtype=F64)
    bias = torch.randn(8, generator=g)
    v = R.scaled(acc, 0.3, 2.0, bias)
    assert _close(v, R.f32_value(0.3) * 2.0 * acc + bias.double()[None]) and v.dtype == F64
    assert R.scaled(acc.float(), 0.5, None, bias).dtype == torch.float32
    A = torch.randn(7, 16, generator=g).to(BF16)                    # TN: [K][lda]
    r, s = R.rowsum(A, 8, 5, 0.5, 2.0)
    assert _close(r, A.double()[:5, :8].sum(0)) and _close(s, A.double()[:5, :8].abs().sum(0))
    c0 = torch.randn(6, 8, generator=g)
    assert _close(R.epi_resid(v, c0), v + c0.double())


def test_row_and_tile_maps_against_loops():
    assert R.e2d_rows(12, 5, 9).tolist() == [(m // 5) * 9 + m % 5 for m in range(12)]
    keep = R.e2d_untouched(12, 5, 9, 27)
    assert [i for i in range(27) if not keep[i]] == sorted((m // 5) * 9 + m % 5 for m in range(12))
    assert R.seg_rows(256, 128, 200, 40).tolist() == [(m // 128) * 200 + 40 + m % 128 for m in range(256)]
    assert R.seg_rows(7, 0, 0, 0).tolist() == list(range(7))
    x = torch.arange(5 * 7, dtype=F64).view(5, 7)
    got = R.tile_sums(x, 2, 4)
    want = [sum(float(x[m, n]) for m in range(5) for n in range(7) if m // 2 == tm and n // 4 == tn) for tm in range(3) for tn in range(2)]
    assert got.tolist() == want
    pos = torch.randn(11, 7, generator=_gen(3))
    tok = torch.tensor([3, 0, 10, 3, 7], dtype=torch.int32)
    assert _close(R.epi_pos(torch.zeros(5, 7, dtype=F64), pos, tok), pos.double()[[3, 0, 10, 3, 7]])
    pm, nm = R.nce_masks(10, 10)
    opos, oneg = so.make_masks(5)
    assert torch.equal(pm, opos) and torch.equal(nm, oneg)


def test_loss_partials_against_a_loop():
    g = _gen(4)
    v, lab = torch.randn(9, 16, generator=g, dtype=F64), torch.randn(9, 16, generator=g)
    d, logits, part = R.epi_loss(v, lab, 4, 8)
    assert _close(d, v - lab.double()) and logits is v
    for tm in range(3):
        for tn in range(2):
            s = sum(float(d[m, n]) ** 2 for m in range(tm * 4, min(9, tm * 4 + 4)) for n in range(tn * 8, tn * 8 + 8))
            assert abs(float(part[tm * 2 + tn]) - s) < 1e-12
    assert abs(float(part.sum()) - float((d * d).sum())) < 1e-10


# ---------------------------------------------------------------------------------------------- activations against autograd
def test_gelu_and_dgelu_are_autograd_of_f_gelu():
    x = (torch.randn(2000, generator=_gen(5), dtype=F64) * 3).requires_grad_(True)
    dy = torch.randn(2000, generator=_gen(6), dtype=F64)
    y = F.gelu(x)                                                    # approximate="none": exact erf
    y.backward(dy)
    grad, act = R.epi_gelu(x.detach())
    assert _close(act, y.detach()) and _close(grad * dy, x.grad)
    aux = grad.to(BF16)                                              # what the forward epilogue stores
    assert _close(R.epi_dgelu(dy, aux), dy * aux.double())
    eg, ea = R.gelu_erf_room(x.detach())
    # the stated erf error, pushed through both formulas numerically: d gelu / d erf = x / 2, d gelu' / d erf = 1 / 2
    assert _close(ea, 0.5 * x.detach().abs() * 1.5e-7) and _close(eg, torch.full_like(eg, 0.75e-7))


def test_relu_and_drelu_are_autograd_of_f_relu_with_the_gate_on_the_bits():
    bits = torch.tensor([0x0000, 0x8000, 0x0001, 0x8001, 0x3F80, 0xBF80, 0x7F00, 0xFF00, 0x7F80, 0xFF80, 0x0080], dtype=torch.int32)
    aux = bits.to(torch.int16).view(BF16)
    assert R.drelu_gate(aux).tolist() == [False, False, True, False, True, False, True, False, True, False, True]
    assert float(aux[2]) > 0 and float(aux[1]) == 0 and str(float(aux[1])) == "-0.0"
    pre = (torch.randn(500, generator=_gen(7), dtype=F64)).requires_grad_(True)
    dy = torch.randn(500, generator=_gen(8), dtype=F64)
    y = F.relu(pre)
    y.backward(dy)
    assert _close(R.epi_relu(pre.detach()), y.detach())
    saved = y.detach().to(BF16)                                      # the forward output, as EPI_RELU stores it
    live = pre.detach().abs() > 1e-30                                 # (bf16 keeps float32's range: nothing positive rounds to zero here)
    assert _close(R.epi_drelu(dy, saved)[live], pre.grad[live])


@pytest.mark.parametrize("seg", [None, (128, 200, 40)])
def test_resid_ln_and_dln_are_autograd_of_layer_norm(seg):
    M, N = 256, 384
    g = _gen(9)
    v = torch.randn(M, N, generator=g, dtype=F64)
    P = 2 * 200 if seg else M
    resid = torch.randn(P, N, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    eps = 1e-6
    c, ln, mean, rstd = R.epi_resid_ln(v, resid, gamma, beta, eps, seg)
    rows = R.seg_rows(M, *(seg or (0, 0, 0)))
    x = (v + resid.double()[rows]).requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.layer_norm(x, (N,), gr, br, R.f32_value(eps))
    dy = torch.randn(M, N, generator=g, dtype=F64)
    y.backward(dy)
    assert _close(c, x.detach()) and _close(ln, y.detach(), 1e-11) and _close(mean, x.detach().mean(1))
    assert _close(rstd, 1 / torch.sqrt(x.detach().var(1, unbiased=False) + R.f32_value(eps)))
    dx, dg, db = R.epi_dln(dy, c, gamma, mean, rstd)
    assert _close(dx, x.grad, 1e-10) and _close(dg, gr.grad, 1e-10) and _close(db, br.grad, 1e-10)


def test_resid_gate_against_a_loop():
    g = _gen(10)
    M, N, rows, p = 7, 8, 3, 0.5
    v, resid = torch.randn(M, N, generator=g, dtype=F64), torch.randn(M, N, generator=g)
    keep = (torch.rand(M, N, generator=g) > p).to(torch.uint8)
    scale = torch.tensor([2.0, 0.0, 2.0])
    out = R.epi_resid_gate(v, resid, keep, p, scale, rows)
    for m in range(M):
        for n in range(N):
            want = float(resid[m, n]) + float(scale[m // rows]) * int(keep[m, n]) / (1 - p) * float(v[m, n])
            assert abs(float(out[m, n]) - want) < 1e-12
    assert torch.equal(out[3:6], resid.double()[3:6])                 # the dropped sample: exactly the residual
    assert _close(R.epi_resid_gate(v, resid, None, 0.0, None, rows), v + resid.double())


# ---------------------------------------------------------------------------------------------- InfoNCE against the oracle
@pytest.mark.parametrize("B", [4, 36])
def test_nce_partials_and_gradient_are_the_oracle_loss(B):
    n, T = 2 * B, 0.07
    f = so.synthetic_features(n, 32, 11).double().requires_grad_(True)
    loss = so.info_nce_loss(T, so.make_masks(B), f)
    loss.backward()
    loss = loss.detach()
    fn = F.normalize(f.detach(), dim=1)
    v = fn @ fn.t() / T
    for bm, bn in ((128, 128), (8, 4), (5, 7)):
        part = R.epi_nce(v, 1 / T, bm, bn)
        assert part.numel() == 2 * ((n + bm - 1) // bm) * ((n + bn - 1) // bn)
        got, lse, pc = R.nce_finalize(part, 1 / T, 2 * n - 2)
        assert abs(float(got) - float(loss)) < 1e-12 * max(1.0, abs(float(loss)))
    # d loss / d v from EPI_NCE_BWD, pulled back to the features through the same normalisation
    Gm = R.epi_nce_bwd(v, float(lse), pc)
    f2 = f.detach().clone().requires_grad_(True)
    fn2 = F.normalize(f2, dim=1)
    ((fn2 @ fn2.t() / T) * Gm).sum().backward()
    assert _close(f2.grad, f.grad, 1e-10)
    assert bool((Gm.diagonal() == 0).all())


# ---------------------------------------------------------------------------------------------- exactness of the integer cases
def test_every_exact_shape_is_exact_in_float32():
    """operands in [-8, 8]: |sum| <= 64 K; alpha in {0.5, 1} (x alpha_dev 2), up to three integer addends of magnitude <= 1024 (bias,
    residual / positional / label / start value): every partial result is a multiple of 0.5 below 2^23, so exact in float32."""
    assert len(set(R.EXACT_SHAPES)) >= 20
    for M, N, K in R.EXACT_SHAPES:
        for alpha in (0.5, 1.0):
            assert R.product_is_exact(K, alpha, 3), (M, N, K)
        assert 64 * K < 1 << 24
    assert not R.product_is_exact(1 << 18, 1.0) and not R.product_is_exact(64, 0.3)
    # and the property itself, on the longest contraction in the list: a float32 sum in a scrambled order equals the float64 one
    K = max(k for _, _, k in R.EXACT_SHAPES)
    g = _gen(12)
    a = torch.randint(-8, 9, (K,), generator=g).double()
    b = torch.randint(-8, 9, (K,), generator=g).double()
    terms = (a * b).float()[torch.randperm(K, generator=g)]
    s = torch.zeros((), dtype=torch.float32)
    for chunk in terms.split(97):
        s = s + chunk.sum()
    assert float(s) * 0.5 + 1024.0 == float((a * b).sum()) * 0.5 + 1024.0
    # DGELU multiplies an exact v by an integer aux in [-8, 8]: still below 2^24 halves
    assert 8 * (64 * K + 1024) * 2 < 1 << 24


# ---------------------------------------------------------------------------------------------- the contraction-tail window
def test_tn_contraction_tail_that_would_wrap_is_refused(bvc):
    """A TN product walks its K rows 64 at a time and relies on the rows past K reading as zero because their byte offsets lie past
    a_bytes / b_bytes.  Those offsets are formed in 32 bits: when roundup64(K) ld 2 passes 2^32 while K ld 2 does not, they wrap
    into the operand (measured on the GPU before launch_gemm refused it: K = 2010, lda = 2^20 + 2^14 with NaN between the rows
    gave NaN in all 9792 outputs).  bvc_op_gemm_kernel runs the launcher's checks without a GPU."""
    import ctypes
    L = bvc._lib
    M, N, K = R.LARGE_TN

    def name(lda, ldb, k=K):
        d = L.GemmDesc()
        d.A, d.B, d.C = 4096, 8192, 4096          # never dereferenced: nothing is launched
        d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, k, lda, ldb, N
        d.alpha, d.epi, d.split_k = 1.0, 0, 1
        d.a_bytes, d.b_bytes = ((k - 1) * lda + M) * 2, ((k - 1) * ldb + N) * 2
        buf = ctypes.create_string_buffer(160)
        rc = L.lib().bvc_op_gemm_kernel(ctypes.byref(d), 1, R.TN, 0, -1, buf, 160)
        return rc, (buf.value if rc == 0 else L.lib().bvc_last_error())

    inside, below = (1 << 20) + (1 << 14), (1 << 20) - 8
    assert K * inside * 2 < 2 ** 32 <= 2048 * inside * 2 and 2048 * below * 2 < 2 ** 32
    for lda, ldb in ((inside, N), (M, inside)):
        rc, msg = name(lda, ldb)
        assert rc != 0 and b"wrap" in msg and b"K=2010" in msg, msg
    for lda, ldb, k in ((below, N, K), (M, below, K), (inside, N, 1984), (M, N, K)):      # below the window; no surplus rows; small
        rc, msg = name(lda, ldb, k)
        assert rc == 0 and msg.startswith(b"bvc::gemm_kernel<128, 128, true, true"), msg


# ---------------------------------------------------------------------------------------------- planted faults
def _correct(seed=13, M=40, N=24, K=64, ldc=32):
    g = _gen(seed)
    A, B = torch.randn(M, K, generator=g).to(BF16), (torch.randn(N, K, generator=g) / 8).to(BF16)
    acc, absacc = R.product(A, B, R.NT, M, N, K)
    return acc, R.product_f32(A, B, R.NT, M, N, K), absacc


def test_checkers_pass_a_correct_result():
    ref, t32, scale = _correct()
    log = R.CaseLog("self-test")
    R.check_f32(log, "f32", t32, ref, t32, scale)
    R.check_bf16(log, "bf16", t32.to(BF16), ref, t32, scale)
    assert "f32" in log.line() and "bf16" in log.line()


def test_planted_two_ulp_error_is_caught():
    ref, t32, scale = _correct()
    got = t32.to(BF16).clone()
    i = (int(ref.abs().argmax()) // ref.shape[1], int(ref.abs().argmax()) % ref.shape[1])
    bits = got.view(torch.int16)
    bits[i] += 2                                                      # two bf16 ulp away from the rounded value
    with pytest.raises(AssertionError, match="over the bf16 bar"):
        R.check_bf16(None, "bf16", got, ref, t32, scale)
    got32 = t32.clone()
    got32[3, 5] += float(16 * R.ulp32(scale[3, 5].reshape(1)))          # an f32 element off by 16 ulp of its scale
    with pytest.raises(AssertionError, match="over the bar"):
        R.check_f32(None, "f32", got32, ref, t32, scale)


def test_planted_chunk_from_the_neighbouring_row_is_caught():
    ref, t32, scale = _correct()
    for dtype, chk in ((torch.float32, R.check_f32), (BF16, R.check_bf16)):
        got = t32.to(dtype).clone()
        got[17, 8:16] = got[18, 8:16]
        with pytest.raises(AssertionError):
            chk(None, "chunk", got, ref, t32, scale)


def test_planted_writes_into_gap_and_guards_are_caught():
    for dtype in (torch.float32, BF16):
        out = R.Guarded(5, 24, 32, dtype, device="cpu")
        out.check("untouched")
        assert bool(torch.isnan(out.t.float()).all()) and out.t.shape == (5, 24) and out.t.stride() == (32, 1)
        out.full[2, 24] = 1.0                                         # the first column of a row gap
        with pytest.raises(AssertionError, match="row gap"):
            out.check("gap")
        out = R.Guarded(5, 24, 32, dtype, device="cpu")
        out.buf[out.g + 5 * 32] = 1.0                                 # the first element behind the payload
        with pytest.raises(AssertionError, match="PAST the end"):
            out.check("back")
        out = R.Guarded(5, 24, 24, dtype, device="cpu")
        out.buf[out.g - 1] = 1.0
        with pytest.raises(AssertionError, match="BEFORE"):
            out.check("front")
    # an accumulated output starts from the values handed in, and a store of the guard pattern's own value is no write
    start = torch.arange(6.0).view(2, 3)
    out = R.Guarded(2, 3, 8, fill=start, device="cpu")
    assert torch.equal(out.t, start) and torch.equal(out.bits().view(torch.float32), start)


def test_planted_displaced_e2d_row_is_caught():
    M, rin, rout, N = 12, 5, 9, 8
    P = 27
    out = R.Guarded(P, N, 16, device="cpu")
    before = out.bits()
    rows = R.e2d_rows(M, rin, rout)
    vals = torch.randn(M, N, generator=_gen(14))
    out.t[rows] = vals
    R.rows_unchanged(before, out.bits(), R.e2d_untouched(M, rin, rout, P), "correct scatter")
    out.check("correct scatter")
    out.t[7] = vals[6]                                                # row 6 -> 10 belongs at 10; a copy lands in the rin .. rout band
    with pytest.raises(AssertionError, match="untouched rows were written"):
        R.rows_unchanged(before, out.bits(), R.e2d_untouched(M, rin, rout, P), "displaced")
    # and a row that went to its neighbour's place fails the value check
    got = vals.clone()
    got[[6, 7]] = got[[7, 6]]
    with pytest.raises(AssertionError):
        R.check_f32(None, "e2d", got, vals.double(), vals, vals.double().abs() + 1)


def test_exact_checker():
    ref = torch.tensor([[3.0, -2.5, 0.0, 257.0]], dtype=F64)
    R.check_exact("f32", ref.float(), ref)
    R.check_exact("bf16", torch.tensor([[3.0, -2.5, -0.0, 256.0]]).to(BF16), ref, True)      # 257 -> 256 (ties to even), -0 == +0
    with pytest.raises(AssertionError, match="exact case differ"):
        R.check_exact("bf16", torch.tensor([[3.0, -2.5, 0.0, 258.0]]).to(BF16), ref, True)
    with pytest.raises(AssertionError, match="exact case differ"):
        R.check_exact("f32", ref.float() + torch.tensor([[0.0, 0.0, 0.0, 1.0]]), ref)
