"""The row and element kernels of csrc/rowops.hip through the C ABI, each against the float64 reference of tests/rowops_ref.py at
every instantiation, launcher branch and edge (tests/test_rowops_ref.py pins those references on the CPU).

Common rules of this file
  * Guard bands.  Every output and workspace is the middle of a larger buffer [guard | payload | guard] (`Guarded`): the payload is
    16-byte aligned, a guard is one row rounded up to 64 elements (at least 64), filled with a fixed bit pattern, and must be
    bit-identical after the call.  Outputs the call must overwrite start as NaN.
  * Bars are per row (per element for the flat kernels), never one global norm.  f32 outputs: 4 x the worst error, against float64,
    of torch's own float32 op on the same device inputs, relative to the row's scale, with a floor of 4 ulp of the reference value
    (`_f32_check`).  The scale of a row is its largest |reference|; for a sum (means, column sums, parameter gradients) it is the
    sum of the magnitudes of its terms, which is what a rounding error of a sum is proportional to.  bf16 outputs: 2^-8 |ref| per
    element plus that f32 budget (`_bf16_check`).  No number is fixed in advance; the kernel's and torch's errors of every case go
    to the parity report (profiles/rowops_parity_report.txt is a copy), one line per case, worst over the runs of the case.
  * Exact cases.  Integer inputs in [-8, 8] and power-of-two scales make every partial sum exact in float32 in any order
    (rows * 8 < 2^24, checked for these shapes in test_rowops_ref.py): the result must equal the reference bit for bit.
  * Refusals are tested only where the launcher checks before it launches.
"""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():   # collected on the CPU box, run on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G     # noqa: E402
from tests import rowops_ref as R   # noqa: E402

L = G.L
bvc = G.bvc
dev = "cuda"
F64 = torch.float64
BF16 = torch.bfloat16
NAN = float("nan")
PAT32, PAT16 = 0x00A5A5A5, 0x5AA5      # guard patterns: a tiny normal float (any add to it shows), a bf16 no kernel here produces


# ---------------------------------------------------------------------------------------------- guarded memory, bars, log
class Guarded:
    """payload `t` of the given shape inside [guard | payload | guard]; fill: "nan", a number or a tensor to copy."""

    def __init__(self, shape, dtype=torch.float32, fill="nan", row=0):
        n = int(math.prod(shape))
        wide = torch.empty(0, dtype=dtype).element_size() == 4
        self.pat = PAT32 if wide else PAT16
        self.g = g = max(64, (row + 63) // 64 * 64)
        self.n = n
        self.buf = torch.empty(2 * g + n, dtype=dtype, device=dev)
        self.ibuf = self.buf.view(torch.int32 if wide else torch.int16)
        self.ibuf.fill_(self.pat)
        self.t = self.buf[g:g + n].view(shape)
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill)
        else:
            self.t.fill_(NAN if fill == "nan" else fill)
        assert self.t.data_ptr() % 16 == 0

    def bits(self):
        return self.ibuf[self.g:self.g + self.n].clone()

    def check(self, what):
        front = self.ibuf[:self.g] != self.pat
        back = self.ibuf[self.g + self.n:] != self.pat
        assert not bool(front.any()), f"{what}: {int(front.sum())} elements written BEFORE the buffer"
        assert not bool(back.any()), f"{what}: {int(back.sum())} elements written PAST the end (first at +{int(back.nonzero()[0])})"


class CaseLog:
    """Worst kernel and torch-f32 error per output of one case; one line of the parity report."""

    def __init__(self, name):
        self.name, self.items = name, {}

    def add(self, key, k, t):
        a, b = self.items.get(key, (0.0, 0.0))
        self.items[key] = (k if not k <= a else a, t if not t <= b else b)      # (a NaN sticks)

    def note(self, key, text):
        self.items[key] = text

    def flush(self):
        parts = [f"{k} {v}" if isinstance(v, str) else f"{k} {v[0]:.2e}/{v[1]:.2e}" for k, v in self.items.items()]
        G.log_parity(f"rowops {self.name}: " + "  ".join(parts) + "   (kernel/torch-f32, relative to the row scale)")


@contextlib.contextmanager
def case_log(name):
    log = CaseLog(name)
    try:
        yield log
    finally:
        log.flush()


def _as_rows(t, ref):
    t = t.to(F64).reshape(ref.shape)
    return t.reshape(1, 1) if t.dim() == 0 else (t[:, None] if t.dim() == 1 else t.reshape(-1, t.shape[-1]))


def _budget(ref, t32, scale):
    """(per-row scale, largest |ref| of the row, worst torch-f32 error relative to the scale)."""
    vmax = ref.abs().amax(-1)
    sc = vmax if scale is None else scale.to(F64).reshape(-1)
    et = (t32 - ref).abs().amax(-1)
    nz = sc > 0
    wt = float((et[nz] / sc[nz]).max()) if bool(nz.any()) else 0.0
    return sc, vmax, wt, nz


def _f32_check(log, key, got, ref, t32, scale=None):
    """f32 output against float64 `ref`, per row (last dimension; a vector is one element per row): error <= max(4 x worst
    torch-f32 error x scale, 4 ulp of the row's largest |ref|)."""
    ref = ref.to(F64)
    got, t32, ref = _as_rows(got, ref), _as_rows(t32, ref), _as_rows(ref, ref)
    sc, vmax, wt, nz = _budget(ref, t32, scale)
    eg = (got - ref).abs().amax(-1)
    wk = float((eg[nz] / sc[nz]).max()) if bool(nz.any()) else float(eg.max())
    log.add(key, wk, wt)
    bar = torch.maximum(4 * wt * sc, 4 * R.ulp32(vmax))
    bad = ~(eg <= bar)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{log.name} {key}: {int(bad.sum())} of {bad.numel()} rows over the bar; row {i}: error {float(eg[i]):.3e}, "
                             f"bar {float(bar[i]):.3e} (torch-f32 worst {wt:.3e} x scale {float(sc[i]):.3e})")


def _bf16_check(log, key, got, ref, t32, scale=None):
    """bf16 output per element: |got - ref| <= 2^-8 |ref| + the f32 budget of its row."""
    ref = ref.to(F64)
    got, t32, ref = _as_rows(got, ref), _as_rows(t32, ref), _as_rows(ref, ref)
    sc, vmax, wt, nz = _budget(ref, t32, scale)
    room = torch.maximum(4 * wt * sc, 4 * R.ulp32(vmax))[:, None]
    over = (got - ref).abs() - (2.0 ** -8 * ref.abs() + room)
    eg = (got - ref).abs().amax(-1)
    log.add(key, float((eg[nz] / sc[nz]).max()) if bool(nz.any()) else float(eg.max()), wt)
    bad = ~(over <= 0)
    if bool(bad.any()):
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{log.name} {key}: {int(bad.sum())} elements over the bf16 bar; first {i}: got {float(got[i[0], i[1]])!r}, "
                             f"ref {float(ref[i[0], i[1]])!r}")


def _ulp_check(log, key, got, ref, ulps):
    """per element: |got - ref| <= ulps x ulp32(ref)."""
    ref = ref.to(F64)
    got = got.to(F64).reshape(ref.shape)
    err = (got - ref).abs() / R.ulp32(ref)
    log.note(key, f"{float(err.max()):.2f} ulp")
    bad = ~(err <= ulps)
    assert not bool(bad.any()), f"{log.name} {key}: {int(bad.sum())} elements beyond {ulps} ulp (worst {float(err.max()):.2f})"


def _same_bits(a, b):
    w = torch.int32 if a.element_size() == 4 else torch.int16
    return torch.equal(a.contiguous().view(w), b.contiguous().view(w))


@contextlib.contextmanager
def _mode(det):
    """the `deterministic` option, set and restored as tests/test_gpu_deterministic.py does"""
    bvc.use_deterministic_algorithms(bool(det))
    try:
        assert L.lib().bvc_get_option(b"deterministic") == int(bool(det))
        yield
    finally:
        bvc.use_deterministic_algorithms(False)
        L.lib()    # push the mode back to the library


def _gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=dev)


def _randint(g, lo, hi, shape, dtype=torch.float32):
    return torch.randint(lo, hi + 1, shape, generator=g, device=dev, dtype=torch.int16).to(dtype)


def _call(fn, *args):
    rc = fn(*args, G.stream())
    torch.cuda.synchronize()
    return rc


# ---------------------------------------------------------------------------------------------- LayerNorm
LN_KINDS = {
    "plain": lambda g, P, D: _randn(g, P, D) * 2 + 0.5,
    "offset": lambda g, P, D: 100 + 0.1 * _randn(g, P, D),          # a mean a thousand times the spread
    "big": lambda g, P, D: 1e4 * _randn(g, P, D),
    "small": lambda g, P, D: 1e-4 * _randn(g, P, D),
    "const1": lambda g, P, D: torch.full((P, D), 1.0, device=dev),
    "const-3": lambda g, P, D: torch.full((P, D), -3.0, device=dev),
}
ALL_VARIANTS = ((1, True), (1, False), (0, True), (0, False))        # (accumulate, bf16 copy)
SWEEP_VARIANTS = ((1, True), (0, False))


def _ln_case(name, M, D, kind="plain", eps=1e-12, rmap=None, int_dy=False, variants=SWEEP_VARIANTS, seed=40):
    """LayerNorm forward, then the backward under both settings of the deterministic option and every (accumulate, bf16 copy) of
    `variants`; float64 and torch-f32 results are computed once and shared by the runs."""
    lib = L.lib()
    g = _gen(seed + D + M)
    P = R.physical_rows(M, rmap)
    rows = R.mapped_rows(M, rmap, dev)
    rm = rmap or (0, 0, 0)
    x = LN_KINDS[kind](g, P, D)
    gamma, beta = 1 + 0.1 * _randn(g, D), 0.1 * _randn(g, D)
    dy = _randint(g, -R.INT_RANGE, R.INT_RANGE, (M, D), BF16) if int_dy else _randn(g, M, D).to(BF16)
    with case_log(name) as log:
        # ---- forward
        y, mean, rstd = Guarded((M, D), BF16, "nan", D), Guarded((M,)), Guarded((M,))
        L.check(_call(lib.bvc_op_layernorm_fwd, G.ptr(x), *rm, G.ptr(gamma), G.ptr(beta), G.ptr(y.t), G.ptr(mean.t), G.ptr(rstd.t),
                      M, D, eps), "ln_fwd")
        for b, w in ((y, "y"), (mean, "mean"), (rstd, "rstd")):
            b.check(f"{name} ln_fwd {w}")
        ry, rmean, rrstd = R.layernorm_fwd(x, gamma, beta, eps, M, rmap)
        xt = x[rows].clone().requires_grad_(True)
        gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        ty, tmean, trstd = torch.native_layer_norm(xt, (D,), gt, bt, R.f32_value(eps))       # what F.layer_norm runs, with its statistics
        _f32_check(log, "mean", mean.t, rmean, tmean.detach().reshape(-1), scale=x[rows].to(F64).abs().mean(1))
        _f32_check(log, "rstd", rstd.t, rrstd, trstd.detach().reshape(-1))
        _bf16_check(log, "y", y.t, ry, ty.detach())
        if kind.startswith("const"):
            # sums of equal small integers are exact: the mean is exact, x - mean == 0, so y is bf16(beta) and rstd is 1/sqrt(eps)
            assert torch.equal(mean.t, x[rows][:, 0]), f"{name}: mean of a constant row is not exact"
            assert _same_bits(y.t, beta.to(BF16)[None].expand(M, D)), f"{name}: y of a constant row is not bf16(beta)"
            want = 1 / math.sqrt(R.f32_value(eps))
            assert float((rstd.t.double() / want - 1).abs().max()) <= 1e-6, f"{name}: rstd of a constant row"
        # ---- backward: references once
        rdx, rdg, rdb = R.layernorm_bwd(dy, x, gamma, eps, M, rmap)
        ty.backward(dy.float())
        tdx, tdg, tdb = xt.grad, gt.grad, bt.grad
        xh = (x[rows].to(F64) - rmean[:, None]) * rrstd[:, None]
        sg, sb = (dy.to(F64) * xh).abs().sum(0), dy.to(F64).abs().sum(0)
        dres0 = _randn(g, P, D)
        dg0 = _randn(g, D)
        db0 = _randint(g, -1024, 1024, (D,)) if int_dy else _randn(g, D)
        wsn = int(lib.bvc_op_layernorm_bwd_workspace(M, D))
        unmapped = torch.ones(P, dtype=torch.bool, device=dev)
        unmapped[rows] = False
        for det in (0, 1):
            for acc, bf in variants:
                runs = []
                for rep in range(2 if det else 1):
                    dres = Guarded((P, D), fill=dres0 if acc else "nan", row=D)
                    dbf = Guarded((P, D), BF16, "nan", D) if bf else None
                    dg, db, ws = Guarded((D,), fill=dg0), Guarded((D,), fill=db0), Guarded((wsn,), fill="nan", row=2 * D)
                    before, before_bf = dres.bits().view(P, D), dbf.bits().view(P, D) if bf else None
                    with _mode(det):
                        L.check(_call(lib.bvc_op_layernorm_bwd, G.ptr(dy), G.ptr(x), *rm, G.ptr(mean.t), G.ptr(rstd.t), G.ptr(gamma),
                                      G.ptr(dres.t), acc, G.ptr(dbf.t) if bf else None, G.ptr(dg.t), G.ptr(db.t), G.ptr(ws.t), M, D),
                                "ln_bwd")
                    tag = f"{name} det={det} acc={acc} bf={int(bf)}"
                    for b, w in ((dres, "dres"), (dbf, "dres_bf16"), (dg, "dgamma"), (db, "dbeta"), (ws, "workspace")):
                        if b is not None:
                            b.check(f"{tag} ln_bwd {w}")
                    runs.append((dres, dbf, dg, db))
                dres, dbf, dg, db = runs[0]
                if det:
                    for a, b in zip(runs[0], runs[1]):
                        assert a is None or _same_bits(a.t, b.t), f"{tag}: two deterministic runs differ"
                total = rdx + dres0[rows].to(F64) if acc else rdx
                ttotal = tdx + dres0[rows] if acc else tdx
                _f32_check(log, "dx", dres.t[rows], total, ttotal)
                if bf:
                    _bf16_check(log, "dx_bf16", dbf.t[rows], total, ttotal)
                if bool(unmapped.any()):       # the rows the map skips keep their pre-fill, bit for bit
                    assert torch.equal(dres.bits().view(P, D)[unmapped], before[unmapped]), f"{tag}: an unmapped row of dres changed"
                    assert not bf or torch.equal(dbf.bits().view(P, D)[unmapped], before_bf[unmapped]), f"{tag}: an unmapped bf16 row changed"
                _f32_check(log, "dgamma", dg.t, dg0.to(F64) + rdg, dg0 + tdg, scale=dg0.to(F64).abs() + sg)
                _f32_check(log, "dbeta", db.t, db0.to(F64) + rdb, db0 + tdb, scale=db0.to(F64).abs() + sb)
                if int_dy:
                    assert torch.equal(db.t.to(F64), db0.to(F64) + rdb), f"{tag}: dbeta of integer dy is not exact"


@pytest.mark.parametrize("M", R.LN_WIDTH_ROWS)
@pytest.mark.parametrize("D", R.LN_WIDTHS)
def test_layernorm_widths(D, M):
    """Every instantiation of ln_fwd_kernel / ln_bwd_kernel at its ends, in the 4-row (M = 5: dead waves in the only group) and the
    16-row tier (M = 16385: one row in the last group):
      D = 384, 512          <32, 4> forward, <8, 32, 4> / <16, 32, 4> backward (half-wave rows; 128 runs in test_layernorm_rows)
      D = 4, 132, 260, 516  <64, 4> forward, <4, 64, 4> / <16, 64, 4> backward with 1, 33, 65, 129 chunks: lane 0 carries an extra
                            round;  192 and 1024 fill the rounds of their lanes evenly
      D = 1028 .. 1536      <64, 6> forward, <4, 64, 6> / <16, 64, 6> backward (kWideChunks): first width, ViT-H, ViT-g, the top.
    dy is Gaussian at M = 5 and integer-valued at M = 16385, where dbeta must then be exact over the 1025 partial rows."""
    _ln_case(f"ln widths D={D} M={M}", M, D, int_dy=M > 1000)


@pytest.mark.parametrize("M", R.LN_ROWS)
@pytest.mark.parametrize("D", R.LN_ROW_WIDTHS)
def test_layernorm_rows(D, M):
    """The tiers and grids of launch_ln_fwd / launch_ln_bwd at D = 128 (half-wave) and 192 (full wave): 1 .. 9 rows (dead half-waves and
    waves of the last group, one group per workgroup), 8203 (4-row tier on a grid stride at D = 192: 2051 groups on 2048 workgroups),
    16383 / 16384 / 16385 (the tier switch and the workspace of bvc_op_layernorm_bwd_workspace on either side), 40001 (16-row tier,
    2501 groups on 2048 workgroups: uneven), 131089 (whole rounds backward, the forward's grid stride in both instantiations).
    dy is integer-valued: dbeta must be exact, so one dropped or doubled row fails whatever M is."""
    _ln_case(f"ln rows D={D} M={M}", M, D, int_dy=True)


@pytest.mark.parametrize("kind,eps", [("offset", 1e-12), ("big", 1e-12), ("small", 1e-6), ("small", 1e-12), ("const1", 1e-12),
                                      ("const-3", 1e-12)])
@pytest.mark.parametrize("D", [192, 384, 1280])
def test_layernorm_ill_conditioned(D, kind, eps):
    """Rows a one-pass variance or a misplaced eps gets wrong: mean 1000 x the spread, scales 1e4 and 1e-4 (eps 1e-6 dominates the
    variance of the latter, 1e-12 does not), constant rows (exact mean, y == bf16(beta), rstd == 1/sqrt(eps))."""
    _ln_case(f"ln {kind} eps={eps:g} D={D} M=37", 37, D, kind=kind, eps=eps, variants=((0, True),))


@pytest.mark.parametrize("rmap", [None, (12, 20, 8)])
@pytest.mark.parametrize("D", [128, 192, 1280])
def test_layernorm_backward_variants(D, rmap):
    """accumulate 0 / 1 (a NaN pre-fill of dres must vanish with 0), bf16 copy present / absent, dgamma / dbeta accumulated onto
    random start values (dbeta exactly: integer dy onto integers), over dense rows and over the row map m -> (m / 12) * 20 + 8 + m % 12
    of 3 clips: x, dres and the bf16 copy are addressed physically, and their 24 unmapped rows must keep their pre-fill."""
    _ln_case(f"ln variants D={D} map={rmap}", 36, D, rmap=rmap, int_dy=True, variants=ALL_VARIANTS)


@pytest.mark.parametrize("D", [1540, 130])
def test_layernorm_refusals(D):
    """D > 1536 and D % 4 != 0 are refused by launch_ln_fwd / launch_ln_bwd / launch_target_select before any launch: an error code,
    and every output as it was."""
    lib = L.lib()
    M = 5
    g = _gen(1)
    x, gamma, beta = _randn(g, M, D), _randn(g, D), _randn(g, D)
    dy = _randn(g, M, D).to(BF16)
    outs = dict(y=Guarded((M, D), BF16, "nan", D), mean=Guarded((M,)), rstd=Guarded((M,)), dres=Guarded((M, D), fill=1.5, row=D),
                dbf=Guarded((M, D), BF16, "nan", D), dg=Guarded((D,), fill=2.5), db=Guarded((D,), fill=3.5),
                ws=Guarded((int(lib.bvc_op_layernorm_bwd_workspace(M, D)),), row=2 * D), sel=Guarded((M, D), row=D))
    was = {k: v.bits() for k, v in outs.items()}
    stats = torch.ones(M, device=dev)
    idx = torch.zeros(M, dtype=torch.int32, device=dev)
    o = outs
    assert _call(lib.bvc_op_layernorm_fwd, G.ptr(x), 0, 0, 0, G.ptr(gamma), G.ptr(beta), G.ptr(o["y"].t), G.ptr(o["mean"].t),
                 G.ptr(o["rstd"].t), M, D, 1e-6) != 0
    assert _call(lib.bvc_op_layernorm_bwd, G.ptr(dy), G.ptr(x), 0, 0, 0, G.ptr(stats), G.ptr(stats), G.ptr(gamma), G.ptr(o["dres"].t), 1,
                 G.ptr(o["dbf"].t), G.ptr(o["dg"].t), G.ptr(o["db"].t), G.ptr(o["ws"].t), M, D) != 0
    assert _call(lib.bvc_op_target_select, G.ptr(x), G.ptr(idx), G.ptr(o["sel"].t), 1, 1, M, M, D, 1e-6) != 0
    for k, v in outs.items():
        v.check(f"refused D={D} {k}")
        assert torch.equal(v.bits(), was[k]), f"refused D={D}: {k} was written"


# ---------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("M", R.COLSUM_BF16_M)
@pytest.mark.parametrize("N", R.COLSUM_BF16_N)
def test_colsum_bf16_exact(N, M):
    """colsum_bf16_kernel / colsum_bf16_det_kernel, bit for bit on integers: one column chunk (N = 8), a second grid column with 1
    (520) and with a whole 512 + 8 tail (1032); ld = N, N + 8, 2 N with large values in the columns past N, which must not leak in;
    rows around the 64-row block (63 / 64 / 65) and the block switch to 256 rows at M = 16384; alpha = 0.25 with and without a
    device scalar of 2; out starts from random integers; both settings of the deterministic option, the second run twice."""
    lib = L.lib()
    g = _gen(50 + N + M)
    with case_log(f"colsum_bf16 N={N} M={M}") as log:
        for ld in (N, N + 8, 2 * N):
            X = _randint(g, -R.INT_RANGE, R.INT_RANGE, (M, ld), BF16)
            X[:, N:] = 30000.0
            out0 = _randint(g, -1000, 1000, (N,))
            for scalar in (None, 2.0):
                s = torch.tensor([scalar], device=dev) if scalar else None
                ref = out0.to(F64) + R.colsum(X, M, N, 0.25 * (scalar or 1.0))
                for det in (0, 1):
                    outs = []
                    for rep in range(2 if det else 1):
                        out = Guarded((N,), fill=out0)
                        with _mode(det):
                            L.check(_call(lib.bvc_op_colsum_bf16, G.ptr(X), M, N, ld, 0.25, G.ptr(s), G.ptr(out.t)), "colsum_bf16")
                        out.check(f"colsum_bf16 N={N} M={M} ld={ld} det={det}")
                        outs.append(out.t)
                    bad = outs[0].to(F64) != ref
                    assert not bool(bad.any()), (f"colsum_bf16 N={N} M={M} ld={ld} scalar={scalar} det={det}: {int(bad.sum())} columns wrong, "
                                                 f"first {int(bad.nonzero()[0])}: {float(outs[0][bad][0])} vs {float(ref[bad][0])}")
                    assert not det or _same_bits(outs[0], outs[1])
        log.note("out", "bit-exact")


def test_colsum_bf16_refusal():
    """N % 8 != 0 is refused by launch_colsum_bf16_scaled before the launch (in both modes)."""
    lib = L.lib()
    X = torch.ones(16, 16, device=dev, dtype=BF16)
    for det in (0, 1):
        out = Guarded((12,), fill=7.0)
        was = out.bits()
        with _mode(det):
            assert _call(lib.bvc_op_colsum_bf16, G.ptr(X), 16, 12, 16, 1.0, None, G.ptr(out.t)) != 0
        out.check("colsum_bf16 refusal")
        assert torch.equal(out.bits(), was)


@pytest.mark.parametrize("M", R.COLSUM_F32_M)
@pytest.mark.parametrize("D", R.COLSUM_F32_D)
def test_colsum_f32(D, M):
    """colsum_f32_kernel / colsum_f32_det_kernel by value: one lane (D = 4), a second grid column with one chunk (260), 384; rows
    around the 256-row block and 1000 (four blocks, the last short); dense rows and the row map m -> (m / 5) * 9 + 3 + m % 5 with
    large values in the unmapped rows; bit-exact on integers, within the f32 budget (torch's sum) on randn; both modes."""
    lib = L.lib()
    g = _gen(60 + D + M)
    with case_log(f"colsum_f32 D={D} M={M}") as log:
        for rmap in (None, (5, 9, 3)):
            P = R.physical_rows(M, rmap)
            rows = R.mapped_rows(M, rmap, dev)
            rm = rmap or (0, 0, 0)
            hole = torch.ones(P, dtype=torch.bool, device=dev)
            hole[rows] = False
            for exact in (True, False):
                X = _randint(g, -R.INT_RANGE, R.INT_RANGE, (P, D)) if exact else _randn(g, P, D)
                X[hole] = 4096.0
                out0 = _randint(g, -1000, 1000, (D,)) if exact else _randn(g, D)
                ref = out0.to(F64) + R.colsum(X, M, D, 1.0, rmap)
                for det in (0, 1):
                    outs = []
                    for rep in range(2 if det else 1):
                        out = Guarded((D,), fill=out0)
                        with _mode(det):
                            L.check(_call(lib.bvc_op_colsum_f32, G.ptr(X), *rm, M, D, G.ptr(out.t)), "colsum_f32")
                        out.check(f"colsum_f32 D={D} M={M} map={rmap} det={det}")
                        outs.append(out.t)
                    assert not det or _same_bits(outs[0], outs[1])
                    if exact:
                        assert torch.equal(outs[0].to(F64), ref), f"colsum_f32 D={D} M={M} map={rmap} det={det}: integers not exact"
                    else:
                        _f32_check(log, "out", outs[0], ref, out0 + X[rows].sum(0), scale=out0.to(F64).abs() + R.colsum_abs(X, M, D, 1.0, rmap))


# ---------------------------------------------------------------------------------------------- token mean
@pytest.mark.parametrize("N", R.TOKEN_MEAN_N)
def test_token_mean(N):
    """token_mean_kernel / token_mean_bwd_kernel for B in {1, 3} and D in {4, 68, 192, 1280} (one column group; a second grid column
    with one live group; three; twenty): N = 1 and 15 leave row phases empty, 16 fills each once, 17 / 197 / 1568 wrap.  Bit-exact on
    integers when N is a power of two (the division is then exact), within the budget of torch's mean otherwise; the backward
    against dmean / N broadcast."""
    lib = L.lib()
    g = _gen(70 + N)
    with case_log(f"token_mean N={N}") as log:
        for B in R.TOKEN_MEAN_B:
            for D in R.TOKEN_MEAN_D:
                tag = f"token_mean B={B} N={N} D={D}"
                for exact in ((True, False) if N & (N - 1) == 0 else (False,)):
                    x = _randint(g, -R.INT_RANGE, R.INT_RANGE, (B, N, D)) if exact else _randn(g, B, N, D) + 0.25
                    out = Guarded((B, D), row=D)
                    L.check(_call(lib.bvc_op_token_mean, G.ptr(x), B, N, D, G.ptr(out.t)), "token_mean")
                    out.check(tag)
                    ref = R.token_mean(x)
                    if exact:
                        assert torch.equal(out.t.to(F64), ref), f"{tag}: integers not exact"
                    else:
                        _f32_check(log, "mean", out.t.reshape(-1), ref.reshape(-1), x.mean(1).reshape(-1), scale=x.to(F64).abs().mean(1))
                dmean = _randn(g, B, D)
                dx = Guarded((B, N, D), row=D)
                L.check(_call(lib.bvc_op_token_mean_bwd, G.ptr(dmean), B, N, D, G.ptr(dx.t)), "token_mean_bwd")
                dx.check(tag + " bwd")
                ref = R.token_mean_bwd(dmean, N).reshape(B * N, D)
                _f32_check(log, "dx", dx.t.view(B * N, D), ref, (dmean / N)[:, None, :].expand(-1, N, -1).reshape(B * N, D))
                if N & (N - 1) == 0:
                    assert torch.equal(dx.t.view(B * N, D).to(F64), ref), f"{tag}: dmean / N with N a power of two is not exact"


# ---------------------------------------------------------------------------------------------- row normalisation
def _row_normalize_case(log, tag, f, dfn, eps, value_rows):
    """forward and backward of one [n][p] problem; fn / inv are checked on every row, df against the reference on `value_rows` and
    for finiteness everywhere."""
    lib = L.lib()
    n, p = f.shape
    fn, inv, df = Guarded((n, p), BF16, "nan", p), Guarded((n,)), Guarded((n, p), row=p)
    L.check(_call(lib.bvc_op_row_normalize, G.ptr(f), G.ptr(fn.t), G.ptr(inv.t), n, p, eps), "row_normalize")
    fn.check(tag + " fn")
    inv.check(tag + " inv")
    rfn, rinv = R.row_normalize(f, eps)
    tfn, tinv = R.row_normalize(f, eps, torch.float32)
    _f32_check(log, "inv", inv.t, rinv, tinv)
    _bf16_check(log, "fn", fn.t, rfn, tfn)
    L.check(_call(lib.bvc_op_row_normalize_bwd, G.ptr(f), G.ptr(inv.t), G.ptr(dfn), G.ptr(df.t), n, p), "row_normalize_bwd")
    df.check(tag + " df")
    assert bool(torch.isfinite(df.t).all()), f"{tag}: df is not finite"
    rdf, tdf = R.row_normalize_bwd(f, dfn, eps), R.row_normalize_bwd(f, dfn, eps, torch.float32)
    _f32_check(log, "df", df.t[value_rows], rdf[value_rows], tdf[value_rows])
    return fn.t, inv.t


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1025])
def test_row_normalize(n):
    """row_normalize_kernel / _bwd_kernel (one wave per row, four rows per workgroup): 1, 3, 4, 5 rows (dead waves, a second
    workgroup) and 1025; p = 4 (one lane), 128, 260 (lane 0 wraps) and 2048 (eight rounds).  inv within the f32 budget, fn within
    the bf16 bar, df within the budget of the same expression in float32."""
    g = _gen(80 + n)
    with case_log(f"row_normalize n={n}") as log:
        for p in (4, 128, 260, 2048):
            f, dfn = _randn(g, n, p) * 3, _randn(g, n, p)
            _row_normalize_case(log, f"row_normalize n={n} p={p}", f, dfn, 1e-8, torch.arange(n, device=dev))


@pytest.mark.parametrize("eps", [1e-8, 1e-3])
def test_row_normalize_clamp(eps):
    """The max(||f||, eps) clamp: a zero row gives fn == 0 and inv == 1/eps, a row of norm eps/4 gives fn = f/eps and inv == 1/eps, and
    the backward of both is finite.  (The backward of the zero row is dfn/eps and is held to the reference; that of the row below
    eps is held to finiteness only: the kernel keeps the unclamped formula there, which differs from the clamp's derivative by
    ||f||^2 / eps^2 relative.)"""
    g = _gen(90)
    e = R.f32_value(eps)
    with case_log(f"row_normalize clamp eps={eps:g}") as log:
        for p in (4, 128, 260, 2048):
            f, dfn = _randn(g, 5, p) * 3, _randn(g, 5, p)
            f[1] = 0
            f[3] = f[3] / f[3].norm() * (0.25 * e)
            fn, inv = _row_normalize_case(log, f"row_normalize clamp eps={eps:g} p={p}", f, dfn, eps, torch.tensor([0, 1, 2, 4], device=dev))
            assert _same_bits(fn[1], torch.zeros(p, device=dev, dtype=BF16)), "fn of a zero row"
            want = torch.tensor([1 / e, 1 / e], dtype=F64, device=dev)
            assert bool(((inv[[1, 3]].to(F64) - want).abs() <= 4 * R.ulp32(want)).all()), f"inv of a clamped row: {inv[[1, 3]].tolist()} vs {1 / e}"


# ---------------------------------------------------------------------------------------------- smooth-L1, EMA
def _seam_inputs(n, seed):
    """z, h with z - h a randn * 2 mix and, planted, differences of exactly 0, +-1 and the float32 neighbours of +-1 on both sides
    (h = 0 there, so z - h is exact), and +-1 from h = 2."""
    g = torch.Generator().manual_seed(seed)
    z, h = torch.randn(n, generator=g) * 2, torch.randn(n, generator=g)
    one = torch.tensor(1.0)
    up, dn = float(torch.nextafter(one, one * 2)), float(torch.nextafter(one, one * 0))
    plant = [(0.0, 0.0), (1.0, 0.0), (-1.0, 0.0), (up, 0.0), (-up, 0.0), (dn, 0.0), (-dn, 0.0), (3.0, 2.0), (1.0, 2.0)]
    if n >= 64:
        spots = list(range(9)) + list(range(n - 9, n))          # the head, and the scalar tail of the last thread
    else:
        spots = list(range(n))
    for j, i in enumerate(spots):
        z[i], h[i] = plant[(j + n) % 9]
    return z.to(dev), h.to(dev)


@pytest.mark.parametrize("n", R.FLAT_SIZES)
def test_smooth_l1(n):
    """smooth_l1_fwd_kernel / _bwd_kernel: n = 1, 2, 3 (scalar tail only), 4, 5, 1023 / 1024 / 1025 (a second workgroup of one
    element) and 2^20 + 3 (1024 workgroups on a grid stride, then the tail).  The loss against the float64 mean within the budget of
    F.smooth_l1_loss; dz per element within 2 ulp of gout / n * clamp(d) with gout = 1024, and exactly +-gout / n where |d| >= 1;
    the guard behind dz holds for every n % 4."""
    lib = L.lib()
    z, h = _seam_inputs(n, 100 + n)
    gout = torch.tensor([1024.0], device=dev)
    with case_log(f"smooth_l1 n={n}") as log:
        ws, loss = Guarded((int(lib.bvc_op_smooth_l1_workspace(n)),)), Guarded((1,))
        L.check(_call(lib.bvc_op_smooth_l1_fwd, G.ptr(z), G.ptr(h), n, G.ptr(ws.t), G.ptr(loss.t)), "smooth_l1_fwd")
        ws.check(f"smooth_l1 n={n} workspace")
        loss.check(f"smooth_l1 n={n} loss")
        _f32_check(log, "loss", loss.t[0], R.smooth_l1(z, h), F.smooth_l1_loss(z, h, beta=1.0))
        dz = Guarded((n,))
        L.check(_call(lib.bvc_op_smooth_l1_bwd, G.ptr(z), G.ptr(h), G.ptr(gout), n, G.ptr(dz.t)), "smooth_l1_bwd")
        dz.check(f"smooth_l1 n={n} dz")
        ref = R.smooth_l1_grad(z, h, 1024.0)
        _ulp_check(log, "dz", dz.t, ref, 2)
        d = z.to(F64) - h.to(F64)
        g32 = (torch.tensor(1024.0) / torch.tensor(float(n))).to(dev)         # the float32 quotient, correctly rounded
        hi, lo = d >= 1, d <= -1
        assert torch.equal(dz.t[hi], g32.expand(int(hi.sum()))) and torch.equal(dz.t[lo], (-g32).expand(int(lo.sum()))), \
            f"smooth_l1 n={n}: dz on the clamped side of the seam is not +-gout/n"
        assert bool((dz.t[d == 0] == 0).all())


@pytest.mark.parametrize("n", R.FLAT_SIZES)
def test_ema(n):
    """ema_kernel at the same sizes.  momentum 1 leaves the target bit-identical, 0 makes it bit-equal to the online weights, 0.996
    is within 2 ulp of the float64 value.  The online weights are the target moved by 1 % of its magnitude, as in training, so the
    two terms have one sign: the three roundings of m k + (1 - m) q are then each at most half an ulp of the result (1 - m is exact
    in float32), which is where the 2 comes from."""
    lib = L.lib()
    g = _gen(110 + n)
    k = _randn(g, n)
    q = k + 0.01 * _randn(g, n) * k.abs()
    with case_log(f"ema n={n}") as log:
        for m in (0.0, 0.996, 1.0):
            t = Guarded((n,), fill=k)
            L.check(_call(lib.bvc_op_ema, G.ptr(t.t), G.ptr(q), n, m), "ema")
            t.check(f"ema n={n} m={m}")
            if m == 1.0:
                assert _same_bits(t.t, k), f"ema n={n}: momentum 1 changed the target"
            elif m == 0.0:
                assert _same_bits(t.t, q), f"ema n={n}: momentum 0 is not the online weights"
            else:
                _ulp_check(log, "target", t.t, R.ema(k, q, m), 2)


# ---------------------------------------------------------------------------------------------- target selection, InfoNCE
@pytest.mark.parametrize("nsets,B,Np", [(4, 3, 5), (3, 3, 5)])
@pytest.mark.parametrize("D", [4, 192, 1024, 1028, 1408])
def test_target_select(D, nsets, B, Np):
    """target_select_kernel<4> (D = 4: one lane; 192; 1024: the top) and <6> (1028: first width; 1408: ViT-g) over 60 rows of
    4 mask sets x 3 clips x 5 tokens, and over 45 rows (not a multiple of the 4 rows of a workgroup): the clip of row m is
    (m / Np) % B.  L = 49; the index list holds 0, L - 1 and repeats.  Per row within the budget of F.layer_norm."""
    lib = L.lib()
    Lq, eps = 49, 1e-6
    rows = nsets * B * Np
    g = _gen(120 + D + rows)
    h = _randn(g, B * Lq, D) * 2 + 0.5
    idx = torch.randint(0, Lq, (rows,), generator=g, device=dev, dtype=torch.int32)
    idx[0], idx[1], idx[2], idx[3], idx[-2], idx[-1] = 0, Lq - 1, 7, 7, 0, Lq - 1
    with case_log(f"target_select D={D} rows={rows}") as log:
        out = Guarded((rows, D), row=D)
        L.check(_call(lib.bvc_op_target_select, G.ptr(h), G.ptr(idx), G.ptr(out.t), nsets, B, Np, Lq, D, eps), "target_select")
        out.check(f"target_select D={D} rows={rows}")
        ref = R.target_select(h, idx, nsets, B, Np, Lq, eps)
        b = (torch.arange(rows, device=dev) // Np) % B
        t32 = F.layer_norm(h, (D,), eps=R.f32_value(eps))[b * Lq + idx.long()]
        _f32_check(log, "out", out.t, ref, t32)


@pytest.mark.parametrize("ntiles", [1, 255, 256, 257, 1000])
def test_nce_finalize(ntiles):
    """nce_finalize_kernel (one workgroup, double accumulation): fewer partials than threads, exactly 256, one more, and four rounds.
    loss, stats[0] = lse = 1/T + log(sum) and stats[1] = -1/npos within 4 ulp of float64."""
    lib = L.lib()
    g = _gen(130 + ntiles)
    partial = torch.rand(2 * ntiles, generator=g, device=dev) * 3 + 0.05
    inv_t, npos = 1 / 0.07, 2 * ntiles + 2
    with case_log(f"nce_finalize ntiles={ntiles}") as log:
        loss, stats = Guarded((1,)), Guarded((2,))
        L.check(_call(lib.bvc_op_nce_finalize, G.ptr(partial), ntiles, inv_t, npos, G.ptr(loss.t), G.ptr(stats.t)), "nce_finalize")
        loss.check("nce loss")
        stats.check("nce stats")
        rl, rlse, rneg = R.nce_finalize(partial, ntiles, inv_t, npos)
        _ulp_check(log, "loss", loss.t, torch.tensor([rl], dtype=F64, device=dev), 4)
        _ulp_check(log, "stats", stats.t, torch.tensor([rlse, rneg], dtype=F64, device=dev), 4)


# ---------------------------------------------------------------------------------------------- pixel targets, patch gather
TOKEN_COUNTS = ((1, 1), (3, 1), (1, 7), (2, 4), (3, 3), (3, 7))          # (clips, tokens per clip): 1, 3, 7, 8, 9, 21 tokens


def _token_lists(B, n, Ltok, g):
    """[B][n] distinct tokens per clip, unordered, the first and the last token of a clip among them."""
    out = torch.empty(B, n, dtype=torch.int32)
    for b in range(B):
        if n == 1:
            out[b, 0] = (0, Ltok - 1, Ltok // 2)[b % 3]
        else:
            mid = torch.randperm(Ltok - 2, generator=g)[:n - 2] + 1
            out[b] = torch.cat([torch.tensor([Ltok - 1]), mid, torch.tensor([0])]).to(torch.int32)
    return out.to(dev)


@pytest.mark.parametrize("C,ts,ps", [(3, 2, 16), (3, 1, 16), (3, 2, 8), (1, 2, 32), (3, 4, 16), (3, 2, 32)])
def test_pixel_labels_and_gather(C, ts, ps):
    """One geometry per branch of launch_labels, on 64 x 96 frames (H != W) of two tubes in time:
      (3, 2, 16)  labels_wave3_kernel<2> (E = 512)          (3, 1, 16)  labels_wave3_kernel<1> (E = 256)
      (3, 2, 8)   labels_wave_kernel<6> (96 chunks)         (1, 2, 32)  labels_wave_kernel<8> (512 chunks, no un-normalisation)
      (3, 4, 16), (3, 2, 32)  labels_kernel, a workgroup per token (768 and 1536 chunks)
    each with norm_pix 0 and 1 and with 1, 3, 7, 8, 9 and 21 tokens, so that the XCD-ordered token walk has a remainder and fewer
    workgroups than XCDs; every clip's list holds its first and its last token.  Targets per token within the budget of the same
    formula in float32; gather_patches_kernel on the same lists is bit-exact against the unfold."""
    lib = L.lib()
    T, H, W = 2 * ts, 64, 96
    Ltok = (T // ts) * (H // ps) * (W // ps)
    K = C * ts * ps * ps
    cg = torch.Generator().manual_seed(140 + C + ts + ps)
    with case_log(f"pixel_labels C={C} ts={ts} ps={ps}") as log:
        for B, n in TOKEN_COUNTS:
            clip = _randn(_gen(150 + B + n), B, T, C, H, W)
            idx = _token_lists(B, n, Ltok, cg)
            tag = f"C={C} ts={ts} ps={ps} tokens={B}x{n}"
            A = Guarded((B * n, K), BF16, "nan", K)
            L.check(_call(lib.bvc_op_gather_patches, G.ptr(clip), G.ptr(idx), G.ptr(A.t), B, n, T, C, H, W, ts, ps), "gather_patches")
            A.check("gather_patches " + tag)
            assert _same_bits(A.t, R.gather_patches(clip, idx, ts, ps).to(BF16)), f"gather_patches {tag}: not the unfold"
            for norm_pix in (0, 1):
                lab = Guarded((B * n, K), row=K)
                L.check(_call(lib.bvc_op_pixel_labels, G.ptr(clip), G.ptr(idx), G.ptr(lab.t), B, n, T, C, H, W, ts, ps, norm_pix), "pixel_labels")
                lab.check(f"pixel_labels {tag} norm_pix={norm_pix}")
                _f32_check(log, f"norm_pix={norm_pix}", lab.t, R.pixel_labels(clip, idx, ts, ps, norm_pix),
                           R.pixel_labels(clip, idx, ts, ps, norm_pix, torch.float32))
