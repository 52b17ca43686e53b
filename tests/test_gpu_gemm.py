"""The GEMM kernels (csrc/gemm.hip, gemm_persist.hip, gemm8.hip, gemm_as.hip) through the C ABI, each against the float64
references of tests/gemm_ref.py (tests/test_gemm_ref.py pins those on the CPU).

Common rules of this file
  * Guard bands and gaps.  Every output, second output, partial buffer and rowsum is the payload of a `Guarded` buffer
    [guard | rows x ldc | guard]; with ldc > N the columns [N, ldc) of every row hold the guard pattern too.  Outputs the call must
    overwrite start as NaN, accumulated ones from random values.  Guards, gaps and EPI_E2D's untouched rows must be bit-identical
    after the call.
  * Bars are per element against float64.  f32 outputs: 4 x the worst error, relative to the element's scale, that torch's own
    float32 product of the same operands shows against the same reference in that case, at least 4 ulp of the scale.  The scale of
    element (m, n) is |alpha| sum_k |a||b| plus the magnitudes of its addends.  bf16 outputs: 2^-8 |ref| plus that room.  The two
    GELU outputs also get the erf approximation's 1.5e-7, propagated (gemm_ref.gelu_erf_room); their scales are 1.13 x the
    pre-activation's for gelu (its Lipschitz constant) and 1.13 + the pre-activation's for gelu' (|gelu'| <= 1.13, |gelu''| < 1).
    Sums of squares (EPI_LOSS partials) and of exponentials (EPI_NCE) get 4 x torch-f32's error of the same sum plus the room of
    their terms, propagated.  No number is fixed in advance; one parity-report line per case (profiles/gemm_parity_report.txt is a copy).
  * Exact cases.  Integer operands in [-8, 8], alpha a power of two, integer addends: every partial sum is exact in float32 in any
    order (64 K < 2^24; tests/test_gemm_ref.py), so f32 outputs equal the reference bit for bit and bf16 outputs its
    round-to-nearest-even.
  * Strided equals contiguous.  Every non-atomic case runs with contiguous operands and outputs and again with lda, ldb, ldc, ldaux
    8, 24 or 72 wider than the row, NaN in the operand gaps and a_bytes / b_bytes from the first to the last element used: bit-identical.
  * Branch reached.  Before each launch bvc_op_gemm_kernel / bvc_op_gemm_gate_kernel names the instantiation; the case asserts it.
"""
import contextlib
import ctypes
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():   # collected on the CPU box, run on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gemm_ref as R     # noqa: E402
from tests import gpu_util as G     # noqa: E402

L = G.L
bvc = G.bvc
dev = "cuda"
F64, BF16, F32 = torch.float64, torch.bfloat16, torch.float32
NT, NN, TN = G.NT, G.NN, G.TN
LAYOUT_NAME = {NT: "NT", NN: "NN", TN: "TN"}
CONTIG = (0, 0, 0, 0)
PADS = ((8, 24, 72, 8), (24, 72, 8, 24), (72, 8, 24, 72))       # (lda, ldb, ldc, ldaux) beyond the row
BF16_OUT = {"BF16", "GELU", "LOSS", "DGELU", "RELU", "DRELU", "NCE_BWD"}


@contextlib.contextmanager
def case_log(name):
    log = R.CaseLog(name)
    t0 = time.perf_counter()
    try:
        yield log
    finally:
        log.note("wall", f"{time.perf_counter() - t0:.2f} s")
        G.log_parity(log.line())


@contextlib.contextmanager
def _option(name, value):
    old = L.set_option(name, value)
    try:
        yield
    finally:
        L.set_option(name, old)


@contextlib.contextmanager
def _det(on):
    """the `deterministic` option, set and restored as tests/test_gpu_deterministic.py does"""
    bvc.use_deterministic_algorithms(bool(on))
    try:
        assert L.lib().bvc_get_option(b"deterministic") == int(bool(on))
        yield
    finally:
        bvc.use_deterministic_algorithms(False)
        L.lib()


def _tf(b):
    return "true" if b else "false"


def kernel_name(layout, tile, stages=2, det=False):
    """the instantiation of gemm_kernel / gemm_det_kernel launch_gemm runs for tile configs 0 / 1 / 2"""
    bm, bn = R.TILES[tile]
    at, bt = layout == TN, layout != NT
    if det:
        return f"bvc::gemm_det_kernel<{bm}, {bn}, {_tf(at)}, {_tf(bt)}>"
    lb = 1 if (stages == 3 and layout == TN) else 2
    return f"bvc::gemm_kernel<{bm}, {bn}, {_tf(at)}, {_tf(bt)}, 2, {lb}, {_tf(stages != 4)}>"


# ---------------------------------------------------------------------------------------------- one problem: inputs, references
class Case:
    def __init__(self, layout, M, N, K, epi="F32", exact=False, alpha=1.0, alpha_dev=None, bias=False, split=1, start=False,
                 rowsum=False, rin=0, rout=0, seed=0, accum=False):
        self.layout, self.M, self.N, self.K, self.epi, self.exact = layout, M, N, K, epi, exact
        self.alpha, self.alpha_dev, self.bias, self.split, self.start, self.rowsum = alpha, alpha_dev, bias, split, start, rowsum
        self.rin, self.rout, self.seed = rin, rout, seed
        # an f32 output ADDS onto what C held when K is split (f32 atomics / the deterministic reduce) or on tile config 13 (`accum`);
        # an unsplit problem overwrites C, whatever it held
        self.adds = start and (split > 1 or accum)
        if exact:
            assert R.product_is_exact(K, alpha * (alpha_dev or 1.0), 3) and (M, N, K) in R.EXACT_SHAPES, (M, N, K)
        self.tag = f"{LAYOUT_NAME[layout]} {M}x{N}x{K} {epi}{' exact' if exact else ''}{f' split{split}' if split > 1 else ''}"
        self._make()

    def _int(self, g, lo, hi, shape, dtype=F32):
        return torch.randint(lo, hi + 1, shape, generator=g, device=dev, dtype=torch.int32).to(dtype)

    def _f32(self, g, *shape):
        return self._int(g, -R.EXACT_ADDEND, R.EXACT_ADDEND, shape) if self.exact else torch.randn(*shape, generator=g, device=dev)

    def _make(self):
        M, N, K, epi = self.M, self.N, self.K, self.epi
        g = torch.Generator(device=dev).manual_seed(1000 + self.seed + 7 * M + 3 * N + K)
        (ra, wa), (rb, wb) = R.storage_shapes(self.layout, M, N, K)
        if self.exact:
            self.A, self.B = self._int(g, -8, 8, (ra, wa), BF16), self._int(g, -8, 8, (rb, wb), BF16)
        elif epi in ("NCE", "NCE_BWD"):        # rows of unit length: the product is a cosine
            f = torch.randn(ra, wa, generator=g, device=dev)
            self.A = self.B = (f / f.norm(dim=1, keepdim=True)).to(BF16)
        else:
            self.A = torch.randn(ra, wa, generator=g, device=dev).to(BF16)
            self.B = (torch.randn(rb, wb, generator=g, device=dev) * K ** -0.5).to(BF16)
        self.adev = torch.tensor([self.alpha_dev], device=dev) if self.alpha_dev is not None else None
        self.biasv = self._f32(g, N) if self.bias else None
        self.resid = self._f32(g, M, N) if epi == "RESID" else None
        self.c0 = self._f32(g, M, N) if self.adds else None
        self.rs0 = self._f32(g, M) if self.rowsum else None
        self.labels = self._f32(g, M, N) if epi == "LOSS" else None
        self.pos = self._f32(g, 37, N) if epi in ("POS", "E2D") else None
        self.rowtok = torch.randint(0, 37, (M,), generator=g, device=dev, dtype=torch.int32) if epi in ("POS", "E2D") else None
        self.aux = None
        if epi == "DGELU":
            self.aux = self._int(g, -8, 8, (M, N), BF16) if self.exact else torch.randn(M, N, generator=g, device=dev).to(BF16)
        if epi == "DRELU":      # +0.0, -0.0, the smallest positive bf16, the smallest negative, ordinary, large and infinite values of both signs
            table = torch.tensor([0x0000, 0x8000, 0x0001, 0x8001, 0x3F80, 0xBF80, 0x4060, 0xC060, 0x7F00, 0xFF00, 0x7F80, 0xFF80, 0x0080, 0x8080],
                                 dtype=torch.int32, device=dev)
            pick = torch.randint(0, len(table), (M, N), generator=g, device=dev)
            pick[0, :min(N, len(table))] = torch.arange(min(N, len(table)), device=dev)        # each of them in the first row, at least
            self.aux = table[pick].to(torch.int16).view(BF16)
        if epi == "NCE_BWD":
            self.labels = torch.tensor([float(self.alpha) + 3.0, -1.0 / (2 * M - 2)], device=dev)      # {lse, pos_coef}
        self._refs = {}

    def refs(self, bm, bn):
        """{output: (kind, ref, t32, scale, extra)}: float64 reference, torch-f32 result, element scale; once per tile shape."""
        if (bm, bn) in self._refs:
            return self._refs[(bm, bn)]
        M, N, K, epi = self.M, self.N, self.K, self.epi
        if not hasattr(self, "_v"):
            acc, absacc = R.product(self.A, self.B, self.layout, M, N, K)
            acc32 = R.product_f32(self.A, self.B, self.layout, M, N, K)
            atot = abs(R.f32_value(self.alpha) * (self.alpha_dev or 1.0))
            self._v = (R.scaled(acc, self.alpha, self.alpha_dev, self.biasv), R.scaled(acc32, self.alpha, self.alpha_dev, self.biasv),
                       atot * absacc + (self.biasv.to(F64).abs()[None, :] if self.bias else 0))
        v, v32, sv = self._v
        out = {}
        if epi in ("F32", "BF16", "F32_BF16"):
            r, t, s = v, v32, sv
            if self.adds:
                r, t, s = v + self.c0.to(F64), v32 + self.c0, sv + self.c0.to(F64).abs()
            out["C"] = ("bf16" if epi == "BF16" else "f32", r, t, s, None)
            if epi == "F32_BF16":
                out["C2"] = ("bf16", r, t, s, None)
        elif epi == "RESID":
            out["C"] = ("f32", R.epi_resid(v, self.resid), v32 + self.resid, sv + self.resid.to(F64).abs(), None)
        elif epi in ("POS", "E2D"):
            out["C"] = ("f32", R.epi_pos(v, self.pos, self.rowtok), v32 + self.pos[self.rowtok.long()],
                        sv + self.pos.to(F64).abs()[self.rowtok.long()], None)
        elif epi == "RELU":
            out["C"] = ("bf16", R.epi_relu(v), v32.clamp_min(0), sv, None)
        elif epi == "GELU":
            (rg, ra), (tg, ta), (eg, ea) = R.epi_gelu(v), R.epi_gelu(v32), R.gelu_erf_room(v)
            out["C"] = ("bf16", rg, tg, 1.13 + sv, eg)
            out["C2"] = ("bf16", ra, ta, 1.13 * sv, ea)
        elif epi == "DGELU":
            out["C"] = ("bf16", R.epi_dgelu(v, self.aux), v32 * self.aux.float(), sv * self.aux.to(F64).abs(), None)
        elif epi == "DRELU":
            gate = R.drelu_gate(self.aux)
            out["C"] = ("bf16", R.epi_drelu(v, self.aux), v32 * gate, sv, None)
        elif epi == "LOSS":
            d, logits, part = R.epi_loss(v, self.labels, bm, bn)
            d32 = v32 - self.labels
            sd = sv + self.labels.to(F64).abs()
            out["C"] = ("bf16", d, d32, sd, None)
            out["C2"] = ("f32", logits, v32, sv, None)
            room_d, _ = R.f32_room(d, d32, sd)
            out["partial"] = ("f32", part, R.tile_sums(d32 * d32, bm, bn), part, R.tile_sums(2 * d.abs() * room_d, bm, bn))
        elif epi == "NCE":
            inv_t = R.f32_value(self.alpha) * (self.alpha_dev or 1.0)
            part = R.epi_nce(v, inv_t, bm, bn)
            t32 = R.epi_nce(v32, inv_t, bm, bn)
            pos, neg = R.nce_masks(M, N, dev)
            room_v, _ = R.f32_room(v, v32, sv)
            scale = torch.stack([part[0::2], R.tile_sums(sv * pos, bm, bn)], 1).reshape(-1)
            extra = torch.stack([R.tile_sums(torch.exp(v - inv_t) * neg * room_v, bm, bn), torch.zeros_like(part[0::2])], 1).reshape(-1)
            out["partial"] = ("f32", part, t32, scale, extra)
        elif epi == "NCE_BWD":
            lse, pc = float(self.labels[0]), float(self.labels[1])
            pos, neg = R.nce_masks(M, N, dev)
            r = R.epi_nce_bwd(v, lse, pc)
            out["C"] = ("bf16", r, R.epi_nce_bwd(v32, lse, pc), torch.exp(v - lse) * (1 + sv) * neg + abs(pc) * pos, None)
        if self.rowsum:
            r, s = R.rowsum(self.A, M, K, self.alpha, self.alpha_dev)
            a32 = self.A.float()[:K, :M].sum(0) * (R.f32_value(self.alpha) * (self.alpha_dev or 1.0))
            out["rowsum"] = ("f32", r + self.rs0.to(F64), a32 + self.rs0, s + self.rs0.to(F64).abs(), None)
        self._refs[(bm, bn)] = out
        return out

    def out_rows(self):
        return (self.M + self.rin - 1) // self.rin * self.rout if self.epi == "E2D" else self.M


def _lay(data, ld_extra):
    """(tensor view, ld, bytes) of a dense 2-D tensor stored with rows ld_extra wider, NaN in the gaps"""
    view, nbytes = R.strided(data, data.shape[1] + ld_extra)
    return view, data.shape[1] + ld_extra, nbytes


def build(c, pads, tile):
    """descriptor and guarded outputs of one problem"""
    pa, pb, pc, paux = pads
    M, N, K, epi = c.M, c.N, c.K, c.epi
    E = G.EPI[epi]
    A, lda, ab = _lay(c.A, pa)
    B, ldb, bb = _lay(c.B, pb) if c.B is not c.A else (A, lda, ab)
    ldc = N + pc
    keep = [A, B]
    outs = {}
    cdt = BF16 if epi in BF16_OUT else F32
    if epi == "NCE":
        Cg = None
    else:
        fill = c.c0 if c.adds else (c.resid if (epi == "RESID" and c.split > 1) else "nan")
        Cg = outs["C"] = R.Guarded(c.out_rows(), N, ldc, cdt, fill)
    if epi in ("GELU", "F32_BF16", "LOSS"):
        outs["C2"] = R.Guarded(M, N, ldc, F32 if epi == "LOSS" else BF16)
    kw = {}
    if epi == "RESID":
        if c.split > 1:
            kw["resid"] = Cg.t
        else:
            kw["resid"] = _lay(c.resid, pc)[0]
    if epi == "LOSS":
        kw["labels"] = _lay(c.labels, pc)[0]
    if epi == "NCE_BWD":
        kw["labels"] = c.labels
    if epi in ("POS", "E2D"):
        kw.update(pos=c.pos, rowtok=c.rowtok)
    if c.aux is not None:
        kw["aux"] = _lay(c.aux, paux)[0]
    if c.rowsum:
        outs["rowsum"] = R.Guarded(1, M, fill=c.rs0)
        kw["rowsum"] = outs["rowsum"].t
    keep += list(kw.values())
    d = G.gemm_desc(A, B, M, N, K, E, Cg.t if Cg is not None else A, ldc=ldc, lda=lda, ldb=ldb, alpha=c.alpha, alpha_dev=c.adev, split_k=c.split,
                    C2=outs["C2"].t if "C2" in outs else None, bias=c.biasv, rin=c.rin, rout=c.rout, **kw)
    d.a_bytes, d.b_bytes = ab, bb
    if c.aux is not None:
        d.ldaux = N + paux
    if epi == "NCE":
        d.C = None
    if epi in ("LOSS", "NCE"):
        bm, bn = R.TILES[tile]
        nt = ((M + bm - 1) // bm) * ((N + bn - 1) // bn)
        assert L.lib().bvc_op_gemm_num_tiles(ctypes.byref(d), tile) == nt
        outs["partial"] = R.Guarded(1, nt * (2 if epi == "NCE" else 1))
        d.partial = outs["partial"].t.data_ptr()
    return d, outs, keep


def launch(cases, tile, stages=-1, pads=CONTIG, expect=None, tag=""):
    """One bvc_op_gemm call over the problems of `cases` (one layout); asserts the instantiation, checks every guard and gap and
    returns, per problem, {output: dense copy}."""
    layout = cases[0].layout
    built = [build(c, pads, tile) for c in cases]
    descs = [b[0] for b in built]
    name = G.gemm_kernel_name(descs, layout, tile, stages)
    if expect is not None:
        assert name == expect, f"{tag}: runs {name}, meant for {expect}"
    before = [b[1]["C"].bits() if c.epi == "E2D" else None for c, b in zip(cases, built)]
    G.run_gemm(descs, layout, tile, stages)
    torch.cuda.synchronize()
    res = []
    for c, (d, outs, keep), was in zip(cases, built, before):
        for k, gb in outs.items():
            gb.check(f"{tag} {c.tag} tile {tile} pads {pads} {k}")
        got = {k: gb.t.clone() for k, gb in outs.items()}
        if c.epi == "E2D":
            R.rows_unchanged(was, outs["C"].bits(), R.e2d_untouched(c.M, c.rin, c.rout, c.out_rows()), f"{tag} {c.tag} tile {tile}")
            got["C"] = outs["C"].t[R.e2d_rows(c.M, c.rin, c.rout).to(dev)].clone()
        res.append(got)
    return res


def check(log, c, got, tile, what):
    bm, bn = R.TILES[tile]
    for k, (kind, ref, t32, scale, extra) in c.refs(bm, bn).items():
        key = f"{c.epi}.{k}" if k != "C" else c.epi
        try:
            (R.check_bf16 if kind == "bf16" else R.check_f32)(log, key, got[k].reshape(ref.shape), ref, t32, scale, extra)
            if c.exact and c.epi not in ("GELU", "NCE", "NCE_BWD") and k != "partial":
                R.check_exact(key, got[k].reshape(ref.shape), ref, kind == "bf16")
        except AssertionError as e:
            raise AssertionError(f"{what} {c.tag} tile {tile}: {e}") from None


def same(a, b, what):
    for k in a:
        assert R.same_bits(a[k], b[k]), f"{what}: output {k} differs bit for bit"


# ---------------------------------------------------------------------------------------------- 1. gemm_kernel
ALL_EPIS = ("F32", "BF16", "GELU", "RESID", "POS", "E2D", "LOSS", "DGELU", "F32_BF16", "RELU", "DRELU")
EPIS = {NT: ALL_EPIS, NN: ALL_EPIS, TN: ALL_EPIS}       # (launch_gemm admits each of them in every layout; NCE / NCE_BWD: test_nce_epilogues)
SWEEP = [(lay, s) for lay in (NT, NN, TN) for s in R.SWEEP_SHAPES] + [(TN, (264, 200, K)) for K in R.TN_RAGGED_K]


def _case(layout, M, N, K, epi, exact, seed=0, **kw):
    e2d = dict(rin=5, rout=9) if epi == "E2D" else {}
    bias = epi in ("F32", "BF16", "GELU", "RESID", "POS", "LOSS", "RELU")
    return Case(layout, M, N, K, epi, exact, alpha=0.5 if exact else 0.75, alpha_dev=2.0 if epi in ("F32_BF16", "RESID") else None,
                bias=bias, seed=seed, **e2d, **kw)


@pytest.mark.parametrize("layout,shape", SWEEP, ids=[f"{LAYOUT_NAME[l]}-{s[0]}x{s[1]}x{s[2]}" for l, s in SWEEP])
def test_gemm_kernel_tiles_stages_epilogues(layout, shape):
    """gemm_kernel<128,128> / <128,64> / <64,64> x the three K-loop forms (stages 2: early refill; 3: the one-workgroup form for TN;
    4: the plain double buffer) x every epilogue, in each layout, on (8, 8) (one partial tile), (136, 72) (ragged on every
    tile shape) and (264, 200) with 1, 2, 3 and 10 K steps (prologue shorter than the ring, the counted-wait tail); TN also with
    K = 1, 63, 65, 200 (contraction rows past K read as zero through a_bytes / b_bytes).  Each (epilogue, tile, stages) runs an
    integer case (bit-exact) and a Gaussian one (bars), contiguous and strided (bit-identical)."""
    M, N, K = shape
    with case_log(f"gemm_kernel {LAYOUT_NAME[layout]} {M}x{N}x{K}") as log:
        n = 0
        for epi in EPIS[layout]:
            for exact in (True, False):
                c = _case(layout, M, N, K, epi, exact)
                for tile in (0, 1, 2):
                    for stages in (2, 3, 4):
                        want = kernel_name(layout, tile, stages)
                        a = launch([c], tile, stages, CONTIG, want, "contiguous")[0]
                        b = launch([c], tile, stages, PADS[n % 3], want, "strided")[0]
                        n += 1
                        same(a, b, f"{c.tag} tile {tile} stages {stages}: strided vs contiguous")
                        check(log, c, a, tile, f"stages {stages}")


SPLITS = [(TN, 264, 200, 640, 2), (TN, 264, 200, 640, 3), (TN, 264, 200, 640, 7), (TN, 264, 200, 128, 3), (TN, 264, 200, 200, 7),
          (NT, 264, 200, 640, 3), (NT, 264, 200, 128, 7), (NN, 136, 72, 192, 2)]


def _split_cases(layout, M, N, K, split, exact):
    yield Case(layout, M, N, K, "F32", exact, alpha=0.5, alpha_dev=2.0, bias=True, split=split, start=True, rowsum=layout == TN, seed=1)
    yield Case(layout, M, N, K, "RESID", exact, alpha=0.5, bias=True, split=split, seed=2)


@pytest.mark.parametrize("layout,M,N,K,split", SPLITS, ids=[f"{LAYOUT_NAME[s[0]]}-{s[1]}x{s[2]}x{s[3]}-split{s[4]}" for s in SPLITS])
def test_split_k_and_deterministic_forms(layout, M, N, K, split):
    """Split-K 2, 3 and 7 on tiles 0 / 1 / 2, with splits that leave a K range empty (K = 128 in 3 or 7, 200 in 7): f32 atomics onto
    random start values with the bias added exactly once, in-place RESID, and for TN the fused bias gradient (rowsum).  Default
    mode: within the bars, bit-exact on integers, ldc > N.  deterministic = 1 (gemm_det_kernel + det_reduce_kernel): the same, two
    runs bit-identical, strided bit-identical to contiguous, and the outputs' gaps checked after the reduce."""
    with case_log(f"split_k {LAYOUT_NAME[layout]} {M}x{N}x{K} split {split}") as log:
        for exact in ((True, False) if R.product_is_exact(K, 1.0, 3) and (M, N, K) in R.EXACT_SHAPES else (False,)):
            for c in _split_cases(layout, M, N, K, split, exact):
                for tile in (0, 1, 2):
                    for pads in (CONTIG, PADS[tile]):
                        check(log, c, launch([c], tile, -1, pads, kernel_name(layout, tile), "atomic")[0], tile, "atomic")
                    with _det(True):
                        want = kernel_name(layout, tile, det=True)
                        runs = [launch([c], tile, -1, p, want, "deterministic")[0] for p in (CONTIG, CONTIG, PADS[tile])]
                    same(runs[0], runs[1], f"{c.tag} tile {tile}: two deterministic runs")
                    same(runs[0], runs[2], f"{c.tag} tile {tile}: deterministic strided vs contiguous")
                    check(log, c, runs[0], tile, "deterministic")


@pytest.mark.parametrize("nprob", [2, 4])
def test_grouped_weight_gradients(nprob):
    """Groups of 2 and 4 TN problems of unequal shapes and mixed split_k in one launch, each with a fused bias gradient, on tiles
    0 / 1 / 2, default and deterministic (and tiles 10 / 11 / 12 / 13 of gemm8.hip in test_gemm8_weight_gradient_groups)."""
    shapes = [(136, 72, 192, 1), (264, 200, 640, 3), (8, 8, 64, 2), (264, 200, 200, 1)][:nprob]
    with case_log(f"grouped TN x{nprob}") as log:
        for exact in (True, False):
            cs = [Case(TN, M, N, K, "F32", exact, alpha=0.5, split=s, start=True, rowsum=True, seed=10 + i) for i, (M, N, K, s) in enumerate(shapes)]
            for tile in (0, 1, 2):
                for det in (False, True):
                    with _det(det):
                        res = launch(cs, tile, -1, PADS[tile], kernel_name(TN, tile, det=det), f"group det={det}")
                        again = launch(cs, tile, -1, CONTIG, kernel_name(TN, tile, det=det), f"group det={det}") if det else None
                    for i, c in enumerate(cs):
                        check(log, c, res[i], tile, f"group det={det}")
                        if det:
                            same(res[i], again[i], f"{c.tag}: deterministic group, strided vs contiguous")


# ---------------------------------------------------------------------------------------------- 7. RELU / DRELU / NCE / NCE_BWD
@pytest.mark.parametrize("n", [72, 264])
def test_nce_epilogues(n):
    """EPI_NCE / EPI_NCE_BWD on the 2B x 2B similarity matrix (2B = 72: one ragged tile; 264: the diagonal crosses tile corners) of
    unit rows, alpha = 1 / T with T = 0.07: each of the two partials of each tile against float64, the gradient per element, on
    tiles 0 / 1 / 2; no partial past bvc_op_gemm_num_tiles may be written (guards)."""
    with case_log(f"nce 2B={n}") as log:
        for epi in ("NCE", "NCE_BWD"):
            c = Case(NT, n, n, 128, epi, False, alpha=1 / 0.07, seed=3)
            for tile in (0, 1, 2):
                a = launch([c], tile, 2, CONTIG, kernel_name(NT, tile), epi)[0]
                b = launch([c], tile, 2, PADS[tile], kernel_name(NT, tile), epi)[0]
                same(a, b, f"{c.tag} tile {tile}: strided vs contiguous")
                check(log, c, a, tile, epi)


def test_drelu_gate_values():
    """EPI_DRELU decodes sign and zero of the packed bf16 aux by hand: with v = 1 everywhere (A = ones, B = one-hot / K) the output
    must be exactly 1 where aux is the smallest positive bf16, an ordinary, large or infinite positive value, and exactly +0 where aux
    is +0.0, -0.0 or negative - on gemm_kernel (tiles 0 / 1 / 2) and on gemm8 class 3 (tile 10)."""
    M, N, K = 200, 192, 256
    A = torch.ones(M, K, device=dev, dtype=BF16)
    W = torch.full((K, N), 1.0 / K, device=dev, dtype=BF16)
    c = Case(NN, M, N, K, "DRELU", False, seed=4)
    gate = R.drelu_gate(c.aux)
    assert bool(gate[0, 2]) and not bool(gate[0, 0]) and not bool(gate[0, 1]) and not bool(gate[0, 3])      # 0x0001 opens; +0, -0, -tiny close
    for tile, want in ((0, kernel_name(NN, 0)), (1, kernel_name(NN, 1)), (2, kernel_name(NN, 2)), (10, "bvc::gemm8_kernel<256, 256, false, true, 3>")):
        for pads in (CONTIG, PADS[0]):
            out = R.Guarded(M, N, N + pads[2], BF16)
            aux, _ = R.strided(c.aux, N + pads[3])
            d = G.gemm_desc(A, W, M, N, K, G.EPI["DRELU"], out.t, ldc=N + pads[2], lda=K, ldb=N, aux=aux)
            d.ldaux = N + pads[3]
            stages = 2 if tile < 10 else -1
            assert G.gemm_kernel_name(d, NN, tile, stages) == want
            G.run_gemm([d], NN, tile, stages)
            torch.cuda.synchronize()
            out.check(f"drelu tile {tile}")
            assert R.same_bits(out.t, gate.to(BF16)), f"drelu tile {tile} pads {pads}: the gate is not (aux > 0) on the bf16 bits"


# ---------------------------------------------------------------------------------------------- 3. persistent kernel
PERSIST = [(6, R.PERSIST_SHAPES[0], 0), (9, R.PERSIST_SHAPES[0], 0), (7, R.PERSIST_SHAPES[1], 1)]


@pytest.mark.parametrize("tile,shape,base", PERSIST, ids=["tile6", "tile9", "tile7"])
def test_persistent_kernel(tile, shape, base):
    """gemm_persist_kernel on the smallest products it accepts (1056 / 1089 tiles, ragged last row and column, K = 128 / 192) with
    every epilogue it takes (tile config 9: the bf16-output ones), NT and NN: within the bars, bit-exact on integers, bitwise equal
    to the per-tile kernel of the same tile shape, strided equal to contiguous."""
    M, N, K = shape
    with case_log(f"persistent tile {tile} {M}x{N}x{K}") as log:
        for layout in (NT, NN):
            for epi in (("BF16", "GELU", "DGELU") if tile == 9 else ("F32", "BF16", "GELU", "RESID", "DGELU", "F32_BF16")):
                for exact in (True, False):
                    c = _case(layout, M, N, K, epi, exact)
                    defer = 0 if tile != 9 else 2 if epi == "GELU" else 1          # (the deferred-store form has a GELU instantiation of its own)
                    want = f"bvc::gemm_persist_kernel<{R.TILES[tile][1]}, {_tf(layout == NN)}, {defer}>"
                    a = launch([c], tile, -1, CONTIG, want, "persistent")[0]
                    same(a, launch([c], tile, -1, PADS[1], want, "persistent strided")[0], f"{c.tag} tile {tile}: strided vs contiguous")
                    same(a, launch([c], base, 2, CONTIG, kernel_name(layout, base), "per-tile")[0], f"{c.tag}: tile {tile} vs tile {base}")
                    check(log, c, a, tile, "persistent")


def test_persistent_auto_route_and_refusal():
    """The auto route takes an eligible product to the persistent kernel; tile configs 6 / 7 / 9 refuse an ineligible one (too few
    tiles; K < 128; a layout or epilogue it does not take) with an error and leave the output as it was."""
    M, N, K = R.PERSIST_SHAPES[0]
    c = _case(NT, M, N, K, "RESID", True)
    with _option("gemm8", -1):
        a = launch([c], -1, -1, CONTIG, "bvc::gemm_persist_kernel<128, false, 0>", "auto")[0]
    check(None, c, a, 0, "auto route")
    for cc, tile in ((_case(NT, 264, 200, 128, "F32", False), 6), (_case(NT, 264, 200, 64, "F32", False), 7),
                     (_case(TN, 264, 200, 128, "F32", False), 6), (_case(NT, 264, 200, 128, "RELU", False), 9)):
        d, outs, keep = build(cc, CONTIG, tile)
        was = outs["C"].bits()
        arr = (L.GemmDesc * 1)(d)
        assert L.lib().bvc_op_gemm(arr, 1, cc.layout, tile, -1, G.stream()) != 0
        assert b"persistent" in L.lib().bvc_last_error()
        torch.cuda.synchronize()
        outs["C"].check("refused")
        assert torch.equal(outs["C"].bits(), was)


# ---------------------------------------------------------------------------------------------- 4. gemm8
G8_CLASS = {"BF16": 0, "GELU": 0, "RELU": 0, "F32": 1, "RESID": 1, "POS": 1, "E2D": 1, "LOSS": 1, "F32_BF16": 1, "DGELU": 3, "DRELU": 3}


@pytest.mark.parametrize("shape", R.GEMM8_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
@pytest.mark.parametrize("tile", [10, 11])
def test_gemm8_epilogue_classes(tile, shape):
    """gemm8_kernel<256, 256 / 128> with every epilogue of its classes 0 (register epilogue: BF16, GELU, RELU), 1 (f32 + side input:
    F32, RESID, POS, E2D, LOSS, F32_BF16) and 3 (DGELU, DRELU), NT and NN, on 200 x 192 x 256 (one ragged tile), 520 x 384 x 384 and
    4360 x 1032 x 128 (more units than CUs on either tile): bars, bit-exact integers, strided equal to contiguous, and the
    bf16-output epilogues bitwise equal to the per-tile kernel."""
    M, N, K = shape
    with case_log(f"gemm8 tile {tile} {M}x{N}x{K}") as log:
        for layout in (NT, NN):
            for epi, ec in G8_CLASS.items():
                for exact in (True, False):
                    c = _case(layout, M, N, K, epi, exact)
                    want = f"bvc::gemm8_kernel<256, {R.TILES[tile][1]}, false, {_tf(layout == NN)}, {ec}>"
                    a = launch([c], tile, -1, CONTIG, want, "gemm8")[0]
                    same(a, launch([c], tile, -1, PADS[2], want, "gemm8 strided")[0], f"{c.tag} tile {tile}: strided vs contiguous")
                    check(log, c, a, tile, "gemm8")
                    if ec != 1 and not exact:
                        same(a, launch([c], 0, 2, CONTIG, kernel_name(layout, 0), "per-tile")[0], f"{c.tag}: tile {tile} vs tile 0")


@pytest.mark.parametrize("tile", [10, 11, 12, 13])
def test_gemm8_weight_gradient_groups(tile):
    """Weight-gradient groups (TN) with fused bias gradients on gemm8's 256 x 256, 256 x 128 and 128 x 384 tiles and on the
    accumulating tile config 13: atomics within the bars and bit-exact on integers; deterministic (class 6 slabs + fixed-order reduce)
    twice bit-identical, with ldc > N and the gaps checked after the reduce.  (Tile config 13 has no split; it accumulates.)"""
    shapes = [(520, 384, 384, 1), (264, 200, 640, 3), (136, 72, 192, 2), (264, 200, 200, 1)]
    bn = {10: 256, 11: 128, 12: 384, 13: 256}[tile]
    bm = 128 if tile == 12 else 256
    with case_log(f"gemm8 dW groups tile {tile}") as log:
        for exact in (True, False):
            cs = [Case(TN, M, N, K, "F32", exact, alpha=0.5, split=1 if tile == 13 else s, start=True, rowsum=True, seed=20 + i, accum=tile == 13)
                  for i, (M, N, K, s) in enumerate(shapes)]
            for det in (False, True):
                want = f"bvc::gemm8_kernel<{bm}, {bn}, true, true, {6 if det else 2}>"
                with _det(det):
                    res = launch(cs, tile, -1, PADS[0], want, f"dW det={det}")
                    again = launch(cs, tile, -1, CONTIG, want, f"dW det={det}") if det else None
                for i, c in enumerate(cs):
                    check(log, c, res[i], 13 if tile == 13 else tile, f"dW det={det}")
                    if det:
                        same(res[i], again[i], f"{c.tag} tile {tile}: deterministic, strided vs contiguous")


@pytest.mark.parametrize("M", [128, 136, 1160])
def test_gemm8_layernorm_epilogues(M):
    """EPI_RESID_LN (class 4, NT) and EPI_DLN (class 5, NN) on 128 x 384 tiles at M = 128 (one full tile), 136 (a ragged second
    tile) and 1160 (ten tiles), dense and - where 128 divides M - through the segment map (seg_rows 128 of every 200 rows, offset 40:
    `resid` of RESID_LN is read, `C` of DLN read and written through it, and the rows outside the segments must stay as they were).
    Per element against float64: C, the bf16 LayerNorm / copy, mean, rstd, dgamma, dbeta (onto random start values); integers: C of
    RESID_LN bit-exact.  Row scales are the row's largest |reference|, sums are scaled by the sum of the magnitudes of their terms."""
    N, K, eps = 384, 128, 1e-6
    with case_log(f"gemm8 row-LN M={M}") as log:
        for seg in ((None, (128, 200, 40)) if M % 128 == 0 else (None,)):
            rows = R.seg_rows(M, *(seg or (0, 0, 0))).to(dev)
            P = (M // 128) * 200 if seg else M
            hole = torch.ones(P, dtype=torch.bool)
            hole[rows.cpu()] = False
            for exact in (True, False):
                g = torch.Generator(device=dev).manual_seed(30 + M + exact)
                rnd = (lambda *s: torch.randint(-1024, 1025, s, generator=g, device=dev).float()) if exact else \
                      (lambda *s: torch.randn(*s, generator=g, device=dev))
                A = torch.randint(-8, 9, (M, K), generator=g, device=dev).to(BF16) if exact else torch.randn(M, K, generator=g, device=dev).to(BF16)
                W = torch.randint(-8, 9, (N, K), generator=g, device=dev).to(BF16) if exact else (torch.randn(N, K, generator=g, device=dev) * K ** -0.5).to(BF16)
                bias, resid = rnd(N), rnd(P, N)
                gamma, beta = 1 + 0.1 * torch.randn(N, generator=g, device=dev), 0.1 * torch.randn(N, generator=g, device=dev)
                # ---- RESID_LN
                acc, absacc = R.product(A, W, NT, M, N, K)
                v, v32 = R.scaled(acc, 0.5, None, bias), R.scaled(R.product_f32(A, W, NT, M, N, K), 0.5, None, bias)
                rc, rln, rmean, rrstd = R.epi_resid_ln(v, resid, gamma, beta, eps, seg)
                c32 = v32 + resid[rows]
                tln, tmean, trstd = torch.native_layer_norm(c32, (N,), gamma, beta, R.f32_value(eps))
                prev = None
                for pa, pb in ((24, 72), (0, 0)):          # operands strided, then contiguous (ldc is N by the epilogue's contract)
                    (As, ab), (Ws, wb) = R.strided(A, K + pa), R.strided(W, K + pb)
                    C, C2, mean, rstd = R.Guarded(M, N), R.Guarded(M, N, dtype=BF16), R.Guarded(1, M), R.Guarded(1, M)
                    d = G.gemm_desc(As, Ws, M, N, K, G.EPI["RESID_LN"], C.t, lda=K + pa, ldb=K + pb, alpha=0.5, bias=bias, resid=resid, C2=C2.t,
                                    ln_gamma=gamma, ln_beta=beta, ln_mean=mean.t, ln_rstd=rstd.t, ln_eps=eps)
                    d.a_bytes, d.b_bytes = ab, wb
                    if seg:
                        d.seg_rows, d.seg_stride, d.seg_off = seg
                    assert G.gemm_kernel_name(d, NT) == "bvc::gemm8_kernel<128, 384, false, false, 4>"
                    G.run_gemm([d], NT)
                    torch.cuda.synchronize()
                    for b, w in ((C, "C"), (C2, "C2"), (mean, "mean"), (rstd, "rstd")):
                        b.check(f"RESID_LN M={M} seg={seg} {w}")
                    now = [b.t.clone() for b in (C, C2, mean, rstd)]
                    assert prev is None or all(R.same_bits(x, y) for x, y in zip(prev, now)), f"RESID_LN M={M} seg={seg}: strided vs contiguous"
                    prev = now
                R.check_f32(log, "RESID_LN", C.t, rc, c32, 0.5 * absacc + bias.double().abs()[None] + resid[rows].double().abs())
                if exact:
                    R.check_exact("RESID_LN C", C.t, rc)
                R.check_bf16(log, "RESID_LN.ln", C2.t, rln, tln, rln.abs().amax(1, keepdim=True).expand(M, N))
                R.check_f32(log, "RESID_LN.mean", mean.t.reshape(-1), rmean, tmean.reshape(-1), rc.abs().mean(1))
                R.check_f32(log, "RESID_LN.rstd", rstd.t.reshape(-1), rrstd, trstd.reshape(-1), rrstd)
                # ---- DLN: g = dY W, LayerNorm backward on the rows of x with the statistics handed in
                dY = A
                Wn =(torch.randint(-8, 9, (K, N), generator=g, device=dev) if exact else torch.randn(K, N, generator=g, device=dev) * K ** -0.5).to(BF16)
                x = torch.randn(M, N, generator=g, device=dev) * 2 + 0.5
                xm = x.mean(1).contiguous()
                xr = (1 / torch.sqrt(x.var(1, unbiased=False) + eps)).contiguous()
                dres0, dg0, db0 = torch.randn(P, N, generator=g, device=dev), torch.randn(N, generator=g, device=dev), torch.randn(N, generator=g, device=dev)
                gacc, gabs = R.product(dY, Wn, NN, M, N, K)
                g32 = R.product_f32(dY, Wn, NN, M, N, K)
                rdx, rdg, rdb = R.epi_dln(gacc, x, gamma, xm, xr)
                tdx, tdg, tdb = R.epi_dln(g32, x, gamma, xm, xr)
                prev = None
                for pa, pb in ((72, 8), (0, 0)):
                    (As, ab), (Ws, wb) = R.strided(dY, K + pa), R.strided(Wn, N + pb)
                    dres, dbf = R.Guarded(P, N, fill=dres0), R.Guarded(M, N, dtype=BF16)
                    dg, db, part = R.Guarded(1, N, fill=dg0), R.Guarded(1, N, fill=db0), R.Guarded(1, 512 * 2 * N)
                    was = dres.bits()
                    d = G.gemm_desc(As, Ws, M, N, K, G.EPI["DLN"], dres.t, lda=K + pa, ldb=N + pb, C2=dbf.t, ln_gamma=gamma, ln_mean=xm, ln_rstd=xr,
                                    ln_x=x, ln_part=part.t, ln_dgamma=dg.t, ln_dbeta=db.t)
                    d.a_bytes, d.b_bytes = ab, wb
                    if seg:
                        d.seg_rows, d.seg_stride, d.seg_off = seg
                    assert G.gemm_kernel_name(d, NN) == "bvc::gemm8_kernel<128, 384, false, true, 5>"
                    G.run_gemm([d], NN)
                    torch.cuda.synchronize()
                    for b, w in ((dres, "dres"), (dbf, "copy"), (dg, "dgamma"), (db, "dbeta"), (part, "scratch")):
                        b.check(f"DLN M={M} seg={seg} {w}")
                    R.rows_unchanged(was, dres.bits(), hole, f"DLN M={M} seg={seg}")
                    now = [dres.t.clone(), dbf.t.clone()]      # (rows are reduced in a fixed order; the parameter gradients go through f32 atomics)
                    assert prev is None or all(R.same_bits(x, y) for x, y in zip(prev, now)), f"DLN M={M} seg={seg}: strided vs contiguous"
                    prev = now
                total, ttotal = rdx + dres0[rows].double(), tdx + dres0[rows]
                sc = (dres0[rows].double().abs() + rdx.abs().amax(1, keepdim=True)).expand(M, N)
                R.check_f32(log, "DLN.dres", dres.t[rows], total, ttotal, sc)
                R.check_bf16(log, "DLN.copy", dbf.t, total, ttotal, sc)
                xh = (x.double() - xm.double()[:, None]) * xr.double()[:, None]
                R.check_f32(log, "DLN.dgamma", dg.t.reshape(-1), dg0.double() + rdg, dg0 + tdg, dg0.double().abs() + (gabs * xh.abs()).sum(0))
                R.check_f32(log, "DLN.dbeta", db.t.reshape(-1), db0.double() + rdb, db0 + tdb, db0.double().abs() + gabs.sum(0))


def test_gemm8_option_and_bias_budget():
    """gemm8 = 1 forces the 256-row kernel for a product it can take, gemm8 = -1 keeps it off; a class-0 output whose tile-padded bias
    exceeds the 32 KiB LDS budget (N = 8200) falls back to the other kernels under gemm8 = 1 and does not fail."""
    c = _case(NT, 520, 384, 384, "RESID", True)
    with _option("gemm8", 1):
        a = launch([c], -1, -1, CONTIG, "bvc::gemm8_kernel<256, 256, false, false, 1>", "forced")[0]
    with _option("gemm8", -1):
        b = launch([c], -1, -1, CONTIG, None, "opt-out")[0]
        assert "gemm8" not in G.gemm_kernel_name(build(c, CONTIG, -1)[0], NT)
    check(None, c, a, 10, "gemm8 = 1")
    same(a, b, "gemm8 = 1 vs gemm8 = -1 on integers")
    M, N, K = 136, 8200, 64
    A = torch.randint(-8, 9, (M, K), device=dev).to(BF16)
    W = torch.randint(-8, 9, (N, K), device=dev).to(BF16)
    bias = torch.randint(-1024, 1025, (N,), device=dev).float()
    out = R.Guarded(M, N, N + 8, BF16)
    d = G.gemm_desc(A, W, M, N, K, G.EPI["BF16"], out.t, ldc=N + 8, bias=bias)
    with _option("gemm8", 1):
        assert "gemm8" not in G.gemm_kernel_name(d, NT)
        G.run_gemm([d], NT)
    torch.cuda.synchronize()
    out.check("wide bias")
    R.check_exact("wide bias", out.t, A.double() @ W.double().t() + bias.double(), True)


# ---------------------------------------------------------------------------------------------- 5. A-stationary kernel
@pytest.mark.parametrize("M,N,K", R.AS_SHAPES, ids=lambda v: str(v))
def test_a_stationary_kernel(M, N, K):
    """gemm_as_kernel (tile configs 15 - 18 and the auto route under gemm8 = 1) at K = 384, N = 128 / 384, M = 8, 136, 424 with BF16
    and GELU: bars, bit-exact integers, bitwise equal to tile config 0, strided equal to contiguous; K != 384 is refused by name."""
    with case_log(f"a-stationary {M}x{N}x{K}") as log:
        for epi in ("BF16", "GELU"):
            for exact in (True, False):
                c = _case(NT, M, N, K, epi, exact)
                base = launch([c], 0, 2, CONTIG, kernel_name(NT, 0), "per-tile")[0]
                for tile in (15, 16, 17, 18):
                    want = f"bvc::gemm_as_kernel<{_tf(epi == 'GELU')}, {_tf(tile in (15, 17))}, {_tf(tile >= 17)}>"
                    a = launch([c], tile, -1, CONTIG, want, "a-stationary")[0]
                    same(a, launch([c], tile, -1, PADS[tile % 3], want, "a-stationary strided")[0], f"{c.tag} tile {tile}: strided vs contiguous")
                    same(a, base, f"{c.tag}: tile {tile} vs tile 0")
                    check(log, c, a, tile, "a-stationary")
                if epi == "BF16":
                    with _option("gemm8", 1):
                        same(launch([c], -1, -1, CONTIG, "bvc::gemm_as_kernel<false, true, false>", "auto")[0], base, f"{c.tag}: auto route vs tile 0")
    c = _case(NT, M, N, 320, "BF16", False)
    d, outs, keep = build(c, CONTIG, 15)
    arr = (L.GemmDesc * 1)(d)
    assert L.lib().bvc_op_gemm(arr, 1, NT, 15, -1, G.stream()) != 0
    assert b"A-stationary kernel) take NT products with K = 384" in L.lib().bvc_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(outs["C"].t.float()).all())


# ---------------------------------------------------------------------------------------------- 6. gated residual
def test_gated_residual():
    """bvc_op_gemm_gate (gemm_gate_kernel) on tiles 0 / 1 / 2 and the auto pick, ragged 333 x 200 x 192, 111 rows per sample (no
    divisor of a tile), hidden dropout p = 0.5 from bvc_dropout_mask_host and stochastic depth with the second sample dropped: its
    rows must equal the residual exactly; ldc > N (the mask is indexed with N, the residual with ldc); bit-exact on integers."""
    dg = bvc.dropgate
    M, N, K = R.GATE_SHAPE
    rows, layer, branch, p = 111, 2, 1, 0.5
    scale = torch.tensor([[[1.0, 1.0, 1.0]] * 2] * 2 + [[[1.0, 1.0, 1.0], [2.0, 0.0, 2.0]]], device=dev)
    drop = L.branch_drop(p, 77, 8, scale, rows)
    keep = dg.dropout_mask_host(77, 8, layer, branch, M, N, p).to(dev)
    with case_log(f"gated residual {M}x{N}x{K}") as log:
        for exact in (True, False):
            c = Case(NT, M, N, K, "RESID", exact, alpha=0.5, bias=True, seed=5)
            acc, absacc = R.product(c.A, c.B, NT, M, N, K)
            v, sv = R.scaled(acc, 0.5, None, c.biasv), 0.5 * absacc + c.biasv.to(F64).abs()[None]
            v32 = R.scaled(R.product_f32(c.A, c.B, NT, M, N, K), 0.5, None, c.biasv)
            ref = R.epi_resid_gate(v, c.resid, keep, p, scale[layer, branch], rows)
            t32 = R.epi_resid_gate(v32, c.resid, keep, p, scale[layer, branch], rows)
            for tile in (-1, 0, 1, 2):
                outs = []
                for pc in (0, 24):
                    out = R.Guarded(M, N, N + pc)
                    resid, _ = R.strided(c.resid, N + pc)
                    d = G.gemm_desc(c.A, c.B, M, N, K, 15, out.t, ldc=N + pc, alpha=0.5, bias=c.biasv, resid=resid)
                    name = ctypes.create_string_buffer(160)
                    L.check(L.lib().bvc_op_gemm_gate_kernel(ctypes.byref(d), tile, name, 160), "bvc_op_gemm_gate_kernel")
                    bm, bn = R.TILES[2 if tile < 0 else tile]
                    assert name.value.decode() == f"bvc::gemm_gate_kernel<{bm}, {bn}>"
                    L.check(L.lib().bvc_op_gemm_gate(ctypes.byref(d), ctypes.byref(drop), layer, branch, tile, G.stream()), "bvc_op_gemm_gate")
                    torch.cuda.synchronize()
                    out.check(f"gate tile {tile} ldc {N + pc}")
                    outs.append(out.t.clone())
                assert R.same_bits(outs[0], outs[1]), f"gate tile {tile}: strided vs contiguous"
                R.check_f32(log, "RESID_GATE", outs[0], ref, t32, 2 * 2 * sv + c.resid.to(F64).abs())
                assert torch.equal(outs[0][rows:2 * rows], c.resid[rows:2 * rows]), "the dropped sample is not exactly the residual"
                if exact:
                    R.check_exact("RESID_GATE", outs[0], ref)


# ---------------------------------------------------------------------------------------------- 8. operand extents past 2 GiB
def _wide(rows, width, ld, data):
    """[rows][width] bf16 stored ld apart in one torch.empty buffer filled with the NaN pattern; only the used columns are written."""
    n = (rows - 1) * ld + width
    buf = torch.empty(n, dtype=BF16, device=dev)
    buf.view(torch.int16).fill_(0x7FC0)
    view = buf.as_strided((rows, width), (ld, 1))
    view.copy_(data)
    return buf, view, n * 2


def test_large_extent_nt_nn():
    """A with lda = 2^20: 1100 rows span 2.3 GB, so the byte offsets stage_tile forms pass 2^31 (not 2^32).  NT and NN on tiles
    0 / 1 / 2 and the auto route, which must keep off gemm8 and the A-stationary kernel; tile configs 10 / 11 / 15 refuse.
    Integers: bit-exact."""
    M, N, K = R.LARGE_NT
    lda = 1 << 20
    g = torch.Generator(device=dev).manual_seed(8)
    with case_log(f"large extent NT/NN lda=2^20 {M}x{N}x{K}") as log:
        for layout, n_, k_ in ((NT, N, K), (NN, N, K), (NT, 128, 384)):
            A = torch.randint(-8, 9, (M, k_), generator=g, device=dev).to(BF16)
            (rb, wb) = R.storage_shapes(layout, M, n_, k_)[1]
            B = torch.randint(-8, 9, (rb, wb), generator=g, device=dev).to(BF16)
            bias = torch.randint(-1024, 1025, (n_,), generator=g, device=dev).float()
            ref = R.scaled(R.product(A, B, layout, M, n_, k_)[0], 0.5, None, bias)
            buf, Av, ab = _wide(M, k_, lda, A)
            assert 2 ** 31 < ab < 2 ** 32
            try:
                for tile in (0, 1, 2, -1, 10, 11, 15):
                    with _option("gemm8", 1 if tile == -1 else 0):
                        out = R.Guarded(M, n_, n_ + 8, BF16)
                        d = G.gemm_desc(Av, B, M, n_, k_, G.EPI["BF16"], out.t, ldc=n_ + 8, lda=lda, alpha=0.5, bias=bias)
                        d.a_bytes = ab
                        arr = (L.GemmDesc * 1)(d)
                        if tile >= 10:
                            was = out.bits()
                            assert L.lib().bvc_op_gemm(arr, 1, layout, tile, -1, G.stream()) != 0, f"tile {tile} took a 2.3 GB operand"
                            torch.cuda.synchronize()
                            assert torch.equal(out.bits(), was)
                            continue
                        stages = 2 if tile >= 0 else -1
                        name = G.gemm_kernel_name(d, layout, tile, stages)
                        assert name.startswith("bvc::gemm_kernel<") if tile < 0 else name == kernel_name(layout, tile), name
                        G.run_gemm([d], layout, tile, stages)
                        torch.cuda.synchronize()
                        out.check(f"large {LAYOUT_NAME[layout]} tile {tile}")
                        R.check_exact(f"large {LAYOUT_NAME[layout]} N={n_} K={k_} tile {tile}", out.t, ref, True)
            finally:
                del buf, Av
                torch.cuda.empty_cache()          # hand the 2.3 GB back before the next one
        log.note("BF16", "bit-exact")


def test_large_extent_tn_contraction_tail():
    """TN with K = 2010 rows of lda elements each.  The last K tile covers rows 1984 .. 2047; rows 2010 .. 2047 must read as zero
    because they lie past a_bytes.
      lda = 2^20 - 8:     2048 lda 2 < 2^32, every surplus offset is past a_bytes: the product must be bit-exact on integers
                          (operand extent 4.2 GB: offsets pass 2^31).
      lda = 2^20 + 2^14:  K lda 2 < 2^32 <= 2048 lda 2: the surplus rows' 32-bit offsets would wrap into the allocation and real data
                          would join the sum (measured before launch_gemm checked it: the NaN planted between the rows came out
                          in all 9792 outputs on every tile), so launch_gemm refuses the problem by name and writes nothing.
                          The same holds for B."""
    M, N, K = R.LARGE_TN
    g = torch.Generator(device=dev).manual_seed(9)
    A = torch.randint(-8, 9, (K, M), generator=g, device=dev).to(BF16)
    B = torch.randint(-8, 9, (K, N), generator=g, device=dev).to(BF16)
    ref = 0.5 * R.product(A, B, TN, M, N, K)[0]
    rs = R.rowsum(A, M, K, 0.5)[0]
    with case_log(f"large extent TN {M}x{N}x{K}") as log:
        for lda, ok in (((1 << 20) - 8, True), ((1 << 20) + (1 << 14), False)):
            for which in ("A", "B"):
                buf, view, nb = _wide(K, M if which == "A" else N, lda, A if which == "A" else B)
                assert 2 ** 31 < nb < 2 ** 32 and (2048 * lda * 2 < 2 ** 32) == ok
                try:
                    for tile in (0, 1, 2, -1):
                        out, rsum = R.Guarded(M, N, N + 24), R.Guarded(1, M, fill=0.0)
                        Ad, Bd = (view, B) if which == "A" else (A, view)
                        d = G.gemm_desc(Ad, Bd, M, N, K, G.EPI["F32"], out.t, ldc=N + 24, lda=lda if which == "A" else M,
                                        ldb=lda if which == "B" else N, alpha=0.5, rowsum=rsum.t)
                        if which == "A":
                            d.a_bytes = nb
                        else:
                            d.b_bytes = nb
                        arr = (L.GemmDesc * 1)(d)
                        if ok:
                            name = G.gemm_kernel_name(d, TN, tile)
                            assert name.startswith("bvc::gemm_kernel<") and (tile < 0 or name == kernel_name(TN, tile)), name
                            G.run_gemm([d], TN, tile)
                            torch.cuda.synchronize()
                            out.check(f"large TN tile {tile}")
                            rsum.check(f"large TN tile {tile} rowsum")
                            R.check_exact(f"large TN {which} ld={lda} tile {tile}", out.t, ref)
                            R.check_exact(f"large TN {which} ld={lda} tile {tile} rowsum", rsum.t.reshape(-1), rs)
                        else:
                            was = out.bits()
                            assert L.lib().bvc_op_gemm(arr, 1, TN, tile, -1, G.stream()) != 0, f"ld={lda} tile {tile}: a wrapping tail was accepted"
                            assert b"wrap" in L.lib().bvc_last_error()
                            torch.cuda.synchronize()
                            assert torch.equal(out.bits(), was)
                finally:
                    del buf, view
                    torch.cuda.empty_cache()      # hand the 4.2 GB back before the next one
        log.note("F32", "bit-exact below the window, refused inside it")
