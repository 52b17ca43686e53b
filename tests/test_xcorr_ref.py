"""CPU checks of the feature-correlation op: the algebra the kernels rest on (tests/xcorr_ref.py, float64) against the published
forms of Barlow Twins, VICReg and linear CKA, the closed-form backward against autograd, the symbols, the refusals the library
makes before it launches anything, and the CPU-tensor errors of the Python layer.  No GPU compute."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as ge
from tests import xcorr_ref as X

F64 = torch.float64


@pytest.fixture(scope="module")
def bvc():
    ge.build()
    return ge.load_package()


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- the published forms
@pytest.mark.parametrize("n,p", [(16, 5), (64, 33)])
def test_barlow_parameters_are_the_published_loss(n, p):
    z1, z2 = X.random_cols(n, p, seed=n, dtype=F64), X.random_cols(n, p, seed=n + 1, dtype=F64)
    z2 = z2 + 0.5 * z1
    bn = torch.nn.BatchNorm1d(p, affine=False).double().train()
    c = bn(z1).T @ bn(z2) / n
    on_diag = torch.diagonal(c).clone().add_(-1).pow_(2).sum()
    off_diag = c.flatten()[:-1].view(p - 1, p + 1)[:, 1:].flatten().clone().pow_(2).sum()
    o = X.forward(z1, z2, X.BARLOW(n))
    assert _rel(o["on"], on_diag) < 1e-12 and _rel(o["off"], off_diag) < 1e-12
    assert _rel(X.barlow_twins(z1, z2), on_diag + 5e-3 * off_diag) < 1e-12


def _off_diagonal(m):
    n = m.shape[0]
    return m.flatten()[:-1].view(n - 1, n + 1)[:, 1:].flatten()


@pytest.mark.parametrize("n,p", [(16, 5), (40, 21)])
def test_vicreg_assembly_is_the_papers_pseudo_code(n, p):
    x = 0.7 * X.random_cols(n, p, seed=3, dtype=F64)          # standard deviations below 1: the hinge is active
    y = x + 0.3 * X.random_cols(n, p, seed=4, dtype=F64)
    repr_loss = F.mse_loss(x, y)
    xc, yc = x - x.mean(dim=0), y - y.mean(dim=0)
    std_x, std_y = torch.sqrt(x.var(dim=0) + 1e-4), torch.sqrt(y.var(dim=0) + 1e-4)
    std_loss = torch.mean(F.relu(1 - std_x)) / 2 + torch.mean(F.relu(1 - std_y)) / 2
    cov_x, cov_y = (xc.T @ xc) / (n - 1), (yc.T @ yc) / (n - 1)
    cov_loss = _off_diagonal(cov_x).pow(2).sum() / p + _off_diagonal(cov_y).pow(2).sum() / p
    assert float(std_loss) > 0
    assert _rel(X.vicreg(x, y), 25.0 * repr_loss + 25.0 * std_loss + 1.0 * cov_loss) < 1e-12


# ---------------------------------------------------------------------------------------------- closed form = autograd
def _const(x, col):
    x = x.clone()
    x[:, col] = 0.25
    return x


GRAD_CASES = [
    # name, n, p, q (None = alias), norm, ddof, dvar, constant column
    ("distinct p != q", 12, 5, 7, 1, 0, False, False), ("distinct q < p", 9, 6, 4, 0, 1, True, False),
    ("alias centre", 10, 6, None, 0, 1, True, False), ("alias standardise", 10, 6, None, 1, 0, True, False),
    ("norm 1 ddof 1 dvar", 11, 4, 4, 1, 1, True, False), ("norm 0 ddof 0", 8, 3, 5, 0, 0, False, False),
    ("constant column", 12, 5, 5, 1, 0, True, True), ("constant column alias", 12, 5, None, 1, 1, False, True),
    ("n 2 ddof 1", 2, 3, 3, 0, 1, True, False),
]


@pytest.mark.parametrize("name,n,p,q,norm,ddof,dvar,const", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_closed_form_gradient_is_autograd(name, n, p, q, norm, ddof, dvar, const):
    x = X.random_cols(n, p, seed=11, dtype=F64)
    y = None if q is None else X.random_cols(n, q, seed=12, dtype=F64) + 0.3 * x[:, :1]
    if const:
        x = _const(x, 1)
        y = None if y is None else _const(y, 3)
    cfg = (norm, ddof, 1e-3, 1.0 / n, 0.7)
    w_on, w_off = 1.3, -0.4
    dvx = torch.randn(p, dtype=F64, generator=_gen(13)) if dvar else None
    dvy = torch.randn(q, dtype=F64, generator=_gen(14)) if dvar and q is not None else None
    ag = X.autograd_grad(x, y, cfg, w_on, w_off, dvx, dvy)
    cg = X.closed_grad(x, y, cfg, w_on, w_off, dvx, dvy)
    sc = X.scales(x, y, cfg, w_on, w_off, dvx, dvy)
    for a, c, s in zip(ag, cg, (sc["dx"], sc["dy"])):
        if a is None:
            assert c is None and q is None
            continue
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        assert bool(((a - c).abs() <= 1e-12 * s).all()), float(((a - c).abs() / s.clamp_min(1e-300)).max())
    if const:
        o = X.forward(x, y, cfg)
        assert float(o["var_x"][1]) == 0.0 and float(o["xh"][:, 1].abs().max()) == 0.0 and abs(float(o["rx"][1]) - 1e-3 ** -0.5) < 1e-9


# ---------------------------------------------------------------------------------------------- CKA
def test_linear_cka_is_the_gram_form_and_has_its_invariances():
    n, p, q = 30, 7, 11
    x = X.random_cols(n, p, seed=21, dtype=F64)
    y = X.random_cols(n, q, seed=22, dtype=F64) + x @ X.random_cols(p, q, seed=23, dtype=F64)
    c = X.linear_cka(x, y)
    assert 0.0 < float(c) < 1.0
    assert _rel(c, X.gram_cka(x, y)) < 1e-12
    assert abs(float(X.linear_cka(x, x)) - 1.0) < 1e-12
    Q, _ = torch.linalg.qr(X.random_cols(p, p, seed=24, dtype=F64))
    Qy, _ = torch.linalg.qr(X.random_cols(q, q, seed=25, dtype=F64))
    assert _rel(X.linear_cka(x @ Q, y), c) < 1e-12 and _rel(X.linear_cka(x, y @ Qy), c) < 1e-12
    assert _rel(X.linear_cka(3.7 * x, y), c) < 1e-12 and _rel(X.linear_cka(x, 0.01 * y + 5.0), c) < 1e-12
    # the op's parameter setting: norm 0, scale 1, t 0 makes on + off the squared Frobenius norm
    o = X.forward(x, y, X.CKA)
    xc, yc = x - x.mean(0), y - y.mean(0)
    assert _rel(o["on"] + o["off"], ((xc.t() @ yc) ** 2).sum()) < 1e-12


# ---------------------------------------------------------------------------------------------- the library
NEW_SYMBOLS = ("bvc_op_xcorr_block_cols", "bvc_op_xcorr_workspace", "bvc_op_xcorr_fwd", "bvc_op_xcorr_bwd")


def test_symbols_are_declared_and_exported(bvc):
    header = open(os.path.join(ge.ROOT, "include", "bvc.h")).read()
    lib = bvc._lib.lib()
    for name in NEW_SYMBOLS:
        assert name in bvc._lib.SYMBOLS and name + "(" in header and getattr(lib, name) is not None


def test_refusals_launch_nothing(bvc):
    """Every refusal is made before any launch: the calls below pass dummy host pointers and a null stream."""
    lib = bvc._lib.lib()
    buf = ctypes.create_string_buffer(64)
    buf2 = ctypes.create_string_buffer(64)
    P, P2 = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf2, ctypes.c_void_p)

    def fwd(n=8, p=16, q=16, norm=1, ddof=0, eps=1e-5, scale=0.125, t=1.0, x=P, y=P2, ldx=None, ldy=None, mean_x=P, var_x=P, mean_y=P,
            var_y=P, stats=P, ws=P):
        return lib.bvc_op_xcorr_fwd(x, p if ldx is None else ldx, y, q if ldy is None else ldy, n, p, q, norm, ddof, eps, scale, t,
                                    mean_x, var_x, mean_y, var_y, stats, ws, None)

    def bwd(n=8, p=16, q=16, norm=1, ddof=0, eps=1e-5, scale=0.125, t=1.0, x=P, y=P2, ldy=None, w=P, dx=P, dy=P, lddx=None, lddy=None,
            block_cols=0, mean_x=P, var_x=P, mean_y=P, var_y=P, ws=P):
        return lib.bvc_op_xcorr_bwd(x, p, y, q if ldy is None else ldy, n, p, q, norm, ddof, eps, scale, t, mean_x, var_x, mean_y, var_y, w,
                                    None, None, block_cols, dx, p if lddx is None else lddx, dy, q if lddy is None else lddy, ws, None)

    odd = ctypes.c_void_p(P.value + 2)
    inf, nan = float("inf"), float("nan")
    cases = [(lambda: fwd(n=0), b"n 0"), (lambda: fwd(n=32769), b"n 32769"), (lambda: fwd(p=0), b"p 0"), (lambda: fwd(p=8193), b"p 8193"),
             (lambda: fwd(q=0), b"q 0"), (lambda: fwd(q=8193), b"q 8193"), (lambda: fwd(n=1, ddof=1), b"n - ddof"),
             (lambda: fwd(norm=2), b"norm"), (lambda: fwd(norm=-1), b"norm"), (lambda: fwd(ddof=2), b"ddof"), (lambda: fwd(ddof=-1), b"ddof"),
             (lambda: fwd(scale=0.0), b"scale"), (lambda: fwd(scale=-1.0), b"scale"), (lambda: fwd(scale=inf), b"scale"),
             (lambda: fwd(scale=nan), b"scale"), (lambda: fwd(t=nan), b"diag_target"), (lambda: fwd(t=inf), b"diag_target"),
             (lambda: fwd(eps=0.0), b"eps"), (lambda: fwd(eps=-1.0), b"eps"), (lambda: fwd(eps=nan), b"eps"), (lambda: fwd(eps=inf), b"eps"),
             (lambda: fwd(ldx=15), b"stride"), (lambda: fwd(ldy=15), b"stride"), (lambda: fwd(x=None), b"null"), (lambda: fwd(y=None), b"null"),
             (lambda: fwd(mean_x=None), b"null"), (lambda: fwd(mean_y=None), b"null"), (lambda: fwd(ws=None), b"null"),
             (lambda: fwd(var_x=None), b"null"), (lambda: fwd(var_y=None), b"null"), (lambda: fwd(stats=None), b"null"),
             (lambda: fwd(x=odd), b"aligned"), (lambda: fwd(y=odd), b"aligned"), (lambda: fwd(ws=odd), b"aligned"),
             (lambda: bwd(x=None), b"null"), (lambda: bwd(y=None), b"null"), (lambda: bwd(ws=None), b"null"),
             (lambda: bwd(mean_x=None), b"null"), (lambda: bwd(var_x=None), b"null"), (lambda: bwd(mean_y=None), b"null"),
             (lambda: bwd(var_y=None), b"null"), (lambda: bwd(ws=odd), b"aligned"),
             (lambda: fwd(y=P, q=8), b"alias"), (lambda: fwd(y=P, ldy=20), b"alias"),
             (lambda: bwd(n=0), b"n 0"), (lambda: bwd(q=9000), b"q 9000"), (lambda: bwd(n=1, ddof=1), b"n - ddof"), (lambda: bwd(norm=3), b"norm"),
             (lambda: bwd(scale=0.0), b"scale"), (lambda: bwd(t=nan), b"diag_target"), (lambda: bwd(eps=0.0), b"eps"),
             (lambda: bwd(w=None), b"null"), (lambda: bwd(dx=None), b"null"), (lambda: bwd(dy=None), b"null"),
             (lambda: bwd(lddx=15), b"stride"), (lambda: bwd(lddy=15), b"stride"), (lambda: bwd(y=P, ldy=20), b"alias"),
             (lambda: bwd(y=P, dy=P), b"alias"), (lambda: bwd(block_cols=-1), b"block_cols")]
    for call, word in cases:
        assert call() != 0 and word in lib.bvc_last_error(), (word, lib.bvc_last_error())
    # eps is not looked at when norm == 0 ... but everything after it still is
    assert fwd(norm=0, eps=0.0, scale=0.0) != 0 and b"scale" in lib.bvc_last_error()
    W = lib.bvc_op_xcorr_workspace
    for bad in ((0, 16, 16, 0), (32769, 16, 16, 0), (8, 0, 16, 0), (8, 16, 8193, 0), (8, 16, 8, 1)):
        assert W(bad[0], bad[1], bad[2], bad[3], 0, 0) == -1 and W(bad[0], bad[1], bad[2], bad[3], 0, 1) == -1
    assert W(8, 16, 16, 0, -1, 1) == -1 and lib.bvc_op_xcorr_block_cols(0, 16, 16) == -1 and lib.bvc_op_xcorr_block_cols(8, 9000, 16) == -1


def test_workspace_sizes_and_automatic_blocking(bvc):
    lib = bvc._lib.lib()
    W = lib.bvc_op_xcorr_workspace
    # the forward holds the transposed operands and one f64 pair per tile: less than one [p][q] f32 array at 2048 x 8192
    assert 0 < W(2048, 8192, 8192, 0, 0, 0) < 8192 * 8192 * 4
    assert W(2048, 8192, 8192, 1, 0, 0) < W(2048, 8192, 8192, 0, 0, 0)
    assert W(300, 257, 129, 0, 0, 0) % 16 == 0 and W(300, 257, 129, 0, 0, 1) % 16 == 0
    # the G block [block_cols][8192] stays under 128 MiB
    assert lib.bvc_op_xcorr_block_cols(2048, 8192, 8192) == 4096 and lib.bvc_op_xcorr_block_cols(128, 2048, 2048) == 2048
    assert lib.bvc_op_xcorr_block_cols(2, 1, 3) == 128
    assert W(300, 300, 257, 0, 0, 1) == W(300, 300, 257, 0, 384, 1) and W(300, 300, 257, 0, 128, 1) < W(300, 300, 257, 0, 0, 1)


def test_cpu_tensors_are_refused(bvc):
    S, XC = bvc.simclr, bvc.xcorr
    a, b = torch.randn(8, 16), torch.randn(8, 16)
    for call in (lambda: XC.cross_correlation(a, b), lambda: XC.cross_correlation(a), lambda: XC.linear_cka(a, b),
                 lambda: S.barlow_twins_loss(a, b), lambda: S.vicreg_loss(a, b), lambda: S.global_barlow_twins_loss(a, b),
                 lambda: S.global_vicreg_loss(a, b)):
        with pytest.raises(bvc._lib.BvcError):
            call()
    with pytest.raises(ValueError):
        XC.cross_correlation(torch.randn(8))
    with pytest.raises(ValueError):
        S.barlow_twins_loss(torch.randn(8, 4), torch.randn(8, 5))
