"""Feature-correlation op on the GPU: bvc_op_xcorr_fwd / _bwd (csrc/xcorr.hip) through the C ABI against the float64 reference of
tests/xcorr_ref.py, and bvc.xcorr / bvc.simclr (barlow_twins_loss, vicreg_loss, linear_cka) on top of them.  The rules of
tests/test_gpu_ntxent.py apply: Guarded buffers with guard bands, outputs and the workspace pre-filled with NaN, x and y with a
NaN-filled row padding (ld = width + pad: reading it poisons the result), the padding of dx / dy must keep its NaN bits, the
workspace is refilled with NaN between the forward and the backward, one parity-report line per case.

Bars (nothing in them comes from the code under test).  The scale of an output element is the float64 sum of the magnitudes of its
terms (xcorr_ref.scales).  The bar of an element is its scale times the larger of
  * 4 x the worst error, relative to the scale, of the same dense formulas run by torch in float32 on the same device inputs, and
  * a rounding bound derived from the roundings of the formulas.  An element of xh carries the rounding of the centring (1), of
    r = 1 / sqrt(var + eps) (4) and of the scaling (1): 6 per operand, 12 per product.  An element of C is a chain of n fused
    multiply-adds (n roundings) times `scale` (1): |dC| <= 2^-24 (n + 16) Cabs.  The square doubles the relative error and rounds
    once more: on / off are held to 2^-24 (2 n + 34) of their scale (xcorr_ref.eps_stats).  G inherits C's error and two roundings of
    its own; dxh is a chain over the `width` columns of the other operand of products with an xh factor; the column sums are float64,
    and the centring of dxh, r and the variance path add fewer than 16: dx / dy are held to 2^-24 (n + width + 48) of their scale
    (xcorr_ref.eps_grad),
with the file's floor of 4 ulp of the reference value.  Means and variances are float64 sums rounded once: at most 1 ulp of the
reference.  The explicit alias and a bit-equal copy promise the same forward bits; their gradients agree within the bars.
"""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():   # collected on the CPU box, run on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G          # noqa: E402
from tests import xcorr_ref as X         # noqa: E402
from tests import rowops_ref as RR       # noqa: E402
from tests.test_gpu_rowops import Guarded, _same_bits     # noqa: E402

L = G.L
bvc = G.bvc
S = bvc.simclr
XC = bvc.xcorr
dev = "cuda"
F64 = torch.float64
NAN = float("nan")


def _gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=_gen(seed), device=dev)


class Ref:
    """float64 reference (autograd), torch-f32 comparator (the dense formulas) and scales of one set of inputs."""

    def __init__(self, x, y, cfg, w, dvx=None, dvy=None):
        w_on, w_off = float(w[0]), float(w[1])
        x64, y64 = x.double(), None if y is None else y.double()
        self.out = X.forward(x64, y64, cfg)
        self.dx, self.dy = X.autograd_grad(x64, y64, cfg, w_on, w_off, dvx, dvy)
        self.t_out = X.forward(x, y, cfg)
        self.t_dx, self.t_dy = X.closed_grad(x, y, cfg, w_on, w_off, dvx, dvy)
        self.sc = X.scales(x, y, cfg, w_on, w_off, dvx, dvy)


def _padded(t, pad):
    n, p = t.shape
    b = torch.full((n, p + pad), NAN, device=dev)
    b[:, :p] = t
    return b


class Run:
    """One forward and one backward through the C ABI on guarded, NaN-filled buffers; y None = the explicit alias."""

    def __init__(self, x, y, cfg, w, dvx=None, dvy=None, pad=0, block_cols=0, ws_fill="nan"):
        norm, ddof, eps, scale, t = cfg
        n, p = x.shape
        alias = y is None
        q = p if alias else y.shape[1]
        ldx, ldy = p + pad, q + pad
        self.xb = _padded(x, pad)
        self.yb = self.xb if alias else _padded(y, pad)
        lib, st = L.lib(), G.stream()
        nf, nb = lib.bvc_op_xcorr_workspace(n, p, q, int(alias), block_cols, 0), lib.bvc_op_xcorr_workspace(n, p, q, int(alias), block_cols, 1)
        assert nf > 0 and nb > 0 and nf % 16 == 0 and nb % 16 == 0
        self.mean_x, self.var_x, self.stats = Guarded((p,), row=p), Guarded((p,), row=p), Guarded((2,))
        self.mean_y, self.var_y = Guarded((q,), row=q), Guarded((q,), row=q)
        self.ws = Guarded((max(nf, nb) // 4,), fill=ws_fill, row=max(p, q))
        self.dxg = Guarded((n, ldx), row=ldx)
        self.dyg = Guarded((n, ldy), row=ldy)
        ptr = lambda g: None if g is None else g.data_ptr()      # noqa: E731
        my, vy = (None, None) if alias else (self.mean_y.t, self.var_y.t)
        L.check(lib.bvc_op_xcorr_fwd(self.xb.data_ptr(), ldx, self.yb.data_ptr(), ldy, n, p, q, norm, ddof, eps, scale, t,
                                     self.mean_x.t.data_ptr(), self.var_x.t.data_ptr(), ptr(my), ptr(vy), self.stats.t.data_ptr(),
                                     self.ws.t.data_ptr(), st), "bvc_op_xcorr_fwd")
        if ws_fill == "nan":
            self.ws.t.fill_(NAN)      # nothing survives from the forward to the backward
        self.w = torch.as_tensor(w, dtype=torch.float32, device=dev).contiguous()
        d32 = lambda v: None if v is None else v.float().contiguous()      # noqa: E731
        self.dvx, self.dvy = d32(dvx), None if alias else d32(dvy)
        L.check(lib.bvc_op_xcorr_bwd(self.xb.data_ptr(), ldx, self.yb.data_ptr(), ldy, n, p, q, norm, ddof, eps, scale, t,
                                     self.mean_x.t.data_ptr(), self.var_x.t.data_ptr(), ptr(my), ptr(vy), self.w.data_ptr(), ptr(self.dvx),
                                     ptr(self.dvy), block_cols, self.dxg.t.data_ptr(), ldx, None if alias else self.dyg.t.data_ptr(), ldy,
                                     self.ws.t.data_ptr(), st), "bvc_op_xcorr_bwd")
        torch.cuda.synchronize()
        for name in ("mean_x", "var_x", "mean_y", "var_y", "stats", "ws", "dxg", "dyg"):
            getattr(self, name).check(name)
        self.alias = alias
        self.dx, self.dy = self.dxg.t[:, :p], None if alias else self.dyg.t[:, :q]
        if pad:
            assert bool(torch.isnan(self.dxg.t[:, p:]).all()) and bool(torch.isnan(self.dyg.t[:, q:]).all()), "the padding of dx / dy was written"
        if alias:
            assert bool(torch.isnan(self.mean_y.t).all() & torch.isnan(self.var_y.t).all() & torch.isnan(self.dyg.t).all()), "alias: a y output was written"
        outs = [self.mean_x.t, self.var_x.t, self.stats.t, self.dx] + ([] if alias else [self.mean_y.t, self.var_y.t, self.dy])
        self.outs = outs
        assert not any(bool(torch.isnan(o).any()) for o in outs), "NaN in an output, or elements not written"


def _check(name, key, got, ref, t32, scale, eps_rel, items, extra=None):
    bar, wt = X.bars(ref, t32, scale, eps_rel)
    if extra is not None:
        bar = bar + extra
    err = (got.double() - ref).abs()
    nz = scale > 0
    wk = float((err[nz] / scale[nz]).max()) if bool(nz.any()) else float(err.max()) if err.numel() else 0.0
    items.append(f"{key} {wk:.2e}/{wt:.2e}")
    bad = ~(err <= bar)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{name} {key}: {int(bad.sum())} of {bad.numel()} elements over the bar; at {i}: error {float(err[i]):.3e}, "
                             f"bar {float(bar[i]):.3e}, scale {float(scale[i]):.3e}, torch-f32 worst {wt:.3e}, kernel worst {wk:.3e}")
    return bar


def _check_moments(name, key, got, ref, t32, items):
    """float64 sum, one rounding: at most 1 ulp of the reference; the comparator's error is reported beside the kernel's, in ulp"""
    ulp = RR.ulp32(ref)
    aerr = (got.double() - ref).abs()
    err = aerr / ulp.clamp_min(1e-300)
    terr = (t32.double() - ref).abs() / ulp.clamp_min(1e-300)
    items.append(f"{key} {float(err.max()):.2f}/{float(terr.max()):.2f} ulp")
    assert bool((aerr <= ulp).all()), f"{name} {key}: {float(err.max()):.3f} ulp from the float64 value"


def check_run(name, run, ref, n):
    items = []
    try:
        o, t = ref.out, ref.t_out
        _check_moments(name, "mean_x", run.mean_x.t, o["mean_x"], t["mean_x"], items)
        _check_moments(name, "var_x", run.var_x.t, o["var_x"], t["var_x"], items)
        if not run.alias:
            _check_moments(name, "mean_y", run.mean_y.t, o["mean_y"], t["mean_y"], items)
            _check_moments(name, "var_y", run.var_y.t, o["var_y"], t["var_y"], items)
        for k, i in (("on", 0), ("off", 1)):
            _check(name, k, run.stats.t[i].reshape(1), o[k].reshape(1), t[k].reshape(1), ref.sc[k].reshape(1), X.eps_stats(n), items)
        p, q = o["C"].shape
        _check(name, "dx", run.dx, ref.dx, ref.t_dx, ref.sc["dx"], X.eps_grad(n, q), items)
        if not run.alias:
            _check(name, "dy", run.dy, ref.dy, ref.t_dy, ref.sc["dy"], X.eps_grad(n, p), items)
    finally:
        G.log_parity(f"xcorr {name}: " + "  ".join(items) + "   (kernel/torch-f32, relative to the element's scale)")


def _cfg(norm, ddof, n):
    return (norm, ddof, 1e-5, 1.0 / (n - ddof), 1.0 if norm else 0.25)


def _case(name, x, y, cfg, seed, dvar=True, w=None, **kw):
    n, p = x.shape
    q = p if y is None else y.shape[1]
    w = _randn(seed, 2).tolist() if w is None else w
    dvx = _randn(seed + 1, p) if dvar else None
    dvy = _randn(seed + 2, q) if dvar and y is not None else None
    ref = Ref(x, y, cfg, w, dvx, dvy)
    run = Run(x, y, cfg, w, dvx, dvy, **kw)
    check_run(name, run, ref, n)
    return run, ref


# ---------------------------------------------------------------------------------------------- shapes
# (n, p, q, pad, alias, norm, ddof, block_cols, dvar): every n edge of the 32-row contraction stage and of the 128-row tile of the dxh
# product, p and q on both sides of the 32-float stage and of the 128-column tile, p != q so that the diagonal ends inside a tile and in
# another tile row than column (300 x 129, 129 x 257, 257 x 3), forced blockings with several blocks and a partial last one (300 and
# 257 columns in blocks of 128), NULL dvar, one realistic shape
SHAPES = [
    (2, 1, 1, 0, False, 0, 1, 0, True), (2, 3, 1, 1, False, 1, 0, 0, False), (3, 1, 3, 8, False, 1, 1, 0, True),
    (31, 127, 128, 0, False, 1, 0, 0, True), (32, 128, 127, 1, False, 0, 1, 0, True), (33, 129, 129, 8, True, 1, 0, 0, True),
    (127, 257, 3, 0, False, 1, 1, 128, True), (128, 300, 129, 1, False, 1, 0, 128, False), (129, 129, 257, 8, False, 0, 0, 128, True),
    (300, 300, 300, 0, True, 0, 1, 128, True), (300, 257, 300, 1, False, 1, 0, 256, True), (300, 3, 3, 8, True, 1, 1, 0, False),
    (33, 300, 127, 0, False, 0, 1, 0, False), (256, 2048, 2048, 0, False, 1, 0, 0, True),
]


@pytest.mark.parametrize("n,p,q,pad,alias,norm,ddof,block_cols,dvar", SHAPES)
def test_against_float64(n, p, q, pad, alias, norm, ddof, block_cols, dvar):
    x = X.random_cols(n, p, seed=n * 10 + p, device=dev)
    y = None if alias else X.random_cols(n, q, seed=n * 10 + q + 1, device=dev) + 0.5 * x[:, :1]
    _case(f"n{n} p{p} q{q} pad{pad} {'alias' if alias else 'distinct'} norm{norm} ddof{ddof} cols{block_cols}", x, y, _cfg(norm, ddof, n),
          seed=n + p + q, dvar=dvar, pad=pad, block_cols=block_cols)


# ---------------------------------------------------------------------------------------------- hard cases
def test_y_is_a_copy_of_x_under_barlow_parameters():
    """C_ii is about 1 and `on` a sum of squared differences near zero: its scale, sum (Cabs_ii + 1)^2, is what the bar is relative to"""
    n, p = 200, 130
    x = X.random_cols(n, p, seed=41, device=dev)
    run, ref = _case("copy barlow", x, x.clone(), X.BARLOW(n), seed=42, pad=1)
    assert float(ref.out["on"]) < 1e-6 * p


def test_columns_with_mean_100():
    n, p, q = 130, 70, 40
    x, y = X.offset_cols(n, p, seed=43, device=dev), X.offset_cols(n, q, seed=44, mean=-100.0, device=dev)
    _case("mean 100 barlow", x, y, X.BARLOW(n), seed=45)
    _case("mean 100 covariance", x, None, X.VICREG(n), seed=46)


def test_constant_columns_under_norm_1():
    n, p, q = 100, 40, 33
    x, y = X.random_cols(n, p, seed=47, device=dev), X.random_cols(n, q, seed=48, device=dev)
    x[:, 5] = 0.75
    y[:, 32] = -3.0
    run, ref = _case("constant columns", x, y, X.BARLOW(n), seed=49)
    assert float(run.var_x.t[5]) == 0.0 and float(run.var_y.t[32]) == 0.0
    assert all(bool(torch.isfinite(o).all()) for o in run.outs)


@pytest.mark.parametrize("alias", [False, True])
def test_strongly_correlated_columns(alias):
    n, p = 256, 130
    x = X.correlated_cols(n, p, seed=50, device=dev)
    y = None if alias else X.correlated_cols(n, p, seed=50, device=dev) + 0.05 * X.random_cols(n, p, seed=51, device=dev)
    run, ref = _case(f"correlated 0.99 {'alias' if alias else 'distinct'}", x, y, X.BARLOW(n), seed=52)
    assert float(ref.out["off"]) > 0.9 * p * (p - 1) * 0.95 ** 2 and float(ref.out["off"]) > 100 * float(ref.out["on"])


def test_a_zero_weight_and_n_2():
    n, p, q = 130, 40, 50
    x, y = X.random_cols(n, p, seed=53, device=dev), X.random_cols(n, q, seed=54, device=dev)
    _case("w_on 0", x, y, X.BARLOW(n), seed=55, w=[0.0, 0.7], dvar=False)
    _case("w_off 0", x, y, X.BARLOW(n), seed=56, w=[-1.3, 0.0], dvar=False)
    run, _ = _case("w 0 0", x, None, X.VICREG(n), seed=57, w=[0.0, 0.0], dvar=False)
    assert bool((run.dx == 0).all())
    x2 = X.random_cols(2, 5, seed=58, device=dev)
    _case("n 2 ddof 1", x2, None, X.VICREG(2), seed=59)
    _case("n 2 ddof 1 distinct", x2, X.random_cols(2, 4, seed=60, device=dev), (1, 1, 1e-4, 1.0, 1.0), seed=61)


# ---------------------------------------------------------------------------------------------- invariants
def test_same_bits_on_every_run_whatever_the_workspace_held_and_for_every_blocking():
    n, p, q = 300, 300, 257
    x, y = X.random_cols(n, p, seed=71, device=dev), X.random_cols(n, q, seed=72, device=dev)
    w, dvx, dvy = [0.8, -0.3], _randn(73, p), _randn(74, q)
    cfg = X.BARLOW(n)
    a = Run(x, y, cfg, w, dvx, dvy, pad=1, block_cols=128)
    others = [Run(x, y, cfg, w, dvx, dvy, pad=1, block_cols=128), Run(x, y, cfg, w, dvx, dvy, pad=1, block_cols=128, ws_fill=0.0),
              Run(x, y, cfg, w, dvx, dvy, pad=1, block_cols=128, ws_fill=1e30), Run(x, y, cfg, w, dvx, dvy, pad=1, block_cols=256),
              Run(x, y, cfg, w, dvx, dvy, pad=1, block_cols=0)]
    for o in others:
        for u, v in zip(a.outs, o.outs):
            assert _same_bits(u, v)


def test_explicit_alias_against_a_bit_equal_copy():
    """The forward promises the same bits; dx of the alias is dx + dy of the copy to rounding (both inside the bars of the alias)"""
    n, p = 130, 129
    x = X.random_cols(n, p, seed=75, device=dev)
    cfg, w, dv = X.VICREG(n), [0.4, 1.1], _randn(76, p)
    ref = Ref(x, None, cfg, w, dv)
    a = Run(x, None, cfg, w, dv, pad=1)
    c = Run(x, x.clone(), cfg, w, dv, torch.zeros_like(dv), pad=1)
    assert _same_bits(a.stats.t, c.stats.t) and _same_bits(a.var_x.t, c.var_x.t) and _same_bits(a.mean_x.t, c.mean_y.t)
    items = []
    _check("alias", "dx", a.dx, ref.dx, ref.t_dx, ref.sc["dx"], X.eps_grad(n, p), items)
    _check("copy", "dx + dy", c.dx.double() + c.dy.double(), ref.dx, ref.t_dx, ref.sc["dx"], X.eps_grad(n, p), items)
    G.log_parity("xcorr alias against copy: " + "  ".join(items))


def test_refused_arguments_write_nothing():
    n, p = 8, 16
    x, y = X.random_cols(n, p, seed=77, device=dev), X.random_cols(n, p, seed=78, device=dev)
    lib, st = L.lib(), G.stream()
    outs = [Guarded((p,), row=p) for _ in range(4)] + [Guarded((2,)), Guarded((65536,)), Guarded((n, p), row=p), Guarded((n, p), row=p)]
    mx, vx, my, vy, stats, ws, dx, dy = outs
    w = torch.ones(2, device=dev)

    def fwd(n_=n, p_=p, q_=p, norm=1, ddof=0, eps=1e-5, scale=0.125, t=1.0, yp=y, ldy=p):
        return lib.bvc_op_xcorr_fwd(x.data_ptr(), p, yp.data_ptr(), ldy, n_, p_, q_, norm, ddof, eps, scale, t, mx.t.data_ptr(), vx.t.data_ptr(),
                                    my.t.data_ptr(), vy.t.data_ptr(), stats.t.data_ptr(), ws.t.data_ptr(), st)

    def bwd(n_=n, p_=p, q_=p, norm=1, ddof=0, eps=1e-5, scale=0.125, t=1.0, yp=y, lddx=p, block_cols=0, wp=w.data_ptr()):
        return lib.bvc_op_xcorr_bwd(x.data_ptr(), p, yp.data_ptr(), p, n_, p_, q_, norm, ddof, eps, scale, t, x.data_ptr(), x.data_ptr(),
                                    y.data_ptr(), y.data_ptr(), wp, None, None, block_cols, dx.t.data_ptr(), lddx, dy.t.data_ptr(), p,
                                    ws.t.data_ptr(), st)

    nan, inf = float("nan"), float("inf")
    for call, word in ((lambda: fwd(n_=0), b"n 0"), (lambda: fwd(n_=40000), b"n 40000"), (lambda: fwd(p_=0), b"p 0"), (lambda: fwd(q_=8200), b"q 8200"),
                       (lambda: fwd(n_=1, ddof=1), b"n - ddof"), (lambda: fwd(norm=2), b"norm"), (lambda: fwd(ddof=3), b"ddof"),
                       (lambda: fwd(scale=0.0), b"scale"), (lambda: fwd(scale=nan), b"scale"), (lambda: fwd(t=inf), b"diag_target"),
                       (lambda: fwd(eps=0.0), b"eps"), (lambda: fwd(ldy=p - 1), b"stride"), (lambda: fwd(yp=x, q_=p - 1, ldy=p), b"alias"),
                       (lambda: bwd(n_=0), b"n 0"), (lambda: bwd(scale=-1.0), b"scale"), (lambda: bwd(eps=nan), b"eps"), (lambda: bwd(lddx=p - 1), b"stride"),
                       (lambda: bwd(yp=x), b"alias"), (lambda: bwd(block_cols=-128), b"block_cols"), (lambda: bwd(wp=None), b"null")):
        assert call() != 0 and word in lib.bvc_last_error(), (word, lib.bvc_last_error())
    torch.cuda.synchronize()
    for o in outs:
        o.check("refused call")
        assert bool(torch.isnan(o.t).all()), "a refused call wrote an output"


# ---------------------------------------------------------------------------------------------- bvc.xcorr / bvc.simclr
def test_barlow_twins_loss_is_the_abi_and_matches_float64():
    n, p, lambd = 130, 100, 5e-3
    z1 = X.random_cols(n, p, seed=81, device=dev)
    z2 = z1 + 0.5 * X.random_cols(n, p, seed=82, device=dev)
    g3 = torch.tensor(3.0, device=dev)
    w = torch.stack([g3, g3 * lambd])
    run, ref = _case("barlow_twins_loss x3", z1, z2, X.BARLOW(n), seed=0, w=w.tolist(), dvar=False)
    a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    loss = S.barlow_twins_loss(a, b, lambd)
    (loss * 3).backward()
    assert loss.dim() == 0 and _same_bits(loss.detach(), run.stats.t[0] + lambd * run.stats.t[1])
    assert _same_bits(a.grad, run.dx) and _same_bits(b.grad, run.dy)
    ref_loss = X.barlow_twins(z1.double(), z2.double(), lambd)
    bar = X.eps_stats(n) * (float(ref.sc["on"]) + lambd * float(ref.sc["off"])) + 4 * float(RR.ulp32(ref_loss))
    assert abs(float(loss) - float(ref_loss)) <= bar
    # a single process gathers nothing: the global loss is the local one, gradient included
    a2, b2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    gl = S.global_barlow_twins_loss(a2, b2, lambd)
    (gl * 3).backward()
    assert _same_bits(gl.detach(), loss.detach()) and _same_bits(a2.grad, a.grad) and _same_bits(b2.grad, b.grad)
    # a non-contiguous and a row-padded input give the bits of the dense one
    at = z1.t().contiguous().t().requires_grad_(True)
    bp = _padded(z2, 3)[:, :p].requires_grad_(True)
    assert not at.is_contiguous() and bp.stride(0) == p + 3
    l2 = S.barlow_twins_loss(at, bp, lambd)
    (l2 * 3).backward()
    assert _same_bits(l2.detach(), loss.detach()) and _same_bits(at.grad, a.grad) and _same_bits(bp.grad, b.grad)


def test_vicreg_loss_is_the_abi_and_matches_float64():
    n, p = 130, 100
    x = 0.7 * X.random_cols(n, p, seed=83, device=dev)
    y = x + 0.3 * X.random_cols(n, p, seed=84, device=dev)
    # the op's share alone (sim_coeff 0): bit-equal to the ABI run with w = {0, 3 cov / p} and dvar from torch's hinge on the op's variance
    a = x.clone().requires_grad_(True)
    l0 = S.vicreg_loss(a, y, sim_coeff=0.0)
    (l0 * 3).backward()
    probe = Run(x, None, X.VICREG(n), [0.0, 0.0])
    v = probe.var_x.t.clone().requires_grad_(True)
    g3 = torch.tensor(3.0, device=dev)
    ((25.0 * (torch.relu(1.0 - torch.sqrt(v + 1e-4)).mean() / 2)) * g3).backward()
    w = torch.stack([g3 * 0, g3 * 1.0 / p])
    run = Run(x, None, X.VICREG(n), w.tolist(), v.grad)
    check_run("vicreg_loss x3 with dvar", run, Ref(x, None, X.VICREG(n), w.tolist(), v.grad), n)
    assert float(v.grad.abs().max()) > 0 and _same_bits(a.grad, run.dx)
    # the whole loss against float64: the op's bars plus the f32 roundings of the torch terms (mse, hinge: 2^-20 of their values)
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    loss = S.vicreg_loss(a, b)
    (loss * 3).backward()
    a64, b64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    l64 = X.vicreg(a64, b64)
    (l64 * 3).backward()
    sx, sy = X.scales(x, None, X.VICREG(n), 0.0, 1.0), X.scales(y, None, X.VICREG(n), 0.0, 1.0)
    bar = X.eps_stats(n) * (float(sx["off"]) + float(sy["off"])) / p + 2.0 ** -20 * float(l64)
    assert abs(float(loss) - float(l64)) <= bar, (float(loss), float(l64), bar)
    for got, r64, t in ((a.grad, a64.grad, x), (b.grad, b64.grad, y)):
        o = X.forward(t.double(), None, X.VICREG(n))
        dv = 3 * 25.0 * torch.autograd.functional.jacobian(lambda u: torch.relu(1 - torch.sqrt(u + 1e-4)).mean() / 2, o["var_x"])
        sc = X.scales(t, None, X.VICREG(n), 0.0, 3.0 / p, dv)["dx"] + 3 * 25.0 * 2 * (x - y).double().abs() / (n * p)
        assert bool(((got.double() - r64).abs() <= X.eps_grad(n, p) * sc + 4 * RR.ulp32(r64)).all())
    # a single process gathers nothing: the global loss is the local one, gradient included
    a2, b2 = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    gl = S.global_vicreg_loss(a2, b2)
    (gl * 3).backward()
    assert _same_bits(gl.detach(), loss.detach()) and _same_bits(a2.grad, a.grad) and _same_bits(b2.grad, b.grad)


def test_bf16_features():
    """Computed in f32 from the bf16 values; the gradient comes back in bf16: one more rounding (relative 2^-8 at most) on the bar"""
    n, p = 130, 64
    z1 = X.random_cols(n, p, seed=85, device=dev).to(torch.bfloat16)
    z2 = (z1.float() + 0.5 * X.random_cols(n, p, seed=86, device=dev)).to(torch.bfloat16)
    ref = Ref(z1.float(), z2.float(), X.BARLOW(n), [1.0, 5e-3])
    a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    loss = S.barlow_twins_loss(a, b)
    loss.backward()
    assert loss.dtype == torch.float32 and a.grad.dtype == torch.bfloat16 and b.grad.dtype == torch.bfloat16
    for got, r, t32, sc in ((a.grad, ref.dx, ref.t_dx, ref.sc["dx"]), (b.grad, ref.dy, ref.t_dy, ref.sc["dy"])):
        bar, _ = X.bars(r, t32, sc, X.eps_grad(n, p))
        assert bool(((got.double() - r).abs() <= bar + 2.0 ** -8 * r.abs()).all())
    l64 = ref.out["on"] + 5e-3 * ref.out["off"]
    assert abs(float(loss) - float(l64)) <= X.eps_stats(n) * (float(ref.sc["on"]) + 5e-3 * float(ref.sc["off"])) + 4 * float(RR.ulp32(l64))


def test_another_tensor_over_the_same_memory_is_an_operand_of_its_own():
    """The library tells the alias case by the pointer; the Python layer must not hand it x.detach(), a view or a column slice of x
    as y: those are distinct operands (y gets no gradient, or a width of its own), computed as a bit-equal copy would be."""
    n, p = 130, 100
    z = X.random_cols(n, p, seed=91, device=dev)
    a = z.clone().requires_grad_(True)
    on, off, vx, vy = XC.cross_correlation(a, a.detach(), norm=1, ddof=0, eps=1e-5, scale=1.0 / n, diag_target=1.0)
    (on * 0.5 + off * 0.25 + (vy * 2.0).sum()).backward()
    b, c = z.clone().requires_grad_(True), z.clone()
    on2, off2, vx2, vy2 = XC.cross_correlation(b, c, norm=1, ddof=0, eps=1e-5, scale=1.0 / n, diag_target=1.0)
    (on2 * 0.5 + off2 * 0.25 + (vy2 * 2.0).sum()).backward()
    assert not bool(torch.isnan(vy).any()) and _same_bits(vy, vy2) and _same_bits(vx, vx2)
    assert _same_bits(on.detach(), on2.detach()) and _same_bits(off.detach(), off2.detach()) and _same_bits(a.grad, b.grad)
    ref = Ref(z, z.clone(), X.BARLOW(n), [0.5, 0.25], None, torch.full((p,), 2.0, device=dev))
    items = []
    _check("x.detach()", "dx", a.grad, ref.dx, ref.t_dx, ref.sc["dx"], X.eps_grad(n, p), items)
    l1 = S.barlow_twins_loss(a, a.view_as(a).detach())
    assert _same_bits(l1.detach(), S.barlow_twins_loss(z, z.clone()))
    # a column slice shares the pointer and has a padded stride: features against a prefix of themselves
    k = 37
    got = XC.linear_cka(z, z[:, :k])
    assert _same_bits(got, XC.linear_cka(z, z[:, :k].clone()))
    G.log_parity("xcorr x.detach() as y: " + "  ".join(items))


@pytest.mark.parametrize("n,p,q", [(300, 100, 257), (300, 100, None)])
def test_linear_cka(n, p, q):
    x = X.random_cols(n, p, seed=87, device=dev)
    y = x if q is None else X.random_cols(n, q, seed=88, device=dev) + x @ X.random_cols(p, q, seed=89, device=dev) * 0.2
    got = XC.linear_cka(x, y)
    ref = X.linear_cka(x.double(), y.double())
    assert got.dim() == 0 and not got.requires_grad
    # three sums of squares, each within eps_stats of its scale; the ratio's relative bound is their sum (a square root halves two of them)
    rel = 0.0
    for u, v, wgt in ((x, y, 1.0), (x, x, 0.5), (y, y, 0.5)):
        sc = X.scales(u, v, X.CKA, 1.0, 1.0)
        o = X.forward(u.double(), v.double(), X.CKA)
        rel += wgt * X.eps_stats(n) * float(sc["on"] + sc["off"]) / float(o["on"] + o["off"])
    err = abs(float(got) - float(ref))
    G.log_parity(f"xcorr linear_cka n{n} p{p} q{q}: value {float(ref):.6f} error {err:.2e} (bar {rel * float(ref) + 2.0 ** -22:.2e})")
    assert err <= rel * float(ref) + 2.0 ** -22
    if q is None:
        assert abs(float(got) - 1.0) <= 2.0 ** -22


@pytest.mark.parametrize("which", ["barlow", "vicreg"])
def test_one_step_lowers_the_loss_and_reaches_the_trunk(which):
    """Two noisy views through a small stand-in trunk and ProjectionHead"""
    B, D = 64, 64
    g = _gen(90)
    base = torch.randn(B, 3 * 8 * 8, generator=g, device=dev)
    v1, v2 = (base + 0.3 * torch.randn(B, 3 * 8 * 8, generator=g, device=dev) for _ in range(2))
    torch.manual_seed(0)
    trunk = nn.Sequential(nn.Linear(3 * 8 * 8, D), nn.Tanh()).to(dev)
    head = S.ProjectionHead(D, D).to(dev)
    params = list(trunk.parameters()) + list(head.parameters())
    crit = S.global_barlow_twins_loss if which == "barlow" else S.global_vicreg_loss
    opt = torch.optim.SGD(params, lr=0.005)
    loss0 = crit(head(trunk(v1)), head(trunk(v2)))
    loss0.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    assert float(trunk[0].weight.grad.abs().max()) > 0
    opt.step()
    with torch.no_grad():
        loss1 = crit(head(trunk(v1)), head(trunk(v2)))
    assert float(loss1) < float(loss0), (float(loss0), float(loss1))
