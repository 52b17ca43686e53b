"""NT-Xent / SupCon loss on the GPU: bvc_op_ntxent_fwd / _bwd (csrc/ntxent.hip) through the C ABI against the float64 reference of
tests/ntxent_ref.py, and bvc.simclr.nt_xent_loss / global_nt_xent_loss on top of them.  The rules of tests/test_gpu_attentive.py
apply: Guarded buffers with guard bands, outputs and the workspace pre-filled with NaN, f with a NaN-filled row padding
(ldf = p + pad: reading it poisons the result), the padding of df must keep its NaN bits, one parity-report line per case.

Bars (nothing in them comes from the code under test).  The scale of an output element is the float64 sum of the magnitudes of its
terms (ntxent_ref.scales).  The bar of an element is its scale times the larger of
  * 4 x the worst error, relative to the scale, of the same dense formulas run by torch in float32 on the same device inputs, and
  * k eps_row, eps_row_i = 2^-23 (2 + A_i + S_i), A_i = max |s_ik - D_i| over the terms whose softmax weight is >= 2^-30,
    S_i = max_k sum_d |zn_id zn_kd| / T.  Derivation: a score is a chain of p f32 products, so its error is at most 2^-24 per
    rounding of sum_d |zn_id zn_kd| / T <= S_i (2^-23 S_i with the roundings of the two normalised operands); exp(s - D) of a
    1-ulp hardware exponential is off by a relative 2^-23 plus the error of its argument, 2^-24 (|s - D|) <= 2^-23 A_i for the
    subtraction and the score error above; the 2 covers the roundings of the sum and of the logarithm.  k = 1 for the row loss;
    k = 4 for df, whose rows mix the exponentials of every row (two per element of E, times the two products of the normalisation
    backward): it takes the largest eps_row of the batch;
with the file's floor of 4 ulp of the reference value.  lse is held ABSOLUTELY: |error| <= max(eps_row_i, 4 x torch's worst
absolute error).  npos and m are exact.  The mean loss is a mean of row losses: its bar is the mean of their bars.
"""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():   # collected on the CPU box, run on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G          # noqa: E402
from tests import ntxent_ref as N        # noqa: E402
from tests import rowops_ref as RR       # noqa: E402
from tests.test_gpu_rowops import Guarded, _same_bits     # noqa: E402

L = G.L
bvc = G.bvc
S = bvc.simclr
dev = "cuda"
F64 = torch.float64
EPS = 1e-8


def _gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _grouping(kind, n, seed):
    """(groups tensor passed to the ABI or None, views, int64 ids for the reference)"""
    if kind[0] == "v":
        views = int(kind[1:])
        return None, views, S.view_groups(n, views, device=dev).long()
    g = torch.randint(0, max(2, n // 3), (n,), generator=_gen(seed), device=dev)
    g[torch.rand(n, generator=_gen(seed + 1), device=dev) < 0.1] = -1           # no group
    g[n // 2] = 10 ** 6                                                          # a singleton class
    return g.to(torch.int32), 0, g.long()


class Ref:
    """float64 reference, torch-f32 comparator and scales of one set of inputs (computed once per case)."""

    def __init__(self, f, ids, T, w=None, gout=1.0):
        f64 = f.double()
        self.w = N.mean_weights(ids, gout) if w is None else w.double()
        self.out = N.forward(f64, ids, T)
        self.df = N.weighted_grad(f64, ids, T, self.w)
        self.t_out = N.forward(f, ids, T)
        self.t_df = N.weighted_grad(f, ids, T, self.w.float())
        self.sc = N.scales(f64, ids, T, self.w)
        self.eps_row = N.eps_row(self.sc)


class Run:
    """One forward and one backward through the C ABI on guarded, NaN-filled buffers."""

    def __init__(self, f, T, groups, views, w, splits=0, block_rows=0, pad=0, ws_fill="nan", eps=EPS):
        n, p = f.shape
        ld = p + pad
        self.fb = torch.full((n, ld), float("nan"), device=dev)
        self.fb[:, :p] = f
        lib, st = L.lib(), G.stream()
        nbytes = lib.bvc_op_ntxent_workspace(n, p, splits, block_rows)
        assert nbytes > 0 and nbytes % 16 == 0
        self.row_loss, self.lse, self.stats = Guarded((n,), row=n), Guarded((n,), row=n), Guarded((2,))
        self.npos = Guarded((n,), dtype=torch.int32, fill=-7, row=n)
        self.ws = Guarded((nbytes // 4,), fill=ws_fill, row=p)
        self.df = Guarded((n, ld), row=ld)
        gp = None if groups is None else groups.data_ptr()
        L.check(lib.bvc_op_ntxent_fwd(self.fb.data_ptr(), ld, gp, views, n, p, T, eps, splits, self.row_loss.t.data_ptr(),
                                      self.lse.t.data_ptr(), self.npos.t.data_ptr(), self.stats.t.data_ptr(), self.ws.t.data_ptr(), st),
                "bvc_op_ntxent_fwd")
        if ws_fill == "nan":
            self.ws.t.fill_(float("nan"))      # nothing survives from the forward to the backward
        w32 = w.float().contiguous()
        L.check(lib.bvc_op_ntxent_bwd(self.fb.data_ptr(), ld, gp, views, n, p, T, eps, self.lse.t.data_ptr(), self.npos.t.data_ptr(),
                                      w32.data_ptr(), splits, block_rows, self.df.t.data_ptr(), ld, self.ws.t.data_ptr(), st),
                "bvc_op_ntxent_bwd")
        torch.cuda.synchronize()
        for name in ("row_loss", "lse", "stats", "npos", "ws", "df"):
            getattr(self, name).check(name)
        self.df_rows = self.df.t[:, :p]
        if pad:
            assert bool(torch.isnan(self.df.t[:, p:]).all()), "the padding of df was written"
        assert not bool(torch.isnan(self.df_rows).any()), "df: NaN or elements not written"
        assert not bool(torch.isnan(self.row_loss.t).any() | torch.isnan(self.lse.t).any() | torch.isnan(self.stats.t).any()), "NaN in an output"
        assert not bool((self.npos.t == -7).any()), "npos not written"


def _check(name, key, got, ref, t32, scale, eps_rel, items):
    bar, wt = N.bars(ref, t32, scale, eps_rel)
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


def check_run(name, run, ref):
    items = []
    try:
        o, t, er = ref.out, ref.t_out, ref.eps_row
        assert torch.equal(run.npos.t.long(), o["npos"]), f"{name}: npos differs"
        assert float(run.stats.t[1]) == float(o["m"]), f"{name}: m {float(run.stats.t[1])} != {int(o['m'])}"
        # lse: absolute; an empty sum (n = 1) is -inf on both sides
        fin = torch.isfinite(o["lse"])
        assert torch.equal(run.lse.t[~fin].double(), o["lse"][~fin])
        terr = float((t["lse"].double() - o["lse"])[fin].abs().max()) if bool(fin.any()) else 0.0
        err = (run.lse.t.double() - o["lse"])[fin].abs()
        items.append(f"lse {float(err.max()) if err.numel() else 0.0:.2e}/{terr:.2e} (abs)")
        bad = ~(err <= torch.clamp(er[fin], min=4 * terr))
        assert not bool(bad.any()), f"{name} lse: {int(bad.sum())} over the bar, worst error {float(err.max()):.3e}, eps_row {float(er.min()):.3e}"
        bar_l = _check(name, "row_loss", run.row_loss.t, o["row_loss"], t["row_loss"], ref.sc["row_loss"], er, items)
        has = o["npos"] > 0
        bar_loss = float(bar_l[has].mean()) if bool(has.any()) else 0.0
        lerr = abs(float(run.stats.t[0]) - float(o["loss"]))
        items.append(f"loss {lerr:.2e} (bar {bar_loss:.2e})")
        assert lerr <= bar_loss + 4 * float(RR.ulp32(o["loss"])), f"{name} loss: error {lerr:.3e}, bar {bar_loss:.3e}"
        _check(name, "df", run.df_rows, ref.df, ref.t_df, ref.sc["df"], 4 * er.amax().reshape(1, 1), items)
    finally:
        G.log_parity(f"ntxent {name}: " + "  ".join(items) + "   (kernel/torch-f32, relative to the element's scale)")


def _case(f, T, kind, seed, w=None, gout=1.0, **kw):
    groups, views, ids = _grouping(kind, f.shape[0], seed)
    ref = Ref(f, ids, T, w, gout)
    return Run(f, T, groups, views, ref.w, **kw), ref


# ---------------------------------------------------------------------------------------------- shapes
# (n, p, pad, key_splits, block_rows, grouping): every n edge of the 128-row / 128-key tile, every p edge of the 32-float K stage,
# forced splits including empty ones (n < 128 x splits), several row blocks with a partial last one (n = 300: 384 padded rows),
# 2, 3 and 4 view-major views whose positives straddle tile boundaries (n >= 257), label ids on odd n, one realistic shape
SHAPES = [
    (1, 1, 0, 0, 0, "v1"), (2, 3, 1, 1, 0, "v2"), (3, 31, 8, 2, 0, "v3"), (127, 32, 0, 3, 0, "labels"), (128, 33, 1, 7, 0, "v4"),
    (129, 100, 0, 0, 0, "v3"), (257, 1, 8, 2, 128, "labels"), (257, 100, 1, 3, 0, "labels"), (300, 768, 0, 7, 0, "v2"),
    (300, 33, 8, 1, 128, "v3"), (300, 100, 1, 2, 256, "v4"), (300, 31, 0, 0, 0, "v2"), (2048, 768, 0, 0, 0, "v2"),
]


@pytest.mark.parametrize("n,p,pad,splits,block_rows,kind", SHAPES)
def test_against_float64(n, p, pad, splits, block_rows, kind):
    f = N.random_rows(n, p, seed=n * 10 + p, device=dev)
    run, ref = _case(f, 0.1, kind, seed=n + p, pad=pad, splits=splits, block_rows=block_rows)
    check_run(f"n{n} p{p} pad{pad} splits{splits} rows{block_rows} {kind}", run, ref)
    if kind == "v2" and n >= 2:
        assert abs(float(ref.out["loss"]) - float(N.masked_cross_entropy(f.double(), 0.1))) < 1e-12


def test_automatic_choices():
    lib = L.lib()
    assert lib.bvc_op_ntxent_splits(2048, 768) == 16 and lib.bvc_op_ntxent_block_rows(2048, 768) == 2048
    assert lib.bvc_op_ntxent_workspace(300, 100, 0, 0) == lib.bvc_op_ntxent_workspace(300, 100, 3, 384)


# ---------------------------------------------------------------------------------------------- hard cases
@pytest.mark.parametrize("T", [0.5, 0.1, 0.07, 0.01])
def test_temperatures_with_the_row_maximum_in_the_first_and_in_the_last_key_tile(T):
    """Duplicated rows: scores reach 1 / T (100 at T = 0.01, where a sum without max subtraction overflows).  Row 0's maximum is at
    key 1 (first key tile), row 5's at key n - 1 (last key tile), row n - 1's at key 5."""
    n, p = 300, 100
    f = N.random_rows(n, p, seed=61, device=dev)
    f[1] = f[0]
    f[n - 1] = f[5]
    for splits in (1, 3):
        run, ref = _case(f, T, "v2", seed=0, splits=splits)
        assert abs(float(ref.out["s"][0, 1]) - 1 / T) < 1e-9 / T and abs(float(ref.out["s"][5, n - 1]) - 1 / T) < 1e-9 / T
        assert bool(torch.isfinite(run.lse.t).all() & torch.isfinite(run.df_rows).all())
        check_run(f"T{T} duplicates splits{splits}", run, ref)


@pytest.mark.parametrize("n,p", [(256, 128), (300, 768)])
def test_correlated_rows(n, p):
    f = N.correlated_rows(n, p, seed=62, device=dev)
    run, ref = _case(f, 0.1, "v2", seed=0)
    check_run(f"correlated cos0.99 n{n} p{p}", run, ref)


def test_label_ids_with_singletons_and_negative_ids():
    n, p = 200, 48
    f = N.random_rows(n, p, seed=63, device=dev)
    g = torch.randint(0, 12, (n,), generator=_gen(64), device=dev)
    g[:40] = -1 - torch.arange(40, device=dev) % 3            # negative ids, equal ones included: no group
    g[40:50] = 100 + torch.arange(10, device=dev)             # singleton classes
    ids = g.long()
    ref = Ref(f, ids, 0.07)
    assert int((ref.out["npos"] == 0).sum()) == 50 and int(ref.out["m"]) == 150
    w = ref.w.clone()
    w[:50] = float("nan")                                      # the weight of a row without positives is not looked at
    run = Run(f, 0.07, g.to(torch.int32), 0, w, splits=2)
    assert bool((run.row_loss.t[:50] == 0).all())
    check_run("labels singletons negative ids", run, ref)


def test_no_row_has_positives():
    n, p = 130, 20
    f = N.random_rows(n, p, seed=65, device=dev)
    g = torch.arange(n, device=dev, dtype=torch.int32)         # every row its own class
    g[::2] = -1
    run = Run(f, 0.1, g, 0, torch.ones(n, device=dev), splits=2)
    assert float(run.stats.t[0]) == 0.0 and float(run.stats.t[1]) == 0.0 and bool((run.row_loss.t == 0).all())
    assert bool((run.df_rows == 0).all()), "df is not exactly 0"
    check_run("no positives", run, Ref(f, g.long(), 0.1, torch.ones(n, device=dev)))


def test_an_all_zero_row():
    """|f_i| = 0 <= eps: the clamp is active, zn_i = 0, every score of the row is 0 and df_i = dzn_i / eps"""
    n, p = 130, 40
    f = N.random_rows(n, p, seed=66, device=dev)
    f[3] = 0.0
    f[129] = 0.0
    run, ref = _case(f, 0.1, "v2", seed=0)
    assert float(ref.df[3].abs().max()) > 1e3
    check_run("zero rows", run, ref)


def test_random_row_weights():
    n, p = 257, 64
    f = N.random_rows(n, p, seed=67, device=dev)
    w = torch.randn(n, generator=_gen(68), device=dev)
    run, ref = _case(f, 0.1, "v2" if n % 2 == 0 else "labels", seed=3, w=w, block_rows=128)
    check_run("random row weights", run, ref)


# ---------------------------------------------------------------------------------------------- invariants
def _out_bits(r):
    return [r.row_loss.t, r.lse.t, r.stats.t, r.npos.t, r.df_rows]


def test_same_bits_on_every_run_and_whatever_the_workspace_held():
    f = N.random_rows(300, 100, seed=71, device=dev)
    ids = S.view_groups(300, 3, device=dev).long()
    w = N.mean_weights(ids)
    a = Run(f, 0.1, None, 3, w, splits=3, block_rows=128)
    b = Run(f, 0.1, None, 3, w, splits=3, block_rows=128)
    c = Run(f, 0.1, None, 3, w, splits=3, block_rows=128, ws_fill=0.0)
    d = Run(f, 0.1, None, 3, w, splits=3, block_rows=128, ws_fill=1e30)
    for o in (b, c, d):
        for x, y in zip(_out_bits(a), _out_bits(o)):
            assert _same_bits(x, y)
    # explicit ids equal to the view-major default give the same bits, and so does another row blocking
    e = Run(f, 0.1, ids.to(torch.int32), 0, w, splits=3, block_rows=256)
    for x, y in zip(_out_bits(a), _out_bits(e)):
        assert _same_bits(x, y)


def test_refused_arguments_write_nothing():
    n, p = 8, 16
    f = N.random_rows(n, p, seed=72, device=dev)
    lib, st = L.lib(), G.stream()
    outs = [Guarded((n,), row=n), Guarded((n,), row=n), Guarded((n,), row=n), Guarded((2,)), Guarded((4096,)), Guarded((n, p), row=p)]
    rl, lse, npos, stats, ws, df = outs
    w = torch.ones(n, device=dev)

    def fwd(n_=n, p_=p, T=0.1, views=2, splits=0):
        return lib.bvc_op_ntxent_fwd(f.data_ptr(), p, None, views, n_, p_, T, EPS, splits, rl.t.data_ptr(), lse.t.data_ptr(), npos.t.data_ptr(),
                                     stats.t.data_ptr(), ws.t.data_ptr(), st)

    def bwd(n_=n, p_=p, T=0.1, views=2, block_rows=0):
        return lib.bvc_op_ntxent_bwd(f.data_ptr(), p, None, views, n_, p_, T, EPS, lse.t.data_ptr(), npos.t.data_ptr(), w.data_ptr(), 0,
                                     block_rows, df.t.data_ptr(), p, ws.t.data_ptr(), st)

    for call, word in ((lambda: fwd(n_=0), b"n 0"), (lambda: fwd(n_=40000), b"n 40000"), (lambda: fwd(p_=0), b"p 0"),
                       (lambda: fwd(p_=8200), b"p 8200"), (lambda: fwd(T=0.0), b"temperature"), (lambda: fwd(T=float("nan")), b"temperature"),
                       (lambda: fwd(views=3), b"views"), (lambda: fwd(views=0), b"views"), (lambda: fwd(splits=-2), b"key_splits"),
                       (lambda: bwd(n_=0), b"n 0"), (lambda: bwd(T=-0.1), b"temperature"), (lambda: bwd(views=5), b"views"),
                       (lambda: bwd(block_rows=-128), b"block_rows")):
        assert call() != 0 and word in lib.bvc_last_error(), (word, lib.bvc_last_error())
    torch.cuda.synchronize()
    for o in outs:
        o.check("refused call")
        assert bool(torch.isnan(o.t).all()), "a refused call wrote an output"


# ---------------------------------------------------------------------------------------------- bvc.simclr
def test_nt_xent_loss_is_the_abi_and_matches_float64():
    n, p, T = 300, 100, 0.1
    f = N.random_rows(n, p, seed=81, device=dev)
    ids = S.view_groups(n, 2, device=dev).long()
    # mean, (loss * 3).backward()
    ref = Ref(f, ids, T, gout=3.0)
    run = Run(f, T, None, 2, ref.w)
    x = f.clone().requires_grad_(True)
    loss = S.nt_xent_loss(x, T)
    (loss * 3).backward()
    assert loss.dim() == 0 and _same_bits(loss.detach(), run.stats.t[0]) and _same_bits(x.grad, run.df_rows)
    check_run("nt_xent_loss mean x3", run, ref)
    # none, random upstream gradients per row; explicit ids in the sample-major layout of the same pairs
    perm = torch.arange(n, device=dev).reshape(2, n // 2).t().reshape(-1)          # sample-major row 2 s + v = view-major row v B + s
    u = torch.randn(n, generator=_gen(82), device=dev)
    x2 = f[perm].clone().requires_grad_(True)
    rows = S.nt_xent_loss(x2, T, groups=S.view_groups(n, 2, "sample", device=dev), reduction="none")
    assert rows.shape == (n,)
    (rows * u).sum().backward()
    ref2 = Ref(f[perm], ids[perm], T, w=u)
    items = []
    _check("none", "row_loss", rows.detach(), ref2.out["row_loss"], ref2.t_out["row_loss"], ref2.sc["row_loss"], ref2.eps_row, items)
    _check("none", "df", x2.grad, ref2.df, ref2.t_df, ref2.sc["df"], 4 * ref2.eps_row.amax().reshape(1, 1), items)
    G.log_parity("ntxent nt_xent_loss none, sample-major ids: " + "  ".join(items))
    # int64 ids on the host are checked and moved; ids beyond int32 are refused
    S.nt_xent_loss(f, T, groups=ids.cpu())
    with pytest.raises(ValueError):
        S.nt_xent_loss(f, T, groups=(ids + 2 ** 31).cpu())
    with pytest.raises(ValueError):
        S.nt_xent_loss(f, T, views=7)
    # a single process gathers nothing: the global loss is the local one, gradient included
    x3 = f.clone().requires_grad_(True)
    gl = S.global_nt_xent_loss(x3, T)
    (gl * 3).backward()
    assert _same_bits(gl.detach(), loss.detach()) and _same_bits(x3.grad, x.grad)
    labels = torch.randint(0, 20, (n,), generator=_gen(83), device=dev)
    assert _same_bits(S.global_nt_xent_loss(f, T, groups_local=labels), S.nt_xent_loss(f, T, groups=labels))


def test_bf16_features():
    """Computed in f32 from the bf16 values; the gradient comes back in bf16: one more rounding (relative 2^-8 at most) on the bar"""
    n, p, T = 130, 64, 0.1
    fb = N.random_rows(n, p, seed=84, device=dev).to(torch.bfloat16)
    ids = S.view_groups(n, 2, device=dev).long()
    ref = Ref(fb.float(), ids, T)
    x = fb.clone().requires_grad_(True)
    loss = S.nt_xent_loss(x, T)
    loss.backward()
    assert loss.dtype == torch.float32 and x.grad.dtype == torch.bfloat16
    bar, _ = N.bars(ref.df, ref.t_df, ref.sc["df"], 4 * ref.eps_row.amax().reshape(1, 1))
    assert bool(((x.grad.double() - ref.df).abs() <= bar + 2.0 ** -8 * ref.df.abs()).all())
    bar_l, _ = N.bars(ref.out["row_loss"], ref.t_out["row_loss"], ref.sc["row_loss"], ref.eps_row)
    assert abs(float(loss) - float(ref.out["loss"])) <= float(bar_l.mean()) + 4 * float(RR.ulp32(ref.out["loss"]))


def test_one_step_lowers_the_loss_and_reaches_the_trunk():
    """Two view-major views (the row order ClipAugment(views=2) returns) through a small stand-in trunk and ProjectionHead"""
    B, D = 64, 64
    g = _gen(85)
    base = torch.randn(B, 3 * 8 * 8, generator=g, device=dev)
    views = torch.cat([base + 0.3 * torch.randn(B, 3 * 8 * 8, generator=g, device=dev) for _ in range(2)])      # rows [:B], [B:]
    torch.manual_seed(0)
    trunk = nn.Sequential(nn.Linear(3 * 8 * 8, D), nn.Tanh()).to(dev)
    head = S.ProjectionHead(D, D).to(dev)
    params = list(trunk.parameters()) + list(head.parameters())
    opt = torch.optim.SGD(params, lr=0.5)
    loss0 = S.global_nt_xent_loss(head(trunk(views)), 0.5)
    loss0.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    assert float(trunk[0].weight.grad.abs().max()) > 0
    opt.step()
    with torch.no_grad():
        loss1 = S.global_nt_xent_loss(head(trunk(views)), 0.5)
    assert float(loss1) < float(loss0), (float(loss0), float(loss1))
