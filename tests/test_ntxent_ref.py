"""CPU checks of the NT-Xent / SupCon loss: the algebra the kernels rest on (tests/ntxent_ref.py, float64), the group-id helpers of
bvc.simclr, the refusals the library makes before it launches anything, and that the bars of tests/test_gpu_ntxent.py can tell f32
arithmetic from bf16 operands.  No GPU compute."""
import ctypes

import pytest
import torch

import __graft_entry__ as ge
from tests import ntxent_ref as N

F64 = torch.float64


@pytest.fixture(scope="module")
def bvc():
    ge.build()
    return ge.load_package()


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _view_major(n, views):
    return torch.arange(n) % (n // views)


@pytest.mark.parametrize("n,p,T", [(8, 5, 0.5), (64, 16, 0.1), (30, 7, 0.07)])
def test_two_view_major_views_are_masked_cross_entropy(n, p, T):
    f = N.random_rows(n, p, seed=n, dtype=F64)
    out = N.forward(f, _view_major(n, 2), T)
    assert int(out["m"]) == n and bool((out["npos"] == 1).all())
    assert abs(float(out["loss"] - N.masked_cross_entropy(f, T))) < 1e-13


def test_label_ids_are_supcon_l_out():
    f = N.random_rows(13, 6, seed=1, dtype=F64)
    labels = torch.tensor([0, 1, 0, 2, 1, 0, 3, 4, 4, -1, -1, 2, 5])      # classes 3 and 5 are singletons, -1 belongs to no group
    out = N.forward(f, labels, 0.2)
    assert abs(float(out["loss"] - N.supcon_l_out(f, labels, 0.2))) < 1e-13
    assert out["npos"].tolist() == [2, 1, 2, 1, 1, 2, 0, 1, 1, 0, 0, 1, 0] and int(out["m"]) == 9


def test_closed_form_gradient_is_autograd():
    f = N.random_rows(12, 5, seed=2, dtype=F64)
    g = torch.tensor([0, 1, 2, 0, 1, 2, 3, 3, -1, 4, 0, -5])
    w = torch.randn(12, dtype=F64, generator=torch.Generator().manual_seed(3))
    fx = f.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: (N.forward(x, g, 0.3)["row_loss"] * w).sum(), (fx,), eps=1e-6, atol=1e-7, rtol=1e-6)
    assert _rel(N.closed_grad(f, g, 0.3, w), N.weighted_grad(f, g, 0.3, w)) < 1e-13
    # the mean, and an all-zero row (the clamp of the norm is active: zn = f / eps)
    f[4] = 0.0
    wm = N.mean_weights(g, 3.0)
    fx = f.clone().requires_grad_(True)
    (N.forward(fx, g, 0.3)["loss"] * 3.0).backward()
    assert _rel(N.closed_grad(f, g, 0.3, wm), fx.grad) < 1e-13 and float(fx.grad[4].abs().max()) > 1e3


def test_a_lone_pair_has_loss_zero():
    out = N.forward(N.random_rows(2, 9, seed=4, dtype=F64), torch.tensor([0, 0]), 0.1)
    assert float(out["loss"]) == 0.0 and out["row_loss"].tolist() == [0.0, 0.0] and int(out["m"]) == 2


def test_rows_without_positives_do_not_count():
    f = N.random_rows(10, 4, seed=5, dtype=F64)
    g = torch.tensor([0, 0, 1, 2, 3, -1, -1, 4, 4, 4])
    out = N.forward(f, g, 0.1)
    lone = torch.tensor([2, 3, 4, 5, 6])
    assert int(out["m"]) == 5 and bool((out["row_loss"][lone] == 0).all()) and bool((out["npos"][lone] == 0).all())
    assert abs(float(out["loss"]) - float(out["row_loss"].sum()) / 5) < 1e-15
    # ... but they are negatives of everybody: dropping them changes the other rows
    keep = torch.tensor([0, 1, 7, 8, 9])
    assert float((N.forward(f[keep], g[keep], 0.1)["row_loss"] - out["row_loss"][keep]).abs().min()) > 1e-6
    # two rows with the same NEGATIVE id are not positives of each other, and nobody has positives: loss 0, gradient 0
    none = torch.tensor([-1, -1, 0, 1, 2, 3, 4, 5, 6, 7])
    o2 = N.forward(f, none, 0.1)
    assert float(o2["loss"]) == 0.0 and int(o2["m"]) == 0
    assert float(N.closed_grad(f, none, 0.1, torch.ones(10, dtype=F64)).abs().max()) == 0.0


def test_group_id_helpers(bvc):
    S = bvc.simclr
    assert S.view_groups(6, 2).tolist() == [0, 1, 2, 0, 1, 2] and S.view_groups(6, 2).dtype == torch.int32
    assert S.view_groups(6, 3, "sample").tolist() == [0, 0, 0, 1, 1, 1]
    assert S.view_groups(6, 3, "view").tolist() == [0, 1, 0, 1, 0, 1]
    assert S.global_groups(2, 4, 6, 2).tolist() == [6, 7, 8, 6, 7, 8]
    assert S.global_groups(1, 2, 6, 3, "sample").tolist() == [2, 2, 2, 3, 3, 3]
    for bad in (lambda: S.view_groups(7, 2), lambda: S.view_groups(6, 0), lambda: S.view_groups(6, 2, "rows"),
                lambda: S.global_groups(4, 4, 6, 2), lambda: S.global_groups(0, 2, 7, 2)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("world,n_local,views", [(4, 6, 2), (3, 12, 3)])
def test_emulated_ranks_reproduce_one_global_batch(bvc, world, n_local, views):
    """W ranks each hold `views` view-major views of their own samples; the gathered rows with global_groups carry the ids of ONE
    view-major batch of all samples, up to the permutation of the rows, and the loss does not depend on that permutation."""
    S = bvc.simclr
    b = n_local // views                       # samples per rank
    Bg = world * b
    feats = N.random_rows(Bg * views, 7, seed=world, dtype=F64)      # the global view-major batch: row v Bg + sample
    ids_global = S.view_groups(Bg * views, views).long()
    # rank r holds samples r b .. (r + 1) b - 1: local row v b + k is global row v Bg + r b + k
    perm = torch.tensor([v * Bg + r * b + k for r in range(world) for v in range(views) for k in range(b)])
    gathered_ids = torch.cat([S.global_groups(r, world, n_local, views) for r in range(world)]).long()
    assert torch.equal(gathered_ids, ids_global[perm])
    a = N.forward(feats, ids_global, 0.1)
    g = N.forward(feats[perm], gathered_ids, 0.1)
    assert abs(float(a["loss"] - g["loss"])) < 1e-13 and _rel(g["row_loss"], a["row_loss"][perm]) < 1e-13


def test_cpu_tensors_and_bad_arguments_are_refused(bvc):
    S = bvc.simclr
    with pytest.raises(bvc._lib.BvcError):
        S.nt_xent_loss(torch.randn(8, 16))
    with pytest.raises(bvc._lib.BvcError):
        S.global_nt_xent_loss(torch.randn(8, 16))
    with pytest.raises(ValueError):
        S.nt_xent_loss(torch.randn(8), 0.1)


NEW_SYMBOLS = ("bvc_op_ntxent_splits", "bvc_op_ntxent_block_rows", "bvc_op_ntxent_workspace", "bvc_op_ntxent_fwd", "bvc_op_ntxent_bwd")


def test_symbols_are_declared_and_exported(bvc):
    import os
    header = open(os.path.join(ge.ROOT, "include", "bvc.h")).read()
    lib = bvc._lib.lib()
    for name in NEW_SYMBOLS:
        assert name in bvc._lib.SYMBOLS and name + "(" in header and getattr(lib, name) is not None


def test_refusals_launch_nothing(bvc):
    """n, p, temperature, views, strides and null pointers are checked before any launch: the calls below pass a dummy host pointer."""
    lib = bvc._lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(n=8, pw=16, T=0.1, views=2, groups=None, ldf=None, splits=0, f=p, eps=1e-8):
        return lib.bvc_op_ntxent_fwd(f, pw if ldf is None else ldf, groups, views, n, pw, T, eps, splits, p, p, p, p, p, None)

    def bwd(n=8, pw=16, T=0.1, views=2, groups=None, block_rows=0, lddf=None):
        return lib.bvc_op_ntxent_bwd(p, pw, groups, views, n, pw, T, 1e-8, p, p, p, 0, block_rows, p, pw if lddf is None else lddf, p, None)

    for call, word in ((lambda: fwd(n=0), b"n 0"), (lambda: fwd(n=32769), b"n 32769"), (lambda: fwd(pw=0), b"p 0"),
                       (lambda: fwd(pw=8193), b"p 8193"), (lambda: fwd(T=0.0), b"temperature"), (lambda: fwd(T=-1.0), b"temperature"),
                       (lambda: fwd(T=float("nan")), b"temperature"), (lambda: fwd(T=float("inf")), b"temperature"),
                       (lambda: fwd(views=0), b"views"), (lambda: fwd(views=3), b"views"), (lambda: fwd(ldf=15), b"stride"),
                       (lambda: fwd(splits=-1), b"key_splits"), (lambda: fwd(splits=257), b"key_splits"), (lambda: fwd(f=None), b"null"),
                       (lambda: fwd(eps=0.0), b"eps"),
                       (lambda: bwd(n=0), b"n 0"), (lambda: bwd(T=0.0), b"temperature"), (lambda: bwd(views=3), b"views"),
                       (lambda: bwd(block_rows=-1), b"block_rows"), (lambda: bwd(lddf=15), b"stride")):
        assert call() != 0 and word in lib.bvc_last_error(), (word, lib.bvc_last_error())
    # with explicit group ids `views` is not looked at
    assert lib.bvc_op_ntxent_workspace(0, 16, 0, 0) == -1 and lib.bvc_op_ntxent_workspace(8, 0, 0, 0) == -1
    assert lib.bvc_op_ntxent_splits(0, 16) == -1 and lib.bvc_op_ntxent_block_rows(8, 9000) == -1
    # automatic choices: at least two workgroups per CU at the config-5 shape, the E block under its cap
    assert lib.bvc_op_ntxent_splits(8192, 768) == 8 and lib.bvc_op_ntxent_splits(100, 64) == 1
    assert lib.bvc_op_ntxent_block_rows(8192, 768) == 8192 and lib.bvc_op_ntxent_block_rows(32768, 768) == 2048
    assert lib.bvc_op_ntxent_block_rows(3, 1) == 128
    ws = lib.bvc_op_ntxent_workspace(300, 100, 0, 0)
    assert ws > 0 and ws % 16 == 0 and lib.bvc_op_ntxent_workspace(300, 100, 7, 128) != ws


# ---------------------------------------------------------------------------------------------- the bars can tell f32 from bf16
def test_bars_reject_the_bf16_operand_model():
    """On the correlated case (cos 0.99, 256 x 128, T = 0.1) the bars of tests/test_gpu_ntxent.py - built from the float64 reference,
    the f32 comparator and eps_row, nothing else - must hold for an f32 run of the closed form and FAIL for the bf16-operand model,
    for the row loss and for the gradient."""
    n, p, T = 256, 128, 0.1
    f = N.correlated_rows(n, p, seed=7)
    g = _view_major(n, 2)
    f64 = f.double()
    cosines = N.normalise(f64) @ N.normalise(f64).t()
    assert 0.985 < float(cosines.mean()) < 0.995
    w = N.mean_weights(g)
    ref = N.forward(f64, g, T)
    ref_df = N.weighted_grad(f64, g, T, w)
    sc = N.scales(f64, g, T, w)
    er = N.eps_row(sc)
    t32 = N.forward(f, g, T)
    t32_df = N.weighted_grad(f, g, T, w.float())
    bar_l, _ = N.bars(ref["row_loss"], t32["row_loss"], sc["row_loss"], er)
    bar_g, _ = N.bars(ref_df, t32_df, sc["df"], 4 * er.amax().reshape(1, 1))
    # the closed form in f32 is inside
    c32 = N.forward(f, g, T)["row_loss"].double()
    assert bool(((c32 - ref["row_loss"]).abs() <= bar_l).all())
    assert bool(((N.closed_grad(f, g, T, w.float()).double() - ref_df).abs() <= bar_g).all())
    # the bf16-operand model is far outside, in most rows
    b_l = (N.forward(f, g, T, bf16=True)["row_loss"].double() - ref["row_loss"]).abs()
    b_g = (N.closed_grad(f, g, T, w.float(), bf16=True).double() - ref_df).abs()
    assert float((b_l / bar_l).max()) > 10 and float((b_l > bar_l).double().mean()) > 0.5
    assert float((b_g / bar_g).max()) > 10 and float((b_g > bar_g).any(1).double().mean()) > 0.5
