"""CPU checks of the prototype cross-entropy (DINO): the algebra the kernels rest on (tests/proto_ce_ref.py, float64), the pair
construction, centre update, temperature schedule and head of bvc.dino against the original's, the refusals the library makes
before it launches anything, and that the bars of tests/test_gpu_proto_ce.py can tell f32 arithmetic from bf16 operands.
No GPU compute."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as ge
from tests import proto_ce_ref as P

F64 = torch.float64


@pytest.fixture(scope="module")
def bvc():
    ge.build()
    return ge.load_package()


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _center(K, seed, scale=0.3):
    return scale * torch.randn(K, dtype=F64, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------- the algebra
@pytest.mark.parametrize("m,K,p,tau_s,tau_t,centred", [(7, 11, 5, 0.1, 0.04, True), (12, 30, 8, 1.0, 0.07, False), (5, 3, 2, 0.1, 1.0, True)])
def test_closed_form_gradients_are_autograd(m, K, p, tau_s, tau_t, centred):
    xs, vs, xt, vt = P.problem(m, K, p, seed=m, dtype=F64)
    c = _center(K, 3) if centred else None
    w = torch.randn(m, dtype=F64, generator=torch.Generator().manual_seed(4))
    a_x, a_v = P.weighted_grad(xs, vs, xt, vt, c, tau_s, tau_t, w)
    c_x, c_v = P.closed_grad(xs, vs, xt, vt, c, tau_s, tau_t, w)
    assert _rel(c_x, a_x) < 1e-12 and _rel(c_v, a_v) < 1e-12
    # the mean's weights are gout / m
    x = xs.clone().requires_grad_(True)
    v = vs.clone().requires_grad_(True)
    (P.forward(x, v, xt, vt, c, tau_s, tau_t)["loss"] * 3.0).backward()
    m_x, m_v = P.closed_grad(xs, vs, xt, vt, c, tau_s, tau_t, torch.full((m,), 3.0 / m, dtype=F64))
    assert _rel(m_x, x.grad) < 1e-12 and _rel(m_v, v.grad) < 1e-12


def test_closed_form_with_a_zero_student_row_and_a_zero_prototype():
    """the clamp of the row norm is active (xsn = xs / eps, dxs = dxsn / eps); a zero prototype row scores 0 and gets no gradient"""
    xs, vs, xt, vt = P.problem(6, 9, 4, seed=2, dtype=F64)
    xs[2] = 0.0
    vs[5] = 0.0
    w = torch.ones(6, dtype=F64) / 6
    a_x, a_v = P.weighted_grad(xs, vs, xt, vt, None, 0.1, 0.04, w)
    c_x, c_v = P.closed_grad(xs, vs, xt, vt, None, 0.1, 0.04, w)
    assert _rel(c_x, a_x) < 1e-12 and _rel(c_v, a_v) < 1e-12
    assert float(c_x[2].abs().max()) > 1e6 and float(c_v[5].abs().max()) == 0.0 and float(a_v[5].abs().max()) == 0.0
    out = P.forward(xs, vs, xt, vt, None, 0.1, 0.04)
    assert out["zero_protos"] == 1 and bool((out["s"][:, 5] == 0).all()) and bool((out["s"][2] == 0).all())


def test_row_loss_is_cross_entropy_with_soft_targets():
    xs, vs, xt, vt = P.problem(9, 17, 6, seed=5, dtype=F64)
    c = _center(17, 6)
    out = P.forward(xs, vs, xt, vt, c, 0.1, 0.04)
    assert _rel(out["row_loss"], F.cross_entropy(out["s"], out["q"], reduction="none")) < 1e-13
    assert abs(float(out["q"].sum(1).max()) - 1) < 1e-13
    # and DINO's own expression over the logits
    lg_s, lg_t = P.logits(xs, vs), P.logits(xt, vt)
    dino = torch.sum(-F.softmax((lg_t - c) / 0.04, dim=-1) * F.log_softmax(lg_s / 0.1, dim=-1), dim=-1)
    assert _rel(out["row_loss"], dino) < 1e-13
    assert _rel(out["batch_center"], lg_t.mean(0)) < 1e-13


def test_row_loss_is_at_least_the_entropy_of_the_targets():
    xs, vs, xt, vt = P.problem(10, 13, 5, seed=7, dtype=F64)
    out = P.forward(xs, vs, xt, vt, None, 0.1, 0.07)
    H = -(out["q"] * torch.log(out["q"])).sum(1)
    assert bool((out["row_loss"] >= H).all()) and float((out["row_loss"] - H).min()) > 1e-6
    # equality when the student's and the teacher's scores coincide: same operands, same temperature, no centre
    same = P.forward(xs, vs, xs, vs, None, 0.07, 0.07)
    Hs = -(same["q"] * torch.log(same["q"])).sum(1)
    assert _rel(same["row_loss"], Hs) < 1e-13
    gx, gv = P.closed_grad(xs, vs, xs, vs, None, 0.07, 0.07, torch.ones(10, dtype=F64))
    assert float(gx.abs().max()) < 1e-13 and float(gv.abs().max()) < 1e-13
    # with different temperatures the gradient is not zero
    gx2, _ = P.closed_grad(xs, vs, xs, vs, None, 0.1, 0.04, torch.ones(10, dtype=F64))
    assert float(gx2.abs().max()) > 1e-3


@pytest.mark.parametrize("K,splits,seed", [(1, 1, 0), (127, 3, 1), (300, 2, 2), (300, 7, 3), (1000, 5, 4)])
def test_online_recurrence_equals_the_dense_value(K, splits, seed):
    """the five-number recurrence over a random tile order, any split count (empty splits included: K = 300 is three tiles)"""
    xs, vs, xt, vt = P.problem(6, K, 8, seed=seed + 20, dtype=F64)
    out = P.forward(xs, vs, xt, vt, _center(K, 9, 2.0), 0.1, 0.04)
    ntiles = (K + 127) // 128
    order = torch.randperm(ntiles, generator=torch.Generator().manual_seed(seed)).tolist()
    for tile_order in (list(range(ntiles)), order, order[::-1]):
        row, Ls, Lt = P.online(out["s"], out["t"], tile_order, splits)
        assert _rel(row, out["row_loss"]) < 1e-12 and _rel(Ls, out["lse_s"]) < 1e-13 and _rel(Lt, out["lse_t"]) < 1e-13


# ---------------------------------------------------------------------------------------------- bvc.dino against the original
@pytest.mark.parametrize("local", [0, 2, 6])
def test_pair_construction_is_the_original_double_loop(bvc, local):
    D = bvc.dino
    B, p, K, views = 5, 6, 19, 2 + local
    student, teacher = P.random_rows(views * B, p, 1, dtype=F64), P.random_rows(2 * B, p, 2, dtype=F64)
    vs, vt = P.random_rows(K, p, 3, dtype=F64), P.random_rows(K, p, 4, dtype=F64)
    c = _center(K, 5)
    want = P.dino_double_loop(P.logits(student, vs), P.logits(teacher, vt), c, 0.1, 0.04, views)
    assert len(D.view_pairs(views, 2)) == 2 * views - 2
    for max_rows in (D.MAX_ROWS, 2 * B, 1):          # one call, chunks of two pairs, one pair per call
        chunks = D.paired_rows(student, teacher, views, 2, max_rows=max_rows)
        got = sum(P.forward(xs, vs, xt, vt, c, 0.1, 0.04)["loss"] * share for xs, xt, share in chunks)
        assert abs(float(got - want)) < 1e-13 * abs(float(want))
        bc = sum(P.forward(xs, vs, xt, vt, c, 0.1, 0.04)["batch_center"] * share for xs, xt, share in chunks)
        assert _rel(bc, P.logits(teacher, vt).mean(0)) < 1e-13
    assert len(D.paired_rows(student, teacher, views, 2)) == 1
    for bad in (lambda: D.paired_rows(student, teacher, 1, 2), lambda: D.paired_rows(student[:-1], teacher, views, 2),
                lambda: D.paired_rows(student, teacher[:-1], views, 2)):
        with pytest.raises(ValueError):
            bad()


def test_centre_update_is_the_original_sum_over_ranks(bvc):
    D = bvc.dino
    B, p, K, world, mom = 4, 6, 11, 3, 0.9
    vt = P.random_rows(K, p, 1, dtype=F64)
    teachers = [P.random_rows(2 * B, p, 10 + r, dtype=F64) for r in range(world)]
    center0 = _center(K, 2).reshape(1, K)
    want = P.center_update_original(center0, [P.logits(t, vt) for t in teachers], mom)
    # every rank's batch_center is the mean of its raw teacher scores over the pair rows; the all-reduce is a mean over the ranks
    bcs = []
    for t in teachers:
        (xs, xt, share), = D.paired_rows(t, t, 2, 2)
        bcs.append(P.forward(xs, vt, xt, vt, None, 0.1, 0.04)["batch_center"])
    mod = D.DINOLoss(K, 2, center_momentum=mom).double()
    mod.center.copy_(center0)
    mod.update_center(sum(bcs) / world)          # one process: AllReduce is the identity
    assert mod.center.shape == (1, K) and _rel(mod.center, want) < 1e-13
    assert list(mod.state_dict()) == ["center"]


def test_teacher_temperature_schedule(bvc):
    mod = bvc.dino.DINOLoss(8, 4, warmup_teacher_temp=0.04, teacher_temp=0.07, warmup_teacher_temp_epochs=4, nepochs=10)
    want = P.teacher_temp_schedule(0.04, 0.07, 4, 10)
    assert len(mod.teacher_temp_schedule) == 10 and bool((mod.teacher_temp_schedule == want).all())
    assert abs(want[0] - 0.04) < 1e-15 and abs(want[1] - 0.05) < 1e-15 and abs(want[3] - 0.07) < 1e-15 and want[9] == 0.07
    flat = bvc.dino.DINOLoss(8, 2)
    assert list(flat.teacher_temp_schedule) == [0.04]


def test_dino_head_keys_shapes_and_initialisation(bvc):
    D = bvc.dino
    head = D.DINOHead(128, 1000, nlayers=3, hidden_dim=256, bottleneck_dim=64)
    shapes = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert shapes == {"mlp.0.weight": (256, 128), "mlp.0.bias": (256,), "mlp.2.weight": (256, 256), "mlp.2.bias": (256,),
                      "mlp.4.weight": (64, 256), "mlp.4.bias": (64,), "last_layer.weight_g": (1000, 1), "last_layer.weight_v": (1000, 64)}
    assert bool((head.last_layer.weight_g == 1).all()) and not head.last_layer.weight_g.requires_grad
    assert all(p.requires_grad for n, p in head.named_parameters() if n != "last_layer.weight_g")
    w = head.mlp._modules["2"].weight.detach()
    assert 0.018 < float(w.std()) < 0.022 and float(w.abs().max()) <= 2.0 and float(head.mlp._modules["2"].bias.detach().abs().max()) == 0.0
    one = D.DINOHead(128, 10, nlayers=1, bottleneck_dim=64)
    assert list(one.state_dict()) == ["mlp.weight", "mlp.bias", "last_layer.weight_g", "last_layer.weight_v"]
    assert tuple(one.mlp.weight.shape) == (64, 128)
    # a checkpoint of the original loads; a learnt gain is refused
    sd = {k: torch.randn_like(v) for k, v in head.state_dict().items()}
    sd["last_layer.weight_g"] = torch.ones(1000, 1)
    head.load_state_dict(sd)
    sd["last_layer.weight_g"][3] = 1.5
    with pytest.raises(ValueError, match="weight_g"):
        head.load_state_dict(sd)
    with pytest.raises(ValueError):
        D.DINOHead(100, 10)
    with pytest.raises(bvc._lib.BvcError):
        head(torch.randn(4, 128))


def test_cpu_tensors_and_bad_arguments_are_refused(bvc):
    D = bvc.dino
    xs, vs, xt, vt = P.problem(4, 6, 8, seed=1)
    with pytest.raises(bvc._lib.BvcError):
        D.prototype_ce(xs, vs, xt, vt)
    with pytest.raises(bvc._lib.BvcError):
        D.dino_loss(torch.cat([xs, xs]), torch.cat([xt, xt]), vs, vt)
    with pytest.raises(ValueError):
        D.prototype_ce(xs, vs, xt[:3], vt)
    with pytest.raises(ValueError):
        D.prototype_ce(xs, vs[:, :4], xt, vt)
    with pytest.raises(ValueError):
        D.prototype_ce(xs.long(), vs, xt, vt)
    with pytest.raises(bvc._lib.BvcError):
        D.update_teacher(torch.nn.Linear(4, 4), torch.nn.Linear(4, 4), 0.99)
    assert bvc.prototype_ce is D.prototype_ce and bvc.DINOLoss is D.DINOLoss and bvc.DINOHead is D.DINOHead
    assert bvc.dino_loss is D.dino_loss and bvc.update_teacher is D.update_teacher


# ---------------------------------------------------------------------------------------------- the C ABI without a GPU
NEW_SYMBOLS = ("bvc_op_proto_ce_splits", "bvc_op_proto_ce_block", "bvc_op_proto_ce_workspace", "bvc_op_proto_ce_fwd", "bvc_op_proto_ce_bwd")


def test_symbols_are_declared_and_exported(bvc):
    header = open(os.path.join(ge.ROOT, "include", "bvc.h")).read()
    lib = bvc._lib.lib()
    for name in NEW_SYMBOLS:
        assert name in bvc._lib.SYMBOLS and name + "(" in header and getattr(lib, name) is not None
    assert "proto_ce.hip" in ge.PRODUCT_SOURCES and "proto_ce.h" in ge.HEADERS


def test_refusals_launch_nothing(bvc):
    """shapes, temperatures, eps, strides, splits, block and null pointers are checked before any launch: the calls below pass a
    dummy host pointer"""
    lib = bvc._lib.lib()
    buf = ctypes.create_string_buffer(64)
    q = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(m=8, K=16, p=16, ts=0.1, tt=0.04, eps=1e-12, splits=0, ld=(None,) * 4, xs=q):
        l = [p if v is None else v for v in ld]
        return lib.bvc_op_proto_ce_fwd(xs, l[0], q, l[1], q, l[2], q, l[3], None, m, K, p, ts, tt, eps, splits, q, q, q, q, None, q, None)

    def bwd(m=8, K=16, p=16, ts=0.1, tt=0.04, block=0, lddxs=None, lddvs=None, w=q):
        return lib.bvc_op_proto_ce_bwd(q, p, q, p, q, p, q, p, None, m, K, p, ts, tt, 1e-12, q, q, w, 0, block, q, p if lddxs is None else lddxs,
                                       q, p if lddvs is None else lddvs, q, None)

    inf, nan = float("inf"), float("nan")
    for call, word in ((lambda: fwd(m=0), b"m 0"), (lambda: fwd(m=32769), b"m 32769"), (lambda: fwd(K=0), b"K 0"),
                       (lambda: fwd(K=262145), b"K 262145"), (lambda: fwd(p=0), b"p 0"), (lambda: fwd(p=8193), b"p 8193"),
                       (lambda: fwd(ts=0.0), b"tau_s"), (lambda: fwd(ts=nan), b"tau_s"), (lambda: fwd(tt=-0.04), b"tau_t"),
                       (lambda: fwd(tt=inf), b"tau_t"), (lambda: fwd(eps=0.0), b"eps"), (lambda: fwd(eps=nan), b"eps"),
                       (lambda: fwd(ld=(15, None, None, None)), b"stride"), (lambda: fwd(ld=(None, 15, None, None)), b"stride"),
                       (lambda: fwd(ld=(None, None, 15, None)), b"stride"), (lambda: fwd(ld=(None, None, None, 15)), b"stride"),
                       (lambda: fwd(splits=-1), b"splits"), (lambda: fwd(splits=2049), b"splits"), (lambda: fwd(xs=None), b"null"),
                       (lambda: bwd(m=0), b"m 0"), (lambda: bwd(ts=0.0), b"tau_s"), (lambda: bwd(block=-1), b"block"),
                       (lambda: bwd(lddxs=15), b"stride"), (lambda: bwd(lddvs=15), b"stride"), (lambda: bwd(w=None), b"null")):
        assert call() != 0 and word in lib.bvc_last_error(), (word, lib.bvc_last_error())
    assert lib.bvc_op_proto_ce_workspace(0, 16, 16, 0, 0) == -1 and lib.bvc_op_proto_ce_workspace(8, 16, 16, -1, 0) == -1
    assert lib.bvc_op_proto_ce_workspace(8, 16, 16, 0, -1) == -1
    assert lib.bvc_op_proto_ce_splits(8, 0, 16) == -1 and lib.bvc_op_proto_ce_block(8, 16, 9000) == -1
    # automatic choices: two workgroups per CU where the prototype tiles allow it, the dS block under 64 MiB
    assert lib.bvc_op_proto_ce_splits(32, 65536, 256) == 512 and lib.bvc_op_proto_ce_splits(1024, 65536, 256) == 64
    assert lib.bvc_op_proto_ce_splits(100, 300, 64) == 3 and lib.bvc_op_proto_ce_splits(32768, 262144, 256) == 2
    assert lib.bvc_op_proto_ce_block(1024, 65536, 256) == 16384 and lib.bvc_op_proto_ce_block(32, 65536, 256) == 65536
    assert lib.bvc_op_proto_ce_block(32768, 262144, 8192) == 512 and lib.bvc_op_proto_ce_block(3, 1, 1) == 128
    ws = lib.bvc_op_proto_ce_workspace(300, 385, 100, 0, 0)
    assert ws > 0 and ws % 16 == 0 and lib.bvc_op_proto_ce_workspace(300, 385, 100, 7, 128) != ws
    assert lib.bvc_op_proto_ce_workspace(300, 385, 100, 0, 0) == lib.bvc_op_proto_ce_workspace(300, 385, 100, 4, 512)
    # the documented sizes (include/bvc.h)
    assert round(lib.bvc_op_proto_ce_workspace(1024, 65536, 256, 0, 0) / 2 ** 20) == 327
    assert round(lib.bvc_op_proto_ce_workspace(32768, 262144, 8192, 0, 0) / 2 ** 30, 1) == 21.2
    assert round(lib.bvc_op_proto_ce_workspace(1024, 65536, 256, 0, 128) / 2 ** 20) == 137          # enough for the forward alone


# ---------------------------------------------------------------------------------------------- the bars can tell f32 from bf16
def test_bars_reject_the_bf16_operand_model():
    """At 256 x 1024 x 256 and tau_t = 0.04 the bars of tests/test_gpu_proto_ce.py - built from the float64 reference, the f32
    comparator and eps_row, nothing else - must hold for an f32 run of the closed forms and FAIL for the model with the four
    normalised operands rounded to bf16, for the row loss and for both gradients."""
    m, K, p, ts, tt = 256, 1024, 256, 0.1, 0.04
    xs, vs, xt, vt = P.problem(m, K, p, seed=11)
    d = [t.double() for t in (xs, vs, xt, vt)]
    w = torch.full((m,), 1.0 / m, dtype=F64)
    ref = P.forward(*d, None, ts, tt)
    ref_x, ref_v = P.weighted_grad(*d, None, ts, tt, w)
    sc = P.scales(*d, None, ts, tt, w)
    er = P.eps_row(sc)
    t32 = P.forward(xs, vs, xt, vt, None, ts, tt)
    t32_x, t32_v = P.weighted_grad(xs, vs, xt, vt, None, ts, tt, w.float())
    ge4 = 4 * er.amax().reshape(1, 1)
    bar_l, _ = P.bars(ref["row_loss"], t32["row_loss"], sc["row_loss"], er)
    bar_x, _ = P.bars(ref_x, t32_x, sc["dxs"], ge4)
    bar_v, _ = P.bars(ref_v, t32_v, sc["dvs"], ge4)
    # the closed forms in f32 are inside
    c_x, c_v = P.closed_grad(xs, vs, xt, vt, None, ts, tt, w.float())
    assert bool(((t32["row_loss"].double() - ref["row_loss"]).abs() <= bar_l).all())
    assert bool(((c_x.double() - ref_x).abs() <= bar_x).all()) and bool(((c_v.double() - ref_v).abs() <= bar_v).all())
    # the bf16-operand model is far outside, in most rows
    b_l = (P.forward(xs, vs, xt, vt, None, ts, tt, bf16=True)["row_loss"].double() - ref["row_loss"]).abs()
    b_x, b_v = P.closed_grad(xs, vs, xt, vt, None, ts, tt, w.float(), bf16=True)
    b_x, b_v = (b_x.double() - ref_x).abs(), (b_v.double() - ref_v).abs()
    assert float((b_l / bar_l).max()) > 10 and float((b_l > bar_l).double().mean()) > 0.5
    assert float((b_x / bar_x).max()) > 10 and float((b_x > bar_x).any(1).double().mean()) > 0.5
    assert float((b_v / bar_v).max()) > 10 and float((b_v > bar_v).any(1).double().mean()) > 0.5
