"""Prototype cross-entropy (DINO) on the GPU: bvc_op_proto_ce_fwd / _bwd (csrc/proto_ce.hip) through the C ABI against the float64
reference of tests/proto_ce_ref.py, and bvc.dino (prototype_ce, dino_loss, DINOLoss, DINOHead, update_teacher) on top of them.  The
rules of tests/test_gpu_ntxent.py apply: Guarded buffers with guard bands, outputs and the workspace pre-filled with NaN, the four
operands with a NaN-filled row padding each (ld = p + pad: reading it poisons the result), the padding of dxs / dvs must keep its
NaN bits, the workspace is poisoned again between the forward and the backward, one parity-report line per case.

Bars (nothing in them comes from the code under test).  The scale of an output element is the float64 sum of the magnitudes of its
terms (proto_ce_ref.scales).  The bar of an element is its scale times the larger of
  * 4 x the worst error, relative to the scale, of the same dense formulas run by torch in float32 on the same device inputs, and
  * k eps_row, eps_row_i = 2^-23 (2 + As_i + Ss_i + At_i + St_i) with As_i = max |s_ik - Ls_i|, At_i = max |t_ik - Lt_i| over the
    terms whose softmax weight is >= 2^-30, Ss_i = max_k sum_d |xsn_id wsn_kd| / tau_s, St_i = max_k (sum_d |xtn_id wtn_kd| +
    |center_k|) / tau_t.  Derivation (the one of tests/test_gpu_ntxent.py with 1 / tau_s and 1 / tau_t in the places of 1 / T): a
    score is a chain of p f32 products, so its error is at most 2^-24 per rounding of sum_d |x_id w_kd| / tau <= S (2^-23 S with the
    roundings of the two normalised operands; the centre's subtraction is inside St); exp(s - L) of a 1-ulp hardware exponential is
    off by a relative 2^-23 plus the error of its argument, 2^-24 |s - L| <= 2^-23 A for the subtraction and the score error above.
    l_i = Ls_i - sum_k q_ik s_ik carries the student's terms through Ls_i and s_ik and the teacher's through q_ik, which multiplies
    |s_ik| inside the element's scale; the 2 covers the roundings of the sums and of the logarithm.  k = 1 for the row loss; k = 4
    for dxs and dvs, whose elements mix the exponentials of every row (two per element of dS, times the two products of the
    normalisation backward): they take the largest eps_row of the batch;
with the file's floor of 4 ulp of the reference value.  lse_s and lse_t are held ABSOLUTELY: |error| <= max(eps_row_i, 4 x torch's
worst absolute error).  batch_center is held to 2^-23 (2 + sum_d |xtn_id wtn_kd|), averaged over the rows.  stats[1], the number of
zero prototype rows, is exact.  The mean loss is a mean of row losses: its bar is the mean of their bars.
"""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():   # collected on the CPU box, run on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G          # noqa: E402
from tests import proto_ce_ref as P      # noqa: E402
from tests import rowops_ref as RR       # noqa: E402
from tests.test_gpu_rowops import Guarded, _mode, _same_bits     # noqa: E402

L = G.L
bvc = G.bvc
D = bvc.dino
dev = "cuda"
F64 = torch.float64
EPS = 1e-12


def _gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


class Ref:
    """float64 reference, torch-f32 comparator and scales of one set of inputs (computed once per case)."""

    def __init__(self, ops, center, ts, tt, w=None, gout=1.0):
        self.ops, self.center, self.ts, self.tt = ops, center, ts, tt
        m = ops[0].shape[0]
        d = [t.double() for t in ops]
        c64 = None if center is None else center.double()
        self.w = torch.full((m,), gout / m, dtype=F64, device=dev) if w is None else w.double()
        self.out = P.forward(*d, c64, ts, tt)
        self.dxs, self.dvs = P.weighted_grad(*d, c64, ts, tt, self.w)
        self.t_out = P.forward(*ops, center, ts, tt)
        self.t_dxs, self.t_dvs = P.weighted_grad(*ops, center, ts, tt, self.w.float())
        self.sc = P.scales(*d, c64, ts, tt, self.w)
        self.eps_row = P.eps_row(self.sc)


def _padded(t, pad):
    n, p = t.shape
    b = torch.full((n, p + pad), float("nan"), device=dev)
    b[:, :p] = t
    return b


class Run:
    """One forward and one backward through the C ABI on guarded, NaN-filled buffers."""

    def __init__(self, ops, center, ts, tt, w, splits=0, block=0, pads=(0, 0, 0, 0), ws_fill="nan", eps=EPS, want_center=True):
        m, p = ops[0].shape
        K = ops[1].shape[0]
        self.bufs = [_padded(t, pad) for t, pad in zip(ops, pads)]
        ld = [p + pad for pad in pads]
        lib, st = L.lib(), G.stream()
        nbytes = lib.bvc_op_proto_ce_workspace(m, K, p, splits, block)
        assert nbytes > 0 and nbytes % 16 == 0
        self.row_loss, self.lse_s, self.lse_t, self.stats = Guarded((m,), row=m), Guarded((m,), row=m), Guarded((m,), row=m), Guarded((2,))
        self.bc = Guarded((K,), row=K)
        self.ws = Guarded((nbytes // 4,), fill=ws_fill, row=p)
        self.dxs, self.dvs = Guarded((m, ld[0]), row=ld[0]), Guarded((K, ld[1]), row=ld[1])
        cp = None if center is None else center.data_ptr()
        b = self.bufs
        L.check(lib.bvc_op_proto_ce_fwd(b[0].data_ptr(), ld[0], b[1].data_ptr(), ld[1], b[2].data_ptr(), ld[2], b[3].data_ptr(), ld[3], cp, m, K,
                                        p, ts, tt, eps, splits, self.row_loss.t.data_ptr(), self.lse_s.t.data_ptr(), self.lse_t.t.data_ptr(),
                                        self.stats.t.data_ptr(), self.bc.t.data_ptr() if want_center else None, self.ws.t.data_ptr(), st),
                "bvc_op_proto_ce_fwd")
        if ws_fill == "nan":
            self.ws.t.fill_(float("nan"))      # nothing survives from the forward to the backward
        w32 = w.float().contiguous()
        L.check(lib.bvc_op_proto_ce_bwd(b[0].data_ptr(), ld[0], b[1].data_ptr(), ld[1], b[2].data_ptr(), ld[2], b[3].data_ptr(), ld[3], cp, m, K,
                                        p, ts, tt, eps, self.lse_s.t.data_ptr(), self.lse_t.t.data_ptr(), w32.data_ptr(), splits, block,
                                        self.dxs.t.data_ptr(), ld[0], self.dvs.t.data_ptr(), ld[1], self.ws.t.data_ptr(), st),
                "bvc_op_proto_ce_bwd")
        torch.cuda.synchronize()
        for name in ("row_loss", "lse_s", "lse_t", "stats", "bc", "ws", "dxs", "dvs"):
            getattr(self, name).check(name)
        self.dxs_rows, self.dvs_rows = self.dxs.t[:, :p], self.dvs.t[:, :p]
        if pads[0]:
            assert bool(torch.isnan(self.dxs.t[:, p:]).all()), "the padding of dxs was written"
        if pads[1]:
            assert bool(torch.isnan(self.dvs.t[:, p:]).all()), "the padding of dvs was written"
        outs = [self.dxs_rows, self.dvs_rows, self.row_loss.t, self.lse_s.t, self.lse_t.t, self.stats.t] + ([self.bc.t] if want_center else [])
        assert not any(bool(torch.isnan(o).any()) for o in outs), "NaN in an output, or elements not written"
        if not want_center:
            assert bool(torch.isnan(self.bc.t).all())


def _check(name, key, got, ref, t32, scale, eps_rel, items):
    bar, wt = P.bars(ref, t32, scale, eps_rel)
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


def _check_lse(name, key, got, ref, t32, er, items):
    terr = float((t32.double() - ref).abs().max())
    err = (got.double() - ref).abs()
    items.append(f"{key} {float(err.max()):.2e}/{terr:.2e} (abs)")
    bad = ~(err <= torch.clamp(er, min=4 * terr))
    assert not bool(bad.any()), f"{name} {key}: {int(bad.sum())} over the bar, worst error {float(err.max()):.3e}, eps_row {float(er.min()):.3e}"


def check_forward(name, run, ref, items, want_center=True):
    o, t, er = ref.out, ref.t_out, ref.eps_row
    assert float(run.stats.t[1]) == float(o["zero_protos"]), f"{name}: stats[1] {float(run.stats.t[1])} != {o['zero_protos']}"
    _check_lse(name, "lse_s", run.lse_s.t, o["lse_s"], t["lse_s"], er, items)
    _check_lse(name, "lse_t", run.lse_t.t, o["lse_t"], t["lse_t"], er, items)
    bar_l = _check(name, "row_loss", run.row_loss.t, o["row_loss"], t["row_loss"], ref.sc["row_loss"], er, items)
    lerr, bar_loss = abs(float(run.stats.t[0]) - float(o["loss"])), float(bar_l.mean())
    items.append(f"loss {lerr:.2e} (bar {bar_loss:.2e})")
    assert lerr <= bar_loss + 4 * float(RR.ulp32(o["loss"])), f"{name} loss: error {lerr:.3e}, bar {bar_loss:.3e}"
    if want_center:
        cerr = (run.bc.t.double() - o["batch_center"]).abs()
        cbar = 2.0 ** -23 * ref.sc["batch_center"]
        items.append(f"batch_center {float((cerr / cbar).max()):.2e} of its bar")
        assert bool((cerr <= cbar).all()), f"{name} batch_center: worst error {float(cerr.max()):.3e}, bar {float(cbar.min()):.3e}"


def check_run(name, run, ref, want_center=True):
    items = []
    try:
        check_forward(name, run, ref, items, want_center)
        ge4 = 4 * ref.eps_row.amax().reshape(1, 1)
        _check(name, "dxs", run.dxs_rows, ref.dxs, ref.t_dxs, ref.sc["dxs"], ge4, items)
        _check(name, "dvs", run.dvs_rows, ref.dvs, ref.t_dvs, ref.sc["dvs"], ge4, items)
    finally:
        G.log_parity(f"proto_ce {name}: " + "  ".join(items) + "   (kernel/torch-f32, relative to the element's scale)")


def _ops(m, K, p, seed):
    return P.problem(m, K, p, seed, device=dev)


def _case(ops, center=None, ts=0.1, tt=0.04, w=None, gout=1.0, **kw):
    ref = Ref(ops, center, ts, tt, w, gout)
    return Run(ops, center, ts, tt, ref.w, **kw), ref


# ---------------------------------------------------------------------------------------------- shapes
# (m, K, p, pads of xs / vs / xt / vt, splits, block): every m and K edge of the 128-row tile, every p edge of the 32-float K stage,
# crossed sparsely; a padding on each operand alone and on all; forced splits including more splits than prototype tiles (empty
# splits); K = 385 in blocks of 128 (four blocks, the last a one-row tail) and in one block; several row tiles (m = 257)
SHAPES = [
    (1, 1, 1, (0, 0, 0, 0), 0, 0), (2, 2, 3, (1, 0, 0, 0), 1, 0), (127, 127, 31, (0, 3, 0, 0), 2, 0), (128, 128, 32, (0, 0, 5, 0), 3, 0),
    (129, 129, 33, (0, 0, 0, 8), 0, 128), (257, 385, 100, (1, 2, 3, 4), 7, 128), (257, 385, 100, (0, 0, 0, 0), 0, 0),
    (2, 1000, 256, (0, 0, 0, 0), 0, 256), (129, 1000, 3, (8, 8, 8, 8), 3, 0), (1, 385, 33, (0, 1, 0, 1), 2, 256),
    (257, 1000, 256, (4, 0, 4, 0), 0, 384), (127, 2, 100, (0, 0, 0, 0), 0, 0), (128, 1, 32, (1, 1, 1, 1), 1, 0),
]


@pytest.mark.parametrize("m,K,p,pads,splits,block", SHAPES)
def test_against_float64(m, K, p, pads, splits, block):
    ops = _ops(m, K, p, seed=m * 7 + K + p)
    center = 0.2 * torch.randn(K, generator=_gen(m + K), device=dev) if (m + K) % 2 else None
    run, ref = _case(ops, center, pads=pads, splits=splits, block=block)
    check_run(f"m{m} K{K} p{p} pads{''.join(map(str, pads))} splits{splits} block{block} centre{int(center is not None)}", run, ref)


def test_automatic_choices():
    lib = L.lib()
    assert lib.bvc_op_proto_ce_splits(1024, 65536, 256) == 64 and lib.bvc_op_proto_ce_block(1024, 65536, 256) == 16384
    assert lib.bvc_op_proto_ce_workspace(300, 385, 100, 0, 0) == lib.bvc_op_proto_ce_workspace(300, 385, 100, 4, 512)


# ---------------------------------------------------------------------------------------------- splits and blocks
def test_splits_and_blocks_agree():
    """K = 385 is four prototype tiles.  Forward splits 1, 2, 3, 9 (five of them empty) and the automatic choice at one block size;
    backward blocks of 128 (four, the last a one-row tail), 256, 512 and the automatic choice (the whole K) at one split count.
    Every choice is within the bars.  With the forward's lse_s / lse_t the same (one split count), dvs is bit-equal across the
    block sizes (each block's contraction over the rows is complete) and dxs, summed block after block, agrees within the bars."""
    m, K, p = 257, 385, 100
    ops = _ops(m, K, p, seed=31)
    center = 0.2 * torch.randn(K, generator=_gen(32), device=dev)
    ref = Ref(ops, center, 0.1, 0.04)
    runs = {}
    for splits, block in ((1, 128), (3, 128), (9, 128), (0, 128), (2, 128), (2, 256), (2, 512), (2, 0)):
        runs[(splits, block)] = r = Run(ops, center, 0.1, 0.04, ref.w, splits=splits, block=block)
        check_run(f"splits{splits} block{block}", r, ref)
    first = runs[(2, 128)]
    for block in (256, 512, 0):
        r = runs[(2, block)]
        assert _same_bits(first.dvs_rows, r.dvs_rows), f"dvs differs between blocks 128 and {block}"
        for x, y in zip(_out_bits(first)[:5], _out_bits(r)[:5]):
            assert _same_bits(x, y), "the forward depends on the backward's block"
    # batch_center does not pass through the splits at all
    assert _same_bits(runs[(1, 128)].bc.t, runs[(9, 128)].bc.t)


# ---------------------------------------------------------------------------------------------- hard cases
@pytest.mark.parametrize("tt", [0.04, 0.07, 1.0])
@pytest.mark.parametrize("ts", [0.1, 1.0])
def test_temperatures_with_the_teacher_maximum_in_the_first_and_in_the_last_tile(ts, tt):
    """Teacher prototypes equal to teacher rows: raw scores of 1, so t reaches 1 / tau_t = 25 above the rest.  Row 0's maximum is at
    k = 1 (first tile), row 5's at k = K - 1 (the last tile's only column, next to the padding), row 7's at k = 300; prototypes 10
    and 20 are identical on the teacher side (a tie: nothing discrete to decide)."""
    m, K, p = 130, 385, 100
    xs, vs, xt, vt = _ops(m, K, p, seed=41)
    vt[1] = xt[0]
    vt[K - 1] = 3.0 * xt[5]
    vt[300] = xt[7]
    vt[20] = vt[10]
    ref = Ref((xs, vs, xt, vt), None, ts, tt)
    q = ref.out["q"]
    assert int(q[0].argmax()) == 1 and int(q[5].argmax()) == K - 1 and int(q[7].argmax()) == 300
    assert torch.equal(ref.out["t"][:, 10], ref.out["t"][:, 20])
    assert abs(float(ref.out["t"][5, K - 1]) - 1 / tt) < 1e-9 / tt
    for splits in (1, 3):
        run = Run((xs, vs, xt, vt), None, ts, tt, ref.w, splits=splits)
        check_run(f"tau_s{ts} tau_t{tt} placed maxima splits{splits}", run, ref)


@pytest.mark.parametrize("kind", ["null", "zero", "ten"])
def test_centres(kind):
    m, K, p = 129, 385, 64
    ops = _ops(m, K, p, seed=43)
    center = None if kind == "null" else torch.zeros(K, device=dev)
    if kind == "ten":
        center[::4] = 10.0 * torch.sign(torch.randn(K, generator=_gen(44), device=dev))[::4]
    run, ref = _case(ops, center, splits=2, block=128)
    check_run(f"centre {kind}", run, ref)
    if kind == "zero":
        other = Run(ops, None, 0.1, 0.04, ref.w, splits=2, block=128)
        for x, y in zip(_out_bits(run), _out_bits(other)):
            assert _same_bits(x, y), "a zero centre and no centre differ"


def test_zero_student_row_zero_teacher_row_and_zero_prototype():
    """|xs_i| = 0 <= eps: the clamp is active, every student score of the row is 0 and dxs_i = dxsn_i / eps; a zero teacher row has
    t_ik = -center_k / tau_t; a zero prototype row of vs is flagged in stats[1], scores 0 and receives dvs_k = 0"""
    m, K, p = 130, 200, 40
    xs, vs, xt, vt = _ops(m, K, p, seed=45)
    xs[3] = 0.0
    xs[129] = 0.0
    xt[4] = 0.0
    vs[77] = 0.0
    center = 0.2 * torch.randn(K, generator=_gen(46), device=dev)
    run, ref = _case((xs, vs, xt, vt), center, block=128)
    assert float(ref.dxs[3].abs().max()) > 1e6 and ref.out["zero_protos"] == 1
    assert float(run.stats.t[1]) == 1.0 and bool((run.dvs_rows[77] == 0).all())
    check_run("zero rows", run, ref)
    # the flag reaches the Python layer: prototype_ce on request, DINOLoss as an attribute of the last forward
    _, flag = D.prototype_ce(xs, vs, xt, vt, center, return_zero_rows=True)
    mod = D.DINOLoss(K, 2).to(dev)
    assert mod.zero_prototype_rows is None
    mod(torch.cat([xs, xs]), torch.cat([xt, xt]), vs, vt, 0)
    assert float(flag) == 1.0 and float(mod.zero_prototype_rows) == 1.0
    # a NaN in a prototype row is no zero row: it is not counted, and the loss shows it
    vs_nan = vs.clone()
    vs_nan[5, 0] = float("nan")
    loss_nan, flag_nan = D.prototype_ce(xs, vs_nan, xt, vt, center, return_zero_rows=True)
    assert float(flag_nan) == 1.0 and bool(torch.isnan(loss_nan))
    vt2 = vt.clone()
    vt2[5] = 0.0
    vt2[6] = 0.0
    run2, ref2 = _case((xs, vs, xt, vt2), center)
    assert float(run2.stats.t[1]) == 3.0
    check_run("zero rows, three zero prototypes", run2, ref2)


def test_row_weights_with_zeros_and_negatives():
    m, K, p = 257, 300, 64
    ops = _ops(m, K, p, seed=47)
    w = torch.randn(m, generator=_gen(48), device=dev)
    w[::3] = 0.0
    run, ref = _case(ops, None, w=w, block=128)
    assert bool((run.dxs_rows[::3] == 0).all())
    check_run("row weights with zeros and negatives", run, ref)


@pytest.mark.parametrize("ts,tt,centred", [(0.07, 0.07, False), (0.1, 0.04, False), (0.07, 0.07, True)])
def test_student_equal_to_teacher(ts, tt, centred):
    """the same operands on both sides: l_i = H(q_i) within the bar when the temperatures are equal and there is no centre, and then
    the gradient vanishes (to rounding: every element within its bar of 0); otherwise it does not"""
    m, K, p = 100, 300, 48
    xs, vs, _, _ = _ops(m, K, p, seed=49)
    center = 0.3 * torch.randn(K, generator=_gen(50), device=dev) if centred else None
    run, ref = _case((xs, vs, xs, vs), center, ts, tt)
    check_run(f"student == teacher tau_s{ts} tau_t{tt} centre{int(centred)}", run, ref)
    if ts == tt and not centred:
        q = ref.out["q"]
        H = -(q * torch.log(q)).sum(1)
        bar, _ = P.bars(ref.out["row_loss"], ref.t_out["row_loss"], ref.sc["row_loss"], ref.eps_row)
        assert bool(((run.row_loss.t.double() - H).abs() <= bar).all())
        assert float(ref.dxs.abs().max()) < 1e-15
    else:
        assert float(run.dxs_rows.abs().max()) > 1e-6 and float(run.dvs_rows.abs().max()) > 1e-6


# ---------------------------------------------------------------------------------------------- invariants
def _out_bits(r):
    return [r.row_loss.t, r.lse_s.t, r.lse_t.t, r.stats.t, r.bc.t, r.dxs_rows, r.dvs_rows]


def test_same_bits_on_every_run_and_whatever_the_workspace_held():
    ops = _ops(257, 385, 100, seed=51)
    center = 0.2 * torch.randn(385, generator=_gen(52), device=dev)
    w = torch.full((257,), 1.0 / 257, device=dev)
    kw = dict(splits=3, block=128, pads=(1, 2, 3, 4))
    a = Run(ops, center, 0.1, 0.04, w, **kw)
    others = [Run(ops, center, 0.1, 0.04, w, **kw), Run(ops, center, 0.1, 0.04, w, **kw), Run(ops, center, 0.1, 0.04, w, ws_fill=0.0, **kw),
              Run(ops, center, 0.1, 0.04, w, ws_fill=1e30, **kw)]
    for o in others:
        for x, y in zip(_out_bits(a), _out_bits(o)):
            assert _same_bits(x, y)
    # without batch_center the other outputs are the same
    e = Run(ops, center, 0.1, 0.04, w, want_center=False, **kw)
    for x, y in zip(_out_bits(a)[:4] + _out_bits(a)[5:], _out_bits(e)[:4] + _out_bits(e)[5:]):
        assert _same_bits(x, y)


def test_forward_alone_fits_the_workspace_of_the_smallest_block():
    """the forward touches only the leading part of the workspace: sized for block = 128 and guarded, with the automatic block larger"""
    m, K, p = 129, 1000, 100
    ops = _ops(m, K, p, seed=55)
    lib, st = L.lib(), G.stream()
    small, full = lib.bvc_op_proto_ce_workspace(m, K, p, 0, 128), lib.bvc_op_proto_ce_workspace(m, K, p, 0, 0)
    assert 0 < small < full and lib.bvc_op_proto_ce_block(m, K, p) == 1024
    outs = [Guarded((m,), row=m), Guarded((m,), row=m), Guarded((m,), row=m), Guarded((2,)), Guarded((K,), row=K)]
    ws = Guarded((small // 4,), row=p)
    L.check(lib.bvc_op_proto_ce_fwd(ops[0].data_ptr(), p, ops[1].data_ptr(), p, ops[2].data_ptr(), p, ops[3].data_ptr(), p, None, m, K, p, 0.1,
                                    0.04, EPS, 0, outs[0].t.data_ptr(), outs[1].t.data_ptr(), outs[2].t.data_ptr(), outs[3].t.data_ptr(),
                                    outs[4].t.data_ptr(), ws.t.data_ptr(), st), "bvc_op_proto_ce_fwd")
    torch.cuda.synchronize()
    ws.check("workspace of the smallest block")
    whole = Run(ops, None, 0.1, 0.04, torch.full((m,), 1.0 / m, device=dev))
    for o, r in zip(outs, (whole.row_loss, whole.lse_s, whole.lse_t, whole.stats, whole.bc)):
        o.check("forward alone")
        assert _same_bits(o.t, r.t)


def test_refused_arguments_write_nothing():
    m, K, p = 8, 12, 16
    xs, vs, xt, vt = _ops(m, K, p, seed=53)
    lib, st = L.lib(), G.stream()
    outs = [Guarded((m,), row=m), Guarded((m,), row=m), Guarded((m,), row=m), Guarded((2,)), Guarded((K,), row=K), Guarded((1 << 16,)),
            Guarded((m, p), row=p), Guarded((K, p), row=p)]
    rl, ls, lt, stats, bc, ws, dxs, dvs = outs
    w = torch.ones(m, device=dev)

    def fwd(m_=m, K_=K, p_=p, ts=0.1, tt=0.04, eps=EPS, splits=0, ldvs=p):
        return lib.bvc_op_proto_ce_fwd(xs.data_ptr(), p, vs.data_ptr(), ldvs, xt.data_ptr(), p, vt.data_ptr(), p, None, m_, K_, p_, ts, tt, eps,
                                       splits, rl.t.data_ptr(), ls.t.data_ptr(), lt.t.data_ptr(), stats.t.data_ptr(), bc.t.data_ptr(),
                                       ws.t.data_ptr(), st)

    def bwd(m_=m, K_=K, p_=p, ts=0.1, tt=0.04, block=0, lddvs=p):
        return lib.bvc_op_proto_ce_bwd(xs.data_ptr(), p, vs.data_ptr(), p, xt.data_ptr(), p, vt.data_ptr(), p, None, m_, K_, p_, ts, tt, EPS,
                                       ls.t.data_ptr(), lt.t.data_ptr(), w.data_ptr(), 0, block, dxs.t.data_ptr(), p, dvs.t.data_ptr(), lddvs,
                                       ws.t.data_ptr(), st)

    nan = float("nan")
    for call, word in ((lambda: fwd(m_=0), b"m 0"), (lambda: fwd(m_=40000), b"m 40000"), (lambda: fwd(K_=0), b"K 0"),
                       (lambda: fwd(K_=300000), b"K 300000"), (lambda: fwd(p_=0), b"p 0"), (lambda: fwd(p_=8200), b"p 8200"),
                       (lambda: fwd(ts=0.0), b"tau_s"), (lambda: fwd(tt=nan), b"tau_t"), (lambda: fwd(eps=-1.0), b"eps"),
                       (lambda: fwd(splits=-2), b"splits"), (lambda: fwd(ldvs=p - 1), b"stride"),
                       (lambda: bwd(m_=0), b"m 0"), (lambda: bwd(tt=-0.1), b"tau_t"), (lambda: bwd(block=-128), b"block"),
                       (lambda: bwd(lddvs=p - 1), b"stride")):
        assert call() != 0 and word in lib.bvc_last_error(), (word, lib.bvc_last_error())
    torch.cuda.synchronize()
    for o in outs:
        o.check("refused call")
        assert bool(torch.isnan(o.t).all()), "a refused call wrote an output"


# ---------------------------------------------------------------------------------------------- bvc.dino
def test_prototype_ce_is_the_abi_and_matches_float64():
    m, K, p, ts, tt = 130, 385, 100, 0.1, 0.04
    ops = _ops(m, K, p, seed=61)
    center = 0.2 * torch.randn(1, K, generator=_gen(62), device=dev)           # the module's [1][K] buffer is taken as it is
    ref = Ref(ops, center.reshape(-1), ts, tt, gout=3.0)
    run = Run(ops, center.reshape(-1), ts, tt, ref.w)
    x, v = ops[0].clone().requires_grad_(True), ops[1].clone().requires_grad_(True)
    xt, vt = ops[2].clone().requires_grad_(True), ops[3].clone().requires_grad_(True)
    loss = D.prototype_ce(x, v, xt, vt, center, ts, tt)
    (loss * 3).backward()
    assert loss.dim() == 0 and _same_bits(loss.detach(), run.stats.t[0])
    assert _same_bits(x.grad, run.dxs_rows) and _same_bits(v.grad, run.dvs_rows) and xt.grad is None and vt.grad is None
    check_run("prototype_ce mean x3", run, ref)
    # none, random upstream gradients per row; strided rows (a column slice of a wider tensor) are read as they are
    u = torch.randn(m, generator=_gen(63), device=dev)
    wide = torch.randn(m, p + 28, generator=_gen(64), device=dev)
    wide[:, :p] = ops[0]
    wide.requires_grad_(True)
    rows = D.prototype_ce(wide[:, :p], ops[1], ops[2], ops[3], center, ts, tt, reduction="none")
    assert rows.shape == (m,)
    (rows * u).sum().backward()
    ref2 = Ref(ops, center.reshape(-1), ts, tt, w=u)
    items = []
    _check("none", "row_loss", rows.detach(), ref2.out["row_loss"], ref2.t_out["row_loss"], ref2.sc["row_loss"], ref2.eps_row, items)
    _check("none", "dxs", wide.grad[:, :p], ref2.dxs, ref2.t_dxs, ref2.sc["dxs"], 4 * ref2.eps_row.amax().reshape(1, 1), items)
    assert bool((wide.grad[:, p:] == 0).all())
    G.log_parity("proto_ce prototype_ce none, strided rows: " + "  ".join(items))
    with pytest.raises(ValueError):
        D.prototype_ce(ops[0], ops[1], ops[2], ops[3], center, reduction="sum")
    with pytest.raises(ValueError):
        D.prototype_ce(ops[0], ops[1], ops[2], ops[3], center[:, :-1])


@pytest.mark.parametrize("dtype,rel", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)])
def test_half_precision_features(dtype, rel):
    """Computed in f32 from the rounded values; the gradients come back in the input dtype: one more rounding on the bar (relative
    2^-8 for bf16, 2^-11 for f16 plus half of f16's smallest subnormal step, 2^-25)"""
    m, K, p, ts, tt = 130, 300, 64, 0.1, 0.04
    ops = [t.to(dtype) for t in _ops(m, K, p, seed=65)]
    ref = Ref([t.float() for t in ops], None, ts, tt)
    x, v = ops[0].clone().requires_grad_(True), ops[1].clone().requires_grad_(True)
    loss = D.prototype_ce(x, v, ops[2], ops[3], None, ts, tt)
    loss.backward()
    assert loss.dtype == torch.float32 and x.grad.dtype == dtype and v.grad.dtype == dtype
    ge4 = 4 * ref.eps_row.amax().reshape(1, 1)
    tiny = 2.0 ** -25 if dtype == torch.float16 else 0.0
    bar_x, _ = P.bars(ref.dxs, ref.t_dxs, ref.sc["dxs"], ge4)
    bar_v, _ = P.bars(ref.dvs, ref.t_dvs, ref.sc["dvs"], ge4)
    assert bool(((x.grad.double() - ref.dxs).abs() <= bar_x + rel * ref.dxs.abs() + tiny).all())
    assert bool(((v.grad.double() - ref.dvs).abs() <= bar_v + rel * ref.dvs.abs() + tiny).all())
    bar_l, _ = P.bars(ref.out["row_loss"], ref.t_out["row_loss"], ref.sc["row_loss"], ref.eps_row)
    assert abs(float(loss) - float(ref.out["loss"])) <= float(bar_l.mean()) + 4 * float(RR.ulp32(ref.out["loss"]))


@pytest.mark.parametrize("local", [0, 2])
def test_dino_loss_against_the_float64_double_loop(local):
    """2 + 0 and 2 + 2 views: the loss against the original's double loop over float64 logits, and the gradient of the student rows -
    a row of a global view reaches the loss through one (2 + 0) or three (2 + 2) pairs, a local one through two"""
    B, p, K, ts, tt = 24, 64, 385, 0.1, 0.04
    views = 2 + local
    student = P.random_rows(views * B, p, 71, device=dev)
    teacher = student[:2 * B] + 0.5 * P.random_rows(2 * B, p, 72, device=dev)
    vs = P.random_rows(K, p, 73, device=dev)
    vt = vs + 0.1 * P.random_rows(K, p, 74, device=dev)
    center = 0.2 * torch.randn(K, generator=_gen(75), device=dev)
    # float64: the double loop, differentiated by autograd
    s64, v64 = student.double().requires_grad_(True), vs.double().requires_grad_(True)
    want = P.dino_double_loop(P.logits(s64, v64), P.logits(teacher.double(), vt.double()), center.double(), ts, tt, views)
    want.backward()
    # the stacked pairs as one problem: reference, comparator and bars of its rows, folded back onto the student rows
    (xs, xt, share), = D.paired_rows(student, teacher, views, 2)
    ref = Ref((xs, vs, xt, vt), center, ts, tt)
    fold = lambda t: sum(torch.nn.functional.pad(t[j * B:(j + 1) * B], (0, 0, b * B, (views - 1 - b) * B))      # noqa: E731
                         for j, (_, b) in enumerate(D.view_pairs(views, 2)))
    assert abs(float(ref.out["loss"] - want)) < 1e-12 and float((fold(ref.dxs) - s64.grad).abs().max()) < 1e-12 * float(s64.grad.abs().max())
    assert float((ref.dvs - v64.grad).abs().max()) < 1e-12 * float(v64.grad.abs().max())
    x, v = student.clone().requires_grad_(True), vs.clone().requires_grad_(True)
    loss, bc, zero_rows = D.dino_loss(x, teacher, v, vt, center, ts, tt, views, 2, return_center=True)
    assert float(zero_rows) == 0.0
    loss.backward()
    bar_l, _ = P.bars(ref.out["row_loss"], ref.t_out["row_loss"], ref.sc["row_loss"], ref.eps_row)
    assert abs(float(loss) - float(want)) <= float(bar_l.mean()) + 4 * float(RR.ulp32(want.detach()))
    ge4 = 4 * ref.eps_row.amax().reshape(1, 1)
    bar_x, _ = P.bars(ref.dxs, ref.t_dxs, ref.sc["dxs"], ge4)
    bar_v, _ = P.bars(ref.dvs, ref.t_dvs, ref.sc["dvs"], ge4)
    ex, ev = (x.grad.double() - s64.grad).abs(), (v.grad.double() - v64.grad).abs()
    assert bool((ex <= fold(bar_x) + 4 * RR.ulp32(s64.grad)).all()) and bool((ev <= bar_v).all())
    cbar = 2.0 ** -23 * ref.sc["batch_center"]
    assert bool(((bc.double() - P.logits(teacher.double(), vt.double()).mean(0)).abs() <= cbar).all())
    G.log_parity(f"proto_ce dino_loss 2+{local} views: loss {abs(float(loss) - float(want)):.2e} (bar {float(bar_l.mean()):.2e})  "
                 f"d student {float((ex / fold(bar_x)).max()):.2f} of its bar  d vs {float((ev / bar_v).max()):.2f} of its bar")


def test_dino_loss_module_over_three_steps():
    """DINOLoss against a float64 restatement: the warm-up temperatures 0.04, 0.055, 0.07, the loss of every step and the centre's
    trajectory center * 0.9 + mean teacher logits * 0.1"""
    B, p, K, views, mom = 16, 64, 300, 4, 0.9
    mod = D.DINOLoss(K, views, warmup_teacher_temp=0.04, teacher_temp=0.07, warmup_teacher_temp_epochs=3, nepochs=3, center_momentum=mom).to(dev)
    assert [round(float(t), 6) for t in mod.teacher_temp_schedule] == [0.04, 0.055, 0.07]
    vs = P.random_rows(K, p, 81, device=dev)
    vt = vs + 0.1 * P.random_rows(K, p, 82, device=dev)
    c64 = torch.zeros(1, K, dtype=F64, device=dev)
    cbar_sum = torch.zeros(K, dtype=F64, device=dev)
    for epoch in range(3):
        student = P.random_rows(views * B, p, 83 + epoch, device=dev)
        teacher = student[:2 * B] + 0.5 * P.random_rows(2 * B, p, 90 + epoch, device=dev)
        before = mod.center.clone()
        loss = mod(student, teacher, vs, vt, epoch)
        tt = float(P.teacher_temp_schedule(0.04, 0.07, 3, 3)[epoch])
        lg_t = P.logits(teacher.double(), vt.double())
        want = P.dino_double_loop(P.logits(student.double(), vs.double()), lg_t, c64, 0.1, tt, views)
        (xs, xt, _), = D.paired_rows(student, teacher, views, 2)
        ref = Ref((xs, vs, xt, vt), before.reshape(-1), 0.1, tt)          # the bars, at the centre the step read
        bar_l, _ = P.bars(ref.out["row_loss"], ref.t_out["row_loss"], ref.sc["row_loss"], ref.eps_row)
        # the float64 trajectory's centre differs from the f32 buffer by its accumulated bar: its effect on t is that over tau_t
        drift = float(cbar_sum.max()) / tt
        assert abs(float(loss) - float(want)) <= float(bar_l.mean()) + 2 * drift * float(ref.sc["row_loss"].mean()) + 4 * float(RR.ulp32(want))
        c64 = P.center_update_original(c64, [lg_t], mom)
        cbar_sum = cbar_sum * mom + 2.0 ** -23 * ref.sc["batch_center"] * (1 - mom) + 2 * RR.ulp32(c64.reshape(-1))
        assert mod.center.shape == (1, K) and bool(((mod.center.double() - c64).abs().reshape(-1) <= cbar_sum).all()), epoch
    assert float(mod.center.abs().max()) > 0


@pytest.mark.parametrize("nlayers,n", [(3, 64), (1, 64), (2, 96)])
def test_dino_head_forward_backward(nlayers, n):
    """against a float64 MLP at the tolerances tests/test_gpu_simclr.py::test_projection_head_forward_backward uses for the bf16 GEMM
    path: 1e-2 (relative L2) for the output, 2e-2 for the gradients (GELU has no gates to flip)"""
    pin, hid, bott, K = 128, 256, 64, 100
    torch.manual_seed(7)
    head = D.DINOHead(pin, K, nlayers=nlayers, hidden_dim=hid, bottleneck_dim=bott)
    with torch.no_grad():
        for name, prm in head.named_parameters():
            if name.endswith("bias"):
                prm.normal_(0, 0.1)
            elif name.endswith("weight"):
                prm.mul_(4.0)                     # std 0.08: activations of order 1 after the first layer
    params = {k: v.detach().clone() for k, v in head.state_dict().items()}
    g = torch.Generator().manual_seed(8)
    x0, dout = torch.randn(n, pin, generator=g), torch.randn(n, bott, generator=g)
    rp = {k: v.double().requires_grad_(True) for k, v in params.items() if k.startswith("mlp")}
    rx = x0.double().requires_grad_(True)
    ro = P.mlp_forward(rx, rp, nlayers)
    ro.backward(dout.double())
    head.to(dev)
    x = x0.to(dev).requires_grad_(True)
    out = head(x)
    assert out.shape == (n, bott) and out.dtype == torch.float32
    out.backward(dout.to(dev))
    torch.cuda.synchronize()
    assert G.rel_err(out.cpu(), ro.detach()) < 1e-2
    assert G.rel_err(x.grad.cpu(), rx.grad) < 2e-2
    named = dict(head.named_parameters())
    for k in rp:
        assert G.rel_err(named[k].grad.cpu(), rp[k].grad) < 2e-2, k
    assert named["last_layer.weight_v"].grad is None and named["last_layer.weight_g"].grad is None


class _Standin(nn.Module):
    """a 64-wide trunk stand-in: a per-feature scale and shift, then tanh"""

    def __init__(self, d):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.bias = nn.Parameter(torch.zeros(d))

    def forward(self, x):
        return torch.tanh(x * self.weight + self.bias)


def _one_step(seed):
    B, d, K = 16, 64, 1000
    torch.manual_seed(seed)
    student = nn.ModuleDict({"trunk": _Standin(d), "head": D.DINOHead(d, K, nlayers=3, hidden_dim=128, bottleneck_dim=64)}).to(dev)
    teacher = copy.deepcopy(student).requires_grad_(False)
    crit = D.DINOLoss(K, 2).to(dev)
    views = P.random_rows(2 * B, d, seed + 1, device=dev)          # two view-major views
    s = student["head"](student["trunk"](views))
    with torch.no_grad():
        t = teacher["head"](teacher["trunk"](views))
    loss = crit(s, t, student["head"], teacher["head"], 0)
    loss.backward()
    return student, teacher, crit, loss


def test_one_training_step():
    student, teacher, crit, loss = _one_step(3)
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    for name, prm in student.named_parameters():
        if prm.requires_grad:
            assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0, name
    assert all(prm.grad is None for prm in teacher.parameters())
    assert not student["head"].last_layer.weight_g.requires_grad and float(crit.center.abs().max()) > 0
    # the teacher moves by exactly (1 - m) of the difference: m = 0.5 is exact in f32 up to the one final rounding
    with torch.no_grad():
        for prm in student.parameters():
            if prm.requires_grad:
                prm.add_(prm.grad, alpha=-0.5)
    before = [prm.detach().clone() for prm in teacher.parameters()]
    D.update_teacher(student, teacher, 0.5)
    for k0, k1, q in zip(before, teacher.parameters(), student.parameters()):
        assert _same_bits(k1.detach(), (k0.double() + 0.5 * (q.detach().double() - k0.double())).float())
    before = [prm.detach().clone() for prm in teacher.parameters()]
    D.update_teacher(student, teacher, 0.996)
    for k0, k1, q in zip(before, teacher.parameters(), student.parameters()):
        want = k0.double() + (1 - 0.996) * (q.detach().double() - k0.double())
        # m and 1 - m are f32 numbers: 2^-25 relative on m, the same absolute amount on 1 - m
        slack = 2.0 ** -24 * (k0.abs().double() + q.detach().abs().double())
        assert bool(((k1.detach().double() - want).abs() <= 2 * RR.ulp32(want) + slack).all())
    assert bool((teacher["head"].last_layer.weight_g == 1).all())


def test_two_identical_training_steps_give_identical_bits():
    """the loss adds no atomics: in the library's deterministic mode (which the head's weight-gradient products need) the whole step
    is bit-reproducible, the gradient a student row collects from its two pairs included"""
    with _mode(True):
        s1, _, c1, loss1 = _one_step(3)
        s2, _, c2, loss2 = _one_step(3)
    assert _same_bits(loss1.detach(), loss2.detach()) and _same_bits(c1.center, c2.center)
    for (name, a), b in zip(s1.named_parameters(), s2.parameters()):
        if a.requires_grad:
            assert _same_bits(a.grad, b.grad), name
