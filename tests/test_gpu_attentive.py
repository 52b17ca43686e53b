"""Attentive pooling on the GPU: bvc_op_attn_pool_fwd / _bwd (csrc/attnpool.hip) through the C ABI against the float64 references of
tests/attentive_ref.py, and bvc.attentive's modules against the unfused module.  The rules of tests/test_gpu_rowops.py apply:
Guarded buffers with guard bands, outputs (and the workspace) pre-filled with NaN, per-row bars against float64, one parity-report
line per case.

Bars (nothing in them comes from the code under test).  The scale of an output element is the float64 sum of the magnitudes of its
terms (attentive_ref.core_scales).  The bar of an element is its scale times the larger of
  * 4 x the worst error, relative to the scale, of the same formulas run by torch in float32 on the same device inputs, and
  * k eps_p, eps_p = 2^-23 (2 + A + S) per (clip, query): A = max |s - lse| over the tokens with p >= 2^-30, S = max_j sum_d |xh_jd u_rd|
    (the f32 rounding of a score and a 1-ulp hardware exp); k = 1 for pooled, 4 for du and dx; a du row takes the largest eps_p of
    its query over the clips, a dx row the largest over the queries of its clip;
with the file's floor of 4 ulp of the reference value.  lse: eps_p is an absolute bar (or 4 x torch's absolute error).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():   # collected on the CPU box, run on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import attentive_ref as A     # noqa: E402
from tests import gpu_util as G          # noqa: E402
from tests import rowops_ref as RR       # noqa: E402
from tests.test_gpu_rowops import Guarded, _same_bits     # noqa: E402

L = G.L
bvc = G.bvc
dev = "cuda"
F64 = torch.float64
EPS = 1e-5


def _gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _inputs(B, N, D, R, seed, xscale=1.5, uscale=None):
    g = _gen(seed)
    x = torch.randn(B, N, D, generator=g, device=dev) * xscale + 0.5 * torch.randn(B, N, 1, generator=g, device=dev)
    u = torch.randn(R, D, generator=g, device=dev) * (uscale if uscale is not None else 2.0 / math.sqrt(D))
    dpooled = torch.randn(B, R, D, generator=g, device=dev)
    return x, u, dpooled


class Run:
    """One forward and one backward through the C ABI on guarded, NaN-filled buffers; x and dx with a row stride of D + pad
    (the padding of x holds NaN: reading it poisons the result; the padding of dx must keep its NaN bits)."""

    def __init__(self, x, u, dpooled, splits=0, pad=0, want_dx=True, ws_fill="nan", eps=EPS):
        B, N, D = x.shape
        R = u.shape[0]
        ld = D + pad
        self.xb = torch.full((B * N, ld), float("nan"), device=dev)
        self.xb[:, :D] = x.reshape(B * N, D)
        nbytes = L.lib().bvc_op_attn_pool_workspace(B, N, D, R, splits)
        assert nbytes > 0 and nbytes % 4 == 0
        self.pooled, self.lse = Guarded((B, R, D), row=D), Guarded((B, R), row=R)
        self.ws = Guarded(((nbytes + 15) // 16 * 4,), fill=ws_fill, row=D)
        self.du = Guarded((R, D), row=D)
        self.dx = Guarded((B * N, ld), row=ld)
        u = u.contiguous()
        dpooled = dpooled.contiguous()
        lib, st = L.lib(), G.stream()
        L.check(lib.bvc_op_attn_pool_fwd(self.xb.data_ptr(), ld, u.data_ptr(), B, N, D, R, eps, splits, self.pooled.t.data_ptr(),
                                         self.lse.t.data_ptr(), self.ws.t.data_ptr(), st), "bvc_op_attn_pool_fwd")
        L.check(lib.bvc_op_attn_pool_bwd(self.xb.data_ptr(), ld, u.data_ptr(), self.pooled.t.data_ptr(), self.lse.t.data_ptr(),
                                         dpooled.data_ptr(), B, N, D, R, eps, splits, self.du.t.data_ptr(),
                                         self.dx.t.data_ptr() if want_dx else None, ld, self.ws.t.data_ptr(), st), "bvc_op_attn_pool_bwd")
        torch.cuda.synchronize()
        for name in ("pooled", "lse", "ws", "du", "dx"):
            getattr(self, name).check(name)
        self.dx_rows = self.dx.t[:, :D].reshape(B, N, D)
        if pad:
            assert bool(torch.isnan(self.dx.t[:, D:]).all()), "the padding of dx was written"
        if not want_dx:
            assert bool(torch.isnan(self.dx.t).all()), "dx written although NULL was passed"
        elif N:
            assert not bool(torch.isnan(self.dx_rows).any()), "dx: NaN or rows not written"
        assert not bool(torch.isnan(self.pooled.t).any() | torch.isnan(self.lse.t).any() | torch.isnan(self.du.t).any()), "NaN in pooled, lse or du"


class Ref:
    """float64 reference, torch-f32 comparator and scales of one set of inputs (computed once per case)."""

    def __init__(self, x, u, dpooled, eps=EPS):
        x64, u64, d64 = x.double(), u.double(), dpooled.double()
        self.pooled, self.lse = A.core(x64, u64, eps)
        self.du, self.dx = A.core_backward(x64, u64, eps, d64)
        self.t_pooled, self.t_lse = A.core(x, u, eps)
        self.t_du, self.t_dx = A.core_backward(x, u, eps, dpooled)
        self.sc = A.core_scales(x64, u64, eps, d64)
        self.eps_p = 2.0 ** -23 * (2 + self.sc["A"] + self.sc["S"])          # [B][R]


def _check(name, key, got, ref, t32, scale, eps_rel, items):
    """|got - ref| <= max(4 x worst torch-f32 relative error, eps_rel) x scale, floor 4 ulp; eps_rel broadcasts against scale"""
    got, t32 = got.double(), t32.double()
    nz = scale > 0
    wt = float(((t32 - ref).abs()[nz] / scale[nz]).max()) if bool(nz.any()) else 0.0
    err = (got - ref).abs()
    wk = float((err[nz] / scale[nz]).max()) if bool(nz.any()) else float(err.max())
    items.append(f"{key} {wk:.2e}/{wt:.2e}")
    bar = torch.maximum(torch.maximum(torch.full_like(scale, 4 * wt), eps_rel.expand_as(scale)) * scale, 4 * RR.ulp32(ref))
    bad = ~(err <= bar)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{name} {key}: {int(bad.sum())} of {bad.numel()} elements over the bar; at {i}: error {float(err[i]):.3e}, "
                             f"bar {float(bar[i]):.3e}, scale {float(scale[i]):.3e}, torch-f32 worst {wt:.3e}, kernel worst {wk:.3e}")


def check_run(name, run, ref, want_dx=True):
    items = []
    try:
        ep = ref.eps_p
        _check(name, "pooled", run.pooled.t, ref.pooled, ref.t_pooled, ref.sc["pooled"], ep[:, :, None], items)
        # lse: absolute
        terr = float((ref.t_lse.double() - ref.lse).abs().max())
        err = (run.lse.t.double() - ref.lse).abs()
        items.append(f"lse {float(err.max()):.2e}/{terr:.2e} (abs)")
        bad = ~(err <= torch.clamp(ep, min=4 * terr))
        assert not bool(bad.any()), f"{name} lse: {int(bad.sum())} over the bar, worst error {float(err.max()):.3e}, eps_p {float(ep.min()):.3e}"
        _check(name, "du", run.du.t, ref.du, ref.t_du, ref.sc["du"], 4 * ep.amax(0)[:, None], items)
        if want_dx:
            _check(name, "dx", run.dx_rows, ref.dx, ref.t_dx, ref.sc["dx"], 4 * ep.amax(1)[:, None, None], items)
    finally:
        G.log_parity(f"attentive {name}: " + "  ".join(items) + "   (kernel/torch-f32, relative to the element's scale)")


# ---------------------------------------------------------------------------------------------- shapes
# (B, N, D, R, splits, pad): every N edge of the 16-token tile, every accumulator-count instantiation (D / 64 <= 4, 12, 16, 24, 32),
# the 8-token tile of the backward with dx above D = 1024, forced splits with N % splits != 0 and N < splits, strided rows
SHAPES = [
    (1, 1, 64, 1, 1, 0), (3, 2, 64, 3, 2, 0), (1, 3, 64, 3, 7, 0), (1, 63, 192, 5, 1, 8), (3, 64, 192, 12, 2, 0), (1, 65, 192, 16, 7, 0),
    (1, 197, 192, 1, 1, 0), (3, 65, 64, 16, 0, 4), (1, 33, 512, 3, 2, 0), (1, 17, 768, 12, 1, 0), (2, 21, 1024, 16, 1, 0),
    (1, 64, 1408, 5, 0, 0), (3, 197, 1408, 12, 2, 4), (1, 19, 2048, 3, 1, 0),
]


@pytest.mark.parametrize("B,N,D,R,splits,pad", SHAPES)
def test_core_against_float64(B, N, D, R, splits, pad):
    x, u, dpooled = _inputs(B, N, D, R, seed=B * 1000 + N + D + R)
    ref = Ref(x, u, dpooled)
    name = f"B{B} N{N} D{D} R{R} splits{splits} pad{pad}"
    run = Run(x, u, dpooled, splits=splits, pad=pad)
    check_run(name, run, ref)
    # dx NULL: nothing of it is written, pooled / lse keep their bits and du its bar (above D = 1024 the backward tiles differently with dx)
    nodx = Run(x, u, dpooled, splits=splits, pad=pad, want_dx=False)
    assert _same_bits(nodx.pooled.t, run.pooled.t) and _same_bits(nodx.lse.t, run.lse.t), "pooled / lse differ between the two runs"
    check_run(name + " dx NULL", nodx, ref, want_dx=False)
    if D <= 1024:
        assert _same_bits(nodx.du.t, run.du.t), "du differs without dx"


def test_auto_splits_cut_a_long_clip():
    B, N, D, R = 1, 197, 192, 3
    assert L.lib().bvc_op_attn_pool_splits(B, N, D, R) == 3      # more than one workgroup per clip by default
    x, u, dpooled = _inputs(B, N, D, R, seed=11)
    check_run("auto splits N197", Run(x, u, dpooled), Ref(x, u, dpooled))


# ---------------------------------------------------------------------------------------------- hard cases
def _hard(kind):
    B, N, D, R = 2, 65, 192, 3
    x, u, dpooled = _inputs(B, N, D, R, seed=21)
    if kind == "onehot30":          # score spreads far above 88: an exp without the running max overflows
        u = torch.zeros(R, D, device=dev)
        for r in range(R):
            u[r, 7 + 50 * r] = 30.0 * (-1) ** r
    elif kind == "zero":
        u = torch.zeros(R, D, device=dev)
    elif kind == "constrow":        # variance 0: rstd = eps^-0.5, xh = 0
        x[0, 5] = 3.25
        x[1, 64] = -1.0
    elif kind == "onetoken":        # u along one token's direction: that token holds all the weight
        xh, _ = A.standardise(x.double(), EPS)
        u = torch.stack([xh[0, 9], 0.5 * xh[1, 64], -xh[0, 0]]).float()
    return x, u, dpooled


@pytest.mark.parametrize("kind", ["onehot30", "zero", "constrow", "onetoken"])
@pytest.mark.parametrize("splits", [1, 2])
def test_hard_cases(kind, splits):
    x, u, dpooled = _hard(kind)
    ref = Ref(x, u, dpooled)
    run = Run(x, u, dpooled, splits=splits)
    assert bool(torch.isfinite(run.pooled.t).all() & torch.isfinite(run.lse.t).all() & torch.isfinite(run.du.t).all()
                & torch.isfinite(run.dx_rows).all())
    check_run(f"{kind} splits{splits}", run, ref)
    if kind == "onehot30":
        s = A.standardise(x.double(), EPS)[0] @ u.double().t()
        assert float((s.amax(1) - s.amin(1)).min()) > 88
    if kind == "zero":
        xh = A.standardise(x.double(), EPS)[0]
        assert torch.allclose(ref.pooled, xh.mean(1, keepdim=True).expand_as(ref.pooled), rtol=0, atol=1e-14)
        assert float((run.lse.t.double() - math.log(x.shape[1])).abs().max()) <= float(ref.eps_p.max())
    if kind == "onetoken":
        p = torch.exp(s_of(x, u) - ref.lse[:, None, :])
        assert float(p[0, 9, 0]) > 1 - 1e-6 and float(p[1, 64, 1]) > 1 - 1e-6


def s_of(x, u):
    return A.standardise(x.double(), EPS)[0] @ u.double().t()


# ---------------------------------------------------------------------------------------------- invariants
def test_same_bits_on_every_run_and_with_a_poisoned_workspace():
    x, u, dpooled = _inputs(3, 197, 192, 12, seed=31)
    a = Run(x, u, dpooled, splits=7)
    b = Run(x, u, dpooled, splits=7)
    c = Run(x, u, dpooled, splits=7, ws_fill=1e30)
    d = Run(x, u, dpooled, splits=7, ws_fill=-3.0)
    for o in (b, c, d):
        for name in ("pooled", "lse", "du", "dx"):
            assert _same_bits(getattr(o, name).t, getattr(a, name).t), name


def test_a_clip_does_not_depend_on_its_neighbours():
    x, u, dpooled = _inputs(3, 65, 192, 5, seed=32)
    a = Run(x, u, dpooled, splits=2)
    x2, dp2 = x.clone(), dpooled.clone()
    x2[0] = 100 * torch.randn_like(x2[0])
    x2[2] = 0.0
    dp2[0] *= -3
    dp2[2] = 0.0
    b = Run(x2, u, dp2, splits=2)
    assert _same_bits(a.pooled.t[1], b.pooled.t[1]) and _same_bits(a.lse.t[1], b.lse.t[1]) and _same_bits(a.dx_rows[1], b.dx_rows[1])
    alone = Run(x[1:2], u, dpooled[1:2], splits=2)
    assert _same_bits(alone.pooled.t[0], a.pooled.t[1]) and _same_bits(alone.dx_rows[0], a.dx_rows[1])


def test_split_counts_agree_within_the_bar():
    x, u, dpooled = _inputs(2, 197, 192, 12, seed=33)
    ref = Ref(x, u, dpooled)
    for s in (1, 2, 7, 13):
        check_run(f"splits agree s{s}", Run(x, u, dpooled, splits=s), ref)


# ---------------------------------------------------------------------------------------------- Python op and modules
def test_attentive_pool_autograd_matches_the_abi():
    x, u, dpooled = _inputs(2, 65, 192, 3, seed=41)
    run = Run(x, u, dpooled, splits=2)
    xg, ug = x.clone().requires_grad_(True), u.clone().requires_grad_(True)
    pooled = bvc.attentive_pool(xg, ug, EPS, splits=2)
    pooled.backward(dpooled)
    assert _same_bits(pooled.detach(), run.pooled.t) and _same_bits(ug.grad, run.du.t) and _same_bits(xg.grad, run.dx_rows)
    # a frozen encoder: no dx is asked for
    u2 = u.clone().requires_grad_(True)
    p2, lse = bvc.attentive.attentive_pool_lse(x, u2, EPS, splits=2)
    p2.backward(dpooled)
    assert _same_bits(u2.grad, run.du.t) and _same_bits(lse, run.lse.t) and not lse.requires_grad
    # a strided view is taken as it is; a transposed one is copied
    wide = torch.full((2, 65, 200), float("nan"), device=dev)
    wide[:, :, :192] = x
    assert _same_bits(bvc.attentive_pool(wide[:, :, :192], u, EPS, splits=2), run.pooled.t)
    assert _same_bits(bvc.attentive_pool(x.transpose(0, 1).contiguous().transpose(0, 1), u, EPS, splits=2), run.pooled.t)
    assert bvc.attentive.splits(2, 65, 192, 3) == L.lib().bvc_op_attn_pool_splits(2, 65, 192, 3)


def _module_case():
    B, N, D, H, C = 2, 65, 192, 3, 10
    sd = A.make_params(D, H, C, seed=51)
    g = _gen(52)
    x = torch.randn(B, N, D, generator=g, device=dev) * 1.5 + 0.5 * torch.randn(B, N, 1, generator=g, device=dev)
    labels = torch.tensor([3, 8], device=dev)
    return B, N, D, H, C, sd, x, labels


def _rows(t):
    return t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])


def test_classifier_against_the_unfused_module():
    """logits, loss and every parameter gradient against the unfused float64 module; the bar of a row is 4 x the worst error of the
    float32 torch unfused module on the same device inputs, relative to the row's largest |reference| (floor 4 ulp)."""
    B, N, D, H, C, sd, x, labels = _module_case()
    sd64 = {k: v.to(dev) for k, v in sd.items()}
    sd32 = {k: v.float() for k, v in sd64.items()}
    lr, sr, gr = A.loss_and_grads(A.unfused_logits, sd64, x.double(), labels, H=H)
    lt, st, gt = A.loss_and_grads(A.unfused_logits, sd32, x, labels, H=H)
    model = bvc.AttentiveClassifier(D, H, C).to(dev)
    model.load_state_dict(sd32)
    logits = model(x)
    loss = bvc.videomae.soft_target_cross_entropy(logits, F.one_hot(labels, C).float())
    assert abs(float(loss.detach()) - float(F.cross_entropy(logits, labels).detach())) < 1e-6
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    got = {"logits": logits.detach(), "loss": loss.detach()}
    ref = {"logits": lr, "loss": sr}
    t32 = {"logits": lt, "loss": st}
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        got[k], ref[k], t32[k] = p.grad, gr[k], gt[k]
    assert set(dict(model.named_parameters())) == set(sd)
    items, fails = [], []
    for k in ref:
        r, g_, t = _rows(ref[k]), _rows(got[k].double()), _rows(t32[k].double())
        sc = r.abs().amax(-1)
        nz = sc > 0
        wt = float(((t - r).abs().amax(-1)[nz] / sc[nz]).max())
        eg = (g_ - r).abs().amax(-1)
        wk = float((eg[nz] / sc[nz]).max())
        items.append(f"{k.replace('pooler.cross_attention_block.', '')} {wk:.2e}/{wt:.2e}")
        bar = torch.maximum(4 * wt * sc, 4 * RR.ulp32(sc))
        if bool((~(eg <= bar)).any()):
            fails.append(f"{k}: kernel {wk:.3e} torch-f32 {wt:.3e}")
    G.log_parity("attentive classifier B2 N65 D192 H3: " + "  ".join(items) + "   (module/torch-f32 unfused, relative to the row's largest |ref|)")
    assert not fails, fails


def test_one_adamw_step_lowers_the_loss():
    B, N, D, H, C, sd, x, labels = _module_case()
    model = bvc.AttentiveClassifier(D, H, C).to(dev)
    opt = bvc.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.0)
    loss0 = F.cross_entropy(model(x), labels)
    loss0.backward()
    opt.step()
    opt.zero_grad()
    with torch.no_grad():
        loss1 = F.cross_entropy(model(x), labels)
    assert float(loss1) < float(loss0), (float(loss0), float(loss1))
