"""LARS and LAMB on the GPU (bvc_amd/optim.py, bvc_op_lars_step_table / bvc_op_lamb_step_table) against the float64 driver of
tests/layerwise_ref.py on its flat stand-in: seg_stats, free-running steps, many groups in one call, GradScaler's skipped step,
gradient-norm clipping, degenerate tensors, parameters outside flat buffers, the adapt=False identities, reproducibility, state dicts
and a real classification model.

Bars.  RTOL, ATOL = 2e-6, 2e-7 are the project's bars for an optimiser step (tests/test_gpu_optim_groups.py); exp_avg / exp_avg_sq take
the existing Adam bars.  ||w|| and ||d|| / ||u|| are sums of positive terms through an f32 chain of at most 16 terms and f64 above it:
2^-20 bounds their error, rtol 2e-6; a ratio is a quotient of two of them: 4e-6.

Gradients are 0.1 x standard normal.  ATOL is one f32 ulp at magnitude 2: the momentum buffer of a group that does not adapt, fed
unit-variance gradients for six steps at momentum 0.9, passes magnitude 4, where ONE correctly rounded f32 operation errs by more
than ATOL and float32(0.9) - 0.9 alone moves the sum by 1e-7.  A plain f32 restatement of the rule in torch on the CPU, on these groups
and sizes against the float64 driver, reaches 1.5 x the bar on ``momentum_buffer`` with unit-variance gradients and 0.24 x with these
(0.17 x on the parameters; LAMB: 0.13 x): at this scale the bar separates a wrong kernel from f32 rounding.

An Inf in the FROZEN stretch of the flat gradient buffer (not exercised here; the semantics are those of the other optimisers):
torch.amp.GradScaler looks at the gradients of the optimiser's parameters only and steps; bvc.amp.GradScaler without max_grad_norm
checks the whole buffer and skips the step; with max_grad_norm it checks the segments the optimiser owns and steps."""
import copy
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_util as G   # noqa: E402
from tests import layerwise_ref as lw   # noqa: E402
from tests.attention_ref import Arena   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402

bvc = G.bvc
dev = torch.device("cuda:0")
RTOL, ATOL = 2e-6, 2e-7
NORM_RTOL, RATIO_RTOL = 2e-6, 4e-6
GRAD_SCALE = 0.1
KINDS = ["lars", "lamb"]
FNS = {"lars": "bvc_op_lars_step_table", "lamb": "bvc_op_lamb_step_table"}

# live tensors of the stand-in: 0 (33, 7)  1 (129)  2 (64, 64)  3 (5)  4 (1)  5 (1023)  6 (49157)  7 (49157)  8 (1023)  9 (1)  10 (5)
# 11 (64, 64)  12 (129)  13 (33, 7).  Three groups: decayed and adapted / 1-D and not adapted / adapted with another trust coefficient
MEMBERS = [[0, 2, 4, 6], [1, 3, 5, 8, 12], [7, 9, 10, 11, 13]]
HYPER = {
    "lars": [dict(lr=0.5, momentum=0.9, weight_decay=0.01, trust_coefficient=0.001),
             dict(lr=0.05, momentum=0.9, weight_decay=0.0, adapt=False),
             dict(lr=0.3, momentum=0.8, weight_decay=0.0, trust_coefficient=0.02, nesterov=True)],
    "lamb": [dict(lr=2e-3, weight_decay=0.01),
             dict(lr=1e-3, weight_decay=0.0, betas=(0.8, 0.95), adapt=False),
             dict(lr=5e-3, weight_decay=0.05, eps=1e-8)],
}


class _Guard:
    """Device buffers with a NaN-filled guard band of their own on either side (one Arena each)."""

    def __init__(self):
        self.arenas = []

    def zeros(self, n, dtype, device=dev):
        A = Arena(dev, x=((int(n),), dtype))
        self.arenas.append(A)
        return A["x"].zero_()

    def check(self):
        for A in self.arenas:
            A.check()


class _Calls:
    """Counts calls of library entry points (the wrapper pattern of tests/test_gpu_optim_groups.py)."""

    def __init__(self, names):
        self.names, self.n = names, {k: 0 for k in names}

    def __enter__(self):
        lib = bvc._lib.lib()
        self.saved = {k: getattr(lib, k) for k in self.names}
        for k, fn in self.saved.items():
            def wrapper(*a, _k=k, _fn=fn):
                self.n[_k] += 1
                return _fn(*a)
            setattr(lib, k, wrapper)
        return self

    def __exit__(self, *exc):
        lib = bvc._lib.lib()
        for k, fn in self.saved.items():
            setattr(lib, k, fn)


def _grads(steps, n, seed=11):
    gen = torch.Generator().manual_seed(seed)
    return [GRAD_SCALE * torch.randn(n, generator=gen) for _ in range(steps)]


def _standin(guard=None, **kw):
    alloc = (lambda n, dtype: guard.zeros(n, dtype)) if guard is not None else None
    return lw.FlatStandIn(bvc, dev, alloc=alloc, **kw)


def _make(kind, groups, guard=None, **kw):
    opt = bvc.optim.LARS(groups, lr=0.1, **kw) if kind == "lars" else bvc.optim.LAMB(groups, **kw)
    if guard is not None:
        opt._zeros = guard.zeros
    return opt


def _three(kind, m, guard=None, members=MEMBERS, hyper=None, **kw):
    """-> (optimiser, driver) on the three groups; the frozen tensor rides in the first group without a gradient."""
    hyper = hyper or HYPER[kind]
    groups = [dict(params=[m.live[i] for i in idx] + ([m.frozen] if gi == 0 else []), **h) for gi, (idx, h) in enumerate(zip(members, hyper))]
    drv = lw.Driver(kind, [p.detach() for p in m.live], [dict(params=idx, **h) for idx, h in zip(members, hyper)],
                    max_grad_norm=kw.get("max_grad_norm"))
    return _make(kind, groups, guard, **kw), drv


def _close(got, want, rtol=RTOL, atol=ATOL, what=""):
    torch.testing.assert_close(got.detach().cpu().double().reshape(-1), want.reshape(-1), rtol=rtol, atol=atol, msg=lambda s: f"{what}: {s}")


def _state(opt, p, key):
    return opt.state[p][key]


def _check_against_driver(kind, opt, drv, params, what, ratios=True):
    for i, p in enumerate(params):
        _close(p, drv.w[i], what=f"{what} tensor {i}")
        if kind == "lars":
            _close(_state(opt, p, "momentum_buffer"), drv.buf[i], what=f"{what} momentum_buffer {i}")
        else:
            _close(_state(opt, p, "exp_avg"), drv.m[i], 1e-5, 1e-7, f"{what} exp_avg {i}")
            _close(_state(opt, p, "exp_avg_sq"), drv.v[i], 1e-5, 1e-9, f"{what} exp_avg_sq {i}")
    if ratios:
        tr = opt.trust_ratios()
        got = torch.stack([tr[p] for p in params]).cpu().double()
        want = torch.tensor([drv.stats[i][2] for i in range(len(params))], dtype=torch.float64)
        torch.testing.assert_close(got, want, rtol=RATIO_RTOL, atol=0.0, msg=lambda s: f"{what} trust ratios: {s}")


def _bits(t):
    return t.detach().clone().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else t.dtype)


def _snapshot(m, opt, params=None):
    """Everything a step may write, as bits: parameters, shadow, per-parameter state, seg_stats of every plan."""
    snap = [_bits(m._flat)] + ([_bits(m._shadow)] if m._shadow is not None else [])
    for p in params or m.live:
        snap += [_bits(v) for _k, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]
    snap += [_bits(pl.lw.stats) for pl in opt._get_plans()[0] if pl.lw is not None]
    return snap


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 1. seg_stats after one step
@pytest.mark.parametrize("kind", KINDS)
def test_seg_stats_of_one_step(kind):
    guard = _Guard()
    m = _standin(guard, shadow=True)
    opt, drv = _three(kind, m, guard)
    g = _grads(1, m.n)[0]
    m._flat_grad.copy_(g)
    (plan,), _ = opt._get_plans()
    R = opt._plan_range(plan)
    R.stats.fill_(float("nan"))                                # every row has to be written, the frozen segment's too
    opt.step()
    drv.step(m.split(g))
    stats = R.stats.cpu().double()
    assert R.nseg == 15 and len(R.owned) == 14
    (frozen,) = set(range(R.nseg)) - set(R.owned)
    assert stats[frozen].tolist() == [0.0, 0.0, 1.0]
    want = torch.tensor([drv.stats[i] for i in range(14)], dtype=torch.float64)
    got = stats[R.owned]
    for col, rtol, name in ((0, NORM_RTOL, "||w||"), (1, NORM_RTOL, "||d|| / ||u||"), (2, RATIO_RTOL, "ratio")):
        torch.testing.assert_close(got[:, col], want[:, col], rtol=rtol, atol=0.0, msg=lambda s, name=name: f"{name}: {s}")
    assert all(got[i, 2] == 1.0 for i in MEMBERS[1])            # the group that does not adapt
    # the 49157-element tensors span four items each with a ragged last one
    first = R.first.cpu()
    assert int(first[R.owned[6] + 1] - first[R.owned[6]]) == 4 and R.nitems == 14 + 2 * 3
    guard.check()


# ---------------------------------------------------------------------------------------------- 2. / 3. six free-running steps
@pytest.mark.parametrize("kind", KINDS)
def test_six_free_running_steps_match_the_float64_driver(kind):
    guard = _Guard()
    m = _standin(guard, shadow=True)
    opt, drv = _three(kind, m, guard)
    lo, hi = m.frozen_at
    frozen0, frozen_shadow0 = _bits(m._flat[lo:hi]), _bits(m._shadow[lo:hi])
    for it, g in enumerate(_grads(6, m.n)):
        m._flat_grad.copy_(g)
        opt.step()
        drv.step(m.split(g))
        _check_against_driver(kind, opt, drv, m.live, f"step {it}")
        assert torch.equal(_bits(m._flat[lo:hi]), frozen0) and torch.equal(_bits(m._shadow[lo:hi]), frozen_shadow0)
        assert torch.equal(_bits(m._shadow), _bits(m._flat.to(torch.bfloat16))), f"step {it}: shadow"
    if kind == "lamb":
        assert [float(_state(opt, p, "step")) for p in m.live] == [6.0] * 14 and drv.t == [6, 6, 6]
        assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    else:
        assert set(opt.state_dict()["state"][0]) == {"momentum_buffer"}
    assert m.frozen not in opt.state or not opt.state[m.frozen]
    guard.check()


# ---------------------------------------------------------------------------------------------- 4. twelve groups, one call per step
def _twelve_hyper(kind, i):
    if kind == "lars":
        return dict(lr=0.05 * (1 + 0.3 * i), momentum=0.5 + 0.03 * i, weight_decay=0.002 * i, trust_coefficient=0.001 * (1 + i),
                    nesterov=i % 3 == 0, adapt=i % 4 != 1)
    return dict(lr=1e-3 * (1 + 0.37 * i), weight_decay=0.01 * i, betas=(0.8 + 0.01 * i, 0.9 + 0.008 * i), eps=1e-6 if i % 2 else 1e-8,
                adapt=i % 4 != 1)


@pytest.mark.parametrize("kind", KINDS)
def test_twelve_groups_take_one_call_per_step_and_no_sync(kind):
    guard = _Guard()
    m = _standin(guard, shadow=True)
    hyper = [_twelve_hyper(kind, i) for i in range(12)]
    members = [[i] for i in range(12)]                           # the last two live tensors belong to no group: left untouched
    opt, drv = _three(kind, m, guard, members=members, hyper=hyper)
    assert len(opt.param_groups) == 12 > bvc._lib.OPT_MAX_GROUPS
    spare0 = [_bits(p) for p in m.live[12:]]
    grads = [g.to(dev) for g in _grads(4, m.n)]
    with _Calls(tuple(FNS.values()) + ("bvc_op_sgd_step_table", "bvc_op_adam_step_table")) as calls:
        for it, g in enumerate(grads):
            m._flat_grad.copy_(g)
            k = (5 * it + 1) % 12                                    # a schedule moves one group's rate per step
            opt.param_groups[k]["lr"] = drv.groups[k]["lr"] = opt.param_groups[k]["lr"] * 0.7
            if it == 0:
                opt.step()
            else:
                torch.cuda.set_sync_debug_mode("error")
                try:
                    opt.step()
                finally:
                    torch.cuda.set_sync_debug_mode("default")
            drv.step(m.split(g.cpu()))
            _check_against_driver(kind, opt, drv, m.live[:12], f"step {it}")
    assert calls.n == {k: (4 if k == FNS[kind] else 0) for k in calls.n}, calls.n
    assert all(torch.equal(_bits(p), b) for p, b in zip(m.live[12:], spare0))
    assert torch.equal(_bits(m._shadow), _bits(m._flat.to(torch.bfloat16)))
    guard.check()


# ---------------------------------------------------------------------------------------------- 5. GradScaler
@pytest.mark.parametrize("scaler_cls", ["torch", "bvc"])
@pytest.mark.parametrize("kind", KINDS)
def test_gradscaler_skips_the_step_with_an_inf(kind, scaler_cls):
    m = _standin(shadow=True)
    opt, drv = _three(kind, m)
    scaler = (torch.amp.GradScaler if scaler_cls == "torch" else bvc.amp.GradScaler)("cuda", init_scale=1024.0)
    scaler.scale(torch.zeros((), device=dev))                      # GradScaler creates its device-side scale lazily
    for it, g in enumerate(_grads(4, m.n, seed=5)):
        g = g.clone()
        bad = it == 2
        if bad:
            g[30000] = float("inf")                                # inside a 49157-element tensor of an adapted group
        assert scaler.get_scale() == (1024.0 if it <= 2 else 512.0)
        before = _snapshot(m, opt) if it else None
        m._flat_grad.copy_(g * scaler.get_scale())
        scaler.step(opt)
        scaler.update()
        drv.step(m.split(g), skip=bad)
        if bad:
            assert _same(_snapshot(m, opt), before)                # parameters, state, step counts, seg_stats, shadow
        _check_against_driver(kind, opt, drv, m.live, f"step {it}")
        assert torch.equal(_bits(m._shadow), _bits(m._flat.to(torch.bfloat16)))
    if kind == "lamb":
        assert [float(_state(opt, p, "step")) for p in m.live] == [3.0] * 14


def test_lars_norm_pass_raises_found_inf_for_owned_elements_only():
    """The LARS item pass applies grad_sqnorm_items_kernel's test to the gradient elements it reads: a NaN inside an owned tensor sets
    *found_inf and the rest of the sequence writes nothing; an Inf in the frozen stretch lies in no item and is not seen."""
    m = _standin(shadow=True)
    opt, _ = _three("lars", m)
    g = _grads(2, m.n, seed=31)
    m._flat_grad.copy_(g[0])
    opt.step()
    before = _snapshot(m, opt)
    opt.grad_scale, opt.found_inf = torch.ones((), device=dev), torch.zeros((), device=dev)
    try:
        bad = g[1].clone()
        bad[30000] = float("nan")
        m._flat_grad.copy_(bad)
        opt.step()
        assert float(opt.found_inf) == 1.0 and _same(_snapshot(m, opt), before)
        assert torch.equal(_bits(m._flat_grad), _bits(bad.to(dev)))          # the gradients were not written back either
        opt.found_inf.zero_()
        bad = g[1].clone()
        bad[m.frozen_at[0]] = float("inf")
        m._flat_grad.copy_(bad)
        opt.step()
        assert float(opt.found_inf) == 0.0 and not _same(_snapshot(m, opt), before)
        assert torch.isfinite(m._flat).all()
    finally:
        del opt.grad_scale, opt.found_inf


# ---------------------------------------------------------------------------------------------- 6. max_grad_norm
@pytest.mark.parametrize("kind", KINDS)
def test_max_grad_norm_active_on_some_steps_and_inactive_on_others(kind):
    m = _standin()
    opt, drv = _three(kind, m, max_grad_norm=1.0)
    coefs = []
    for it, (g, mul) in enumerate(zip(_grads(5, m.n, seed=7), (1.0, 0.01, 0.5, 0.02, 1.0))):
        g = g * mul                                              # ||g|| ~ 33 mul: the clip is active at 1 and 0.5, inactive at 0.01 and 0.02
        m._flat_grad.copy_(g)
        opt.step()
        drv.step(m.split(g))
        _check_against_driver(kind, opt, drv, m.live, f"step {it}")
        assert abs(float(opt.grad_norm) - drv.grad_norm) <= 1e-5 * drv.grad_norm
        assert abs(float(opt.clip_coef) - drv.clip_coef) <= 1e-5 * drv.clip_coef
        coefs.append(drv.clip_coef)
    assert [c < 1.0 for c in coefs] == [True, False, True, False, True]


# ---------------------------------------------------------------------------------------------- 7. degenerate tensors
@pytest.mark.parametrize("kind", KINDS)
def test_degenerate_tensors_fall_back_to_ratio_one(kind):
    m = _standin(shadow=True)
    m.live[2].data.zero_()                                        # an all-zero adapted tensor
    m._shadow.copy_(m._flat.to(torch.bfloat16))
    hyper = [dict(h, adapt=True) for h in HYPER[kind]]
    hyper[2]["weight_decay"] = 0.0                                # tensor 11 sits in this group: zero gradient, zero decay
    opt, drv = _three(kind, m, hyper=hyper)
    g = _grads(1, m.n, seed=3)[0]
    a, b = m.offsets[11]
    g[a:b] = 0.0
    m._flat_grad.copy_(g)
    before11 = _bits(m.live[11])
    opt.step()
    drv.step(m.split(g))
    tr = opt.trust_ratios()
    assert float(tr[m.live[2]]) == 1.0 and float(tr[m.live[11]]) == 1.0
    assert drv.stats[2][2] == 1.0 and drv.stats[11][2] == 1.0
    assert torch.equal(_bits(m.live[11]), before11)               # a zero update
    for i in (4, 9):                                              # the one-element tensors adapt like any other
        assert drv.stats[i][2] != 1.0
    _check_against_driver(kind, opt, drv, m.live, "degenerate")
    (plan,), _ = opt._get_plans()
    assert torch.isfinite(m._flat).all() and torch.isfinite(plan.lw.stats).all()
    assert all(torch.isfinite(v).all() for p in m.live for v in opt.state[p].values() if torch.is_tensor(v))
    assert torch.equal(_bits(m._shadow), _bits(m._flat.to(torch.bfloat16)))


# ---------------------------------------------------------------------------------------------- 8. parameters outside flat buffers
@pytest.mark.parametrize("kind", KINDS)
def test_loose_linear_steps_together_with_the_flat_buffer(kind):
    m = _standin()
    torch.manual_seed(3)
    lin = torch.nn.Linear(19, 7).to(dev)
    h = HYPER[kind]
    groups = [dict(params=[m.live[i] for i in MEMBERS[0]] + [lin.weight], **h[0]), dict(params=[m.live[i] for i in MEMBERS[1]] + [lin.bias], **h[1]),
              dict(params=[m.live[i] for i in MEMBERS[2]], **h[2])]
    opt = _make(kind, groups)
    drv = lw.Driver(kind, [p.detach() for p in m.live] + [lin.weight.detach(), lin.bias.detach()],
                    [dict(params=MEMBERS[0] + [14], **h[0]), dict(params=MEMBERS[1] + [15], **h[1]), dict(params=MEMBERS[2], **h[2])])
    lin.weight.grad, lin.bias.grad = torch.zeros_like(lin.weight), torch.zeros_like(lin.bias)
    params = m.live + [lin.weight, lin.bias]
    with _Calls((FNS[kind],)) as calls:
        for it, g in enumerate(_grads(4, m.n + 19 * 7 + 7, seed=13)):
            m._flat_grad.copy_(g[:m.n])
            gw, gb = g[m.n:m.n + 133].view(7, 19), g[m.n + 133:]
            lin.weight.grad.copy_(gw)
            lin.bias.grad.copy_(gb)
            opt.step()
            drv.step(m.split(g) + [gw, gb])
            _check_against_driver(kind, opt, drv, params, f"step {it}")
    assert calls.n[FNS[kind]] == 4 * 3                           # the flat buffer, the weight, the bias: the same entry point
    assert float(opt.trust_ratios()[lin.bias]) == 1.0 and float(opt.trust_ratios()[lin.weight]) != 1.0


@pytest.mark.parametrize("kind", KINDS)
def test_loose_runs_that_join_and_part_keep_their_state(kind):
    """Two memory-adjacent parameters outside any flat buffer whose gradients are adjacent on some steps (one run, two segments) and
    apart on others (two runs), as autograd's fresh gradient allocations can fall: the state follows every regrouping."""
    gen = torch.Generator().manual_seed(29)
    store = torch.randn(256, generator=gen).to(dev)
    a, b = torch.nn.Parameter(store[:128].view(8, 16)), torch.nn.Parameter(store[128:])
    h = dict(HYPER[kind][0])
    opt = _make(kind, [dict(params=[a, b], **h)])
    drv = lw.Driver(kind, [a.detach(), b.detach()], [dict(params=[0, 1], **h)])
    joint, room = torch.zeros(256, device=dev), torch.zeros(384, device=dev)
    apart = (room[:128], room[256:])                              # 128 elements between the two gradients
    with _Calls((FNS[kind],)) as calls:
        for it, together in enumerate((False, True, False, True, True, False)):
            ga, gb = GRAD_SCALE * torch.randn(128, generator=gen), GRAD_SCALE * torch.randn(128, generator=gen)
            a.grad, b.grad = (joint[:128].view(8, 16), joint[128:]) if together else (apart[0].view(8, 16), apart[1])
            a.grad.copy_(ga.view(8, 16))
            b.grad.copy_(gb)
            opt.step()
            drv.step([ga, gb])
            _check_against_driver(kind, opt, drv, [a, b], f"step {it}")
    assert calls.n[FNS[kind]] == 3 * 2 + 3 * 1
    if kind == "lamb":
        assert float(opt.state[a]["step"]) == float(opt.state[b]["step"]) == 6.0


# ---------------------------------------------------------------------------------------------- 9. adapt=False is SGD / AdamW
@pytest.mark.parametrize("kind", KINDS)
def test_without_adaptation_the_step_is_sgd_or_adamw(kind):
    m, twin = _standin(), _standin()
    assert torch.equal(m._flat, twin._flat)
    if kind == "lars":
        hyper = [dict(lr=0.05, momentum=0.9, weight_decay=0.01), dict(lr=0.02, momentum=0.5, weight_decay=0.0, nesterov=True),
                 dict(lr=0.1, momentum=0.8, weight_decay=0.003)]
    else:
        hyper = [dict(lr=2e-3, weight_decay=0.01, eps=1e-6), dict(lr=1e-3, weight_decay=0.0, betas=(0.8, 0.95), eps=1e-6),
                 dict(lr=5e-3, weight_decay=0.05, eps=1e-8)]
    mine = [dict(params=[m.live[i] for i in idx], adapt=False, **h) for idx, h in zip(MEMBERS, hyper)]
    theirs = [dict(params=[twin.live[i] for i in idx], **h) for idx, h in zip(MEMBERS, hyper)]
    opt = _make(kind, mine)
    ropt = bvc.optim.SGD(theirs, lr=0.1, momentum=0.9) if kind == "lars" else bvc.optim.AdamW(theirs)
    for it, g in enumerate(_grads(6, m.n, seed=17)):
        m._flat_grad.copy_(g)
        twin._flat_grad.copy_(g)
        opt.step()
        ropt.step()
        for i, (p, r) in enumerate(zip(m.live, twin.live)):
            torch.testing.assert_close(p.data, r.data, rtol=RTOL, atol=ATOL, msg=lambda s, i=i, it=it: f"step {it} tensor {i}: {s}")
    assert all(float(v) == 1.0 for v in opt.trust_ratios().values())


# ---------------------------------------------------------------------------------------------- 10. reproducibility
def _run_three(kind):
    m = _standin(shadow=True)
    opt, _ = _three(kind, m)
    for g in _grads(3, m.n, seed=19):
        m._flat_grad.copy_(g)
        opt.step()
    torch.cuda.synchronize()
    return _snapshot(m, opt)


@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_give_the_same_bits_without_deterministic_mode(kind):
    assert not torch.are_deterministic_algorithms_enabled() and not bvc.are_deterministic_algorithms_enabled()
    assert _same(_run_three(kind), _run_three(kind))


# ---------------------------------------------------------------------------------------------- 11. state dict
@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_round_trip_into_fresh_and_stepped_optimisers(kind):
    m = _standin()
    opt, _ = _three(kind, m)
    g = _grads(4, m.n, seed=23)

    def two(o, a, b):
        for x in (a, b):
            m._flat_grad.copy_(x)
            o.step()
    two(opt, g[0], g[1])
    kept, params = copy.deepcopy(opt.state_dict()), m._flat.clone()
    two(opt, g[2], g[3])
    record = _snapshot(m, opt)
    m._flat.copy_(params)
    fresh, _ = _three(kind, m)
    fresh.load_state_dict(kept)
    two(fresh, g[2], g[3])
    assert _same(_snapshot(m, fresh), record)
    m._flat.copy_(params)
    opt.load_state_dict(kept)                                     # into an optimiser that has already stepped
    two(opt, g[2], g[3])
    assert _same(_snapshot(m, opt), record)
    if kind == "lamb":
        assert all(float(st["step"]) == 4.0 for st in opt.state_dict()["state"].values())


# ---------------------------------------------------------------------------------------------- 12. a real model
def test_classification_model_takes_three_lars_steps():
    cfg = dataclasses.replace(vo.TINY, num_frames=2, tubelet_size=1, image_size=64, patch_size=16)      # the smallest of test_gpu_dropout.py's matrix
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    torch.manual_seed(0)
    model = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(num_labels=10, **kw)).to(dev).train()
    named = {n: p for n, p in model.named_parameters() if p.requires_grad}
    index = {id(p): i for i, p in enumerate(named.values())}
    groups = bvc.optim.adaptive_param_groups(model, 0.05)
    hyper = dict(lr=0.1, momentum=0.9, trust_coefficient=0.001)
    opt = bvc.optim.LARS(groups, **hyper)
    drv = lw.Driver("lars", [p.detach() for p in named.values()],
                    [dict(params=[index[id(p)] for p in g["params"]], weight_decay=g["weight_decay"], adapt=g["adapt"], **hyper) for g in groups])
    with _Calls((FNS["lars"],)) as calls:
        for it in range(3):
            px, y = vo.synthetic_batch(cfg, 3, it, 0.9)[0].to(dev), torch.tensor([it, 7 - it, 4], device=dev)
            opt.zero_grad()
            model(pixel_values=px, labels=y).loss.backward()
            grads = [p.grad.detach().clone() for p in named.values()]
            opt.step()
            drv.step(grads)
            for n, p in named.items():
                _close(p, drv.w[index[id(p)]], what=f"step {it} {n}")
    plans, loose = opt._get_plans()
    assert len(plans) == 1 and plans[0].module is model and sum(len(ps) for ps in loose.values()) == 4      # fc_norm and the classifier
    assert 3 * (1 + 2) <= calls.n[FNS["lars"]] <= 3 * (1 + 4)    # per step: one call for the flat buffer, one per loose run (2 to 4)
    tr = opt.trust_ratios()
    assert all(float(tr[p]) == 1.0 for p in groups[1]["params"]) and all(0.0 < float(tr[p]) != 1.0 for p in groups[0]["params"])
    ptr, n = model._shadow_base(), model._numel
    assert ptr is not None                                       # the fused steps kept the copy current

    class _Dev:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<i2", "data": (ptr, False), "version": 2}
    assert torch.equal(torch.as_tensor(_Dev(), device=dev), model._flat.to(torch.bfloat16).view(torch.int16))
    model.eval()
    px = vo.synthetic_batch(cfg, 3, 9, 0.9)[0].to(dev)
    with torch.no_grad():
        logits = model(pixel_values=px).logits
        again = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(num_labels=10, **kw))
        again.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
        assert torch.equal(logits, again.to(dev).eval()(pixel_values=px).logits)
