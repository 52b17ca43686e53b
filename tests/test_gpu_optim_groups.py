"""The fused optimisers with MORE parameter groups than the by-value struct carries (bvc_amd/optim.py, bvc_op_sgd_step_table /
bvc_op_adam_step_table): one launch per flat module through a device table of hyper-parameters, against torch.optim on clones and,
bit for bit, against the by-value kernels; GradScaler's skipped step; load_state_dict into an optimiser that has already stepped;
layer-wise learning-rate decay on a real classification model.

The stand-in flat module holds the tensor sizes 33 x 7, 129, 64 x 64, a frozen tensor (no gradient), 5, 1, 1023 and then the six live
sizes once more in reverse order: twelve live tensors, one per group at twelve groups.  Segments begin at offsets that are no
multiples of four, quads straddle segment boundaries, and a 1024-element block holds several segments."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_util as G   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402

bvc = G.bvc
dev = torch.device("cuda:0")
RTOL, ATOL = 2e-6, 2e-7                       # the project's bars for an optimiser step against torch (test_gpu_ops.py)

LIVE = [(33, 7), (129,), (64, 64), (5,), (1,), (1023,)]
SHAPES = LIVE[:3] + [None] + LIVE[3:] + LIVE[::-1]      # None: the frozen tensor, in the middle of the first set
FROZEN = 10


class _FlatStandIn:
    """What the optimisers need of a flat module (flat.py): `_flat`, `_flat_grad`, `_shadow_base()`, membership of flat._MODULES."""

    def __init__(self, seed=0, shadow=False):
        gen = torch.Generator().manual_seed(seed)
        n = sum(FROZEN if s is None else int(np.prod(s)) for s in SHAPES)
        self._flat = torch.randn(n, generator=gen).to(dev)
        self._flat_grad = torch.zeros(n, device=dev)
        self._shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev) if shadow else None
        self.live, o = [], 0
        for s in SHAPES:
            k = FROZEN if s is None else int(np.prod(s))
            p = torch.nn.Parameter(self._flat[o:o + k].view(s or (k,)), requires_grad=s is not None)
            if s is None:
                self.frozen, self.frozen_at = p, (o, o + k)
            else:
                p.grad = self._flat_grad[o:o + k].view(s)
                self.live.append(p)
            o += k
        bvc.flat._MODULES.add(self)

    def _shadow_base(self):
        return None if self._shadow is None else self._shadow.data_ptr()


def _owns(module, ptr):
    return module._flat.data_ptr() <= ptr < module._flat.data_ptr() + 4 * module._flat.numel()


def _grads(steps, n, seed=11):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen).to(dev) for _ in range(steps)]


def _clones(m):
    return [torch.nn.Parameter(p.detach().clone()) for p in m.live]


def _feed(m, ref, g, scale=1.0):
    """The step's gradient into the flat gradient buffer (scaled as a GradScaler's backward leaves it) and onto the clones."""
    m._flat_grad.copy_(g * scale)
    for p, r in zip(m.live, ref):
        r.grad = p.grad.detach().clone()


def _hyper(i, adam):
    if adam:
        return dict(lr=1e-3 * (1 + 0.37 * i), weight_decay=0.01 * i, betas=(0.8 + 0.01 * i, 0.9 + 0.008 * i))
    return dict(lr=0.02 * (1 + 0.21 * i), weight_decay=0.003 * i, momentum=0.5 + 0.03 * i)


def _twelve(m, ref, adam):
    """One live tensor per group, twelve groups with distinct hyper-parameters; the frozen tensor rides in group 4 without a gradient."""
    mine = [dict(params=[p] + ([m.frozen] if i == 4 else []), **_hyper(i, adam)) for i, p in enumerate(m.live)]
    theirs = [dict(params=[r], **_hyper(i, adam)) for i, r in enumerate(ref)]
    return mine, theirs


class _Calls:
    """Counts calls of library entry points (the wrapper pattern of test_gpu_jepa.py), optionally only those whose first argument -
    the parameter address - lies in a given flat module."""

    def __init__(self, names, module=None):
        self.names, self.module, self.n = names, module, {k: 0 for k in names}

    def __enter__(self):
        lib = bvc._lib.lib()
        self.saved = {k: getattr(lib, k) for k in self.names}
        for k, fn in self.saved.items():
            def wrapper(*a, _k=k, _fn=fn):
                if self.module is None or _k.endswith("_prepare") or _owns(self.module, int(a[0])):
                    self.n[_k] += 1
                return _fn(*a)
            setattr(lib, k, wrapper)
        return self

    def __exit__(self, *exc):
        lib = bvc._lib.lib()
        for k, fn in self.saved.items():
            setattr(lib, k, fn)


ADAM_FNS = ("bvc_op_adam_step_table", "bvc_op_adam_step_segments", "bvc_op_adam_step", "bvc_op_adam_prepare")
SGD_FNS = ("bvc_op_sgd_step_table", "bvc_op_sgd_step_segments", "bvc_op_sgd_step")


# ---------------------------------------------------------------------------------------------- 1. twelve groups against torch
@pytest.mark.parametrize("adam", [True, False], ids=["adamw", "sgd_nesterov"])
def test_twelve_groups_match_torch_with_one_table_call_per_step(adam):
    m = _FlatStandIn()
    ref = _clones(m)
    frozen0 = m.frozen.detach().clone()
    mine, theirs = _twelve(m, ref, adam)
    if adam:
        opt, ropt = bvc.optim.AdamW(mine), torch.optim.AdamW(theirs, foreach=False)
    else:
        opt, ropt = bvc.optim.SGD(mine, lr=0.1, nesterov=True, momentum=0.9), torch.optim.SGD(theirs, lr=0.1, nesterov=True, momentum=0.9, foreach=False)
    with _Calls(ADAM_FNS if adam else SGD_FNS) as calls:
        for it, g in enumerate(_grads(4, m._flat.numel())):
            _feed(m, ref, g)
            k = (5 * it + 1) % 12                                    # a schedule moves one group's rate per step
            opt.param_groups[k]["lr"] = ropt.param_groups[k]["lr"] = opt.param_groups[k]["lr"] * 0.7
            opt.step()
            ropt.step()
            torch.cuda.synchronize()
            for i, (p, r) in enumerate(zip(m.live, ref)):
                torch.testing.assert_close(p.data, r.data, rtol=RTOL, atol=ATOL, msg=lambda s, i=i, it=it: f"step {it} tensor {i}: {s}")
    table = "bvc_op_adam_step_table" if adam else "bvc_op_sgd_step_table"
    assert calls.n == {k: (4 if k == table else 0) for k in calls.n}, calls.n      # one table call per step, nothing per run
    assert torch.equal(m.frozen.detach(), frozen0)
    sd, rsd = opt.state_dict(), ropt.state_dict()
    index = {id(p): i for i, p in enumerate(q for g in opt.param_groups for q in g["params"])}
    for p, r in zip(m.live, ref):
        st, rst = sd["state"][index[id(p)]], ropt.state[r]
        if adam:
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 4.0
            assert torch.allclose(st["exp_avg"], rst["exp_avg"], rtol=1e-5, atol=1e-7)
            assert torch.allclose(st["exp_avg_sq"], rst["exp_avg_sq"], rtol=1e-5, atol=1e-9)
        else:
            assert set(st) == {"momentum_buffer"}
            torch.testing.assert_close(st["momentum_buffer"], rst["momentum_buffer"], rtol=RTOL, atol=ATOL)
    assert index[id(m.frozen)] not in sd["state"] and len(rsd["state"]) == 12


# ---------------------------------------------------------------------------------------------- 2. the by-value path is the oracle
def _run_four_steps(kind, split):
    """Four groups of three tensors each (by value), or every group split into three groups of the same hyper-parameters (table).
    kind: "adamw" (decoupled decay), "adam" (the decay enters the gradient) or "sgd_nesterov"."""
    adam = kind != "sgd_nesterov"
    m = _FlatStandIn(shadow=True)
    order = [0, 7, 3, 10, 1, 4, 9, 6, 2, 11, 5, 8]                  # the groups interleave in memory
    groups = []
    for gi in range(4):
        ps = [m.live[j] for j in order[3 * gi:3 * gi + 3]]
        if gi == 2:
            ps.append(m.frozen)
        groups += [dict(params=[p], **_hyper(gi, adam)) for p in ps[:3]] if split else [dict(params=ps, **_hyper(gi, adam))]
        if split and gi == 2:
            groups[-1]["params"].append(m.frozen)
    opt = getattr(bvc.optim, "AdamW" if kind == "adamw" else "Adam")(groups) if adam else bvc.optim.SGD(groups, lr=0.1, nesterov=True, momentum=0.9)
    fns = ADAM_FNS if adam else SGD_FNS
    with _Calls(fns) as calls:
        for it, g in enumerate(_grads(4, m._flat.numel())):
            m._flat_grad.copy_(g)
            for gr in opt.param_groups:
                gr["lr"] = gr["lr"] * (1.0 - 0.1 * it)
            opt.step()
    torch.cuda.synchronize()
    used = fns[0] if split else fns[1]
    assert calls.n == {k: (4 if k == used else 0) for k in fns}, calls.n
    sd = opt.state_dict()["state"]
    index = {id(p): i for i, p in enumerate(q for g in opt.param_groups for q in g["params"])}
    state = [{k: v.detach().clone() for k, v in sd[index[id(p)]].items()} for p in m.live]
    return m._flat.clone(), m._shadow.clone(), state, m._flat_grad.clone()


@pytest.mark.parametrize("kind", ["adamw", "adam", "sgd_nesterov"])
def test_table_kernels_equal_by_value_kernels_bit_for_bit(kind):
    flat4, shadow4, state4, grad4 = _run_four_steps(kind, split=False)
    flat12, shadow12, state12, grad12 = _run_four_steps(kind, split=True)
    assert torch.equal(flat4, flat12) and torch.equal(grad4, grad12)
    assert torch.equal(shadow4.view(torch.int16), shadow12.view(torch.int16))
    for a, b in zip(state4, state12):
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    # the shadow is the bf16 image of the parameters wherever a group owns them, and untouched (zero) under the frozen tensor
    m = _FlatStandIn()
    lo, hi = m.frozen_at
    want = flat12.to(torch.bfloat16)
    want[lo:hi] = 0
    assert torch.equal(shadow12.view(torch.int16), want.view(torch.int16))


# ---------------------------------------------------------------------------------------------- 3. GradScaler
def test_gradscaler_skips_a_step_for_every_group():
    m = _FlatStandIn()
    ref = _clones(m)
    mine, theirs = _twelve(m, ref, True)
    opt, ropt = bvc.optim.AdamW(mine), torch.optim.AdamW(theirs, foreach=False)
    scaler, rscaler = bvc.amp.GradScaler("cuda", init_scale=1024.0), torch.amp.GradScaler("cuda", init_scale=1024.0)
    for s in (scaler, rscaler):
        s.scale(torch.zeros((), device=dev))                         # GradScaler creates its device-side scale lazily
    index = {id(p): i for i, p in enumerate(q for g in opt.param_groups for q in g["params"])}
    steps = lambda: [float(opt.state_dict()["state"][index[id(p)]]["step"]) for p in m.live]      # noqa: E731
    with _Calls(ADAM_FNS) as calls:
        for it, g in enumerate(_grads(3, m._flat.numel(), seed=5)):
            assert scaler.get_scale() == rscaler.get_scale()
            g = g.clone()
            if it == 1:
                g[4500] = float("inf")                               # inside a live tensor of the flat gradient buffer
            before = m._flat.clone()
            _feed(m, ref, g, scale=scaler.get_scale())
            scaler.step(opt)
            scaler.update()
            rscaler.step(ropt)
            rscaler.update()
            torch.cuda.synchronize()
            if it == 1:
                assert torch.equal(m._flat, before) and steps() == [1.0] * 12
            for p, r in zip(m.live, ref):
                torch.testing.assert_close(p.data, r.data, rtol=RTOL, atol=ATOL)
    assert steps() == [2.0] * 12 and scaler.get_scale() == rscaler.get_scale() == 512.0
    assert calls.n == {"bvc_op_adam_step_table": 3, "bvc_op_adam_step_segments": 0, "bvc_op_adam_step": 0, "bvc_op_adam_prepare": 0}


# ---------------------------------------------------------------------------------------------- 4. load_state_dict, warmed optimiser
@pytest.mark.parametrize("ngroups", [4, 12])
@pytest.mark.parametrize("adam", [True, False], ids=["adamw", "sgd_nesterov"])
def test_load_state_dict_into_an_optimiser_that_has_stepped(adam, ngroups):
    m = _FlatStandIn()
    per = 12 // ngroups
    groups = [dict(params=m.live[per * i:per * i + per], **_hyper(i, adam)) for i in range(ngroups)]
    opt = bvc.optim.AdamW(groups) if adam else bvc.optim.SGD(groups, lr=0.1, nesterov=True, momentum=0.9)
    g = _grads(4, m._flat.numel(), seed=23)

    def two(a, b):
        for x in (a, b):
            m._flat_grad.copy_(x)
            opt.step()
    two(g[0], g[1])
    kept, params = copy.deepcopy(opt.state_dict()), m._flat.clone()
    two(g[2], g[3])
    record = m._flat.clone()
    m._flat.copy_(params)
    opt.load_state_dict(kept)
    two(g[2], g[3])
    torch.cuda.synchronize()
    assert torch.equal(m._flat, record)
    if adam:
        assert all(float(st["step"]) == 4.0 for st in opt.state_dict()["state"].values())


# ---------------------------------------------------------------------------------------------- 5. a real model under layer decay
def test_classification_model_under_layer_decay():
    cfg = vo.TINY
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    kw["num_hidden_layers"] = 3
    torch.manual_seed(0)
    model = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(num_labels=10, **kw)).to(dev).train()
    batches = [(vo.synthetic_batch(cfg, 2, s, 0.9)[0].to(dev), torch.tensor([s, 7 - s], device=dev)) for s in range(2)]
    groups = bvc.optim.layer_decay_param_groups(model, 1e-3, 0.05, 0.75)
    assert len(groups) == 2 * (3 + 2) > bvc._lib.OPT_MAX_GROUPS
    idle = torch.nn.Parameter(torch.ones(3, device=dev))             # a group that never gets a gradient must not disturb the step
    groups.append({"params": [idle], "name": "idle", "lr_scale": 1.0})
    named = dict(model.named_parameters())
    twins = {n: torch.nn.Parameter(p.detach().clone()) for n, p in named.items()}
    name_of = {id(p): n for n, p in named.items()}
    opt = bvc.optim.AdamW(groups, lr=1e-3)
    ropt = torch.optim.AdamW([dict({k: v for k, v in g.items() if k != "params"}, params=[twins[name_of[id(p)]] for p in g["params"]])
                              for g in groups[:-1]], lr=1e-3, foreach=False)
    scaler = bvc.amp.GradScaler("cuda", init_scale=1024.0)
    with _Calls(ADAM_FNS, module=model) as calls:
        for it, (px, y) in enumerate(batches):
            bvc.optim.set_base_lr(opt, 1e-3 * (it + 1) / 2)           # warm-up
            bvc.optim.set_base_lr(ropt, 1e-3 * (it + 1) / 2)
            opt.zero_grad()
            scaler.scale(model(pixel_values=px, labels=y).loss).backward()
            inv = 1.0 / scaler.get_scale()
            for n, p in named.items():
                twins[n].grad = p.grad.detach().clone() * inv
            scaler.step(opt)
            scaler.update()
            ropt.step()
            torch.cuda.synchronize()
            for n, p in named.items():
                torch.testing.assert_close(p.data, twins[n].data, rtol=RTOL, atol=ATOL, msg=lambda s, n=n, it=it: f"step {it} {n}: {s}")
    # the encoder's flat buffer: one table call per step, no per-run launch; fc_norm and the classifier stay on the per-run path
    assert calls.n["bvc_op_adam_step_table"] == 2 and calls.n["bvc_op_adam_step_segments"] == 0 and calls.n["bvc_op_adam_step"] == 0
    assert torch.equal(idle.detach(), torch.ones(3, device=dev))
    plans, loose = opt._get_plans()
    assert len(plans) == 1 and plans[0].module is model and plans[0].table
    # autograd hands fc_norm and the classifier fresh gradient tensors every step: the encoder's plan and its flat state must survive that
    exp_avg = plans[0].state[0].data_ptr()
    for ps in loose.values():
        for p in ps:
            p.grad = p.grad.clone()
    again, _ = opt._get_plans()
    assert again[0] is plans[0] and again[0].state[0].data_ptr() == exp_avg
    assert sorted(name_of[id(p)] for ps in loose.values() for p in ps) == ["classifier.bias", "classifier.weight", "fc_norm.bias", "fc_norm.weight"]


# ---------------------------------------------------------------------------------------------- 6. unchanged below nine groups
@pytest.mark.parametrize("adam", [True, False], ids=["adamw", "sgd_nesterov"])
def test_four_groups_stay_on_the_by_value_entry_points(adam):
    m = _FlatStandIn()
    groups = [dict(params=m.live[3 * i:3 * i + 3], **_hyper(i, adam)) for i in range(4)]
    opt = bvc.optim.AdamW(groups) if adam else bvc.optim.SGD(groups, lr=0.1, nesterov=True, momentum=0.9)
    fns = ADAM_FNS if adam else SGD_FNS
    with _Calls(fns) as calls:
        for g in _grads(3, m._flat.numel()):
            m._flat_grad.copy_(g)
            opt.step()
    torch.cuda.synchronize()
    assert calls.n == {k: (3 if k == fns[1] else 0) for k in fns}, calls.n
    assert not opt._get_plans()[0][0].table
