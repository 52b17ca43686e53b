"""The float64 references of the layer-wise optimisers (tests/layerwise_ref.py) on the host, WITHOUT a GPU: with ``adapt=False`` they are
torch's momentum SGD / AdamW, the fallbacks of the trust ratio, LARS's invariance under a rescaled gradient, and the grouping helpers
(``bvc.optim.adaptive_param_groups``; ``layer_decay_param_groups`` output handed to ``bvc.optim.LARS`` / ``LAMB`` unchanged)."""
import pytest
import torch

from oracle import videomae_oracle as vo
from tests import layerwise_ref as lw

F64 = torch.float64
SIZES = [(7, 5), (13,), (1,), (64, 3)]


def _tensors(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen, dtype=F64) for s in SIZES]


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("nesterov", [False, True])
def test_lars_without_adaptation_is_torch_momentum_sgd(nesterov):
    w0 = _tensors(0)
    twins = [torch.nn.Parameter(w.clone()) for w in w0]
    hyper = [dict(lr=0.05, momentum=0.9, weight_decay=0.01), dict(lr=0.02, momentum=0.5, weight_decay=0.0)]
    drv = lw.Driver("lars", w0, [dict(params=[0, 1], adapt=False, nesterov=nesterov, **hyper[0]),
                                 dict(params=[2, 3], adapt=False, nesterov=nesterov, **hyper[1])])
    ropt = torch.optim.SGD([dict(params=twins[:2], **hyper[0]), dict(params=twins[2:], **hyper[1])], lr=0.1, momentum=0.9,
                           nesterov=nesterov, foreach=False)
    for it in range(6):
        grads = _tensors(100 + it)
        for p, g in zip(twins, grads):
            p.grad = g.clone()
        ropt.step()
        drv.step(grads)
        for i, p in enumerate(twins):
            assert _rel(drv.w[i], p.data) < 1e-12 and _rel(drv.buf[i], ropt.state[p]["momentum_buffer"]) < 1e-12, (it, i)
            assert drv.stats[i][2] == 1.0


def test_lamb_without_adaptation_is_torch_adamw():
    w0 = _tensors(1)
    twins = [torch.nn.Parameter(w.clone()) for w in w0]
    hyper = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01), dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-8, weight_decay=0.0)]
    drv = lw.Driver("lamb", w0, [dict(params=[0, 1], adapt=False, **hyper[0]), dict(params=[2, 3], adapt=False, **hyper[1])])
    ropt = torch.optim.AdamW([dict(params=twins[:2], **hyper[0]), dict(params=twins[2:], **hyper[1])], foreach=False)
    for it in range(6):
        grads = _tensors(200 + it)
        for p, g in zip(twins, grads):
            p.grad = g.clone()
        ropt.step()
        drv.step(grads)
        for i, p in enumerate(twins):
            st = ropt.state[p]
            assert _rel(drv.w[i], p.data) < 1e-12 and _rel(drv.m[i], st["exp_avg"]) < 1e-12 and _rel(drv.v[i], st["exp_avg_sq"]) < 1e-12, (it, i)
    assert drv.t == [6, 6]


def test_skipped_steps_and_clipping_in_the_driver():
    w0, grads = _tensors(2), _tensors(3)
    a = lw.Driver("lamb", w0, [dict(params=[0, 1, 2, 3], lr=1e-2)], max_grad_norm=0.5)
    a.step(grads, skip=True)
    assert a.t == [0] and all(torch.equal(x, y) for x, y in zip(a.w, w0))
    a.step(grads)
    norm = float(torch.sqrt(sum((g ** 2).sum() for g in grads)))
    assert a.t == [1] and abs(a.grad_norm - norm) < 1e-12 * norm and a.clip_coef == min(1.0, 0.5 / (norm + 1e-6)) < 1.0
    b = lw.Driver("lamb", w0, [dict(params=[0, 1, 2, 3], lr=1e-2)])
    b.step([g * a.clip_coef for g in grads])
    assert all(torch.equal(x, y) for x, y in zip(a.w, b.w))


def test_trust_ratio_fallbacks():
    gen = torch.Generator().manual_seed(4)
    g, w = torch.randn(50, generator=gen, dtype=F64), torch.randn(50, generator=gen, dtype=F64)
    zero = torch.zeros(50, dtype=F64)
    # an all-zero tensor: ratio 1 (plain step), for either rule
    w1, buf, stats = lw.lars_step(zero, g, zero, lr=0.1, weight_decay=0.1)
    assert stats == (0.0, float(g.norm()), 1.0) and torch.equal(buf, g) and torch.equal(w1, -0.1 * g)
    _w, _m, _v, stats = lw.lamb_step(zero, g, zero, zero, 1, lr=0.1)
    assert stats[0] == 0.0 and stats[2] == 1.0
    # LARS with a zero gradient and no decay: ||d|| = 0, ratio 1, nothing moves
    w1, buf, stats = lw.lars_step(w, zero, zero, lr=0.1, weight_decay=0.0)
    assert stats == (float(w.norm()), 0.0, 1.0) and torch.equal(w1, w) and torch.equal(buf, zero)
    # otherwise the rules' ratios
    _w, _buf, stats = lw.lars_step(w, g, zero, lr=0.1, weight_decay=0.1, trust_coefficient=0.02)
    assert stats[2] == 0.02 * float(w.norm()) / float((g + 0.1 * w).norm())
    _w, _buf, stats = lw.lars_step(w, g, zero, lr=0.1, adapt=False)
    assert stats[2] == 1.0


@pytest.mark.parametrize("nesterov", [False, True])
def test_lars_without_decay_is_invariant_under_a_rescaled_gradient(nesterov):
    w0 = _tensors(5)
    groups = [dict(params=[0, 1, 2, 3], lr=0.3, momentum=0.9, weight_decay=0.0, trust_coefficient=0.01, nesterov=nesterov)]
    a, b = lw.Driver("lars", w0, groups), lw.Driver("lars", w0, groups)
    for it in range(4):
        grads = _tensors(300 + it)
        a.step(grads)
        b.step([1000.0 * g for g in grads])
        for x, y in zip(a.w, b.w):
            assert _rel(x, y) < 1e-12


class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.proj = torch.nn.Linear(6, 4)
        self.norm = torch.nn.LayerNorm(4)
        self.head = torch.nn.Linear(4, 3, bias=False)
        self.table = torch.nn.Parameter(torch.zeros(2, 4))
        self.frozen = torch.nn.Parameter(torch.zeros(3, 3), requires_grad=False)


def test_adaptive_param_groups_split(bvc):
    m = _Small()
    named = dict(m.named_parameters())
    adapt, plain = bvc.optim.adaptive_param_groups(m, 0.05, no_adapt=("table",))
    assert (adapt["weight_decay"], adapt["adapt"], plain["weight_decay"], plain["adapt"]) == (0.05, True, 0.0, False)
    ids = lambda g: {id(p) for p in g["params"]}      # noqa: E731
    assert ids(adapt) == {id(named["proj.weight"]), id(named["head.weight"])}
    assert ids(plain) == {id(named[n]) for n in ("proj.bias", "norm.weight", "norm.bias", "table")}
    # both classes take the groups as they are; the remaining keys come from the constructor
    lars = bvc.optim.LARS([adapt, plain], lr=0.2, trust_coefficient=0.002)
    assert [(g["adapt"], g["weight_decay"], g["lr"], g["trust_coefficient"], g["momentum"]) for g in lars.param_groups] == \
        [(True, 0.05, 0.2, 0.002, 0.9), (False, 0.0, 0.2, 0.002, 0.9)]
    lamb = bvc.optim.LAMB(bvc.optim.adaptive_param_groups(m, 0.05))
    assert [(g["adapt"], g["weight_decay"], g["eps"], g["betas"]) for g in lamb.param_groups] == \
        [(True, 0.05, 1e-6, (0.9, 0.999)), (False, 0.0, 1e-6, (0.9, 0.999))]
    assert len(lamb.param_groups[0]["params"]) == 3          # without the name, the 2-D table is adapted


def test_layer_decay_groups_are_accepted_unchanged(bvc):
    kw = {k: v for k, v in vo.TINY.__dict__.items() if k != "decoder_norm_eps"}
    kw["num_hidden_layers"] = 3
    model = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(num_labels=5, **kw))
    groups = bvc.optim.layer_decay_param_groups(model, 1e-3, 0.05, 0.75)
    for cls, extra in ((bvc.optim.LARS, dict(lr=0.1)), (bvc.optim.LAMB, {})):
        opt = cls(groups, **extra)
        assert len(opt.param_groups) == len(groups) == 10
        for g, src in zip(opt.param_groups, groups):
            assert g["adapt"] is True and g["lr_scale"] == src["lr_scale"] and g["lr"] == src["lr"] and g["name"] == src["name"]
            assert g["weight_decay"] == (0.0 if g["name"].endswith("no_decay") else 0.05)
    with pytest.raises(ValueError):
        bvc.optim.LARS(groups, lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError):
        bvc.optim.LAMB(groups, betas=(1.0, 0.999))
