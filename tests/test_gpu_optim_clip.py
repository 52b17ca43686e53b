"""Gradient-norm clipping inside the fused optimisers (bvc.optim.SGD / Adam / AdamW(max_grad_norm=...)), against
``torch.nn.utils.clip_grad_norm_`` followed by the unclipped ``torch.optim`` step on clones, on a tiny flat classification model:

  four_groups   encoder / head x decay / no decay: the by-value entry points
  layer_decay   layer-wise learning-rate decay, 12 groups: the device-table entry points
  frozen_layer  four groups with encoder layer 1 frozen: its stretch of the flat gradient buffer belongs to nobody

``fc_norm`` and the classifier live outside the flat buffer in all of them (loose runs).  Five gradient sets are taken once from real
backward passes of the model (each at its own magnitude, so that the clip is active on some steps and inactive on others), and every
run - the torch twin and each route through the library - is fed the same sets; the twin's runs are computed once per case and
shared.  RTOL / ATOL are the project's bars for an optimiser step against torch; the bar on the norm is the derived one of
test_gpu_grad_norm.py: (S + ceil(log2(n / S)) + 2) 2^-24 on the sum of squares, half of it on the norm."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_util as G   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402

bvc = G.bvc
dev = torch.device("cuda:0")
RTOL, ATOL = 2e-6, 2e-7                       # the project's bars for an optimiser step against torch (test_gpu_ops.py)
LAYERS, STEPS = 4, 5
FACTORS = (1.0, 0.3, 2.5, 0.6, 1.7)          # the magnitude of each gradient set
SCALE = 65536.0
FROZEN_PREFIX = "videomae.encoder.layer.1."
NEW_FNS = ("bvc_op_grad_sqnorm_items", "bvc_op_clip_finalize", "bvc_op_scale_by_dev")


def _norm_bar(n):
    chain = bvc._lib.lib().bvc_op_grad_norm_chain()
    return 0.5 * (chain + max(0, math.ceil(math.log2(max(n, 1) / chain))) + 2) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------- model, groups, gradient sets
def _model(frozen=False):
    """(the helper of test_gpu_optim_groups.py::test_classification_model_under_layer_decay)"""
    cfg = vo.TINY
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    kw["num_hidden_layers"] = LAYERS
    torch.manual_seed(0)
    model = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(num_labels=10, **kw)).to(dev).train()
    if frozen:
        for n, p in model.named_parameters():
            if n.startswith(FROZEN_PREFIX):
                p.requires_grad_(False)
    return model


def _batch(seed):
    return vo.synthetic_batch(vo.TINY, 2, seed, 0.9)[0].to(dev), torch.tensor([seed, 7 - seed], device=dev)


_SETS = []


def _gradient_sets():
    """STEPS gradient sets {name: f32 tensor} from real backward passes (one batch each), scaled by FACTORS; computed once."""
    if not _SETS:
        model = _model()
        for s in range(STEPS):
            model.zero_grad()
            px, y = _batch(s)
            model(pixel_values=px, labels=y).loss.backward()
            _SETS.append({n: p.grad.detach().clone() * FACTORS[s] for n, p in model.named_parameters() if p.grad is not None})
        torch.cuda.synchronize()
    return _SETS


def _groups(config, model, adam):
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    if config == "layer_decay":
        groups = bvc.optim.layer_decay_param_groups(model, 1e-3 if adam else 0.05, 0.05, 0.75)
        assert len(groups) >= 12 > bvc._lib.OPT_MAX_GROUPS
        return groups
    out = []
    for i, (head, plain) in enumerate(((False, False), (False, True), (True, False), (True, True))):
        ps = [p for n, p in named if (not n.startswith("videomae.")) == head and (p.ndim == 1) == plain]
        assert ps
        hyper = dict(lr=1e-3 * (1 + 0.4 * i), weight_decay=0.0 if plain else 0.05, betas=(0.9 - 0.02 * i, 0.95)) if adam else \
            dict(lr=0.05 * (1 + 0.3 * i), weight_decay=0.0 if plain else 0.01, momentum=0.9 - 0.05 * i)
        out.append(dict(params=ps, **hyper))
    return out


def _make(adam, groups, bvc_side, **kw):
    if adam:
        return bvc.optim.AdamW(groups, lr=1e-3, **kw) if bvc_side else torch.optim.AdamW(groups, lr=1e-3, foreach=False)
    if bvc_side:
        return bvc.optim.SGD(groups, lr=0.05, momentum=0.9, nesterov=True, **kw)
    return torch.optim.SGD(groups, lr=0.05, momentum=0.9, nesterov=True, foreach=False)


class _Case:
    """A fresh model with its optimiser-ready gradients (one real forward / backward: the gradient views and the bf16 shadow exist)."""

    def __init__(self, config, adam):
        self.config, self.adam = config, adam
        self.model = _model(frozen=config == "frozen_layer")
        px, y = _batch(0)
        self.model(pixel_values=px, labels=y).loss.backward()
        self.named = dict(self.model.named_parameters())
        self.live = {n: p for n, p in self.named.items() if p.grad is not None}
        assert (config == "frozen_layer") == any(n.startswith(FROZEN_PREFIX) and n not in self.live for n in self.named)
        for n, p in self.live.items():                      # gradients of the loose parameters: tensors of their own that stay put
            if not n.startswith("videomae."):
                p.grad = p.grad.detach().clone()
        self.n_live = sum(p.numel() for p in self.live.values())

    def feed(self, k, scale=1.0):
        for n, p in self.live.items():
            p.grad.copy_(_gradient_sets()[k][n] * scale)

    def optimiser(self, **kw):
        return _make(self.adam, _groups(self.config, self.model, self.adam), True, **kw)

    def shadow_matches_a_fresh_cast(self):
        m = self.model
        ptr = m._shadow_base()
        assert ptr is not None                              # the fused steps kept the copy current
        n = m._numel

        class _Dev:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<i2", "data": (ptr, False), "version": 2}
        shadow = torch.as_tensor(_Dev(), device=dev)
        return torch.equal(shadow, m._flat.to(torch.bfloat16).view(torch.int16))

    def flat_offset(self, name):
        return (self.named[name].data_ptr() - self.model._flat.data_ptr()) // 4


_TWINS = {}


def _twin(config, adam, max_norm, seq=tuple(range(STEPS))):
    """torch.optim (foreach=False) with torch's clip_grad_norm_ on clones, fed the gradient sets `seq`: per step the f64 norm of the
    unclipped gradients, torch's own f32 norm, the clipped gradients and the parameters after the step.  Computed once per case."""
    key = (config, adam, max_norm, seq)
    if key not in _TWINS:
        case = _Case(config, adam)
        twins = {n: torch.nn.Parameter(p.detach().clone()) for n, p in case.live.items()}
        name_of = {id(p): n for n, p in case.named.items()}
        groups = [dict({k: v for k, v in g.items() if k != "params"}, params=[twins[name_of[id(p)]] for p in g["params"]])
                  for g in _groups(config, case.model, adam)]
        opt = _make(adam, groups, False)
        record = []
        for k in seq:
            for n, t in twins.items():
                t.grad = _gradient_sets()[k][n].clone()
            norm64 = math.sqrt(sum(float(t.grad.double().square().sum()) for t in twins.values()))
            norm32 = float(torch.nn.utils.clip_grad_norm_(list(twins.values()), max_norm if max_norm is not None else float("inf"), foreach=False))
            opt.step()
            record.append(dict(norm64=norm64, norm32=norm32, grads={n: t.grad.clone() for n, t in twins.items()},
                               params={n: t.detach().clone() for n, t in twins.items()}))
        torch.cuda.synchronize()
        _TWINS[key] = record
    return _TWINS[key]


def _threshold(config, adam):
    """max_norm strictly between the smallest and the largest norm the twin sees: active on some steps, inactive on others."""
    norms = sorted(r["norm64"] for r in _twin(config, adam, None))
    max_norm = math.sqrt(norms[1] * norms[-2])
    assert norms[0] < max_norm < norms[-1]
    assert any(n > max_norm for n in norms) and any(n < max_norm for n in norms)
    return max_norm


def _compare(case, opt, want, what, max_norm=None, grads=True):
    torch.cuda.synchronize()
    for n, p in case.live.items():
        torch.testing.assert_close(p.data, want["params"][n], rtol=RTOL, atol=ATOL, msg=lambda s, n=n: f"{what} parameter {n}: {s}")
        if grads:
            torch.testing.assert_close(p.grad, want["grads"][n], rtol=RTOL, atol=ATOL, msg=lambda s, n=n: f"{what} gradient {n}: {s}")
    if max_norm is not None:
        got, ref = float(opt.grad_norm), want["norm64"]
        rel = abs(got - ref) / ref
        print(f"{what}: grad_norm {got:.9g} f64 {ref:.9g} rel {rel:.2e} bar {_norm_bar(case.n_live):.2e} torch {want['norm32']:.9g}")
        assert rel <= _norm_bar(case.n_live), f"{what}: grad_norm {got} vs {ref} (rel {rel:.3e})"
        assert abs(want["norm32"] - ref) / ref < 1e-5
        coef = float(opt.clip_coef)
        assert abs(coef - min(1.0, max_norm / (ref + 1e-6))) <= 1e-6
        assert coef == 1.0 if ref < max_norm * (1 - 1e-5) else coef < 1.0
    assert case.shadow_matches_a_fresh_cast(), f"{what}: the bf16 shadow is not the cast of the parameters"


class _Calls:
    """Counts calls of library entry points by wrapping ``_lib.lib()``'s functions (the pattern of test_gpu_optim_groups.py)."""

    def __init__(self, names):
        self.names, self.n, self.args = list(names), {k: 0 for k in names}, {k: [] for k in names}

    def __enter__(self):
        lib = bvc._lib.lib()
        self.saved = {k: getattr(lib, k) for k in self.names}
        for k, fn in self.saved.items():
            def wrapper(*a, _k=k, _fn=fn):
                self.n[_k] += 1
                self.args[_k].append(a[0] if a else None)
                return _fn(*a)
            setattr(lib, k, wrapper)
        return self

    def __exit__(self, *exc):
        lib = bvc._lib.lib()
        for k, fn in self.saved.items():
            setattr(lib, k, fn)


def _loose_runs(opt):
    _plans, loose = opt._get_plans()
    return sum(len(opt._group_runs(gi, ps)) for gi, ps in loose.items())


CONFIGS = ["four_groups", "layer_decay", "frozen_layer"]
KINDS = [pytest.param(True, id="adamw"), pytest.param(False, id="sgd_nesterov")]


# ---------------------------------------------------------------------------------------------- 1. parity without a scaler
@pytest.mark.parametrize("adam", KINDS)
@pytest.mark.parametrize("config", CONFIGS)
def test_fused_clip_matches_torch_clip_then_step(config, adam):
    max_norm = _threshold(config, adam)
    twin = _twin(config, adam, max_norm)
    case = _Case(config, adam)
    opt = case.optimiser(max_grad_norm=max_norm)
    coefs = []
    with _Calls(NEW_FNS + ("bvc_op_nonfinite_check",)) as calls:
        for k in range(STEPS):
            case.feed(k)
            opt.step()
            _compare(case, opt, twin[k], f"{config} step {k}", max_norm)
            coefs.append(float(opt.clip_coef))
    assert any(c == 1.0 for c in coefs) and any(c < 1.0 for c in coefs), coefs      # the clip was active on some steps, inactive on others
    plans, _ = opt._get_plans()
    assert len(plans) == 1 and plans[0].table == (config == "layer_decay") and plans[0].norm is not None
    assert (-1 in plans[0].groups) == (config == "frozen_layer")
    runs = _loose_runs(opt)
    assert runs >= 1
    assert calls.n == {"bvc_op_grad_sqnorm_items": STEPS * (1 + runs), "bvc_op_clip_finalize": STEPS, "bvc_op_scale_by_dev": 0,
                       "bvc_op_nonfinite_check": 0}, calls.n


# ---------------------------------------------------------------------------------------------- 2. bvc.amp.GradScaler
@pytest.mark.parametrize("adam", KINDS)
@pytest.mark.parametrize("config", CONFIGS)
def test_fused_clip_under_bvc_gradscaler(config, adam):
    """Scale 65536: inf check and norm are ONE read per flat buffer and step.  Step 2 carries an Inf in an owned gradient element: it is
    skipped, parameters and optimiser state stay bit for bit, the scale is halved.  In frozen_layer step 3 carries an Inf in the
    frozen layer's stretch of the flat gradient buffer, which belongs to nobody: that step is NOT skipped."""
    max_norm = _threshold(config, adam)
    seq = (0, 1, 3, 4)
    twin = _twin(config, adam, max_norm, seq)
    case = _Case(config, adam)
    opt = case.optimiser(max_grad_norm=max_norm)
    scaler = bvc.amp.GradScaler("cuda", init_scale=SCALE, growth_interval=1000)
    scaler.scale(torch.zeros((), device=dev))                         # GradScaler creates its device-side scale lazily
    flat_grad = case.model._flat_grad
    lo, hi = flat_grad.data_ptr(), flat_grad.data_ptr() + 4 * flat_grad.numel()
    done = 0
    with _Calls(NEW_FNS + ("bvc_op_nonfinite_check",)) as calls:
        for k in range(STEPS):
            case.feed(k, scale=scaler.get_scale())
            if k == 2:
                victim = "videomae.encoder.layer.2.intermediate.dense.weight"
                assert victim in case.live
                case.live[victim].grad.view(-1)[12345] = float("inf")
                plans, _ = opt._get_plans()
                before = [case.model._flat.clone()] + [p.detach().clone() for n, p in case.live.items() if not n.startswith("videomae.")]
                state = [t.clone() for t in plans[0].state if torch.is_tensor(t)] if plans[0].state is not None else []
            if k == 3 and config == "frozen_layer":
                at = case.flat_offset(FROZEN_PREFIX + "output.dense.weight") + 77
                flat_grad[at] = float("inf")
            scaler.step(opt)
            scaler.update()
            torch.cuda.synchronize()
            if k == 2:
                after = [case.model._flat] + [p.detach() for n, p in case.live.items() if not n.startswith("videomae.")]
                assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, after))
                now = [t for t in plans[0].state if torch.is_tensor(t)]
                assert len(now) == len(state) and all(torch.equal(a, b) for a, b in zip(state, now))
                assert scaler.get_scale() == SCALE / 2
                assert not math.isfinite(float(opt.grad_norm))          # grad_norm reports the nonfinite value of the skipped step
                continue
            # (a skipped step leaves the scaled gradients as they are; every other step leaves them unscaled and clipped)
            _compare(case, opt, twin[done], f"{config} scaled step {k}", max_norm)
            done += 1
    assert done == len(seq) and scaler.get_scale() == SCALE / 2
    runs = _loose_runs(opt)
    in_flat = sum(1 for a in calls.args["bvc_op_grad_sqnorm_items"] if lo <= int(a) < hi)
    assert in_flat == STEPS                                                           # one read of the flat gradient buffer per step
    assert calls.n == {"bvc_op_grad_sqnorm_items": STEPS * (1 + runs), "bvc_op_clip_finalize": STEPS, "bvc_op_scale_by_dev": 0,
                       "bvc_op_nonfinite_check": 0}, calls.n


# ---------------------------------------------------------------------------------------------- 3. the other scaler routes
@pytest.mark.parametrize("route", ["torch_scaler", "unscale_first"])
@pytest.mark.parametrize("adam", KINDS)
def test_fused_clip_on_the_other_scaler_routes(adam, route):
    """torch's own GradScaler (its stock inf check, then the step takes the norms itself), and scaler.unscale_(opt) before
    scaler.step(opt) (torch hands grad_scale=None: the step sees unscaled gradients)."""
    config = "layer_decay"
    max_norm = _threshold(config, adam)
    twin = _twin(config, adam, max_norm)
    case = _Case(config, adam)
    opt = case.optimiser(max_grad_norm=max_norm)
    scaler = (torch.amp.GradScaler if route == "torch_scaler" else bvc.amp.GradScaler)("cuda", init_scale=SCALE, growth_interval=1000)
    scaler.scale(torch.zeros((), device=dev))
    with _Calls(NEW_FNS) as calls:
        for k in range(STEPS):
            case.feed(k, scale=SCALE)
            if route == "unscale_first":
                scaler.unscale_(opt)
            scaler.step(opt)
            scaler.update()
            _compare(case, opt, twin[k], f"{route} step {k}", max_norm)
    assert calls.n["bvc_op_grad_sqnorm_items"] == STEPS * (1 + _loose_runs(opt)) and calls.n["bvc_op_clip_finalize"] == STEPS


# ---------------------------------------------------------------------------------------------- 4. the immediate form
def test_immediate_clip_then_unclipped_step_equals_the_fused_form():
    config, adam = "four_groups", True
    max_norm = _threshold(config, adam)
    twin = _twin(config, adam, max_norm)
    fused, plain = _Case(config, adam), _Case(config, adam)
    fopt, popt = fused.optimiser(max_grad_norm=max_norm), plain.optimiser()
    with _Calls(NEW_FNS) as calls:
        for k in range(STEPS):
            fused.feed(k)
            plain.feed(k)
            fopt.step()
            norm = bvc.optim.clip_grad_norm_(plain.model.parameters(), max_norm)
            assert norm.ndim == 0 and norm.is_cuda
            clipped = {n: p.grad.clone() for n, p in plain.live.items()}
            popt.step()
            torch.cuda.synchronize()
            ref = twin[k]
            assert abs(float(norm) - ref["norm64"]) / ref["norm64"] <= _norm_bar(plain.n_live)
            assert abs(float(norm) - ref["norm32"]) / ref["norm32"] <= 2 * _norm_bar(plain.n_live)      # torch's function, itself f32
            for n, p in plain.live.items():
                torch.testing.assert_close(clipped[n], ref["grads"][n], rtol=RTOL, atol=ATOL)
                torch.testing.assert_close(p.data, fused.live[n].data, rtol=RTOL, atol=ATOL)
            _compare(plain, popt, ref, f"immediate step {k}")
    # per step: the fused form takes its norms and one finalize; the immediate form a norm, one finalize and one scaling per run of
    # adjacent tensors (the whole flat module is one run)
    runs = len(bvc.optim.SGD._contiguous_runs(list(plain.live.values())))
    assert 2 <= runs <= 5
    assert calls.n == {"bvc_op_grad_sqnorm_items": STEPS * (1 + _loose_runs(fopt) + runs), "bvc_op_clip_finalize": 2 * STEPS,
                       "bvc_op_scale_by_dev": STEPS * runs}, calls.n
    with pytest.raises(RuntimeError, match="non-finite"):
        plain.feed(0)
        plain.live["classifier.weight"].grad[0, 0] = float("nan")
        bvc.optim.clip_grad_norm_(plain.model.parameters(), max_norm, error_if_nonfinite=True)


# ---------------------------------------------------------------------------------------------- 5. per-parameter norms
@pytest.mark.parametrize("config", ["four_groups", "frozen_layer"])
def test_per_parameter_gradient_norms(config):
    case = _Case(config, True)
    case.feed(2)
    with _Calls(NEW_FNS) as calls:
        norms = bvc.optim.grad_norms(case.model)
        again = bvc.optim.grad_norms(case.model)
    torch.cuda.synchronize()
    assert calls.n == {"bvc_op_grad_sqnorm_items": 2, "bvc_op_clip_finalize": 0, "bvc_op_scale_by_dev": 0}      # one launch pair per call
    assert set(norms) == set(case.live) | {"total"} and all(v.ndim == 0 and v.is_cuda for v in norms.values())
    assert all(torch.equal(norms[k], again[k]) for k in norms)
    total = 0.0
    for n, p in case.live.items():
        ref = float(p.grad.double().norm())
        total += ref * ref
        if ref == 0.0:
            assert float(norms[n]) == 0.0, n
        else:
            assert abs(float(norms[n]) - ref) / ref <= _norm_bar(p.numel()), (n, float(norms[n]), ref)
    total = math.sqrt(total)
    assert abs(float(norms["total"]) - total) / total <= _norm_bar(case.n_live)


# ---------------------------------------------------------------------------------------------- 6. no clipping requested
@pytest.mark.parametrize("adam", KINDS)
def test_without_max_grad_norm_a_step_makes_the_calls_it_made_before(adam):
    """Every bvc_op_* entry point is wrapped: with max_grad_norm=None a step under bvc.amp.GradScaler calls exactly what it called
    before clipping existed - one inf check per range, one by-value step per flat buffer, the per-run calls - and no new entry point."""
    case = _Case("four_groups", adam)
    opt = case.optimiser()
    assert opt.max_grad_norm is None
    scaler = bvc.amp.GradScaler("cuda", init_scale=SCALE, growth_interval=1000)
    scaler.scale(torch.zeros((), device=dev))
    names = [k for k in bvc._lib.SYMBOLS if k.startswith("bvc_op_")]
    steps = 2
    with _Calls(names) as calls:
        for k in range(steps):
            case.feed(k, scale=SCALE)
            scaler.step(opt)
            scaler.update()
    torch.cuda.synchronize()
    runs = _loose_runs(opt)
    if adam:
        want = {"bvc_op_nonfinite_check": 1 + runs, "bvc_op_adam_step_segments": 1, "bvc_op_adam_prepare": runs, "bvc_op_adam_step": runs}
    else:
        want = {"bvc_op_nonfinite_check": 1 + runs, "bvc_op_sgd_step_segments": 1, "bvc_op_sgd_step": runs}
    assert {k: v for k, v in calls.n.items() if v} == {k: steps * v for k, v in want.items()}, {k: v for k, v in calls.n.items() if v}
    assert opt._clip is None and opt._get_plans()[0][0].norm is None
