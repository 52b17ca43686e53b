"""output_hidden_states / output_attentions of VideoMAEForVideoClassification on the GPU, on its three paths (the no_grad encode,
the linear probe, the fine-tuning context).

References: tests/introspection_ref.py.  Bars:
  hidden_states[i]   against the float64 oracle ('embed' / 'enc<i>' of vo.encode): whole-tensor relative error < 2e-2, the
                     project's per-layer tap bar
  attentions[i]      with the upstream error factored out: against the float64 attention recomputed from the RETURNED
                     hidden_states[i] and the oracle's parameters, per row (attention_ref.row_err), <= ROW_BAR x the worst row of
                     the bf16 rounding model (layer_attention_bf16) on the same input; never above 2e-2
  the fixture        tests/golden/videomae_introspect_tiny.json (transformers, eager): hidden rows and norms < 2e-2; attention rows
                     <= ROW_BAR x the worst row of the end-to-end rounding model against the same fixture rows (the upstream
                     error cannot be factored out of a fixture), never above 2e-2
Every figure is printed and logged before anything is asserted.
"""
import dataclasses
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import attention_ref as R   # noqa: E402
from tests import gpu_util as G   # noqa: E402
from tests import introspection_ref as IR   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402
from tools.make_videomae_cls_golden import head_params   # noqa: E402

bvc = G.bvc
V = bvc.videomae
dev = torch.device("cuda:0")
NL = 10
ROW_BAR = 2.5
CAP = 2e-2
BATCH = 2

CONFIGS = {
    "tiny": (vo.TINY, 0),                                                              # N = 32, heads of 64
    "n144": (dataclasses.replace(vo.TINY, num_frames=8, image_size=96), 0),            # N = 144: ragged against 128
    # heads of 80: hidden sizes are multiples of 64 in this library, so the smallest such stack has four heads (320 wide)
    "d80": (dataclasses.replace(vo.TINY, hidden_size=320, num_attention_heads=4, intermediate_size=640), 0),       # in place
    "d80-pad": (dataclasses.replace(vo.TINY, hidden_size=320, num_attention_heads=4, intermediate_size=640), 1),   # zero-padded to 96
}


def _model(cfg, params, **extra):
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    m = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(num_labels=NL, **kw, **extra))
    sd = {k: v for k, v in params.items() if k.startswith("videomae.")}
    sd.update(dict(zip(("fc_norm.weight", "fc_norm.bias", "classifier.weight", "classifier.bias"), head_params(cfg.hidden_size, NL, 5))))
    m.load_state_dict(sd)
    return m.to(dev)


_REF = {}


def _reference(name):
    """(cfg, params, pixels, float64 hidden states) of one configuration, computed once and left unchanged."""
    if name not in _REF:
        cfg = CONFIGS[name][0]
        params = vo.make_params(cfg, seed=0)
        pixels, _ = vo.synthetic_batch(cfg, BATCH, 0)
        hs, _ = IR.encoder_states(cfg, params, pixels)
        _REF[name] = (cfg, params, pixels, hs)
    return _REF[name]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _shapes(cfg, out, B):
    L, H, N, D = cfg.num_hidden_layers, cfg.num_attention_heads, cfg.seq_len, cfg.hidden_size
    assert isinstance(out.hidden_states, tuple) and len(out.hidden_states) == L + 1
    assert isinstance(out.attentions, tuple) and len(out.attentions) == L
    for h in out.hidden_states:
        assert h.shape == (B, N, D) and h.dtype == torch.float32 and not h.requires_grad
    for a in out.attentions:
        assert a.shape == (B, H, N, N) and a.dtype == torch.float32 and not a.requires_grad
    # views of one allocation each
    assert len({h.untyped_storage().data_ptr() for h in out.hidden_states}) == 1
    assert len({a.untyped_storage().data_ptr() for a in out.attentions}) == 1


def _run_paths(m, px):
    """{path: (flags-on output, flags-off logits)} on the no_grad encode, the linear probe and the fine-tuning context."""
    on = dict(output_hidden_states=True, output_attentions=True, output_last_hidden_state=True)
    res = {}
    m.eval()
    with torch.no_grad():
        res["eval"] = (m(pixel_values=px, **on), m(pixel_values=px).logits)
    enc = [p for n, p in m.named_parameters() if n.startswith("videomae.")]
    for p in enc:
        p.requires_grad = False
    out = m(pixel_values=px, **on)                       # eval mode, grad mode on, fc_norm trainable: _FcNormProbe
    assert out.logits.requires_grad and m._train.h is None
    out.logits.sum().backward()
    assert m.fc_norm.weight.grad is not None
    res["probe"] = (out, m(pixel_values=px).logits.detach())
    for p in enc:
        p.requires_grad = True
    m.train()
    out = m(pixel_values=px, **on)                       # _ClsTrain
    assert m._train.h is not None and out.logits.requires_grad
    out.logits.sum().backward()                          # the backward still runs after the per-layer outputs were read
    assert all(p.grad is not None for p in enc)
    off = m(pixel_values=px)
    res["train"] = (out, off.logits.detach())
    assert off.hidden_states is None and off.attentions is None
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("name", list(CONFIGS))
def test_per_layer_outputs_on_every_path(name):
    cfg, params, pixels, ref_hs = _reference(name)
    old = bvc._lib.set_option("head_pad", CONFIGS[name][1])
    try:
        m = _model(cfg, params)
        res = _run_paths(m, pixels.to(dev))
    finally:
        bvc._lib.set_option("head_pad", old)
    L = cfg.num_hidden_layers
    ev = res["eval"][0]
    for path, (out, off_logits) in res.items():
        _shapes(cfg, out, BATCH)
        assert torch.equal(_bits(out.logits.detach()), _bits(off_logits)), f"{path}: logits change with the flags"
        assert torch.equal(_bits(out.hidden_states[-1]), _bits(out.last_hidden_state)), path
        for i in range(L + 1):
            assert torch.equal(_bits(out.hidden_states[i]), _bits(ev.hidden_states[i])), f"{path}: hidden_states[{i}] differs from eval's"
        for i in range(L):
            assert torch.equal(_bits(out.attentions[i]), _bits(ev.attentions[i])), f"{path}: attentions[{i}] differs from eval's"
    # accuracy, on the eval path's outputs (the other paths' are the same bits)
    fails = []
    hs = [h.cpu() for h in ev.hidden_states]
    for i in range(L + 1):
        e = G.rel_err(hs[i], ref_hs[i])
        G.log_parity(f"introspect {name}: hidden_states[{i}] rel err {e:.2e}")
        if not e < 2e-2:
            fails.append(f"hidden_states[{i}]: {e:.3e}")
    for i in range(L):
        got = ev.attentions[i].cpu()
        ref = IR.layer_attention(cfg, params, i, hs[i])
        mod = IR.layer_attention_bf16(cfg, params, i, hs[i])
        k_row, at = R.row_err(got, ref)
        m_row, _ = R.row_err(mod, ref)
        rowsum = float((got.double().sum(-1) - 1).abs().max())
        G.log_parity(f"introspect {name}: attentions[{i}] row {k_row:.2e} / model {m_row:.2e} = {k_row / m_row:.2f} at {at}; "
                     f"|rowsum - 1| {rowsum:.1e}")
        if not (k_row <= ROW_BAR * m_row and k_row <= CAP):
            fails.append(f"attentions[{i}]: worst row {k_row:.3e} at {at}, {k_row / m_row:.2f} x the model's {m_row:.3e}")
        if not rowsum <= 1e-4:
            fails.append(f"attentions[{i}]: |rowsum - 1| = {rowsum:.3e}")
    assert not fails, (name, fails)


def test_tiny_against_the_transformers_fixture(golden_dir):
    fx = json.load(open(os.path.join(golden_dir, IR.FIXTURE)))
    cfg, params, pixels, _ = _reference("tiny")
    assert fx["config"] == cfg.__dict__ and fx["batch"] == BATCH and fx["seed"] == 0 and fx["weight_seed"] == 0
    m = _model(cfg, params).eval()
    with torch.no_grad():
        out = m(pixel_values=pixels.to(dev), output_hidden_states=True, output_attentions=True)
    got = IR.fixture_view([h.cpu() for h in out.hidden_states], [a.cpu() for a in out.attentions])
    mod = IR.fixture_view(*IR.encoder_states_bf16(cfg, params, pixels))
    t = lambda v: torch.tensor(v, dtype=torch.float64)      # noqa: E731
    fails = []
    for i in range(cfg.num_hidden_layers + 1):
        e = G.rel_err(t(got["hidden_rows"][i]), t(fx["hidden_rows"][i]))
        en = abs(got["hidden_norm"][i] - fx["hidden_norm"][i]) / fx["hidden_norm"][i]
        G.log_parity(f"introspect fixture: hidden rows[{i}] rel err {e:.2e}, norm {en:.2e}")
        if not (e < 2e-2 and en < 2e-2):
            fails.append(f"hidden[{i}]: rows {e:.3e}, norm {en:.3e}")
    for i in range(cfg.num_hidden_layers):
        k_row, at = R.row_err(t(got["attention_rows"][i]), t(fx["attention_rows"][i]))
        m_row, _ = R.row_err(t(mod["attention_rows"][i]), t(fx["attention_rows"][i]))
        en = float(((t(got["attention_norm"][i]) - t(fx["attention_norm"][i])).abs() / t(fx["attention_norm"][i])).max())
        G.log_parity(f"introspect fixture: attention rows[{i}] row {k_row:.2e} / model {m_row:.2e} = {k_row / m_row:.2f} at {at}; norm {en:.2e}")
        if not (k_row <= ROW_BAR * m_row and k_row <= CAP and en < CAP):
            fails.append(f"attention[{i}]: worst row {k_row:.3e}, {k_row / m_row:.2f} x the model's {m_row:.3e}; norm {en:.3e}")
    assert not fails, fails


def test_config_defaults_turn_the_outputs_on():
    cfg, params, pixels, _ = _reference("tiny")
    m = _model(cfg, params, output_hidden_states=True).eval()
    with torch.no_grad():
        out = m(pixel_values=pixels.to(dev))
        assert len(out.hidden_states) == cfg.num_hidden_layers + 1 and out.attentions is None and out.last_hidden_state is None
        out = m(pixel_values=pixels.to(dev), output_hidden_states=False, output_attentions=True)
        assert out.hidden_states is None and len(out.attentions) == cfg.num_hidden_layers


def test_through_distributed_data_parallel(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setenv("BVC_COMM", "torch")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29547"
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        cfg, params, pixels, _ = _reference("tiny")
        m = _model(cfg, params).train()
        w = bvc.DistributedDataParallel(m, device_ids=[0], output_device=0)
        out = w(pixel_values=pixels.to(dev), output_hidden_states=True, output_attentions=True)
        _shapes(cfg, out, BATCH)
        out.logits.sum().backward()
        plain = m(pixel_values=pixels.to(dev), output_hidden_states=True, output_attentions=True)
        assert torch.equal(_bits(plain.hidden_states[-1]), _bits(out.hidden_states[-1]))
        assert torch.equal(_bits(plain.attentions[0]), _bits(out.attentions[0]))
        plain.logits.sum().backward()
        torch.cuda.synchronize()
    finally:
        bvc.comm.reset()
        dist.destroy_process_group()


def test_hidden_states_include_the_drop_path_gates():
    """Train mode with drop_path_rate = 0.5 (rates linspace(0, 0.5, depth): layer 0 never drops, so the stack is four layers deep):
    the hidden states are those of the forward that ran.  One seed gives the same bits twice; a clip both of whose branches a
    layer dropped (model.drop_path_scale) leaves that layer unchanged, bitwise; a clip that kept a branch does not."""
    cfg = dataclasses.replace(vo.TINY, num_hidden_layers=4)
    params = vo.make_params(cfg, seed=0)
    B = 8
    px = vo.synthetic_batch(cfg, B, 1)[0].to(dev)
    m = _model(cfg, params, drop_path_rate=0.5).train()
    found = 0
    for seed in range(6):
        runs = []
        for _ in range(2):
            torch.manual_seed(seed)
            out = m(pixel_values=px, output_hidden_states=True)
            runs.append(([h.clone() for h in out.hidden_states], m.drop_path_scale.clone()))
        (hs, scale), (hs2, scale2) = runs
        assert torch.equal(scale, scale2)
        for a, b in zip(hs, hs2):
            assert torch.equal(_bits(a), _bits(b)), "hidden states differ between two runs under one seed"
        assert scale.shape == (cfg.num_hidden_layers, 2, B)
        for i in range(cfg.num_hidden_layers):
            for b in range(B):
                same = torch.equal(_bits(hs[i + 1][b]), _bits(hs[i][b]))
                dropped = float(scale[i, 0, b]) == 0.0 and float(scale[i, 1, b]) == 0.0
                assert same == dropped, (seed, i, b, same, dropped)
                found += dropped
        if found:
            break
    assert found, "no clip had both branches of a layer dropped in six seeds"
    # the eval-mode forward of the same module is ungated
    m.eval()
    with torch.no_grad():
        ev = m(pixel_values=px, output_hidden_states=True).hidden_states
    ref, _ = IR.encoder_states(cfg, params, px.cpu())
    assert G.rel_err(ev[-1].cpu(), ref[-1]) < 2e-2


def test_errors(monkeypatch):
    cfg, params, pixels, _ = _reference("tiny")
    m = _model(cfg, params).eval()
    need = V.attentions_nbytes(m.config, BATCH)
    monkeypatch.setattr(V, "free_device_memory", lambda device: need - 1)      # nothing is allocated: the check comes first
    with torch.no_grad():
        with pytest.raises(ValueError, match=str(need)):
            m(pixel_values=pixels.to(dev), output_attentions=True)
        out = m(pixel_values=pixels.to(dev), output_hidden_states=True)      # hidden states are not subject to it
        assert len(out.hidden_states) == cfg.num_hidden_layers + 1
    m.train()
    with pytest.raises(ValueError, match=str(need)):
        m(pixel_values=pixels.to(dev), output_attentions=True)
    monkeypatch.undo()
    assert V.free_device_memory(dev) > need
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    pre = bvc.VideoMAEForPreTraining(bvc.VideoMAEConfig(**kw)).to(dev)
    mask = vo.synthetic_batch(cfg, BATCH, 0)[1].to(dev)
    for flag in ("output_hidden_states", "output_attentions"):
        with pytest.raises(NotImplementedError, match=r"tap\("):
            pre(pixels.to(dev), bool_masked_pos=mask, **{flag: True})
    assert pre(pixels.to(dev), bool_masked_pos=mask, output_hidden_states=False, output_attentions=False).loss is not None
    # the C entry point outside its window: no forward has run on a fresh fine-tuning context
    import ctypes
    h = ctypes.c_void_p()
    cc = m.config.to_c()
    bvc._lib.check(bvc._lib.lib().bvc_videomae_cls_create(ctypes.byref(cc), 1, ctypes.byref(h)), "cls_create")
    try:
        buf = torch.empty(16, device=dev)
        o = bvc._lib.introspect(buf, None)
        assert bvc._lib.lib().bvc_videomae_cls_introspect(h, ctypes.byref(o), G.stream()) == -3      # BVC_ERR_STATE
        assert b"cls_introspect" in bvc._lib.lib().bvc_last_error()
    finally:
        bvc._lib.lib().bvc_videomae_cls_destroy(h)
