"""CPU checks of the per-layer-output interface: the config fields and their defaults, the pre-training model's refusal, the size
formulas and the pre-allocation check, the new C-ABI symbols.  No GPU compute."""
import inspect

import pytest
import torch

import __graft_entry__ as ge
from oracle import videomae_oracle as vo

ge.build()
bvc = ge.load_package()
V = bvc.videomae
KW = {k: v for k, v in vo.TINY.__dict__.items() if k != "decoder_norm_eps"}


def test_config_fields_and_defaults():
    c = bvc.VideoMAEConfig()
    assert c.output_hidden_states is False and c.output_attentions is False
    c = bvc.VideoMAEConfig(output_hidden_states=True, output_attentions=1)
    assert c.output_hidden_states is True and c.output_attentions is True
    sig = inspect.signature(bvc.VideoMAEForVideoClassification.forward)
    assert sig.parameters["output_hidden_states"].default is None and sig.parameters["output_attentions"].default is None
    assert callable(bvc.attention_probs) and bvc.attention_probs is bvc._ops.attention_probs


def test_pretraining_model_refuses_truthy_flags_and_accepts_falsy_ones():
    m = bvc.VideoMAEForPreTraining(bvc.VideoMAEConfig(**KW))
    px = torch.zeros(1, vo.TINY.num_frames, 3, vo.TINY.image_size, vo.TINY.image_size)
    mask = torch.zeros(1, vo.TINY.seq_len, dtype=torch.bool)
    for name in ("output_hidden_states", "output_attentions"):
        with pytest.raises(NotImplementedError, match=r"tap\("):
            m(px, bool_masked_pos=mask, **{name: True})
        with pytest.raises(bvc._lib.BvcError):        # accepted: the call goes on to the (absent) GPU
            m(px, bool_masked_pos=mask, **{name: False})
    with pytest.raises(bvc._lib.BvcError):
        m(px, bool_masked_pos=mask, output_hidden_states=None, output_attentions=None)


def test_size_formulas():
    base = bvc.VideoMAEConfig()
    assert base.seq_length == 1568
    assert V.attentions_nbytes(base, 1) == 12 * 12 * 1568 * 1568 * 4 == 1_416_167_424
    assert V.attentions_nbytes(base, 37) // 12 > 2 ** 32        # 37 clips: ONE layer's slice is past 32-bit byte offsets
    assert V.hidden_states_nbytes(base, 1) == 13 * 1568 * 768 * 4
    tiny = bvc.VideoMAEConfig(**KW)
    assert V.attentions_nbytes(tiny, 2) == 2 * 2 * 2 * 32 * 32 * 4 and V.hidden_states_nbytes(tiny, 2) == 3 * 2 * 32 * 128 * 4


def test_allocation_shapes_and_the_memory_check(monkeypatch):
    tiny = bvc.VideoMAEConfig(**KW)
    need = V.attentions_nbytes(tiny, 3)
    monkeypatch.setattr(V, "free_device_memory", lambda device: need)
    hs, att = V.alloc_introspection(tiny, 3, "cpu", True, True)
    assert hs.shape == (3, 3, 32, 128) and att.shape == (2, 3, 2, 32, 32) and hs.dtype == att.dtype == torch.float32
    views = tuple(hs.unbind(0))
    assert len(views) == tiny.num_hidden_layers + 1 and all(v.shape == (3, 32, 128) for v in views)
    assert all(v.untyped_storage().data_ptr() == hs.untyped_storage().data_ptr() for v in views)      # views of ONE allocation
    assert len(att.unbind(0)) == tiny.num_hidden_layers and att.unbind(0)[1].shape == (3, 2, 32, 32)
    assert V.alloc_introspection(tiny, 3, "cpu", False, False) == (None, None)
    hs, att = V.alloc_introspection(tiny, 3, "cpu", True, False)
    assert att is None and hs is not None
    monkeypatch.setattr(V, "free_device_memory", lambda device: need - 1)
    with pytest.raises(ValueError, match=str(need)):
        V.alloc_introspection(tiny, 3, "cpu", False, True)
    hs, att = V.alloc_introspection(tiny, 3, "cpu", True, False)      # hidden states alone are not subject to the check
    assert hs is not None


def test_new_symbols_in_lib_table():
    for name in ("bvc_op_attention_probs", "bvc_videomae_encode_ex", "bvc_videomae_cls_introspect"):
        assert name in bvc._lib.SYMBOLS
        assert getattr(bvc._lib.lib(), name) is not None
    o = bvc._lib.introspect(None, None)
    assert o is None
    t = torch.zeros(4)
    o = bvc._lib.introspect(t, None)
    assert o.hidden_states == t.data_ptr() and not o.attentions


def test_op_rejects_bad_arguments_without_a_gpu():
    lib = bvc._lib.lib()
    assert lib.bvc_op_attention_probs(None, None, None, 1, 1, 1, 64, 0.0, None) != 0 and b"op_attention_probs" in lib.bvc_last_error()
    import ctypes
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    assert lib.bvc_op_attention_probs(p, p, p, 1, 1, 1, 48, 0.0, None) != 0 and b"head_dim 48" in lib.bvc_last_error()
    assert lib.bvc_op_attention_probs(p, p, p, 0, 1, 1, 64, 0.0, None) != 0 and b"empty shape" in lib.bvc_last_error()
    assert lib.bvc_op_attention_probs(p, p, p, 1, 1, 1, 64, -1.0, None) != 0
    # qkv of 4 GiB or more: the buffer descriptor cannot cover it
    assert lib.bvc_op_attention_probs(p, p, p, 4096, 1024, 3, 64, 0.0, None) != 0 and b"4 GiB" in lib.bvc_last_error()
    with pytest.raises(ValueError):
        bvc.attention_probs(torch.zeros(4, 6), torch.zeros(4), 1, 4, 1, 2)
