"""CPU checks of VideoMAEForVideoClassification fine-tuning: the path rule and transformers' problem_type inference as pure
functions, the new C-ABI symbols, and state-dict keys / shapes (unchanged by the fine-tuning path).  No GPU compute."""
import torch

import __graft_entry__ as ge
from oracle import videomae_oracle as vo

ge.build()
bvc = ge.load_package()
V = bvc.videomae


def test_path_rule():
    assert V.classification_path(True, True, True) == "train"
    for training, grad, trainable in [(False, True, True), (True, False, True), (True, True, False), (False, False, False),
                                      (False, True, False), (True, False, False), (False, False, True)]:
        assert V.classification_path(training, grad, trainable) == "encode"


def test_problem_type_inference_and_write_back():
    assert V.infer_problem_type(1, torch.zeros(2)) == "regression"
    assert V.infer_problem_type(1, torch.zeros(2, dtype=torch.long)) == "regression"
    assert V.infer_problem_type(10, torch.zeros(2, dtype=torch.long)) == "single_label_classification"
    assert V.infer_problem_type(10, torch.zeros(2, dtype=torch.int)) == "single_label_classification"
    assert V.infer_problem_type(10, torch.zeros(2, 10)) == "multi_label_classification"
    cfg = bvc.VideoMAEConfig(num_labels=3)
    logits = torch.randn(4, 3)
    y = torch.tensor([0, -100, 2, 1])
    loss = V.classification_loss(cfg, logits, y)
    assert cfg.problem_type == "single_label_classification"
    assert torch.equal(loss, torch.nn.functional.cross_entropy(logits[[0, 2, 3]], y[[0, 2, 3]]))
    cfg = bvc.VideoMAEConfig(num_labels=3, problem_type="multi_label_classification")      # an explicit type wins
    yl = torch.tensor([0, 1, 2, 1])
    t = torch.nn.functional.one_hot(yl, 3).float()
    assert torch.equal(V.classification_loss(cfg, logits, t), torch.nn.functional.binary_cross_entropy_with_logits(logits, t))
    cfg = bvc.VideoMAEConfig(num_labels=1)
    z, yr = torch.randn(4, 1), torch.randn(4)
    assert torch.equal(V.classification_loss(cfg, z, yr), torch.nn.functional.mse_loss(z.squeeze(), yr))
    assert cfg.problem_type == "regression"


def test_new_symbols_in_lib_table():
    for name in ("bvc_videomae_cls_create", "bvc_videomae_cls_destroy", "bvc_videomae_cls_forward_px", "bvc_videomae_cls_backward",
                 "bvc_videomae_cls_shadow", "bvc_videomae_encoder_fc_norm_backward"):
        assert name in bvc._lib.SYMBOLS
        assert getattr(bvc._lib.lib(), name) is not None


def test_state_dict_keys_and_shapes_unchanged():
    shapes = vo.param_shapes(vo.TINY)
    enc = {k: v for k, v in shapes.items() if k.startswith("videomae.")}
    kw = {k: v for k, v in vo.TINY.__dict__.items() if k != "decoder_norm_eps"}
    D = vo.TINY.hidden_size
    for nl in (0, 7):
        m = bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(num_labels=nl, **kw))
        sd = m.state_dict()
        want = dict(enc, **{"fc_norm.weight": (D,), "fc_norm.bias": (D,)})
        if nl:
            want.update({"classifier.weight": (nl, D), "classifier.bias": (nl,)})
        assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in want.items()}
        assert m._train.h is None
        m.train()
        import copy
        c = copy.deepcopy(m)                # the fine-tuning context is not shared by a copy
        assert c._train is not m._train and c._train.h is None
        assert set(c.state_dict()) == set(sd)
