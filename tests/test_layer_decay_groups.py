"""Layer-wise learning-rate decay on the host, WITHOUT a GPU: the grouping helper (bvc_amd/optim.py ``layer_decay_param_groups`` /
``set_base_lr``) on a classification model and a JEPA encoder, and the plan that carries more than ``OPT_MAX_GROUPS`` parameter
groups through one launch per flat module (``_build_table_plans``)."""
import re
import types

import pytest
import torch

from oracle import videomae_oracle as vo

L = 3           # encoder layers of both models: the smallest configurations, three layers
LR, WD, DECAY = 1e-3, 0.05, 0.75


def _cls_model(bvc, num_labels=5):
    kw = {k: v for k, v in vo.TINY.__dict__.items() if k != "decoder_norm_eps"}
    kw["num_hidden_layers"] = L
    return bvc.VideoMAEForVideoClassification(bvc.VideoMAEConfig(num_labels=num_labels, **kw))


def _jepa_encoder(bvc):
    return bvc.jepa.VisionTransformer(img_size=[64], patch_size=16, num_frames=2, tubelet_size=1, embed_dim=128, depth=L, num_heads=2)


def _cls_id(name):
    if name.startswith("videomae.embeddings."):
        return 0
    hit = re.match(r"videomae\.encoder\.layer\.(\d+)\.", name)
    return int(hit.group(1)) + 1 if hit else L + 1


def _jepa_id(name):
    if name == "pos_embed" or name.startswith("patch_embed."):
        return 0
    hit = re.match(r"blocks\.(\d+)\.", name)
    if hit:
        return int(hit.group(1)) + 1
    assert name.startswith("norm."), name
    return L + 1


def _check_groups(model, groups, layer_id, no_weight_decay=()):
    named = dict(model.named_parameters())
    name_of = {id(p): n for n, p in named.items()}
    trainable = {n for n, p in named.items() if p.requires_grad}
    seen = []
    for g in groups:
        assert set(g) == {"name", "lr_scale", "lr", "weight_decay", "params"} and g["params"]
        k, half = re.fullmatch(r"layer_(\d+)_(decay|no_decay)", g["name"]).groups()
        k = int(k)
        assert g["lr_scale"] == pytest.approx(DECAY ** (L + 1 - k), rel=1e-12) and g["lr"] == pytest.approx(LR * g["lr_scale"], rel=1e-12)
        assert g["weight_decay"] == (WD if half == "decay" else 0.0)
        for p in g["params"]:
            n = name_of[id(p)]
            seen.append(n)
            assert layer_id(n) == k, n
            plain = p.ndim == 1 or n.endswith(".bias") or n in no_weight_decay
            assert plain == (half == "no_decay"), n
    assert sorted(seen) == sorted(trainable)                        # every trainable parameter in exactly one group
    expected = {(layer_id(n), named[n].ndim == 1 or n.endswith(".bias") or n in no_weight_decay) for n in trainable}
    assert len(groups) == len(expected) <= 2 * (L + 2)              # 2 (L + 2) minus the halves that would be empty
    assert len({g["name"] for g in groups}) == len(groups)
    return expected


def test_classification_model_groups(bvc):
    m = _cls_model(bvc)
    groups = bvc.optim.layer_decay_param_groups(m, LR, WD, DECAY)
    expected = _check_groups(m, groups, _cls_id)
    # fc_norm and the classifier: the head, at the full rate; the embeddings at decay^(L + 1)
    by_name = {g["name"]: g for g in groups}
    assert by_name[f"layer_{L + 1}_decay"]["lr"] == LR and by_name["layer_0_decay"]["lr_scale"] == pytest.approx(DECAY ** (L + 1))
    head = {id(p) for g in groups if g["name"].startswith(f"layer_{L + 1}_") for p in g["params"]}
    assert {id(p) for p in list(m.fc_norm.parameters()) + list(m.classifier.parameters())} <= head
    assert len(expected) == 2 * (L + 2)                             # every layer has matrices and biases here
    torch.optim.AdamW(groups)                                       # the dicts are what torch's optimisers take
    assert len(bvc.optim.AdamW(groups).param_groups) == len(groups)


def test_no_weight_decay_names_and_frozen_parameters(bvc):
    m = _cls_model(bvc)
    skip = ("videomae.embeddings.patch_embeddings.projection.weight",)
    frozen = "videomae.encoder.layer.1.attention.attention.query.weight"
    dict(m.named_parameters())[frozen].requires_grad_(False)
    groups = bvc.optim.layer_decay_param_groups(m, LR, WD, DECAY, no_weight_decay=skip)
    _check_groups(m, groups, _cls_id, no_weight_decay=skip)
    assert "layer_0_decay" not in {g["name"] for g in groups}       # its only matrix moved to the no-decay half: no empty group
    assert all(p is not dict(m.named_parameters())[frozen] for g in groups for p in g["params"])


def test_jepa_encoder_groups_leave_the_frozen_table_out(bvc):
    enc = _jepa_encoder(bvc)
    assert not enc.pos_embed.requires_grad
    groups = bvc.optim.layer_decay_param_groups(enc, LR, WD, DECAY)
    _check_groups(enc, groups, _jepa_id)
    assert all(p is not enc.pos_embed for g in groups for p in g["params"])
    names = {g["name"] for g in groups}
    assert f"layer_{L + 1}_decay" not in names and f"layer_{L + 1}_no_decay" in names      # the final norm has no matrix
    assert len(groups) == 2 * (L + 2) - 1


def test_set_base_lr_rescales_every_group(bvc):
    m = _cls_model(bvc)
    groups = bvc.optim.layer_decay_param_groups(m, LR, WD, DECAY)
    extra = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.AdamW(groups + [{"params": [extra]}], lr=LR)  # a group without lr_scale follows the base rate itself
    bvc.optim.set_base_lr(opt, 4e-4)
    for g in opt.param_groups:
        assert g["lr"] == pytest.approx(4e-4 * g.get("lr_scale", 1.0), rel=1e-12)
    assert opt.param_groups[-1]["lr"] == 4e-4
    assert len({g["lr"] for g in opt.param_groups}) == L + 2


def test_unknown_module_type_raises(bvc):
    with pytest.raises(TypeError):
        bvc.optim.layer_decay_param_groups(torch.nn.Linear(4, 4), LR, WD, DECAY)
    with pytest.raises(TypeError):
        bvc.optim.layer_decay_param_groups(bvc.jepa.vit_predictor(sequence_shape=(2, 4, 4), embed_dim=128, predictor_embed_dim=128, depth=1,
                                                                  num_heads=2), LR, WD, DECAY)


# ---------------------------------------------------------------------------------------------- the plan for nine or more groups
def _module(n):       # the stand-in flat module of tests/test_optim_plan.py
    m = types.SimpleNamespace()
    m._flat = torch.zeros(n)
    m._flat_grad = torch.zeros(n)
    return m


def _param(m, off, size):
    p = torch.nn.Parameter(m._flat[off:off + size])
    p.grad = m._flat_grad[off:off + size]
    return p


def test_table_plan_for_more_groups_than_the_by_value_struct(bvc):
    from bvc_amd import optim
    ng = bvc._lib.OPT_MAX_GROUPS + 4
    m = _module(16 * ng + 40)
    ps = [_param(m, 16 * i, 16) for i in range(ng)]
    ps[5].grad = None                                               # frozen: belongs to no segment
    outside = torch.nn.Parameter(torch.zeros(7))
    outside.grad = torch.zeros(7)
    groups = [{"params": [p]} for p in ps]
    groups[3]["params"].append(outside)
    groups.append({"params": []})                                   # an empty group takes a row of the table and nothing else
    inside = {id(p) for p in ps}
    plans, loose = optim._build_table_plans(groups, owner=lambda p: m if id(p) in inside else None)
    assert len(plans) == 1 and plans[0].table and plans[0].module is m
    plan = plans[0]
    assert plan.seg_start.tolist() == [0, 16, 32, 48, 64, 80, 96] + [16 * i for i in range(7, ng + 1)] + [16 * ng + 40]
    assert plan.seg_group.tolist() == [0, 1, 2, 3, 4, -1] + list(range(6, ng)) + [-1]
    assert plan.blk_seg.tolist() == [0]
    assert set(loose) == {3} and loose[3][0] is outside             # no empty lists: only groups with parameters outside flat buffers
    # the by-value builder answers as before: no plan, every group listed
    old_plans, old_loose = optim._build_plans(groups)
    assert old_plans == [] and sorted(old_loose) == list(range(len(groups))) and old_loose[len(groups) - 1] == [] and len(old_loose[5]) == 0
    assert not optim._Plan(m, [(0, ps[0], 0)]).table
    with pytest.raises(bvc._lib.BvcError):
        optim._build_table_plans([{"params": []}] * (bvc._lib.OPT_TABLE_MAX_GROUPS + 1))


def test_table_constants_and_symbols(bvc):
    assert bvc._lib.OPT_MAX_GROUPS == 8 and bvc._lib.OPT_TABLE_MAX_GROUPS == 1024
    for name in ("bvc_op_sgd_step_table", "bvc_op_adam_step_table"):
        assert name in bvc._lib.SYMBOLS and getattr(bvc._lib.lib(), name) is not None
    # argument checks happen before anything is launched: no GPU needed to see them
    lib = bvc._lib.lib()
    assert lib.bvc_op_sgd_step_table(*([None] * 3), 0, *([None] * 3), 0, 0, *([None] * 10), 0, None, None) != 0


def test_empty_groups_give_no_runs(bvc):
    opt = bvc.optim.AdamW([{"params": [torch.nn.Parameter(torch.zeros(2))]}])
    assert opt._group_runs(0, []) == []
    sgd = bvc.optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(2))]}], lr=0.1)
    assert sgd._group_runs(0, []) == []


@pytest.mark.parametrize("cls", ["SGD", "Adam", "AdamW"])
def test_load_state_dict_drops_the_cached_plans(bvc, cls):
    opt = getattr(bvc.optim, cls)([torch.nn.Parameter(torch.zeros(2))], lr=0.1)
    opt._plans, opt._runs = ("key", [], {}), {0: ("key", [])}
    opt.load_state_dict(opt.state_dict())
    assert opt._plans is None and opt._runs == {}


def test_plans_survive_moved_gradients_of_loose_parameters(bvc):
    """Autograd allocates the gradients of parameters outside flat buffers anew every step; where such a parameter is first or last of
    its group the key moves, and the plans (with the flat optimiser state on them) must be kept - but not when a flat parameter moved."""
    from bvc_amd import optim
    m = _module(64)
    a, b = _param(m, 0, 32), _param(m, 32, 32)
    outside = torch.nn.Parameter(torch.zeros(7))
    outside.grad = torch.zeros(7)
    groups = [{"params": [a]}, {"params": [b, outside]}]
    plans, loose = optim._build_table_plans(groups, owner=lambda p: m if p is a or p is b else None)
    key = optim._plans_key(groups)
    assert optim._plans_still_valid((key, plans, loose), key)
    outside.grad = torch.zeros(7)
    moved = optim._plans_key(groups)
    assert moved != key and optim._plans_still_valid((key, plans, loose), moved)
    b.grad = torch.zeros(32)                                         # no longer a view of the flat gradient buffer
    assert not optim._plans_still_valid((key, plans, loose), optim._plans_key(groups))
    b.grad = m._flat_grad[32:64]
    assert optim._plans_still_valid((key, plans, loose), optim._plans_key(groups))
    a.grad = None                                                    # frozen after the table was built
    assert not optim._plans_still_valid((key, plans, loose), optim._plans_key(groups))
    a.grad = m._flat_grad[0:32]
    outside.grad = None
    assert not optim._plans_still_valid((key, plans, loose), optim._plans_key(groups))
