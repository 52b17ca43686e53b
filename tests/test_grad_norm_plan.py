"""Gradient-norm clipping on the host, WITHOUT a GPU: the work list the norm pass runs over (``bvc_grad_norm_items_host`` through
``bvc.optim.grad_norm_work_list``) on ragged segment tables, the CPU fallback of ``bvc.optim.clip_grad_norm_`` and the validation of
``max_grad_norm``."""
import pytest
import torch


def _table(lengths_and_owners):
    """[(length, group)] -> (seg_start, seg_group)"""
    starts, groups, pos = [0], [], 0
    for k, g in lengths_and_owners:
        pos += k
        starts.append(pos)
        groups.append(g)
    return starts, groups


def _pad_to_3_mod_4(segments, hole):
    """a hole at the end, long enough (1..4) for the total to be 3 modulo 4"""
    n = sum(k for k, _ in segments)
    return segments + [((3 - n) % 4 or 4, hole)]


def _tables(cap):
    H = -1      # a hole: owned by nobody
    return {
        "length_one": _table([(1, 0)]),
        "cap": _table([(cap, 3)]),
        "cap_plus_one": _table([(cap + 1, 0)]),
        "three_caps_plus_five": _table([(3 * cap + 5, 7)]),
        "hole_front": _table([(9, H), (130, 0), (cap + 1, 1)]),
        "hole_middle": _table([(130, 0), (2 * cap + 3, H), (1, 2), (cap, 1)]),
        "hole_end": _table([(1, 0), (3, 1), (cap + 1, 2), (77, H)]),
        # everything at once, n % 4 == 3: holes front / middle / end, 1, cap, cap + 1 and 3 cap + 5, an empty owned segment
        "ragged": _table(_pad_to_3_mod_4([(2, H), (1, 0), (3, H), (3, 1), (1025, 0), (0, 4), (cap, 2), (5, H), (cap + 1, 3), (3 * cap + 5, 0),
                                          (6, 1)], H)),
        "only_holes": _table([(5, H), (cap + 9, H)]),
        "empty": ([0], []),
    }


NAMES = ["length_one", "cap", "cap_plus_one", "three_caps_plus_five", "hole_front", "hole_middle", "hole_end", "ragged", "only_holes", "empty"]


@pytest.mark.parametrize("name", NAMES)
def test_work_list_properties(bvc, name):
    cap = bvc._lib.lib().bvc_op_grad_norm_item_cap()
    assert cap >= 4 and cap % 4 == 0
    starts, groups = _tables(cap)[name]
    n, nseg = starts[-1], len(groups)
    if name == "ragged":
        assert n % 4 == 3
    items, first = bvc.optim.grad_norm_work_list(starts, groups)
    items, first = items.tolist(), first.tolist()
    assert len(first) == nseg + 1 and first[0] == 0 and first[-1] == len(items)
    covered = torch.zeros(n, dtype=torch.int32)
    for start, length, seg in items:
        assert 1 <= length <= cap                                        # no item exceeds the cap (and none is empty)
        assert 0 <= seg < nseg and groups[seg] >= 0                       # holes have no items
        assert starts[seg] <= start and start + length <= starts[seg + 1]   # no item crosses a segment boundary
        covered[start:start + length] += 1
    owned = torch.zeros(n, dtype=torch.int32)
    for s in range(nseg):
        if groups[s] >= 0:
            owned[starts[s]:starts[s + 1]] = 1
    assert torch.equal(covered, owned)                                    # each owned element exactly once, nothing else at all
    for s in range(nseg):                                                 # seg_first_item: a segment's items are adjacent and ascending
        mine = items[first[s]:first[s + 1]]
        assert all(seg == s for _, _, seg in mine)
        assert [i for i, it in enumerate(items) if it[2] == s] == list(range(first[s], first[s + 1]))
        if groups[s] < 0:
            assert not mine
        else:
            assert sum(k for _, k, _ in mine) == starts[s + 1] - starts[s]
            pos = starts[s]
            for start, length, _ in mine:
                assert start == pos
                pos += length
    if name == "three_caps_plus_five":
        assert [k for _, k, _ in items] == [cap, cap, cap, 5]
    if name == "empty":
        assert items == [] and first == [0]


def test_work_list_rejects_a_descending_table(bvc):
    with pytest.raises(bvc._lib.BvcError):
        bvc.optim.grad_norm_work_list([0, 10, 5], [0, 0])
    with pytest.raises(bvc._lib.BvcError):
        bvc.optim.grad_norm_work_list([0, 10], [0, 0])


def test_chain_is_exported_next_to_the_cap(bvc):
    L = bvc._lib.lib()
    cap, chain = L.bvc_op_grad_norm_item_cap(), L.bvc_op_grad_norm_chain()
    assert 1 <= chain <= cap and cap % chain == 0


@pytest.mark.parametrize("max_norm", [0.05, 1e6])
def test_clip_grad_norm_on_cpu_tensors_is_torchs_bit_for_bit(bvc, max_norm):
    gen = torch.Generator().manual_seed(3)
    shapes = [(7, 5), (33,), (1,), (4, 4, 3)]
    mine = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes] + [torch.nn.Parameter(torch.zeros(2))]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    for p, q in zip(mine[:-1], theirs[:-1]):
        p.grad = torch.randn(p.shape, generator=gen) * 3
        q.grad = p.grad.clone()
    a = bvc.optim.clip_grad_norm_((p for p in mine), max_norm)                # a generator, as model.parameters() is
    b = torch.nn.utils.clip_grad_norm_(theirs, max_norm)
    assert torch.equal(a, b)
    for p, q in zip(mine[:-1], theirs[:-1]):
        assert torch.equal(p.grad, q.grad)
    assert mine[-1].grad is None
    # another norm type and a single tensor take the same road
    assert torch.equal(bvc.optim.clip_grad_norm_(mine[0], 0.01, norm_type=1.0), torch.nn.utils.clip_grad_norm_(theirs[0], 0.01, norm_type=1.0))
    assert torch.equal(mine[0].grad, theirs[0].grad)


@pytest.mark.parametrize("cls", ["SGD", "Adam", "AdamW"])
def test_max_grad_norm_validation(bvc, cls):
    make = getattr(bvc.optim, cls)
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (-1.0, float("nan"), -0.0001):
        with pytest.raises(ValueError):
            make(p, lr=0.1, max_grad_norm=bad)
    with pytest.raises(TypeError):
        make(p, 0.1, 0.9, 0.0, 0.0, False, False, 1.0) if cls == "SGD" else make(p, 0.1, (0.9, 0.99), 1e-8, 0.0, False, False, 1.0)   # keyword-only
    assert make(p, lr=0.1).max_grad_norm is None
    assert make(p, lr=0.1, max_grad_norm=0.0).max_grad_norm == 0.0
    assert make(p, lr=0.1, max_grad_norm=2).max_grad_norm == 2.0
    assert make(p, lr=0.1, max_grad_norm=float("inf")).max_grad_norm == float("inf")
