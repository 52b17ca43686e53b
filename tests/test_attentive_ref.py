"""CPU checks of the attentive probe: the algebra the kernel rests on (tests/attentive_ref.py, float64), the module's interface,
and the refusals the library makes before it launches anything.  No GPU compute."""
import ctypes

import pytest
import torch

import __graft_entry__ as ge
from tests import attentive_ref as A

F64 = torch.float64


@pytest.fixture(scope="module")
def bvc():
    ge.build()
    return ge.load_package()


def _tokens(B, N, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, D, generator=g, dtype=F64) * 1.5 + 0.3 * torch.randn(B, N, 1, generator=g, dtype=F64)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("H", [1, 3, 12])
@pytest.mark.parametrize("complete_block", [True, False])
def test_folded_equals_unfused(H, complete_block):
    D, B, N, C = 24 * H if H < 12 else 48, 2, 13, 5
    sd = A.make_params(D, H, C, complete_block=complete_block, seed=H)
    x = _tokens(B, N, D, seed=H)
    labels = torch.tensor([1, 4])
    lu, su, gu = A.loss_and_grads(A.unfused_logits, sd, x, labels, H=H)
    lf, sf, gf = A.loss_and_grads(A.folded_logits, sd, x, labels, H=H)
    assert _rel(lf, lu) < 1e-12 and abs(float(sf - su)) < 1e-12 * abs(float(su))
    assert set(gu) == set(gf) == set(sd)
    for k in sd:
        assert _rel(gf[k], gu[k]) < 1e-12, k


def test_gradcheck_of_reference_core():
    x = _tokens(2, 5, 8, seed=3).requires_grad_(True)
    u = (torch.randn(3, 8, dtype=F64, generator=torch.Generator().manual_seed(4))).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: A.core(a, b, 1e-5)[0], (x, u), eps=1e-6, atol=1e-7, rtol=1e-6)


def test_hand_backward_equals_autograd():
    g = torch.Generator().manual_seed(5)
    x = _tokens(3, 17, 32, seed=5).requires_grad_(True)
    u = torch.randn(5, 32, dtype=F64, generator=g).requires_grad_(True)
    dpooled = torch.randn(3, 5, 32, dtype=F64, generator=g)
    pooled, _ = A.core(x, u, 1e-5)
    dx_a, du_a = torch.autograd.grad(pooled, (x, u), dpooled)
    du, dx = A.core_backward(x.detach(), u.detach(), 1e-5, dpooled)
    assert _rel(du, du_a) < 1e-12 and _rel(dx, dx_a) < 1e-12


def test_zero_queries_give_the_mean_and_log_n():
    x = _tokens(2, 9, 16, seed=6)
    pooled, lse = A.core(x, torch.zeros(4, 16, dtype=F64), 1e-5)
    xh, _ = A.standardise(x, 1e-5)
    assert torch.allclose(pooled, xh.mean(1, keepdim=True).expand(-1, 4, -1), rtol=0, atol=1e-15)
    assert torch.allclose(lse, torch.full_like(lse, 9.0).log(), rtol=0, atol=1e-15)


def test_constant_added_to_a_heads_scores_changes_nothing():
    H, D = 3, 24
    sd = A.make_params(D, H, 4, seed=7)
    x = _tokens(2, 11, D, seed=7)
    a = A.unfused_logits(sd, x, H)
    b = A.unfused_logits(sd, x, H, score_shift=torch.tensor([3.0, -7.0, 0.5], dtype=F64))
    assert _rel(b, a) < 1e-12
    # which is why the folded form may drop c_h = scale q_h . (Wk_h beta + bk_h)
    assert _rel(A.folded_logits(sd, x, H), a) < 1e-12


@pytest.mark.parametrize("complete_block,qkv_bias", [(True, True), (False, False)])
def test_state_dict_keys_shapes_and_round_trip(bvc, complete_block, qkv_bias):
    D, H, C = 64, 4, 7
    m = bvc.AttentiveClassifier(D, H, C, complete_block=complete_block, qkv_bias=qkv_bias, mlp_ratio=2.0)
    want = {k: tuple(v.shape) for k, v in A.make_params(D, H, C, mlp_ratio=2.0, complete_block=complete_block, qkv_bias=qkv_bias).items()}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert want["pooler.query_tokens"] == (1, 1, D) and want[A.P + "xattn.kv.weight"] == (2 * D, D)
    # initialisation: truncated normal weights and query, zero biases, unit norm weights
    sd = m.state_dict()
    assert float(sd[A.P + "norm1.weight"].min()) == 1.0 and float(sd[A.P + "xattn.proj.bias"].abs().max()) == 0.0
    assert 0 < float(sd["linear.weight"].abs().max()) <= 2.0 and float(sd["pooler.query_tokens"].std()) < 0.05
    src = {k: v.float() for k, v in A.make_params(D, H, C, mlp_ratio=2.0, complete_block=complete_block, qkv_bias=qkv_bias, seed=3).items()}
    m.load_state_dict(src)
    for k, v in m.state_dict().items():
        assert torch.equal(v, src[k]), k
    assert isinstance(bvc.AttentivePooler(D, H), torch.nn.Module) and bvc.attentive.attentive_pool is bvc.attentive_pool
    # the module's folded queries are the reference's
    u, _ = m.pooler.folded_queries()
    assert _rel(u.detach().double(),A.folded_u({k: v.double() for k, v in src.items()}, H)) < 1e-5


def test_cpu_tensors_raise(bvc):
    with pytest.raises(bvc._lib.BvcError):
        bvc.attentive_pool(torch.zeros(1, 4, 64), torch.zeros(2, 64))
    with pytest.raises(bvc._lib.BvcError):
        bvc.AttentiveClassifier(64, 4, 3)(torch.zeros(1, 4, 64))
    with pytest.raises(ValueError):
        bvc.attentive_pool(torch.zeros(1, 4, 64), torch.zeros(2, 32))
    with pytest.raises(ValueError):
        bvc.AttentivePooler(64, 17)


@pytest.mark.parametrize("B,N,D,R,splits,word", [(1, 8, 100, 4, 0, b"D 100"), (1, 8, 64, 17, 0, b"R 17"), (1, 0, 64, 4, 0, b"N 0"),
                                                 (1, 8, 2112, 4, 0, b"D 2112"), (1, 8, 64, 0, 0, b"R 0"), (0, 8, 64, 4, 0, b"B 0"),
                                                 (1, 8, 64, 4, 257, b"splits 257")])
def test_refusals_before_launch(bvc, B, N, D, R, splits, word):
    lib = bvc._lib.lib()
    assert lib.bvc_op_attn_pool_workspace(B, N, D, R, splits) == -1 and word in lib.bvc_last_error()
    if splits == 0:
        assert lib.bvc_op_attn_pool_splits(B, N, D, R) == -1 and word in lib.bvc_last_error()
    buf = (ctypes.c_float * 64)()        # never dereferenced: the shape is refused first
    p = ctypes.addressof(buf)
    assert lib.bvc_op_attn_pool_fwd(p, D, p, B, N, D, R, 1e-5, splits, p, p, p, None) != 0 and word in lib.bvc_last_error()
    assert lib.bvc_op_attn_pool_bwd(p, D, p, p, p, p, B, N, D, R, 1e-5, splits, p, None, D, p, None) != 0 and word in lib.bvc_last_error()


def test_sizes_and_argument_refusals(bvc):
    lib = bvc._lib.lib()
    assert lib.bvc_op_attn_pool_workspace(3, 197, 192, 12, 7) == 3 * 7 * 12 * (192 + 2) * 4
    s = lib.bvc_op_attn_pool_splits(4, 1568, 768, 12)
    assert 1 <= s <= 1568 // 64 and lib.bvc_op_attn_pool_splits(256, 1568, 768, 12) == 4 and lib.bvc_op_attn_pool_splits(1, 3, 64, 1) == 1
    assert lib.bvc_op_attn_pool_workspace(4, 1568, 768, 12, 0) == lib.bvc_op_attn_pool_workspace(4, 1568, 768, 12, s)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf) // 16 * 16 + 16
    assert lib.bvc_op_attn_pool_fwd(p, 64, None, 1, 1, 64, 1, 1e-5, 1, p, p, p, None) != 0 and b"null" in lib.bvc_last_error()
    assert lib.bvc_op_attn_pool_fwd(p, 63, p, 1, 1, 64, 1, 1e-5, 1, p, p, p, None) != 0 and b"stride" in lib.bvc_last_error()
    assert lib.bvc_op_attn_pool_fwd(p, 66, p, 1, 1, 64, 1, 1e-5, 1, p, p, p, None) != 0 and b"stride" in lib.bvc_last_error()
    assert lib.bvc_op_attn_pool_fwd(p + 4, 64, p, 1, 1, 64, 1, 1e-5, 1, p, p, p, None) != 0 and b"aligned" in lib.bvc_last_error()
    assert lib.bvc_op_attn_pool_bwd(p, 64, p, p, p, p, 1, 1, 64, 1, 1e-5, 1, p, p, 60, p, None) != 0 and b"dx" in lib.bvc_last_error()
