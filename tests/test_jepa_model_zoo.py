"""CPU checks of the JEPA model zoo: the six encoder factories of pretraining/predictive/vision_transformer.py:544-590 (tiny, small,
base, large, huge, giant) build with the reference's state-dict keys and shapes, the C ABI accepts the head widths they need (80 / 88
zero-padded to 96, the ViT-Ti predictor's 128) and still refuses what stays unsupported, and every product of a ViT-H / ViT-g layer
selects a GEMM kernel that exists.  No GPU compute: layouts and kernel selection are host code."""
import ctypes

import pytest

from oracle import jepa_oracle as jo
from tools.bench_legs import JEPA_GFLOP, jepa_gflop

# vision_transformer.py:544-590: (embed_dim, depth, num_heads, MLP width = int(embed_dim * mlp_ratio))
ZOO = {
    "vit_tiny": (192, 12, 3, 768),
    "vit_small": (384, 12, 6, 1536),
    "vit_base": (768, 12, 12, 3072),
    "vit_large": (1024, 24, 16, 4096),
    "vit_huge": (1280, 32, 16, 5120),
    "vit_giant": (1408, 40, 16, 6144),
}
BVC_ERR_INVALID = -1


@pytest.mark.parametrize("name", sorted(ZOO))
def test_factory_state_dict_has_the_reference_keys_and_shapes(bvc, name):
    D, depth, heads, inter = ZOO[name]
    enc = getattr(bvc.jepa, name)(img_size=[224], num_frames=2, tubelet_size=1)
    assert (enc.embed_dim, enc.num_heads) == (D, heads)
    assert bvc.jepa.VIT_EMBED_DIMS[name] == D
    sd = enc.state_dict()
    blocks = {k.split(".")[1] for k in sd if k.startswith("blocks.")}
    assert blocks == {str(i) for i in range(depth)}
    assert tuple(sd["pos_embed"].shape) == (1, 392, D)
    assert tuple(sd["patch_embed.proj.weight"].shape) == (D, 3, 1, 16, 16)
    for i in (0, depth - 1):
        assert tuple(sd[f"blocks.{i}.attn.qkv.weight"].shape) == (3 * D, D)
        assert tuple(sd[f"blocks.{i}.attn.proj.weight"].shape) == (D, D)
        assert tuple(sd[f"blocks.{i}.mlp.fc1.weight"].shape) == (inter, D)
        assert tuple(sd[f"blocks.{i}.mlp.fc2.weight"].shape) == (D, inter)
    cfg = jo.JepaConfig(embed_dim=D, depth=depth, num_heads=heads, mlp_ratio=inter / D)
    want = jo.encoder_shapes(cfg)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in want.items()}


@pytest.mark.parametrize("name", ["vit_tiny", "vit_huge", "vit_giant"])
def test_get_model_builds_the_new_encoders_and_their_predictors(bvc, name):
    enc, pred = bvc.jepa.get_model("cpu", patch_size=16, tubelet_size=1, num_frames=2, model_name=name, image_size=224)
    D, _, heads, _ = ZOO[name]
    assert enc.embed_dim == D and enc.num_heads == heads
    assert pred.num_heads == enc.num_heads
    psd = pred.state_dict()
    assert tuple(psd["predictor_embed.weight"].shape) == (384, D)
    assert tuple(psd["predictor_proj.weight"].shape) == (D, 384)
    assert tuple(psd["predictor_blocks.0.attn.qkv.weight"].shape) == (3 * 384, 384)


def _vit_numel(bvc, D, heads, inter=None):
    L = bvc._lib
    cfg = L.VitConfigC(224, 16, 3, 2, 1, D, 2, heads, inter or 4 * D, 1e-6)
    return L.lib().bvc_vit_param_numel(ctypes.byref(cfg))


def _pred_numel(bvc, D, P, heads):
    L = bvc._lib
    cfg = L.PredictorConfigC(392, D, P, 2, heads, 4 * P, 1e-6)
    return L.lib().bvc_predictor_param_numel(ctypes.byref(cfg))


def test_abi_accepts_the_new_head_widths_and_refuses_the_rest(bvc):
    assert _vit_numel(bvc, 1280, 16) > 0             # head dim 80 (ViT-H)
    assert _vit_numel(bvc, 1408, 16, 6144) > 0       # head dim 88 (ViT-g)
    assert _vit_numel(bvc, 1536, 12) > 0             # head dim 128, the widest width
    assert _vit_numel(bvc, 192, 3) > 0               # ViT-Ti encoder: 64
    assert _vit_numel(bvc, 1088, 8) == BVC_ERR_INVALID     # head dim 136
    assert _vit_numel(bvc, 1600, 20) == BVC_ERR_INVALID    # width 1600 (head dim 80)
    assert _vit_numel(bvc, 1280, 32) > 0             # 40: a multiple of 8 (runs padded to 64)
    assert _vit_numel(bvc, 1280, 64) == BVC_ERR_INVALID    # 20: not a multiple of 8
    assert _pred_numel(bvc, 192, 384, 3) > 0         # ViT-Ti predictor: head dim 128
    assert _pred_numel(bvc, 1280, 384, 16) > 0       # ViT-H predictor: 24 (padded to 32)
    assert _pred_numel(bvc, 1408, 384, 16) > 0
    assert _pred_numel(bvc, 1536, 384, 16) > 0
    assert _pred_numel(bvc, 1024, 1088, 8) == BVC_ERR_INVALID   # head dim 136
    assert _pred_numel(bvc, 1600, 384, 16) == BVC_ERR_INVALID   # width 1600


@pytest.mark.parametrize("D", [192, 1280, 1408])
def test_positional_encoding_matches_the_oracle(bvc, D):
    # ceil(D / 6) * 2 channels per axis: 3 * 428 = 1284 > 1280 and 3 * 470 = 1410 > 1408 are truncated to D
    a = bvc.jepa.positional_encoding_3d((2, 14, 14), D)
    b = jo.positional_encoding_3d((2, 14, 14), D)
    assert a.shape == b.shape == (1, 392, D)
    assert float((a - b).abs().max()) == 0.0


def test_gflop_helper_reproduces_the_committed_counts():
    for name, want in (("vit_base", 160.6), ("vit_large", 473.2)):
        D, depth, _, inter = ZOO[name]
        assert abs(jepa_gflop(D, depth, inter) - want) / want < 1e-3
        assert JEPA_GFLOP[name] == want
    for name in ("vit_tiny", "vit_huge", "vit_giant"):
        D, depth, _, inter = ZOO[name]
        assert abs(jepa_gflop(D, depth, inter) - JEPA_GFLOP[name]) / JEPA_GFLOP[name] < 1e-3


def _desc(L, M, N, K, epi, layout):
    d = L.GemmDesc()
    d.A, d.B, d.C = 4096, 8192, 4096          # never dereferenced: nothing is launched
    d.M, d.N, d.K = M, N, K
    d.alpha, d.epi, d.split_k, d.ldc = 1.0, epi, 1, N
    d.a_bytes, d.b_bytes = M * K * 2, N * K * 2
    d.lda, d.ldb = {0: (K, K), 1: (K, N), 2: (M, N)}[layout]
    return d


def _kernel(L, descs, layout, tile=-1):
    arr = (L.GemmDesc * len(descs))(*descs)
    buf = ctypes.create_string_buffer(160)
    L.check(L.lib().bvc_op_gemm_kernel(arr, len(descs), layout, tile, -1, buf, 160), "bvc_op_gemm_kernel")
    return buf.value.decode()


@pytest.mark.parametrize("name", ["vit_huge", "vit_giant"])
@pytest.mark.parametrize("M", [16 * 100, 16 * 392])
def test_every_layer_product_selects_an_existing_kernel(bvc, name, M):
    """One encoder layer at 16 samples of 100 (context) and 392 (target) tokens: forward NT products, input-gradient NN products and
    the weight-gradient TN group, with the padded attention width Da = 16 x 96 = 1536 on the q | k | v and proj side."""
    L = bvc._lib
    D, _, heads, inter = ZOO[name]
    Da = heads * 96
    NT, NN, TN = 0, 1, 2
    BF16, GELU, RESID, DGELU = 1, 2, 3, 7
    fwd = [(M, 3 * Da, D, BF16), (M, D, Da, RESID), (M, inter, D, GELU), (M, D, inter, RESID)]
    bwd = [(M, inter, D, DGELU), (M, D, inter, 0), (M, Da, D, 0), (M, D, 3 * Da, 0)]
    for m, n, k, epi in fwd:
        assert _kernel(L, [_desc(L, m, n, k, epi, NT)], NT).startswith("bvc::"), (m, n, k)
    for m, n, k, epi in bwd:
        assert _kernel(L, [_desc(L, m, n, k, epi, NN)], NN).startswith("bvc::"), (m, n, k)
    group = [_desc(L, D, inter, M, 0, TN), _desc(L, inter, D, M, 0, TN), _desc(L, D, Da, M, 0, TN), _desc(L, 3 * Da, D, M, 0, TN)]
    arr = (L.GemmDesc * len(group))(*group)
    tile = L.lib().bvc_op_gemm_plan_dw(arr, len(group))
    assert tile >= 0
    assert _kernel(L, list(arr), TN, tile).startswith("bvc::")
