"""CPU checks of the VideoMAE sizes (bvc.videomae_config / VIDEOMAE_ARCHS: small, base, large, huge): each builds with transformers'
state-dict keys and shapes, the C ABI accepts huge's 80-wide heads in both stacks and still refuses what stays unsupported, every
product of a huge encoder and decoder layer selects a GEMM kernel that exists, and videomae_gflop reproduces the headline's count.
No GPU compute: layouts and kernel selection are host code."""
import ctypes

import pytest

from tools.bench_legs import videomae_gflop

BVC_ERR_INVALID = -1
# (hidden, layers, heads, decoder hidden, decoder heads) of the VideoMAE (v1) pre-training models
ZOO = {"small": (384, 12, 6, 192, 3), "base": (768, 12, 12, 384, 6), "large": (1024, 24, 16, 512, 8), "huge": (1280, 32, 16, 640, 8)}


@pytest.mark.parametrize("arch", sorted(ZOO))
def test_config_has_the_published_shape(bvc, arch):
    c = bvc.videomae_config(arch)
    D, depth, heads, Dd, Hd = ZOO[arch]
    assert bvc.VIDEOMAE_ARCHS[arch] == ZOO[arch]
    assert (c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.intermediate_size) == (D, depth, heads, 4 * D)
    assert (c.decoder_hidden_size, c.decoder_num_attention_heads, c.decoder_num_hidden_layers, c.decoder_intermediate_size) == (Dd, Hd, 4, 4 * Dd)
    assert (c.patch_size, c.tubelet_size, c.num_frames, c.image_size, c.norm_pix_loss) == (16, 2, 16, 224, True)


def test_base_is_get_config(bvc):
    class Args:
        architecture, num_frames, tubelet_size = "base", 16, 2
    a, b = bvc.get_config(224, Args()).__dict__, bvc.videomae_config("base").__dict__
    assert a == b


def test_overrides_and_unknown_architecture(bvc):
    c = bvc.videomae_config("huge", num_hidden_layers=2, num_frames=4)
    assert (c.num_hidden_layers, c.num_frames, c.hidden_size, c.intermediate_size) == (2, 4, 1280, 5120)
    with pytest.raises(ValueError):
        bvc.videomae_config("giant")


def _transformers_shapes(arch, **kw):
    transformers = pytest.importorskip("transformers")
    D, _, heads, Dd, Hd = ZOO[arch]
    cfg = transformers.VideoMAEConfig(image_size=224, patch_size=16, num_channels=3, num_frames=16, tubelet_size=2, hidden_size=D,
                                      num_hidden_layers=kw.get("num_hidden_layers", ZOO[arch][1]), num_attention_heads=heads,
                                      intermediate_size=4 * D, initializer_range=0.02, use_mean_pooling=True, decoder_num_attention_heads=Hd,
                                      decoder_hidden_size=Dd, decoder_num_hidden_layers=4, decoder_intermediate_size=4 * Dd, norm_pix_loss=True)
    model = transformers.VideoMAEForPreTraining(cfg)
    return {k: tuple(v.shape) for k, v in model.state_dict().items()}


@pytest.mark.parametrize("arch", sorted(ZOO))
def test_state_dict_equals_transformers(bvc, arch):
    # full depth for every size but huge (32 layers of 1280 would only repeat the first two); huge's layout is checked at 2 layers
    depth = {"huge": 2}.get(arch, ZOO[arch][1])
    want = _transformers_shapes(arch, num_hidden_layers=depth)
    sd = bvc.VideoMAEForPreTraining(bvc.videomae_config(arch, num_hidden_layers=depth)).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want


def test_huge_classification_model_has_the_encoder_keys(bvc):
    cfg = bvc.videomae_config("huge", num_hidden_layers=2, num_labels=0)
    sd = bvc.VideoMAEForVideoClassification(cfg).state_dict()
    assert tuple(sd["videomae.encoder.layer.1.attention.attention.query.weight"].shape) == (1280, 1280)
    assert tuple(sd["fc_norm.weight"].shape) == (1280,)


def _numel(bvc, **kw):
    c = bvc.videomae_config("huge", num_hidden_layers=2, **kw).to_c()
    return bvc._lib.lib().bvc_videomae_param_numel(ctypes.byref(c))


def test_abi_accepts_huge_and_refuses_the_rest(bvc):
    L = bvc._lib.lib()
    for arch in ZOO:
        c = bvc.videomae_config(arch).to_c()
        assert L.bvc_videomae_param_numel(ctypes.byref(c)) > 0, arch
    full = bvc.videomae_config("huge").to_c()
    assert L.bvc_videomae_param_count(ctypes.byref(full)) == 16 * (32 + 4) + 8     # 16 per layer (264 for base)
    assert _numel(bvc) > 0                                                        # 80 / 80
    assert _numel(bvc, hidden_size=1408, intermediate_size=5632) > 0              # encoder heads of 88
    assert _numel(bvc, hidden_size=1536, num_attention_heads=12) > 0              # 128, the widest row
    assert _numel(bvc, decoder_hidden_size=384, decoder_num_attention_heads=16) > 0   # decoder heads of 24 (run padded to 32)
    assert _numel(bvc, num_attention_heads=64) == BVC_ERR_INVALID                 # head dim 20: not a multiple of 8
    assert b"head_dim 20" in L.bvc_last_error()
    assert _numel(bvc, hidden_size=1088, num_attention_heads=8) == BVC_ERR_INVALID    # head dim 136
    assert _numel(bvc, decoder_hidden_size=1088, decoder_num_attention_heads=8) == BVC_ERR_INVALID
    assert b"decoder head_dim 136" in L.bvc_last_error()
    assert _numel(bvc, hidden_size=1600, num_attention_heads=20) == BVC_ERR_INVALID   # width 1600 (head dim 80)
    assert b"1536" in L.bvc_last_error()
    assert _numel(bvc, decoder_hidden_size=1600, decoder_num_attention_heads=20) == BVC_ERR_INVALID
    assert _numel(bvc, hidden_size=1300, num_attention_heads=13) == BVC_ERR_INVALID   # 100: not a multiple of 8


def test_head_pad_option_round_trips(bvc):
    L = bvc._lib
    assert L.lib().bvc_get_option(b"head_pad") == 0
    assert L.set_option("head_pad", 1) == 0
    assert L.lib().bvc_get_option(b"head_pad") == 1
    assert L.set_option("head_pad", 0) == 1
    assert L.lib().bvc_set_option(b"head_pad", 2) == BVC_ERR_INVALID
    assert L.lib().bvc_get_option(b"head_pad") == 0


def test_attention_width_follows_head_pad(bvc):
    L = bvc._lib
    f = L.lib().bvc_op_attention_width
    assert [f(hd) for hd in (24, 32, 40, 64, 72, 80, 88, 96, 104, 128)] == [32, 32, 64, 64, 96, 80, 88, 96, 128, 128]
    old = L.set_option("head_pad", 1)
    try:
        assert [f(hd) for hd in (24, 64, 80, 88, 96, 128)] == [32, 64, 96, 96, 96, 128]
    finally:
        L.set_option("head_pad", old)
    assert f(80) == 80
    assert f(20) == BVC_ERR_INVALID and f(136) == BVC_ERR_INVALID


def test_create_refuses_a_batch_past_the_4_gib_operand_extent(bvc):
    """VideoMAE-H's decoder fc1 output is 1568 x 2560 bf16 = 8 028 160 bytes per clip: 534 clips stay below 4 GiB, 535 do not.  The
    refusal comes before any allocation (no GPU needed) and names the largest batch that fits."""
    L = bvc._lib.lib()
    c = bvc.videomae_config("huge").to_c()
    ctx = ctypes.c_void_p()
    assert L.bvc_videomae_create(ctypes.byref(c), 535, 1408, ctypes.byref(ctx)) == BVC_ERR_INVALID
    assert not ctx.value
    msg = L.bvc_last_error()
    assert b"4 GiB" in msg and b"decoder" in msg and b"at most 534 clips" in msg, msg


def test_row_ln_selection_at_the_new_head_widths(bvc):
    L = bvc._lib.lib()
    # the fused 128 x 384 row epilogues stay 384-only: the decoders of small / large / huge take the separate LayerNorm passes
    for width, heads in ((192, 3), (512, 8), (640, 8), (1280, 16)):
        assert L.bvc_op_row_ln_selected(64 * 1568, width, 4 * width, heads) == 0, width


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


@pytest.mark.parametrize("stack", ["encoder", "decoder"])
@pytest.mark.parametrize("clips", [16, 64])
def test_every_huge_layer_product_selects_an_existing_kernel(bvc, stack, clips):
    """One huge layer at 16 / 64 clips: encoder 160 visible tokens x 1280, decoder 1568 tokens x 640, heads of 80 in place (the
    attention width is the model width: no padded columns), forward NT, input-gradient NN and the weight-gradient TN group."""
    L = bvc._lib
    D, N = (1280, 160) if stack == "encoder" else (640, 1568)
    M, inter = clips * N, 4 * D
    NT, NN, TN = 0, 1, 2
    BF16, GELU, RESID, DGELU = 1, 2, 3, 7
    fwd = [(M, 3 * D, D, BF16), (M, D, D, RESID), (M, inter, D, GELU), (M, D, inter, RESID)]
    bwd = [(M, inter, D, DGELU), (M, D, inter, 0), (M, D, D, 0), (M, D, 3 * D, 0)]
    for m, n, k, epi in fwd:
        assert _kernel(L, [_desc(L, m, n, k, epi, NT)], NT).startswith("bvc::"), (m, n, k)
    for m, n, k, epi in bwd:
        assert _kernel(L, [_desc(L, m, n, k, epi, NN)], NN).startswith("bvc::"), (m, n, k)
    group = [_desc(L, D, inter, M, 0, TN), _desc(L, inter, D, M, 0, TN), _desc(L, D, D, M, 0, TN), _desc(L, 3 * D, D, M, 0, TN)]
    arr = (L.GemmDesc * len(group))(*group)
    tile = L.lib().bvc_op_gemm_plan_dw(arr, len(group))
    assert tile >= 0
    assert _kernel(L, list(arr), TN, tile).startswith("bvc::")


def test_gflop_helper(bvc):
    assert round(videomae_gflop(bvc.videomae_config("base")), 3) == 202.295
    # the larger sizes cost more per clip in order, and the counting is linear in the encoder depth
    g = {a: videomae_gflop(bvc.videomae_config(a)) for a in ZOO}
    assert g["small"] < g["base"] < g["large"] < g["huge"]
    one, two = (videomae_gflop(bvc.videomae_config("huge", num_hidden_layers=n)) for n in (1, 2))
    assert abs(g["huge"] - (one + 31 * (two - one))) < 1e-6 * g["huge"]
