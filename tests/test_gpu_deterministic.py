"""Deterministic mode on the GPU (bvc.use_deterministic_algorithms / torch.use_deterministic_algorithms / option "deterministic"):
every check runs with the mode on and compares runs with torch.equal.  The products whose default kernels add by f32 atomics in
scheduling order - split-K / accumulating weight gradients, fused bias gradients, LayerNorm parameter partials, column sums - must
give the same bits launch after launch, also while a streaming copy loads HBM from a second stream, and the first result must stay
within the default mode's fp32 bars."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():   # collected on the CPU box, run on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import gpu_util as G   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402

L = G.L
bvc = G.bvc
dev = "cuda"


@pytest.fixture
def det():
    old = {k: L.set_option(k, v) for k, v in (("gemm8", 0), ("row_ln", 0))}
    bvc.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        bvc.use_deterministic_algorithms(False)
        L.lib()    # push the mode back to the library
        for k, v in old.items():
            L.set_option(k, v)


def _repeat_under_load(run, n=20):
    """run() -> tuple of tensors; n launches, a streaming copy on a second stream during each; returns the first result"""
    noise_src = torch.randn(64 * 1024 * 1024 // 4, device=dev)
    noise_dst = torch.empty_like(noise_src)
    side = torch.cuda.Stream()
    first = None
    for it in range(n):
        with torch.cuda.stream(side):
            noise_dst.copy_(noise_src)
        out = run()
        torch.cuda.synchronize()
        if first is None:
            first = tuple(t.clone() for t in out)
        else:
            for a, b in zip(out, first):
                assert torch.equal(a, b), f"launch {it} differs from launch 0"
    return first


def _dw_case(Mtok, D, I, split, seed=7):
    dy, act = G.bf16_randn(Mtok, D, seed=seed), G.bf16_randn(Mtok, I, seed=seed + 1)
    base = [torch.randn(D, I, device=dev), torch.randn(I, D, device=dev)]
    bias0 = [torch.randn(D, device=dev), torch.randn(I, device=dev)]

    def run():
        outs = [b.clone() for b in base]
        bs = [b.clone() for b in bias0]
        descs = [G.gemm_desc(dy, act, D, I, Mtok, G.EPI["F32"], outs[0], rowsum=bs[0], split_k=split),
                 G.gemm_desc(act, dy, I, D, Mtok, G.EPI["F32"], outs[1], rowsum=bs[1], split_k=split)]
        return descs, outs, bs

    refs = [dy.float().t() @ act.float(), act.float().t() @ dy.float()]
    sums = [dy.float().sum(0), act.float().sum(0)]
    return run, base, bias0, refs, sums


@pytest.mark.parametrize("g8,tile,split", [(-1, -1, 2), (-1, -1, 5), (-1, -1, 24), (-1, 0, 5), (1, 10, 2), (1, 11, 5), (1, 12, 24),
                                           (1, 13, 1)])
def test_weight_gradients_are_bitwise_reproducible(det, g8, tile, split):
    L.set_option("gemm8", g8)
    Mtok, D, I = 5000, 384, 1536
    make, base, bias0, refs, sums = _dw_case(Mtok, D, I, split)

    def run():
        descs, outs, bs = make()
        G.run_gemm(descs, G.TN, tile)
        return tuple(outs + bs)

    first = _repeat_under_load(run)
    for o, b0, r in zip(first[:2], base, refs):
        assert G.rel_err(o - b0, r) < 2e-5
    for b, b0, s in zip(first[2:], bias0, sums):
        assert float((b - b0 - s).abs().max()) < 2e-2 * math.sqrt(Mtok / 1000.0)


def test_split_k_without_bias_gradient_and_ragged_tokens(det):
    M, N, K = 256, 128, 1000
    A, B = G.bf16_randn(K, M, seed=5), G.bf16_randn(K, N, seed=6)
    C0 = torch.randn(M, N, device=dev)

    def run():
        C = C0.clone()
        G.run_gemm([G.gemm_desc(A, B, M, N, K, G.EPI["F32"], C, split_k=7, alpha=0.5)], G.TN, -1)
        return (C,)

    (C,) = _repeat_under_load(run, 5)
    assert G.rel_err(C, C0 + 0.5 * (A.float().t() @ B.float())) < 1e-5


@pytest.mark.parametrize("M,N", [(2560, 768), (25000, 384)])
def test_colsum_is_bitwise_reproducible(det, M, N):
    X = G.bf16_randn(M, N, seed=50)
    out0 = torch.randn(N, device=dev)
    s = torch.tensor([2.0], device=dev)

    def run():
        out = out0.clone()
        L.check(L.lib().bvc_op_colsum_bf16(G.ptr(X), M, N, N, 0.25, G.ptr(s), G.ptr(out), G.stream()), "colsum")
        return (out,)

    (out,) = _repeat_under_load(run)
    assert float((out - (out0 + 0.5 * X.float().sum(0))).abs().max()) < 1e-3 * max(1.0, math.sqrt(M))


@pytest.mark.parametrize("M,D", [(1000, 384), (70001, 384), (20000, 768)])
def test_layernorm_backward_parameter_reduce_is_bitwise_reproducible(det, M, D):
    g = torch.Generator().manual_seed(40)
    x = (torch.randn(M, D, generator=g) * 2 + 0.5).to(dev)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    beta = (0.1 * torch.randn(D, generator=g)).to(dev)
    y = torch.zeros(M, D, device=dev, dtype=torch.bfloat16)
    mean, rstd = torch.zeros(M, device=dev), torch.zeros(M, device=dev)
    L.check(L.lib().bvc_op_layernorm_fwd(G.ptr(x), 0, 0, 0, G.ptr(gamma), G.ptr(beta), G.ptr(y), G.ptr(mean), G.ptr(rstd),
                                         M, D, 1e-12, G.stream()), "ln_fwd")
    dy = G.bf16_randn(M, D, seed=41)
    ws = torch.zeros(int(L.lib().bvc_op_layernorm_bwd_workspace(M, D)), device=dev)

    def run():
        dres = torch.zeros(M, D, device=dev)
        dres_bf = torch.zeros(M, D, device=dev, dtype=torch.bfloat16)
        dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        L.check(L.lib().bvc_op_layernorm_bwd(G.ptr(dy), G.ptr(x), 0, 0, 0, G.ptr(mean), G.ptr(rstd), G.ptr(gamma), G.ptr(dres), 1,
                                             G.ptr(dres_bf), G.ptr(dg), G.ptr(db), G.ptr(ws), M, D, G.stream()), "ln_bwd")
        return dres, dg, db

    _, dg, db = _repeat_under_load(run)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-12).backward(dy.float())
    assert G.rel_err(dg, gr.grad) < 1e-4 and G.rel_err(db, br.grad) < 1e-4


# --------------------------------------------------------------------------- whole VideoMAE-base backward
def _model(cfg, params):
    kw = {k: v for k, v in cfg.__dict__.items() if k != "decoder_norm_eps"}
    m = bvc.VideoMAEForPreTraining(bvc.VideoMAEConfig(**kw))
    m.load_state_dict(params)
    return m.to(dev).train()


def _grads(model, px, mk, n=3, load=False):
    runs = []
    noise_src = torch.randn(64 * 1024 * 1024 // 4, device=dev) if load else None
    noise_dst = torch.empty_like(noise_src) if load else None
    side = torch.cuda.Stream()
    for _ in range(n):
        for p in model.parameters():
            p.grad = None
        if load:
            with torch.cuda.stream(side):
                noise_dst.copy_(noise_src)
        out = model(px, bool_masked_pos=mk)
        out.loss.backward()
        torch.cuda.synchronize()
        runs.append((float(out.loss), model.flat_grads().clone()))
    return runs


@pytest.mark.parametrize("clips,g8,row_ln,load", [(64, 0, 0, True), (16, 1, 1, False), (16, 1, -1, False)])
def test_videomae_base_backward_is_bitwise_reproducible(det, clips, g8, row_ln, load):
    """The flat gradient of three backward passes on identical inputs: today (mode off) ~6 % of its elements differ between runs
    at 64 clips (test_gpu_videomae.py::test_gradient_run_to_run_spread_at_64_clips); with the mode on, none."""
    L.set_option("gemm8", g8)
    L.set_option("row_ln", row_ln)
    cfg = vo.BASE
    params = vo.make_params(cfg, seed=0)
    pixels, mask = vo.synthetic_batch(cfg, clips, seed=5, mask_ratio=0.9)
    model = _model(cfg, params)
    runs = _grads(model, pixels.to(dev), mask.to(dev), load=load)
    for loss, g in runs[1:]:
        assert loss == runs[0][0]
        assert torch.equal(g, runs[0][1]), f"{100 * float((g != runs[0][1]).float().mean()):.3f} % of the gradient elements differ"


def test_deterministic_and_default_gradients_agree_at_the_spread_bar():
    cfg = vo.BASE
    params = vo.make_params(cfg, seed=0)
    pixels, mask = vo.synthetic_batch(cfg, 16, seed=5, mask_ratio=0.9)
    model = _model(cfg, params)
    px, mk = pixels.to(dev), mask.to(dev)
    (loss0, g0), = _grads(model, px, mk, n=1)
    bvc.use_deterministic_algorithms(True)
    try:
        (loss1, g1), = _grads(model, px, mk, n=1)
    finally:
        bvc.use_deterministic_algorithms(False)
        L.lib()
    assert loss0 == loss1
    assert float((g1 - g0).abs().max()) <= 5e-6 * float(g0.abs().max())


def test_torch_flag_alone_gives_bitwise_equal_runs():
    cfg = vo.BASE
    params = vo.make_params(cfg, seed=0)
    pixels, mask = vo.synthetic_batch(cfg, 16, seed=6, mask_ratio=0.9)
    model = _model(cfg, params)
    old = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert not bvc.are_deterministic_algorithms_enabled()
        runs = _grads(model, pixels.to(dev), mask.to(dev), n=2)
        assert L.lib().bvc_get_option(b"deterministic") == 1
    finally:
        torch.use_deterministic_algorithms(old)
        L.lib()
    assert torch.equal(runs[1][1], runs[0][1])
    assert L.lib().bvc_get_option(b"deterministic") == int(old)


@pytest.mark.parametrize("M,D,rin,rout,roff", [(20000, 384, 0, 0, 0), (64 * 1411, 384, 1411, 1568, 157), (3000, 768, 0, 0, 0)])
def test_colsum_f32_is_bitwise_reproducible(det, M, D, rin, rout, roff):
    """bvc_op_colsum_f32 - the mask-token gradient's column sum (strided rows: the masked tail of every clip)"""
    rows = (M // rin) * rout if rin > 0 else M
    X = torch.randn(rows, D, device=dev)
    out0 = torch.randn(D, device=dev)

    def run():
        out = out0.clone()
        L.check(L.lib().bvc_op_colsum_f32(G.ptr(X), rin, rout, roff, M, D, G.ptr(out), G.stream()), "colsum_f32")
        return (out,)

    (out,) = _repeat_under_load(run)
    sel = X.view(M // rin, rout, D)[:, roff:roff + rin].reshape(M, D) if rin > 0 else X
    assert float((out - (out0 + sel.double().sum(0).float())).abs().max()) < 1e-5 * math.sqrt(M)


# --------------------------------------------------------------------------- training loops, JEPA, SimCLR, parity
def _videomae_loop(cfg, params, batches):
    model = _model(cfg, params)
    model._ensure_flat(dev)
    opt = bvc.optim.SGD(model.parameters(), lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4)
    scaler = torch.amp.GradScaler("cuda")
    losses = []
    for px, mk in batches:
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model(px, bool_masked_pos=mk).loss
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    params_out = {k: v.detach().clone() for k, v in model.state_dict().items()}
    moms = [opt.state[p]["momentum_buffer"].clone() for p in model.parameters() if p in opt.state]
    return losses, params_out, moms


def test_videomae_training_loop_is_bitwise_reproducible(det):
    """the reference's loop body (pretrain_videomae.py:300-317: forward, scaler.scale(loss).backward(), fused SGD-Nesterov step,
    scaler.update) for five steps, twice from the same state and the same masks: losses, parameters and momentum bitwise equal"""
    cfg = vo.BASE
    params = vo.make_params(cfg, seed=3)
    batches = []
    for it in range(5):
        pixels, mask = vo.synthetic_batch(cfg, 8, seed=200 + it, mask_ratio=0.9)
        batches.append((pixels.to(dev), mask.to(dev)))
    la, pa, ma = _videomae_loop(cfg, params, batches)
    lb, pb, mb = _videomae_loop(cfg, params, batches)
    assert len(ma) == len(mb) > 0
    for a, b in zip(la, lb):
        assert torch.equal(a, b), (float(a), float(b))
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    for a, b in zip(ma, mb):
        assert torch.equal(a, b)
    assert float(la[-1]) < float(la[0])


def _jepa_loop(enc, pred, tgt, x, me, mp, steps):
    opt = bvc.optim.SGD([{"params": [p for p in enc.parameters() if p.requires_grad]},
                         {"params": [p for p in pred.parameters() if p.requires_grad]}], lr=0.05, momentum=0.9, nesterov=True)
    scaler = bvc.amp.GradScaler("cuda")
    losses = []
    for _ in range(steps):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            with torch.no_grad():
                h = bvc.jepa.select_targets(tgt(x), mp)
            z = pred(enc(x, me), me, mp)
            loss = bvc.jepa.smooth_l1_loss(z, h)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        opt.zero_grad()
        bvc.jepa.ema_update(enc, tgt, 0.9)
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return losses, [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in (enc, pred, tgt)]


def _assert_same_run(ra, rb):
    (la, sa), (lb, sb) = ra, rb
    for a, b in zip(la, lb):
        assert torch.equal(a, b), (float(a), float(b))
    for da, db in zip(sa, sb):
        for k in da:
            assert torch.equal(da[k], db[k]), k


def test_jepa_tiny_step_is_bitwise_reproducible(det):
    """encoder, predictor (mask-token column sum), smooth-L1, fused SGD, EMA: three steps twice from the same state"""
    from oracle import jepa_oracle as jo
    from tests.test_gpu_jepa import _modules
    cfg = jo.TINY
    enc_p = jo.make_params(jo.encoder_shapes(cfg), cfg, 26)
    pred_p = jo.make_params(jo.predictor_shapes(cfg), cfg, 27)
    imgs, m_enc, m_pred = jo.synthetic_inputs(cfg, 4, 6, 8, 4)
    x, me, mp = imgs.to(dev), [m.to(dev) for m in m_enc], [m.to(dev) for m in m_pred]
    runs = [_jepa_loop(*_modules(cfg, enc_p, pred_p, enc_p), x, me, mp, 3) for _ in range(2)]
    _assert_same_run(*runs)


def test_jepa_vit_b_step_is_bitwise_reproducible(det):
    """the same at ViT-B/16 (2 x 224^2 inputs, 8 samples, N_ctx 100, N_pred 25 x 4): two steps twice from the same state"""
    import copy
    torch.manual_seed(0)
    enc0, pred0 = bvc.jepa.get_model(dev, patch_size=16, tubelet_size=1, num_frames=2, model_name="vit_base", image_size=224)
    sd = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in (enc0, pred0)]
    B = 8
    g = torch.Generator().manual_seed(1)
    x = ((torch.randint(0, 256, (B, 2, 3, 224, 224), generator=g, dtype=torch.uint8).float() / 255 - 0.5) / 0.25).to(dev)
    me = [torch.stack([torch.sort(torch.randperm(196, generator=g)[:100]).values for _ in range(B)]).to(dev)]
    mp = [(torch.stack([torch.sort(torch.randperm(196, generator=g)[:25]).values for _ in range(B)]) + 196).to(dev) for _ in range(4)]
    runs = []
    for _ in range(2):
        enc, pred = copy.deepcopy(enc0), copy.deepcopy(pred0)
        enc.load_state_dict(sd[0])
        pred.load_state_dict(sd[1])
        tgt = copy.deepcopy(enc)
        for p in tgt.parameters():
            p.requires_grad = False
        runs.append(_jepa_loop(enc, pred, tgt, x, me, mp, 2))
    _assert_same_run(*runs)


def test_simclr_head_and_info_nce_step_is_bitwise_reproducible(det):
    """projection head (TN products with fused bias gradients) + info_nce_loss + SGD: three steps twice from the same state"""
    from functools import partial
    B, pin, pout = 256, 2048, 128
    torch.manual_seed(4)
    head = bvc.simclr.ProjectionHead(pin, pout).to(dev)     # the fc that _adapt_model_simclr installs (pretrain_simclr.py:71-77)
    sd = {k: v.detach().clone() for k, v in head.state_dict().items()}
    feats = torch.randn(2 * B, pin, device=dev)
    criterion = partial(bvc.simclr.info_nce_loss, 0.1, bvc.simclr.make_masks(B, dev))
    runs = []
    for _ in range(2):
        head.load_state_dict(sd)
        opt = torch.optim.SGD(head.parameters(), lr=0.05, momentum=0.9, nesterov=True)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = criterion(head(feats))
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        runs.append((losses, [{k: v.detach().clone() for k, v in head.state_dict().items()}]))
    _assert_same_run(*runs)


@pytest.mark.parametrize("case", ["base_b16_s0", "base_b64_s0"])
def test_transformers_fixture_parity_with_the_mode_on(det, golden_dir, case):
    """test_gpu_videomae.py's whole-step parity (loss and probes 1e-3, every per-tensor gradient norm 2e-2) with the mode on"""
    from tests.test_gpu_videomae import _check_against_transformers_fixture
    _check_against_transformers_fixture(golden_dir, case, f"{case} deterministic")
