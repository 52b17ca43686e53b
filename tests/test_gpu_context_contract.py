"""What every model context promises its caller, straight through the C ABI (include/bvc.h): the size of the bf16 shadow, a vouch for
it that holds for exactly one forward, the forward / backward state machine with its refusals, and an identity token list that is
ready whichever stream the first forward runs on.

Everything is compared bit for bit (torch.equal) between contexts of one build, in deterministic mode; nothing here needs an oracle.

The vouch case scales "the parameters" by 1.5 behind the library's back.  A forward reads the weight matrices of its products through
the bf16 shadow and everything else (biases, LayerNorm weights, positions, the mask token) from the f32 buffer itself, so only the
matrices are scaled: then the forward after a vouch equals the one before the change exactly if and only if it used the stale shadow.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():   # collected on the CPU box, run on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import gpu_util as G   # noqa: E402
from oracle import jepa_oracle as jo   # noqa: E402
from oracle import videomae_oracle as vo   # noqa: E402

L = G.L
dev = "cuda"
B = 2
NC, NP, NSETS = 7, 5, 2     # the golden spec of the JEPA fixtures


@pytest.fixture(autouse=True)
def det():
    G.bvc.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        G.bvc.use_deterministic_algorithms(False)


def _last_error():
    return L.lib().bvc_last_error().decode()


def _table(prefix, cfg):
    """[(name, offset, numel, ndim)] of a flat layout, through bvc_<prefix>_param_count / _param_info."""
    lib = L.lib()
    out = []
    for i in range(getattr(lib, f"bvc_{prefix}_param_count")(ctypes.byref(cfg))):
        name = ctypes.create_string_buffer(256)
        off, n, nd, shape = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(), (ctypes.c_int64 * 5)()
        L.check(getattr(lib, f"bvc_{prefix}_param_info")(ctypes.byref(cfg), i, name, 256, ctypes.byref(off), ctypes.byref(n), ctypes.byref(nd), shape))
        out.append((name.value.decode(), off.value, n.value, nd.value))
    return out


class Ctx:
    """One training context over the C ABI: `prefix` names its entry points, `numel` is the length of its flat parameter buffer."""
    prefix = table_prefix = None

    def __init__(self, max_batch=B):
        self.max_batch = max_batch
        self.h = ctypes.c_void_p()
        L.check(self.create(max_batch), f"{self.prefix}_create")

    def __del__(self):
        if getattr(self, "h", None):
            getattr(L.lib(), f"bvc_{self.prefix}_destroy")(self.h)

    def params(self):
        g = torch.Generator().manual_seed(3)
        return (torch.randn(self.numel, generator=g) * 0.05).to(dev)

    def scale_matrices(self, p, factor):
        for name, off, n, nd in _table(self.table_prefix, self.cfg):
            if nd >= 2 and name.endswith("weight") and off < self.numel:
                p[off:off + n] *= factor

    def shadow(self, valid):
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        L.check(getattr(L.lib(), f"bvc_{self.prefix}_shadow")(self.h, valid, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def step(self, p):
        """forward + backward: every output and every gradient buffer"""
        rc, outs = self.forward(p)
        L.check(rc, "forward")
        rc, grads = self.backward()
        L.check(rc, "backward")
        torch.cuda.synchronize()
        return outs + grads


def _videomae_cfg():
    c = L.VideoMAEConfigC()
    for name, _ in c._fields_:
        setattr(c, name, type(getattr(c, name))(getattr(vo.TINY, name)))
    return c


class VideoMAEInputs:
    cfg = _videomae_cfg()
    table_prefix = "videomae"
    pixels, mask = vo.synthetic_batch(vo.TINY, B, seed=0, mask_ratio=0.75)
    nmask = int(mask[0].sum())
    seq = mask.shape[1]
    patch = vo.TINY.num_channels * vo.TINY.tubelet_size * vo.TINY.patch_size ** 2
    D = vo.TINY.hidden_size

    def clips(self, batch):
        reps = -(-batch // B)
        return self.pixels.repeat(reps, 1, 1, 1, 1)[:batch].contiguous().to(dev), self.mask.repeat(reps, 1)[:batch].contiguous().to(torch.uint8).to(dev)


class Pretrain(VideoMAEInputs, Ctx):
    prefix = "videomae"
    numel = L.lib().bvc_videomae_param_numel(ctypes.byref(VideoMAEInputs.cfg))

    def create(self, max_batch):
        return L.lib().bvc_videomae_create(ctypes.byref(self.cfg), max_batch, self.nmask, ctypes.byref(self.h))

    def forward(self, p, batch=B):
        px, mask = self.clips(batch)
        loss, logits = torch.zeros(1, device=dev), torch.zeros(batch * self.nmask, self.patch, device=dev)
        rc = L.lib().bvc_videomae_forward(self.h, G.ptr(px), G.ptr(mask), batch, G.ptr(p), G.ptr(loss), G.ptr(logits), G.stream())
        return rc, [loss, logits]

    def backward(self):
        grads, one = torch.empty(self.numel, device=dev), torch.ones(1, device=dev)
        return L.lib().bvc_videomae_backward(self.h, G.ptr(one), G.ptr(grads), L.BUCKET_FN(), None, G.stream()), [grads]


class Finetune(VideoMAEInputs, Ctx):
    prefix = "videomae_cls"
    numel = L.lib().bvc_videomae_encoder_param_numel(ctypes.byref(VideoMAEInputs.cfg))

    def create(self, max_batch):
        return L.lib().bvc_videomae_cls_create(ctypes.byref(self.cfg), max_batch, ctypes.byref(self.h))

    def fc_norm(self):
        g = torch.Generator().manual_seed(4)
        return (1 + 0.1 * torch.randn(self.D, generator=g)).to(dev), (0.1 * torch.randn(self.D, generator=g)).to(dev)

    def forward(self, p, batch=B):
        px, _ = self.clips(batch)
        w, b = self.fc_norm()
        pooled, tokens = torch.zeros(batch, self.D, device=dev), torch.zeros(batch * self.seq, self.D, device=dev)
        rc = L.lib().bvc_videomae_cls_forward_px(self.h, G.ptr(px), None, batch, G.ptr(p), G.ptr(w), G.ptr(b), 1e-12, G.ptr(pooled), G.ptr(tokens),
                                                 G.stream())
        return rc, [pooled, tokens]

    def backward(self):
        g = torch.Generator().manual_seed(5)
        dpooled = torch.randn(B, self.D, generator=g).to(dev)
        grads, dw, db = torch.empty(self.numel, device=dev), torch.empty(self.D, device=dev), torch.empty(self.D, device=dev)
        rc = L.lib().bvc_videomae_cls_backward(self.h, G.ptr(dpooled), G.ptr(grads), G.ptr(dw), G.ptr(db), L.BUCKET_FN(), None, G.stream())
        return rc, [grads, dw, db]


class JepaInputs:
    j = jo.TINY
    imgs, (ctx_idx,), pred_idx = jo.synthetic_inputs(j, B, 0, NC, NP, NSETS)
    D = j.embed_dim


class Vit(JepaInputs, Ctx):
    prefix = table_prefix = "vit"
    j = JepaInputs.j
    cfg = L.VitConfigC(j.image_size, j.patch_size, j.in_chans, j.num_frames, j.tubelet_size, j.embed_dim, j.depth, j.num_heads,
                       int(j.embed_dim * j.mlp_ratio), j.eps)
    numel = L.lib().bvc_vit_param_numel(ctypes.byref(cfg))

    def create(self, max_batch):
        return L.lib().bvc_vit_create(ctypes.byref(self.cfg), max_batch, ctypes.byref(self.h))

    def forward(self, p, batch=B):
        reps = -(-batch // B)
        imgs = self.imgs.repeat(reps, 1, 1, 1, 1)[:batch].contiguous().to(dev)
        idx = self.ctx_idx.repeat(reps, 1)[:batch].to(torch.int32).contiguous().to(dev)
        out = torch.zeros(batch * NC, self.D, device=dev)
        return L.lib().bvc_vit_forward(self.h, G.ptr(imgs), G.ptr(idx), batch, NC, G.ptr(p), G.ptr(out), G.stream()), [out]

    def backward(self):
        g = torch.Generator().manual_seed(5)
        dout, grads = torch.randn(B * NC, self.D, generator=g).to(dev), torch.empty(self.numel, device=dev)
        return L.lib().bvc_vit_backward(self.h, G.ptr(dout), G.ptr(grads), L.BUCKET_FN(), None, G.stream()), [grads]


class Predictor(JepaInputs, Ctx):
    prefix = table_prefix = "predictor"
    j = JepaInputs.j
    cfg = L.PredictorConfigC(j.seq_len, j.embed_dim, j.pred_dim, j.pred_depth, j.num_heads, int(j.pred_dim * j.mlp_ratio), j.eps)
    numel = L.lib().bvc_predictor_param_numel(ctypes.byref(cfg))

    def create(self, max_batch):
        return L.lib().bvc_predictor_create(ctypes.byref(self.cfg), max_batch, NSETS, NC + NP, ctypes.byref(self.h))

    def forward(self, p, batch=B):
        reps = -(-batch // B)
        g = torch.Generator().manual_seed(6)
        z = torch.randn(batch * NC, self.D, generator=g).to(dev)
        ic = self.ctx_idx.repeat(reps, 1)[:batch].to(torch.int32).contiguous().to(dev)
        ip = torch.stack([m.repeat(reps, 1)[:batch] for m in self.pred_idx]).to(torch.int32).contiguous().to(dev)
        out = torch.zeros(NSETS * batch * NP, self.D, device=dev)
        rc = L.lib().bvc_predictor_forward(self.h, G.ptr(z), G.ptr(ic), G.ptr(ip), batch, NC, NSETS, NP, G.ptr(p), G.ptr(out), G.stream())
        return rc, [out]

    def backward(self):
        g = torch.Generator().manual_seed(5)
        dout = torch.randn(NSETS * B * NP, self.D, generator=g).to(dev)
        grads, dz = torch.empty(self.numel, device=dev), torch.empty(B * NC, self.D, device=dev)
        return L.lib().bvc_predictor_backward(self.h, G.ptr(dout), G.ptr(grads), G.ptr(dz), G.stream()), [grads, dz]


TRAINING = [Pretrain, Finetune, Vit, Predictor]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", TRAINING)
def test_shadow_holds_the_parameters_the_context_reads(kind):
    c = kind()
    p, n = c.shadow(-1)
    assert p and n == kind.numel > 0


@pytest.mark.parametrize("kind", TRAINING)
def test_a_vouch_is_consumed_by_exactly_one_forward(kind):
    c = kind()
    p = c.params()
    rc, f0 = c.forward(p)
    L.check(rc, "forward")
    torch.cuda.synchronize()
    c.scale_matrices(p, 1.5)
    c.shadow(1)
    rc, f1 = c.forward(p)
    L.check(rc, "forward")
    rc, f2 = c.forward(p)
    L.check(rc, "forward")
    other = kind()
    rc, fresh = other.forward(p)
    L.check(rc, "forward")
    torch.cuda.synchronize()
    assert _same(f1, f0), "the forward after a vouch did not use the stale shadow"
    assert not any(torch.equal(x, y) for x, y in zip(f2, f0)), "the vouch outlived one forward"
    assert _same(f2, fresh)


def _encode(h, px, p):
    batch = px.shape[0]
    pooled, tokens = torch.zeros(batch, VideoMAEInputs.D, device=dev), torch.zeros(batch * VideoMAEInputs.seq, VideoMAEInputs.D, device=dev)
    L.check(L.lib().bvc_videomae_encode(h, G.ptr(px), batch, G.ptr(p), None, None, 0.0, G.ptr(tokens), G.ptr(pooled), G.stream()), "encode")
    return [pooled, tokens]


class Inference(VideoMAEInputs, Ctx):
    prefix = "videomae_encoder"
    numel = Finetune.numel

    def create(self, max_batch):
        return L.lib().bvc_videomae_encoder_create(ctypes.byref(self.cfg), max_batch, ctypes.byref(self.h))

    def forward(self, p, batch=B):
        return 0, _encode(self.h, self.clips(batch)[0], p)


def test_the_inference_context_always_casts():
    c = Inference()
    p = c.params()
    _, f0 = c.forward(p)
    torch.cuda.synchronize()
    c.scale_matrices(p, 1.5)
    _, f1 = c.forward(p)
    other = Inference()
    _, fresh = other.forward(p)
    torch.cuda.synchronize()
    assert not any(torch.equal(x, y) for x, y in zip(f1, f0))
    assert _same(f1, fresh)


@pytest.mark.parametrize("kind", TRAINING)
def test_state_machine_refusals_leave_the_context_usable(kind):
    ref = kind()
    p = ref.params()
    want = ref.step(p)
    c = kind()

    def usable():
        assert _same(c.step(p), want)

    rc, _ = c.backward()                        # before any forward
    assert rc != 0 and "no forward state" in _last_error()
    usable()
    rc, _ = c.backward()                        # a second backward after one forward
    assert rc != 0 and "no forward state" in _last_error()
    usable()
    rc, _ = c.forward(p, batch=c.max_batch + 1)
    assert rc != 0 and f"[1, {c.max_batch}]" in _last_error(), _last_error()
    usable()


@pytest.mark.parametrize("kind", [Inference, Finetune])
def test_identity_list_is_ready_for_a_first_forward_on_any_stream(kind):
    p = kind().params()
    _, want = kind().forward(p)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                  # non-blocking: it does not wait for work on the null stream
    with torch.cuda.stream(side):
        c = kind()                              # the list is filled on the null stream at creation
        _, got = c.forward(p)
    torch.cuda.synchronize()
    assert _same(got, want)
