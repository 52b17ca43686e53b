"""The attention kernels of csrc/attention.hip (through the C ABI) at every shape their dispatch distinguishes, held per ROW to a
multiple of the error of the project's own rounding model, with neighbours that must not leak and memory that must not be touched.

Reference, model, metric, inputs and the guarded arena: tests/attention_ref.py (pinned on the CPU by tests/test_attention_ref.py).
Every operand and output of every launch here is carved from an `Arena`: NaN-reading guard bands on both sides of each, outputs
pre-filled with NaN, and every test ends with `Arena.check()` and a no-NaN check of what the kernels wrote.

What each N reaches (128-row blocks of four 32-row waves; `tail_split` by the rows left in the last block; the whole-head backward
`attn_bwd_head_kernel<64, NBT>` for width 64 up to N = 160, NBT = 0 up to 128 and 5 above; every other width and length runs
attn_bwd_dq_kernel + attn_bwd_dkdv_kernel):
    1 7 16 31 32   one block, gs = 4, partial MFMA row / key groups below 32          head<64,0>
    33 64          one block, gs = 2                                                    head<64,0>
    65 96          one block, three owning waves                                        head<64,0>
    97 127         one block, four owning waves (127: ragged)                           head<64,0>
    128            one full block, no tail                                              head<64,0>
    129            full block + gs = 4 with ONE row                                     head<64,5>
    159 160        full block + gs = 4 (31 / 32 rows)                                   head<64,5>
    161 172        full block + gs = 2; the hand-over to the two-kernel form            dq + dkdv
    200 224        full block + three owning waves                                      dq + dkdv
    255            full block + four owning waves, ragged                               dq + dkdv
    256 384        two / three full blocks, no tail                                     dq + dkdv
    257            two full blocks + gs = 4 with one row                                dq + dkdv
    864            six full blocks + three owning waves (96 rows): the decode-subset step's decoder length; 172 is its other one
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():   # collected on the CPU box, run on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import attention_ref as R   # noqa: E402
from tests import gpu_util as G   # noqa: E402

L = G.L
dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32

WIDTHS = [32, 64, 80, 88, 96, 128]
NS = [1, 7, 16, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, 159, 160, 161, 172, 200, 224, 255, 256, 257, 384, 864]
STARRED = [32, 97, 128, 160, 172, 200, 256, 864]      # these also run sharp, shift and headscale
CASES = [(N, kind) for N in NS for kind in (R.KINDS if N in STARRED else R.KINDS[:1])]
ROW_BAR = 2.5      # x the model's worst row of the same case and tensor
GRADS = ("dq", "dk", "dv")


def _path(HD, N):
    """(backward kernel, tail regime) the launchers of csrc/attention.hip pick - for the report only."""
    bwd = "dq+dkdv" if HD != 64 or N > 160 else "head<64,5>" if N > 128 else "head<64,0>"
    rows = N - (N - 1) // 128 * 128
    tail = "none" if rows == 128 else "gs=4" if rows <= 32 else "gs=2" if rows <= 64 else "3 waves" if rows <= 96 else "4 waves"
    return bwd, f"{(N + 127) // 128} blk, tail {rows}: {tail}"


def _whole_head(HD, N):
    return HD == 64 and N <= 160      # attn_bwd_head_kernel: leaves `delta` untouched


def _arena(B, N, H, HD):
    D = H * HD
    # bands as wide as 192 rows of the widest array: a whole 128-row block (or the whole-head kernel's 192-row image) of rows
    # past the last clip stays inside the arena, whichever array it is computed from
    return R.Arena(dev, guard=192 * 3 * D * 2, qkv=((B * N, 3 * D), BF), dctx=((B * N, D), BF), ctx=((B * N, D), BF), lse=((B * H, N), F32),
                   delta=((B * H, N), F32), dqkv=((B * N, 3 * D), BF))


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _fwd(A, B, N, H, HD, scale=None):
    a = (G.ptr(A["qkv"]), G.ptr(A["ctx"]), G.ptr(A["lse"]), B, N, H, HD)
    if scale is None:
        L.check(L.lib().bvc_op_attention_fwd(*a, G.stream()), "attention_fwd")
    else:
        L.check(L.lib().bvc_op_attention_fwd_scaled(*a, scale, G.stream()), "attention_fwd_scaled")


def _bwd(A, B, N, H, HD, scale=None, part=None):
    a = (G.ptr(A["qkv"]), G.ptr(A["ctx"]), G.ptr(A["dctx"]), G.ptr(A["lse"]), G.ptr(A["delta"]), G.ptr(A["dqkv"]), B, N, H, HD)
    if part is not None:
        L.check(L.lib().bvc_op_attention_bwd_part(*a, part, G.stream()), "attention_bwd_part")
    elif scale is None:
        L.check(L.lib().bvc_op_attention_bwd(*a, G.stream()), "attention_bwd")
    else:
        L.check(L.lib().bvc_op_attention_bwd_scaled(*a, scale, G.stream()), "attention_bwd_scaled")


OUTS = ("ctx", "lse", "delta", "dqkv")


def _run(A, B, N, H, HD, scale=None, parts=False):
    """Outputs to NaN, forward, backward; returns copies of the four outputs."""
    for n in OUTS:
        A[n].fill_(float("nan"))
    _fwd(A, B, N, H, HD, scale)
    if parts:
        _bwd(A, B, N, H, HD, part=1)
        _bwd(A, B, N, H, HD, part=2)
    else:
        _bwd(A, B, N, H, HD, scale)
    torch.cuda.synchronize()
    return {n: A[n].clone() for n in OUTS}


def _finish(A, out, HD, N):
    """What every test ends with: no guard band touched, no NaN in what the kernels wrote."""
    A.check()
    for n in OUTS:
        if n == "delta" and _whole_head(HD, N):
            continue
        assert not torch.isnan(out[n].float()).any(), f"NaN left in {n}"


def _split_out(out, B, N, H, HD):
    D = H * HD
    g = out["dqkv"].float()
    return dict(ctx=out["ctx"].float(), dq=g[:, :D], dk=g[:, D:2 * D], dv=g[:, 2 * D:])


def _one_key_bound(qkv, dctx, B, H, HD):
    """N = 1: softmax over one key is 1, so dS = P (dP - delta) is EXACTLY zero and so are dq and dk - a relative error does not
    exist.  What a correct kernel may leave is the f32 round-off of dP - delta: both are sums of the same HD products do_i v_i
    (o = v exactly), each sum off by at most HD roundings of 2^-24 relative to sum |do_i v_i|, doubled for the MFMA's block-wise
    alignment of its addends; dS = that x scale (bf16), and dq = dS k, dk = dS q (bf16: 1 + 2^-7).  Returns the bound on the norm
    of each (clip, head)'s single dq and dk row, [B][H]."""
    x = qkv.double().view(B, 3, H, HD)
    ds = 4 * HD * 2.0 ** -24 * (dctx.double().view(B, H, HD) * x[:, 2]).abs().sum(-1) * HD ** -0.5
    return dict(dq=ds * x[:, 1].norm(dim=-1) * (1 + 2.0 ** -7), dk=ds * x[:, 0].norm(dim=-1) * (1 + 2.0 ** -7))


def _parity(out, qkv, dctx, B, N, H, HD, label):
    """The whole-tensor bars of tests/test_gpu_ops.py, the lse bar of test_attention_sharp_softmax, and the per-row bar: every
    figure is printed and logged before anything is asserted."""
    ref = dict(zip(("ctx", "lse", "dq", "dk", "dv"), R.reference(qkv, dctx, B, N, H, HD)))
    mod = dict(zip(("ctx", "lse", "dq", "dk", "dv"), R.model(qkv, dctx, B, N, H, HD)))
    got = _split_out(out, B, N, H, HD)
    hv = lambda t: R.heads(t, B, N, H, HD)      # noqa: E731
    lse_err = float(((out["lse"].double() - ref["lse"]).abs() / ref["lse"].abs().clamp(min=1)).max())
    rows, fails = [], []
    for name in ("ctx",) + GRADS:
        if N == 1 and name in ("dq", "dk"):
            assert float(ref[name].abs().max()) == 0.0
            bound = _one_key_bound(qkv, dctx, B, H, HD)[name]
            worst = float((hv(got[name]).double().norm(dim=-1)[:, :, 0] / bound).max())
            rows.append(f"{name} exact-zero reference, |got| / round-off bound {worst:.2f}")
            if not worst <= 1.0:
                fails.append(f"{name}: |got| is {worst:.2f} x the round-off bound of a zero gradient")
            continue
        whole = R.whole_err(got[name], ref[name])
        k_row, k_at = R.row_err(hv(got[name]), hv(ref[name]))
        m_row, _ = R.row_err(hv(mod[name]), hv(ref[name]))
        ratio = k_row / m_row if m_row > 0 else (0.0 if k_row == 0 else float("inf"))
        rows.append(f"{name} whole {whole:.2e} row {k_row:.2e} / model {m_row:.2e} = {ratio:.2f} at {k_at}")
        if not whole < (1e-2 if name == "ctx" else 2e-2):
            fails.append(f"{name}: whole-tensor {whole:.3e}")
        # (an exactly right tensor has no error to hold against the model's: N = 1, where ctx = v and dv = dO to the bit)
        if not (k_row < ROW_BAR * m_row or k_row == 0.0):
            fails.append(f"{name}: worst row {k_row:.3e} at (clip, head, row) {k_at} is {ratio:.2f} x the model's {m_row:.3e}")
    bwd, tail = _path(HD, N)
    G.log_parity(f"attn_edges d{HD} N{N} B{B} H{H} {label} [{bwd}; {tail}]: lse {lse_err:.1e}; " + "; ".join(rows))
    if not lse_err < 1e-3:
        fails.append(f"lse: {lse_err:.3e}")
    assert not fails, (HD, N, label, fails)


# --------------------------------------------------------------------------- parity grid
@pytest.mark.parametrize("N,kind", CASES, ids=[f"N{n}-{k}" for n, k in CASES])
@pytest.mark.parametrize("HD", WIDTHS)
def test_attention_edge_parity(HD, N, kind):
    B, H = 3, 3      # the middle clip and the middle head have neighbours on both sides
    qkv, dctx = (t.to(dev) for t in R.inputs(kind, B, N, H, HD, seed=7919 * HD + 31 * N + R.KINDS.index(kind)))
    A = _arena(B, N, H, HD)
    A["qkv"].copy_(qkv), A["dctx"].copy_(dctx)
    first = _run(A, B, N, H, HD)
    second = _run(A, B, N, H, HD)
    for n in OUTS:
        assert _same_bits(first[n], second[n]), f"{n} differs between two launches"
    _parity(first, qkv, dctx, B, N, H, HD, kind)
    assert _same_bits(A["qkv"], qkv) and _same_bits(A["dctx"], dctx)      # operands untouched
    _finish(A, first, HD, N)


# --------------------------------------------------------------------------- neighbour invariance
def _perturbed(qkv, dctx, B, N, H, HD, b0, h0):
    """Every row of the other clips and every column of the other heads x 64 (exact in bf16, finite); (b0, h0) untouched."""
    f = torch.full((B, 1, 1, H, 1), 64.0, device=qkv.device)
    f[b0, 0, 0, h0, 0] = 1.0
    q2 = (qkv.float().view(B, N, 3, H, HD) * f).reshape(qkv.shape).to(BF)
    d2 = (dctx.float().view(B, N, 1, H, HD) * f).reshape(dctx.shape).to(BF)
    assert torch.isfinite(q2.float()).all() and torch.isfinite(d2.float()).all()
    return q2, d2


def _target(out, B, N, H, HD, b0, h0):
    """The (b0, h0) part of every output."""
    D = H * HD
    r = slice(b0 * N, (b0 + 1) * N)
    t = dict(ctx=out["ctx"][r, h0 * HD:(h0 + 1) * HD], lse=out["lse"][b0 * H + h0])
    for i, n in enumerate(GRADS):
        t[n] = out["dqkv"][r, i * D + h0 * HD:i * D + (h0 + 1) * HD]
    if not _whole_head(HD, N):
        t["delta"] = out["delta"][b0 * H + h0]
    return t


def _check_invariance(A, qkv, dctx, base, B, N, H, HD, b0, h0):
    q2, d2 = _perturbed(qkv, dctx, B, N, H, HD, b0, h0)
    A["qkv"].copy_(q2), A["dctx"].copy_(d2)
    pert = _run(A, B, N, H, HD)
    want, got = _target(base, B, N, H, HD, b0, h0), _target(pert, B, N, H, HD, b0, h0)
    bad = [n for n in want if not _same_bits(want[n].contiguous(), got[n].contiguous())]
    assert not bad, f"(clip {b0}, head {h0}) of {bad} changed with its neighbours' values (d{HD}, N{N})"
    return pert


@pytest.mark.parametrize("N", [33, 97, 129, 160, 200, 257])
@pytest.mark.parametrize("HD", WIDTHS)
def test_attention_result_depends_on_its_own_clip_and_head_only(HD, N):
    """Rows past a clip's end are masked, not diluted; the 16 / 8 columns of the next head inside the 96-wide image of an 80 / 88
    head, and the whole-head kernel's prefetch of the next head's images and statistics, never reach a result: scaling every
    other clip and head by 64 leaves the middle (clip, head)'s ctx, lse, dq, dk, dv (and delta) bit-identical."""
    B, H = 3, 3
    qkv, dctx = (t.to(dev) for t in R.inputs("gauss", B, N, H, HD, seed=104729 + 7919 * HD + N))
    A = _arena(B, N, H, HD)
    A["qkv"].copy_(qkv), A["dctx"].copy_(dctx)
    base = _run(A, B, N, H, HD)
    pert = _check_invariance(A, qkv, dctx, base, B, N, H, HD, 1, 1)
    _finish(A, base, HD, N)
    _finish(A, pert, HD, N)


# --------------------------------------------------------------------------- persistent whole-head loop
@pytest.mark.parametrize("B,H,target", [(20, 13, 257), (5, 1, None)])
def test_attention_whole_head_loop_every_head(B, H, target):
    """attn_bwd_head_kernel is persistent: one workgroup per CU walks (clip, head) pairs blockIdx.x, + gridDim.x, ...  260 pairs on
    256 CUs give four workgroups a second round (next head's images and statistics fetched under the first one's phase 2); five
    pairs leave most of the chip without work.  Every (clip, head) is held to the per-row bar - the worst row is taken over all
    of them - and head 257, one of the second round, must not see its neighbours."""
    HD, N = 64, 97
    qkv, dctx = (t.to(dev) for t in R.inputs("gauss", B, N, H, HD, seed=4242 + B))
    A = _arena(B, N, H, HD)
    A["qkv"].copy_(qkv), A["dctx"].copy_(dctx)
    base = _run(A, B, N, H, HD)
    _parity(base, qkv, dctx, B, N, H, HD, f"gauss whole-head loop of {B * H}")
    _finish(A, base, HD, N)
    if target is not None:
        pert = _check_invariance(A, qkv, dctx, base, B, N, H, HD, target // H, target % H)
        _finish(A, pert, HD, N)


# --------------------------------------------------------------------------- small equalities
@pytest.mark.parametrize("HD,N", [(64, 161), (64, 864), (96, 129)])
def test_attention_backward_parts_give_the_bits_of_the_whole(HD, N):
    """bvc_op_attention_bwd_part 1 (dQ, delta) then 2 (dK, dV) = bvc_op_attention_bwd, bit for bit."""
    B, H = 3, 3
    qkv, dctx = (t.to(dev) for t in R.inputs("gauss", B, N, H, HD, seed=555 + HD + N))
    A = _arena(B, N, H, HD)
    A["qkv"].copy_(qkv), A["dctx"].copy_(dctx)
    whole = _run(A, B, N, H, HD)
    parts = _run(A, B, N, H, HD, parts=True)
    for n in OUTS:
        assert _same_bits(whole[n], parts[n]), n
    _finish(A, whole, HD, N)
    _finish(A, parts, HD, N)


@pytest.mark.parametrize("HD,N", [(32, 129), (64, 129), (64, 161), (80, 129), (88, 129), (96, 129), (128, 129)])
def test_attention_scaled_entry_points_give_the_bits_of_the_plain_ones(HD, N):
    """softmax_scale = 1 / sqrt(head_dim) evaluated in float32, as the launchers do for softmax_scale = 0."""
    B, H = 3, 3
    scale = float(np.float32(1.0) / np.sqrt(np.float32(HD)))
    assert scale == float(np.float32(scale)) and abs(scale - 1 / math.sqrt(HD)) < 1e-7
    qkv, dctx = (t.to(dev) for t in R.inputs("gauss", B, N, H, HD, seed=777 + HD + N))
    A = _arena(B, N, H, HD)
    A["qkv"].copy_(qkv), A["dctx"].copy_(dctx)
    plain = _run(A, B, N, H, HD)
    scaled = _run(A, B, N, H, HD, scale=scale)
    for n in OUTS:
        if n == "delta" and _whole_head(HD, N):
            continue
        assert _same_bits(plain[n], scaled[n]), n
    _finish(A, plain, HD, N)
    _finish(A, scaled, HD, N)
