"""DINO self-distillation (Caron et al. 2021; the [CLS] half of iBOT / DINOv2 uses the same head and loss) on the fused f32
prototype cross-entropy of csrc/proto_ce.hip (include/bvc.h, bvc_op_proto_ce_fwd / _bwd).

  prototype_ce   one (teacher view, student view) pair: sum_k -softmax((t - center) / tau_t)_k log_softmax(s / tau_s)_k per row,
                 s and t the cosine scores of the rows against the student's and the teacher's prototypes.  No [m][K] array exists
                 in the forward; the backward holds two blocks of dS.
  dino_loss      the mean over all pairs (teacher view a, student view b != a) of view-major multi-crop batches.
  DINOLoss       the module of the original (buffer ``center`` [1][out_dim], teacher-temperature warm-up, momentum centre update).
  DINOHead       the projection head with the original's state-dict keys; forward returns the BOTTLENECK rows, the logits never exist.
  update_teacher the EMA of the teacher, bvc_op_ema per parameter tensor.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib, _ops

PROTO_EPS = 1e-12          # the clamp of the row norms, F.normalize's default
MAX_ROWS = 32768           # rows of one bvc_op_proto_ce call (include/bvc.h)


def _workspace(m, K, p, device, backward):
    """the backward's workspace, or the forward's: the leading part, whose size is that of the smallest block (include/bvc.h)"""
    L = _lib.lib()
    nbytes = L.bvc_op_proto_ce_workspace(m, K, p, 0, 0 if backward else 128)
    if nbytes < 0:
        raise _lib.BvcError(f"bvc_op_proto_ce_workspace: {L.bvc_last_error().decode()}")
    return torch.empty((nbytes + 15) // 16 * 4, dtype=torch.float32, device=device)


def _rows(x):
    """f32 rows with a dense last dimension, strided as they are where that is legal"""
    x = x.detach().float()
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


class _ProtoCE(torch.autograd.Function):
    """(row_loss [m], loss, batch_center [K], zero prototype rows) of bvc_op_proto_ce_fwd; the backward takes the upstream gradients
    of row_loss and loss as row weights.  The teacher side and the centre get no gradient."""

    @staticmethod
    def forward(ctx, xs, vs, xt, vt, center, tau_s, tau_t):
        a, b, c, d = _rows(xs), _rows(vs), _rows(xt), _rows(vt)
        m, p = a.shape
        K = b.shape[0]
        dev = a.device
        cen = None if center is None else center.detach().float().reshape(-1).clone()      # the module updates its buffer in place
        ws = _workspace(m, K, p, dev, False)
        row_loss = torch.empty(m, dtype=torch.float32, device=dev)
        lse_s = torch.empty(m, dtype=torch.float32, device=dev)
        lse_t = torch.empty(m, dtype=torch.float32, device=dev)
        stats = torch.empty(2, dtype=torch.float32, device=dev)
        bc = torch.empty(K, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().bvc_op_proto_ce_fwd(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0),
                                                      d.data_ptr(), d.stride(0), None if cen is None else cen.data_ptr(), m, K, p, tau_s, tau_t,
                                                      PROTO_EPS, 0, row_loss.data_ptr(), lse_s.data_ptr(), lse_t.data_ptr(), stats.data_ptr(),
                                                      bc.data_ptr(), ws.data_ptr(), _lib.current_stream_ptr()), "bvc_op_proto_ce_fwd")
        ctx.save_for_backward(a, b, c, d, lse_s, lse_t, *(() if cen is None else (cen,)))
        ctx.taus, ctx.dtypes = (tau_s, tau_t), (xs.dtype, vs.dtype)
        zero_rows = stats[1].clone()
        ctx.mark_non_differentiable(bc, zero_rows)
        return row_loss, stats[0], bc, zero_rows

    @staticmethod
    def backward(ctx, drow, dloss, _dbc, _dzero):
        a, b, c, d, lse_s, lse_t, *rest = ctx.saved_tensors
        cen = rest[0] if rest else None
        m, p = a.shape
        K = b.shape[0]
        dev = a.device
        w = (drow.detach().float() + dloss.detach().float() / m).contiguous()      # device arithmetic, no synchronisation
        ws = _workspace(m, K, p, dev, True)
        dxs = torch.empty((m, p), dtype=torch.float32, device=dev)
        dvs = torch.empty((K, p), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().bvc_op_proto_ce_bwd(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0),
                                                      d.data_ptr(), d.stride(0), None if cen is None else cen.data_ptr(), m, K, p, ctx.taus[0],
                                                      ctx.taus[1], PROTO_EPS, lse_s.data_ptr(), lse_t.data_ptr(), w.data_ptr(), 0, 0,
                                                      dxs.data_ptr(), p, dvs.data_ptr(), p, ws.data_ptr(), _lib.current_stream_ptr()),
                       "bvc_op_proto_ce_bwd")
        return dxs.to(ctx.dtypes[0]), dvs.to(ctx.dtypes[1]), None, None, None, None, None


def _check_operands(who, xs, vs, xt, vt, center):
    for name, t in (("xs", xs), ("vs", vs), ("xt", xt), ("vt", vt)):
        if not (isinstance(t, torch.Tensor) and t.dim() == 2 and t.is_floating_point()):
            raise ValueError(f"{who}: {name} must be a floating-point tensor with two dimensions")
    m, p = xs.shape
    K = vs.shape[0]
    if xt.shape != (m, p) or vs.shape[1] != p or vt.shape != (K, p):
        raise ValueError(f"{who}: xs {tuple(xs.shape)}, xt {tuple(xt.shape)}, vs {tuple(vs.shape)}, vt {tuple(vt.shape)} do not fit "
                         "(rows (m, p) twice, prototypes (K, p) twice)")
    if center is not None and center.numel() != K:
        raise ValueError(f"{who}: center holds {center.numel()} elements, not K = {K}")
    if not all(t.is_cuda for t in (xs, vs, xt, vt)) or (center is not None and not center.is_cuda):
        raise _lib.BvcError(f"{who} runs on a GPU only (libbvc_hip.so has no CPU path)")
    if len({t.device for t in (xs, vs, xt, vt)} | ({center.device} if center is not None else set())) != 1:
        raise ValueError(f"{who}: the operands must be on one device")


def prototype_ce(xs, vs, xt, vt, center=None, student_temp=0.1, teacher_temp=0.04, reduction="mean", return_zero_rows=False):
    """DINO's cross-entropy of one (teacher view, student view) pair: student rows xs (m, p) and their paired teacher rows xt (m, p)
    against the student's and the teacher's prototype weights vs, vt (K, p), the ``weight_v`` of a DINOHead's last layer:
    l_i = sum_k -softmax((xtn_i . wtn_k - center_k) / teacher_temp)_k log_softmax(xsn_i . wsn_k / student_temp)_k, rows and prototypes
    L2-normalised (a prototype row of norm 0 scores 0 and receives no gradient).  "mean" averages the rows, "none" returns l [m].

    Gradients go to xs and vs, in their dtypes; xt, vt and center are detached.  Any floating dtype, computed in f32; rows with a
    dense last dimension are read as they are.  Nothing here synchronises the stream.

    return_zero_rows=True also returns the op's device flag: a 0-dim f32 tensor, the number of rows of vs plus the number of rows of
    vt whose norm is exactly 0.  Reading it synchronises; look at it where the step synchronises anyway (when the loss is logged)."""
    _check_operands("prototype_ce", xs, vs, xt, vt, center)
    if reduction not in ("mean", "none"):
        raise ValueError(f"prototype_ce: reduction {reduction!r} is neither 'mean' nor 'none'")
    row_loss, loss, _, zero_rows = _ProtoCE.apply(xs, vs, xt, vt, center, float(student_temp), float(teacher_temp))
    out = loss if reduction == "mean" else row_loss
    return (out, zero_rows) if return_zero_rows else out


def view_pairs(student_views, teacher_views=2):
    """[(a, b)]: teacher view a against student view b != a, in the order of the original's double loop"""
    return [(a, b) for a in range(teacher_views) for b in range(student_views) if b != a]


def dino_loss(student, teacher, vs, vt, center=None, student_temp=0.1, teacher_temp=0.04, student_views=2, teacher_views=2,
              return_center=False):
    """DINO's loss over multi-crop batches: student (student_views * B, p) and teacher (teacher_views * B, p) bottleneck rows, both
    view-major (rows [v B, (v + 1) B) are view v: what ClipAugment(views=...) returns); the first teacher_views student views are the
    teacher's views.  The mean over all pairs (teacher view a, student view b != a) of prototype_ce.

    The paired operands are built from slices and torch.cat alone, so a student row's gradients from its pairs are added in a fixed
    order and the step stays bit-reproducible.  All pairs go through ONE call of the op (chunks of whole pairs beyond 32768 rows),
    which fills its 128-row tiles better than one call per pair.  With local crops each pair recomputes its teacher product; at the
    batch sizes of this project that is cheap (the product is K x p per row either way), and a three-product kernel that shares it
    is not built.  return_center=True returns (loss, batch_center [K], zero_rows): the mean raw teacher score per prototype over the
    teacher's views and rows, and the op's device count of zero prototype rows (see prototype_ce)."""
    total, bc_total, zero_rows = None, None, None
    for xs, xt, share in paired_rows(student, teacher, student_views, teacher_views):
        _check_operands("dino_loss", xs, vs, xt, vt, center)
        _, loss, bc, zero_rows = _ProtoCE.apply(xs, vs, xt, vt, center, float(student_temp), float(teacher_temp))
        total = loss * share if total is None else total + loss * share
        bc_total = bc * share if bc_total is None else bc_total + bc * share
    return (total, bc_total, zero_rows) if return_center else total


def paired_rows(student, teacher, student_views, teacher_views=2, max_rows=MAX_ROWS):
    """[(xs, xt, share)]: the rows of all pairs of dino_loss, stacked pair after pair by slices and torch.cat, in chunks of whole
    pairs of at most max_rows rows; share = the chunk's fraction of the pairs (the weight of its mean in the mean over pairs)"""
    student_views, teacher_views = int(student_views), int(teacher_views)
    if teacher_views < 1 or student_views < teacher_views or student_views * teacher_views - teacher_views < 1:
        raise ValueError(f"dino_loss: {student_views} student views and {teacher_views} teacher views give no pair")
    if teacher.dim() != 2 or student.dim() != 2 or teacher.shape[0] % teacher_views:
        raise ValueError("dino_loss: student and teacher must be (views * B, p) rows")
    B = teacher.shape[0] // teacher_views
    if B < 1 or student.shape[0] != student_views * B:
        raise ValueError(f"dino_loss: {student.shape[0]} student rows are not {student_views} views of {B} samples")
    teacher = teacher.detach()
    pairs = view_pairs(student_views, teacher_views)
    per_call = max(1, max_rows // B)
    out = []
    for i in range(0, len(pairs), per_call):
        chunk = pairs[i:i + per_call]
        out.append((torch.cat([student[b * B:(b + 1) * B] for _, b in chunk]), torch.cat([teacher[a * B:(a + 1) * B] for a, _ in chunk]),
                    len(chunk) / len(pairs)))
    return out


class DINOLoss(nn.Module):
    """The loss module of the original (main_dino.py DINOLoss): the buffer ``center`` [1][out_dim] (a DINO checkpoint's loss state
    loads), the linear teacher-temperature warm-up indexed by epoch, and the momentum update of the centre."""

    def __init__(self, out_dim, student_views, warmup_teacher_temp=0.04, teacher_temp=0.04, warmup_teacher_temp_epochs=0, nepochs=1,
                 student_temp=0.1, center_momentum=0.9, teacher_views=2):
        super().__init__()
        self.student_temp, self.center_momentum = float(student_temp), float(center_momentum)
        self.student_views, self.teacher_views = int(student_views), int(teacher_views)
        self.register_buffer("center", torch.zeros(1, out_dim))
        # of the last forward: the op's device count of prototype rows of norm 0 in either head (0-dim tensor; reading it synchronises)
        self.zero_prototype_rows = None
        self.teacher_temp_schedule = np.concatenate((np.linspace(warmup_teacher_temp, teacher_temp, warmup_teacher_temp_epochs),
                                                     np.ones(max(0, nepochs - warmup_teacher_temp_epochs)) * teacher_temp))

    @staticmethod
    def _prototypes(head):
        return head if isinstance(head, torch.Tensor) else head.last_layer.weight_v

    def forward(self, student, teacher, student_head, teacher_head, epoch):
        """student, teacher: the bottleneck rows the two heads returned; student_head, teacher_head: the DINOHeads (or their
        last_layer.weight_v).  Returns the loss and moves the centre; neither synchronises."""
        temp = float(self.teacher_temp_schedule[epoch])
        loss, bc, self.zero_prototype_rows = dino_loss(student, teacher, self._prototypes(student_head), self._prototypes(teacher_head),
                                                       self.center, self.student_temp, temp, self.student_views, self.teacher_views,
                                                       return_center=True)
        self.update_center(bc)
        return loss

    @torch.no_grad()
    def update_center(self, batch_center):
        """center = center * momentum + mean over ranks of batch_center * (1 - momentum)"""
        from .distributed import AllReduce
        bc = AllReduce.apply(batch_center.reshape(1, -1))
        self.center.mul_(self.center_momentum).add_(bc * (1.0 - self.center_momentum))


# ---------------------------------------------------------------------------------------------- the head
class _MLP(torch.autograd.Function):
    """Linear -> GELU -> ... -> Linear on the bf16 GEMM: hidden layers with the GELU epilogue (which stores gelu' for the backward),
    the last layer with f32 output; backward with DGELU, weight gradients with the bias gradient as their row sum."""

    @staticmethod
    def forward(ctx, x, *params):
        n = x.shape[0]
        E = _ops.EPI
        ws = [_ops.cast_bf16(w.detach()) for w in params[0::2]]
        bs = [b.detach().float() for b in params[1::2]]
        acts, grads = [_ops.cast_bf16(x.detach())], []
        for w, b in zip(ws[:-1], bs[:-1]):
            h = torch.empty((n, w.shape[0]), dtype=torch.bfloat16, device=x.device)
            dh = torch.empty_like(h)
            _ops.gemm(_ops.gemm_desc(acts[-1], w, n, w.shape[0], w.shape[1], E["GELU"], dh, C2=h, bias=b), _ops.NT)
            acts.append(h)
            grads.append(dh)
        out = torch.empty((n, ws[-1].shape[0]), dtype=torch.float32, device=x.device)
        _ops.gemm(_ops.gemm_desc(acts[-1], ws[-1], n, ws[-1].shape[0], ws[-1].shape[1], E["F32"], out, bias=bs[-1]), _ops.NT)
        ctx.save_for_backward(*ws, *acts, *grads)
        ctx.nl, ctx.x_dtype = len(ws), x.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        nl = ctx.nl
        saved = ctx.saved_tensors
        ws, acts, grads = saved[:nl], saved[nl:2 * nl], saved[2 * nl:]
        n = acts[0].shape[0]
        dev = acts[0].device
        E = _ops.EPI
        d = _ops.cast_bf16(dout)
        out = [None] * (2 * nl)
        for l in range(nl - 1, -1, -1):
            po, pi = ws[l].shape
            dw = torch.empty((po, pi), dtype=torch.float32, device=dev)
            db = torch.zeros(po, dtype=torch.float32, device=dev)
            _ops.gemm(_ops.gemm_desc(d, acts[l], po, pi, n, E["F32"], dw, rowsum=db), _ops.TN)
            out[2 * l], out[2 * l + 1] = dw, db
            if l > 0:
                dh = torch.empty((n, pi), dtype=torch.bfloat16, device=dev)
                _ops.gemm(_ops.gemm_desc(d, ws[l], n, pi, po, E["DGELU"], dh, aux=grads[l - 1]), _ops.NN)
                d = dh
            else:
                dx = torch.empty((n, pi), dtype=torch.float32, device=dev)
                _ops.gemm(_ops.gemm_desc(d, ws[l], n, pi, po, E["F32"], dx), _ops.NN)
        return (dx.to(ctx.x_dtype), *out)


class _Linear(nn.Module):
    """weight / bias holder with nn.Linear's parameter names"""

    def __init__(self, pin, pout):
        super().__init__()
        self.weight = nn.Parameter(nn.init.trunc_normal_(torch.empty(pout, pin), std=0.02))
        self.bias = nn.Parameter(torch.zeros(pout))


class _Prototypes(nn.Module):
    """The weight-normalised last layer of the original (nn.utils.weight_norm(nn.Linear(bottleneck_dim, out_dim, bias=False))) with
    the gain frozen at one (norm_last_layer=True): weight_g [out_dim][1] of ones, weight_v [out_dim][bottleneck_dim]."""

    def __init__(self, pin, pout):
        super().__init__()
        self.weight_g = nn.Parameter(torch.ones(pout, 1), requires_grad=False)
        self.weight_v = nn.Parameter(nn.Linear(pin, pout, bias=False).weight.detach().clone())

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        g = state_dict.get(prefix + "weight_g")
        if g is not None and not bool((g == 1).all()):
            raise ValueError(f"DINOHead: {prefix}weight_g is not all ones; a learnable gain of the last layer (norm_last_layer=False) "
                             "is not implemented")
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class DINOHead(nn.Module):
    """The DINO projection head with the original's state-dict keys: mlp.0.*, mlp.2.*, mlp.4.* (nlayers=3; ``mlp.weight`` / ``mlp.bias``
    for nlayers=1), last_layer.weight_g, last_layer.weight_v.  Truncated-normal weights of std 0.02 and zero biases in the MLP.

    forward(x) returns the BOTTLENECK rows (m, bottleneck_dim), f32: the loss normalises them and scores them against
    ``last_layer.weight_v`` itself (prototype_ce, dino_loss, DINOLoss), so the (m, out_dim) logits never exist.  The MLP runs on the
    library's bf16 GEMM with the GELU / DGELU epilogues; every width must be a multiple of 64."""

    def __init__(self, in_dim, out_dim, nlayers=3, hidden_dim=2048, bottleneck_dim=256):
        super().__init__()
        nlayers = max(int(nlayers), 1)
        widths = [in_dim] + [hidden_dim] * (nlayers - 1) + [bottleneck_dim]
        if any(w % 64 for w in widths):
            raise ValueError(f"DINOHead: the widths {widths} must be multiples of 64")
        self.nlayers = nlayers
        if nlayers == 1:
            self.mlp = _Linear(in_dim, bottleneck_dim)
        else:
            self.mlp = nn.Module()
            for i in range(nlayers):
                self.mlp.add_module(str(2 * i), _Linear(widths[i], widths[i + 1]))
        self.last_layer = _Prototypes(bottleneck_dim, out_dim)

    def _linears(self):
        return [self.mlp] if self.nlayers == 1 else [self.mlp._modules[str(2 * i)] for i in range(self.nlayers)]

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.BvcError("DINOHead runs on a GPU only (libbvc_hip.so has no CPU path)")
        params = [t for lin in self._linears() for t in (lin.weight, lin.bias)]
        if x.shape[-1] != params[0].shape[1]:
            raise ValueError(f"DINOHead: input width {x.shape[-1]} is not in_dim {params[0].shape[1]}")
        return _MLP.apply(x.reshape(-1, x.shape[-1]), *params)


@torch.no_grad()
def update_teacher(student_module, teacher_module, m):
    """teacher = teacher * m + student * (1 - m), bvc_op_ema per parameter tensor (jepa.ema_update does the same in one launch for a
    pair of flat encoders, and is used where both modules are such): the head's loose parameters follow the trunk."""
    if hasattr(student_module, "flat_parameters") and hasattr(teacher_module, "flat_parameters"):
        from .jepa import ema_update
        return ema_update(student_module, teacher_module, m)
    ps, pt = list(student_module.parameters()), list(teacher_module.parameters())
    if len(ps) != len(pt):
        raise ValueError(f"update_teacher: {len(ps)} student and {len(pt)} teacher parameter tensors")
    L, st = _lib.lib(), None
    for q, k in zip(ps, pt):
        if q.shape != k.shape or q.dtype != torch.float32 or k.dtype != torch.float32 or not (q.is_contiguous() and k.is_contiguous()):
            raise ValueError("update_teacher: the parameters must be contiguous f32 tensors of equal shapes")
        if not (q.is_cuda and k.is_cuda):
            raise _lib.BvcError("update_teacher runs on a GPU only (libbvc_hip.so has no CPU path)")
        with torch.cuda.device(k.device):
            st = _lib.current_stream_ptr()
            _lib.check(L.bvc_op_ema(k.data_ptr(), q.data_ptr(), k.numel(), float(m), st), "bvc_op_ema")
    if hasattr(teacher_module, "_shadow_invalidate"):
        teacher_module._shadow_invalidate()
