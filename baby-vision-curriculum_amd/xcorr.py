"""Feature cross-correlation with a reduced epilogue (csrc/xcorr.hip, include/bvc.h: bvc_op_xcorr_fwd / _bwd).

  cross_correlation(x, y)   (on, off, var_x, var_y) of C = scale xh^T yh without ever storing C; differentiable in all four
  linear_cka(x, y)          |xc^T yc|_F^2 / (|xc^T xc|_F |yc^T yc|_F): how alike two sets of embeddings of the same n inputs are

Barlow Twins and VICReg (bvc.simclr.barlow_twins_loss / vicreg_loss) are parameter settings of cross_correlation.  Everything is
computed in f32 on the f32-input MFMA whatever the dtype of the features; nothing here synchronises the stream.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _workspace(n, p, q, alias, backward, device):
    L = _lib.lib()
    nbytes = L.bvc_op_xcorr_workspace(n, p, q, int(alias), 0, int(backward))
    if nbytes < 0:
        raise _lib.BvcError(f"bvc_op_xcorr_workspace: {L.bvc_last_error().decode()}")
    return torch.empty((nbytes + 15) // 16 * 4, dtype=torch.float32, device=device)


def _f32_rows(t):
    """f32 rows with unit column stride; a padded row stride is taken as it is"""
    f = t.detach().float()
    if f.stride(1) != 1 or f.stride(0) < f.shape[1]:
        f = f.contiguous()
    return f


class _XCorr(torch.autograd.Function):
    """(on, off, var_x[, var_y]) of bvc_op_xcorr_fwd; y None is the alias case.  The upstream gradients of on / off travel as the
    device vector w, those of the variances as dvar_*."""

    @staticmethod
    def forward(ctx, x, y, norm, ddof, eps, scale, target):
        xf = _f32_rows(x)
        alias = y is None
        yf = xf if alias else _f32_rows(y)
        if not alias and yf.data_ptr() == xf.data_ptr():
            # another tensor over x's storage (x.detach(), a view, a column slice): the library tells the alias case by the pointer,
            # but here y is an operand of its own with a gradient of its own, so it gets memory of its own
            yf = yf.clone()
        n, p = xf.shape
        q = yf.shape[1]
        dev = xf.device
        ws = _workspace(n, p, q, alias, False, dev)
        mean_x, var_x = torch.empty(p, dtype=torch.float32, device=dev), torch.empty(p, dtype=torch.float32, device=dev)
        mean_y = var_y = None
        if not alias:
            mean_y, var_y = torch.empty(q, dtype=torch.float32, device=dev), torch.empty(q, dtype=torch.float32, device=dev)
        stats = torch.empty(2, dtype=torch.float32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().bvc_op_xcorr_fwd(xf.data_ptr(), xf.stride(0), yf.data_ptr(), yf.stride(0), n, p, q, norm, ddof, eps, scale,
                                                   target, mean_x.data_ptr(), var_x.data_ptr(), ptr(mean_y), ptr(var_y), stats.data_ptr(),
                                                   ws.data_ptr(), _lib.current_stream_ptr()), "bvc_op_xcorr_fwd")
        ctx.save_for_backward(xf, mean_x, var_x, *(() if alias else (yf, mean_y, var_y)))
        ctx.cfg = (norm, ddof, eps, scale, target)
        ctx.dtypes = (x.dtype, None if alias else y.dtype)
        if alias:
            return stats[0], stats[1], var_x
        return stats[0], stats[1], var_x, var_y

    @staticmethod
    @once_differentiable
    def backward(ctx, don, doff, dvar_x, dvar_y=None):
        xf, mean_x, var_x, *rest = ctx.saved_tensors
        alias = not rest
        yf, mean_y, var_y = (xf, None, None) if alias else rest
        norm, ddof, eps, scale, target = ctx.cfg
        n, p = xf.shape
        q = yf.shape[1]
        dev = xf.device
        w = torch.stack([don.detach().float().reshape(()), doff.detach().float().reshape(())]).contiguous()
        dvx = dvar_x.detach().float().contiguous()
        dvy = None if alias else dvar_y.detach().float().contiguous()
        ws = _workspace(n, p, q, alias, True, dev)
        dx = torch.empty((n, p), dtype=torch.float32, device=dev)
        dy = None if alias else torch.empty((n, q), dtype=torch.float32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().bvc_op_xcorr_bwd(xf.data_ptr(), xf.stride(0), yf.data_ptr(), yf.stride(0), n, p, q, norm, ddof, eps, scale,
                                                   target, mean_x.data_ptr(), var_x.data_ptr(), ptr(mean_y), ptr(var_y), w.data_ptr(),
                                                   dvx.data_ptr(), ptr(dvy), 0, dx.data_ptr(), p, ptr(dy), q, ws.data_ptr(),
                                                   _lib.current_stream_ptr()), "bvc_op_xcorr_bwd")
        return dx.to(ctx.dtypes[0]), None if alias else dy.to(ctx.dtypes[1]), None, None, None, None, None


def _check_features(who, x, y):
    for name, t in (("x", x), ("y", y)):
        if t is None:
            continue
        if not (isinstance(t, torch.Tensor) and t.dim() == 2 and t.is_floating_point()):
            raise ValueError(f"{who}: {name} must be a floating-point tensor (n, width)")
        if not t.is_cuda:
            raise _lib.BvcError(f"{who} runs on a GPU only (libbvc_hip.so has no CPU path)")
    if y is not None and (y.shape[0] != x.shape[0] or y.device != x.device):
        raise ValueError(f"{who}: x and y must have the same number of rows and live on the same device")


def cross_correlation(x, y=None, norm=1, ddof=0, eps=1e-5, scale=None, diag_target=1.0):
    """(on, off, var_x, var_y) of the columns of x (n, p) and y (n, q); y=None (or y is x) is the auto-covariance of x, where
    var_y is var_x.  Any other tensor over x's memory (x.detach(), a view, a column slice) is an operand of its own.  Per column:
    centred (norm=0) or standardised with 1 / sqrt(var + eps) (norm=1), var = sum (x - mean)^2 / (n - ddof).  C = scale xh^T yh (scale=None: 1 / n), on = sum_i (C_ii - diag_target)^2, off = sum_{i != j} C_ij^2; C is never stored.
    Computed in f32 whatever the dtype; the gradients come back in the inputs' dtypes."""
    _check_features("cross_correlation", x, y)
    if y is x:
        y = None
    n = x.shape[0]
    scale = 1.0 / n if scale is None else float(scale)
    if y is None:
        on, off, var_x = _XCorr.apply(x, None, int(norm), int(ddof), float(eps), scale, float(diag_target))
        return on, off, var_x, var_x
    return _XCorr.apply(x, y, int(norm), int(ddof), float(eps), scale, float(diag_target))


def linear_cka(x, y):
    """Linear centred kernel alignment (Kornblith et al. 2019) of two sets of embeddings of the same n inputs, x (n, p) and y (n, q):
    |xc^T yc|_F^2 / (|xc^T xc|_F |yc^T yc|_F) with centred columns; 1 for y = x, invariant under orthogonal maps and isotropic
    rescaling of either argument.  Forward only; three calls of the op, combined on the device: a 0-dim f32 tensor."""
    _check_features("linear_cka", x, y)
    with torch.no_grad():
        def frob2(a, b):
            on, off, _, _ = cross_correlation(a, b, norm=0, ddof=0, scale=1.0, diag_target=0.0)
            return on + off
        return frob2(x, y) / torch.sqrt(frob2(x, None) * frob2(y, None))
