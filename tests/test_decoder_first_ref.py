"""The algebra of the first decoder layer by position (stack.h LayerFirst; DESIGN.md, "First decoder layer by position"), in float64
torch on the CPU: for rows that enter a pre-LN layer as token + pos[p], the by-position formulas - S[p] = the sum of d qkv over the rows
at position p, dWqkv += T1^T S, dbqkv += colsum S, LayerNorm 1's dgamma / dbeta and d token from LN1bwd_p(S[p] Wqkv) - equal what
autograd gives for the per-row computation."""
import torch


def _ln(x, gamma, beta, eps):
    mu = x.mean(-1, keepdim=True)
    rstd = (x.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    xhat = (x - mu) * rstd
    return xhat * gamma + beta, xhat, rstd


def _ln_bwd(dy, xhat, rstd, gamma):
    g = dy * gamma
    return (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True)) * rstd


def test_by_position_backward_equals_per_row_backward():
    torch.manual_seed(0)
    dt = torch.float64
    B, Lp, nvis, ndec, D, eps = 3, 10, 3, 5, 16, 1e-6
    # per clip: nvis visible positions, ndec decoded ones, the other two neither (a decoder subset); position 0 is decoded by nobody
    dec_idx = torch.stack([(torch.randperm(Lp - 1)[:ndec] + 1).sort().values for _ in range(B)])
    token = torch.randn(D, dtype=dt, requires_grad=True)
    pos = torch.randn(Lp, D, dtype=dt)
    vis = torch.randn(B, nvis, D, dtype=dt, requires_grad=True)
    gamma = torch.randn(D, dtype=dt, requires_grad=True)
    beta = torch.randn(D, dtype=dt, requires_grad=True)
    Wqkv = torch.randn(3 * D, D, dtype=dt, requires_grad=True)
    bqkv = torch.randn(3 * D, dtype=dt, requires_grad=True)
    dqkv = torch.randn(B, nvis + ndec, 3 * D, dtype=dt)      # what attention's backward hands the layer
    dresid = torch.randn(B, nvis + ndec, D, dtype=dt)         # the residual gradient that reaches LayerNorm 1

    # per row, by autograd
    x = torch.cat([vis, token + pos[dec_idx]], dim=1)
    y, _, _ = _ln(x, gamma, beta, eps)
    qkv = y @ Wqkv.t() + bqkv
    ((qkv * dqkv).sum() + (x * dresid).sum()).backward()

    # by position
    with torch.no_grad():
        t0 = token + pos
        T1, xhat, rstd = _ln(t0, gamma, beta, eps)
        T2 = T1 @ Wqkv.t() + bqkv
        assert torch.allclose(T2[dec_idx], qkv[:, nvis:], rtol=0, atol=1e-12)
        S = torch.zeros(Lp, 3 * D, dtype=dt)
        for b in range(B):
            S.index_add_(0, dec_idx[b], dqkv[b, nvis:])
        assert bool((S[0] == 0).all())
        yv, xhat_v, rstd_v = _ln(vis, gamma, beta, eps)
        dq_v = dqkv[:, :nvis]
        dW = dq_v.reshape(-1, 3 * D).t() @ yv.reshape(-1, D) + S.t() @ T1
        db = dq_v.sum((0, 1)) + S.sum(0)
        dy_v, dy_t = dq_v @ Wqkv, S @ Wqkv
        dgamma = (dy_v * xhat_v).sum((0, 1)) + (dy_t * xhat).sum(0)
        dbeta = dy_v.sum((0, 1)) + dy_t.sum(0)
        dtoken = dresid[:, nvis:].sum((0, 1)) + _ln_bwd(dy_t, xhat, rstd, gamma).sum(0)
        dvis = dresid[:, :nvis] + _ln_bwd(dy_v, xhat_v, rstd_v, gamma)
    for name, got, want in (("dWqkv", dW, Wqkv.grad), ("dbqkv", db, bqkv.grad), ("dgamma", dgamma, gamma.grad), ("dbeta", dbeta, beta.grad),
                            ("dtoken", dtoken, token.grad), ("dvisible", dvis, vis.grad)):
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 1e-12 * max(scale, 1.0), name
