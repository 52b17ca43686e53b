"""Dense torch references of the feature cross-correlation op (csrc/xcorr.hip), in the dtype of their inputs: float64 is the
reference, float32 the comparator (as tests/ntxent_ref.py).  cfg = (norm, ddof, eps, scale, t); y=None is the alias case.

    mu_j = mean_i x_ij,  var_j = sum_i (x_ij - mu_j)^2 / (n - ddof),  r_j = norm ? 1 / sqrt(var_j + eps) : 1,  xh = (x - mu) r
    C = scale xh^T yh,  on = sum_i (C_ii - t)^2,  off = sum_{i != j} C_ij^2
"""
import torch

F64 = torch.float64
BARLOW = lambda n: (1, 0, 1e-5, 1.0 / n, 1.0)           # noqa: E731
VICREG = lambda n: (0, 1, 0.0, 1.0 / (n - 1), 0.0)      # noqa: E731
CKA = (0, 0, 0.0, 1.0, 0.0)


def centre(x, norm, ddof, eps):
    n = x.shape[0]
    mu = x.mean(0)
    xc = x - mu
    var = (xc * xc).sum(0) / (n - ddof)
    r = 1.0 / torch.sqrt(var + eps) if norm else torch.ones_like(var)
    return mu, var, r, xc * r


def _eye(p, q, device):
    return torch.eye(p, q, dtype=torch.bool, device=device)


def forward(x, y, cfg):
    norm, ddof, eps, scale, t = cfg
    mx, vx, rx, xh = centre(x, norm, ddof, eps)
    my, vy, ry, yh = (mx, vx, rx, xh) if y is None else centre(y, norm, ddof, eps)
    C = scale * (xh.t() @ yh)
    eye = _eye(*C.shape, x.device)
    on = ((C - t)[eye] ** 2).sum()
    off = (C.masked_fill(eye, 0.0) ** 2).sum()
    return {"mean_x": mx, "var_x": vx, "mean_y": my, "var_y": vy, "rx": rx, "ry": ry, "xh": xh, "yh": yh, "C": C, "on": on, "off": off}


def autograd_grad(x, y, cfg, w_on, w_off, dvar_x=None, dvar_y=None):
    """(dx, dy) of w_on on + w_off off + dvar_x . var_x + dvar_y . var_y by autograd; dy None in the alias case (dx is the whole gradient)"""
    xa = x.detach().clone().requires_grad_(True)
    ya = None if y is None else y.detach().clone().requires_grad_(True)
    o = forward(xa, ya, cfg)
    L = w_on * o["on"] + w_off * o["off"]
    if dvar_x is not None:
        L = L + (dvar_x.to(x.dtype) * o["var_x"]).sum()
    if dvar_y is not None and y is not None:
        L = L + (dvar_y.to(x.dtype) * o["var_y"]).sum()
    L.backward()
    return xa.grad, None if ya is None else ya.grad


def _g(C, t, w_on, w_off):
    eye = _eye(*C.shape, C.device)
    return torch.where(eye, 2 * w_on * (C - t), 2 * w_off * C)


def _dx(x, mu, r, xh, dxh, dvar, norm, ddof):
    n = x.shape[0]
    a = torch.zeros_like(mu) if dvar is None else dvar.to(x.dtype).clone()
    if norm:
        a = a - 0.5 * r * r * (dxh * xh).sum(0)
    return r * (dxh - dxh.mean(0)) + 2 * (x - mu) * a / (n - ddof)


def closed_grad(x, y, cfg, w_on, w_off, dvar_x=None, dvar_y=None):
    """The formulas of the kernel's backward (include/bvc.h)"""
    norm, ddof, eps, scale, t = cfg
    o = forward(x, y, cfg)
    G = _g(o["C"], t, w_on, w_off)
    if y is None:
        return _dx(x, o["mean_x"], o["rx"], o["xh"], scale * o["xh"] @ (G + G.t()), dvar_x, norm, ddof), None
    dx = _dx(x, o["mean_x"], o["rx"], o["xh"], scale * o["yh"] @ G.t(), dvar_x, norm, ddof)
    dy = _dx(y, o["mean_y"], o["ry"], o["yh"], scale * o["xh"] @ G, dvar_y, norm, ddof)
    return dx, dy


def scales(x, y, cfg, w_on, w_off, dvar_x=None, dvar_y=None):
    """Per output element, the float64 sum of the magnitudes of its terms: Cabs = scale |xh|^T |yh|; on: sum (Cabs_ii + |t|)^2;
    off: sum Cabs_ij^2; dx: the backward's formulas with every term replaced by its magnitude."""
    norm, ddof, eps, scale, t = cfg
    x = x.double()
    y = None if y is None else y.double()
    n = x.shape[0]
    o = forward(x, y, cfg)
    axh, ayh = o["xh"].abs(), o["yh"].abs()
    Cabs = scale * (axh.t() @ ayh)
    eye = _eye(*Cabs.shape, x.device)
    Gabs = torch.where(eye, 2 * abs(w_on) * (Cabs + abs(t)), 2 * abs(w_off) * Cabs)

    def sdx(xx, mu, r, ah, dxh_abs, dvar):
        a = torch.zeros_like(mu) if dvar is None else dvar.double().abs()
        if norm:
            a = a + 0.5 * r * r * (dxh_abs * ah).sum(0)
        return r * (dxh_abs + dxh_abs.mean(0)) + 2 * (xx - mu).abs() * a / (n - ddof)

    out = {"on": ((Cabs + abs(t))[eye] ** 2).sum(), "off": (Cabs.masked_fill(eye, 0.0) ** 2).sum()}
    if y is None:
        out["dx"] = sdx(x, o["mean_x"], o["rx"], axh, scale * axh @ (Gabs + Gabs.t()), dvar_x)
        out["dy"] = None
    else:
        out["dx"] = sdx(x, o["mean_x"], o["rx"], axh, scale * ayh @ Gabs.t(), dvar_x)
        out["dy"] = sdx(y, o["mean_y"], o["ry"], ayh, scale * axh @ Gabs, dvar_y)
    return out


def eps_stats(n):
    """Rounding bound of on / off relative to their scale.  An element of xh carries the rounding of the centring (1), of r
    (var, + eps, sqrt, reciprocal: 4) and of the scaling (1): 6 per operand, 12 per product; the chain of n fused multiply-adds
    adds n, the multiplication by `scale` 1: |dC_ab| <= 2^-24 (n + 13) Cabs_ab, rounded up to 2^-24 (n + 16).  The square doubles the
    relative error and rounds once more (the subtraction of t is covered by |t| in the scale): 2^-24 (2 n + 34).  The sums are float64."""
    return 2.0 ** -24 * (2 * n + 34)


def eps_grad(n, width):
    """Rounding bound of dx / dy relative to their scale: G inherits C's 2^-24 (n + 16) and two roundings of its own, dxh is a chain
    over the `width` columns of the other operand with xh's 6 on each term, and the column sums (float64), the centring of dxh, r
    and the variance path add fewer than 16: 2^-24 (n + width + 48)."""
    return 2.0 ** -24 * (n + width + 48)


def bars(ref, t32, scale, eps_rel):
    """Element bar = scale x max(4 x the worst relative-to-scale error of the comparator, eps_rel), floor 4 ulp of the reference.
    Returns (bar, worst comparator error relative to scale)."""
    from tests import rowops_ref as RR
    ref, scale = ref.double(), scale.double()
    nz = scale > 0
    wt = float(((t32.double() - ref).abs()[nz] / scale[nz]).max()) if bool(nz.any()) else 0.0
    bar = torch.maximum(scale * max(4 * wt, eps_rel), 4 * RR.ulp32(ref))
    return bar, wt


# ---------------------------------------------------------------------------------------------- CKA
def linear_cka(x, y):
    xc, yc = x - x.mean(0), y - y.mean(0)
    return ((xc.t() @ yc) ** 2).sum() / torch.sqrt(((xc.t() @ xc) ** 2).sum() * ((yc.t() @ yc) ** 2).sum())


def gram_cka(x, y):
    """HSIC form over the [n][n] Gram matrices (Kornblith et al. 2019, eq. 3 and 4)"""
    n = x.shape[0]
    H = torch.eye(n, dtype=x.dtype, device=x.device) - 1.0 / n
    K, Lm = H @ (x @ x.t()) @ H, H @ (y @ y.t()) @ H
    return (K * Lm).sum() / torch.sqrt((K * K).sum() * (Lm * Lm).sum())


# ---------------------------------------------------------------------------------------------- losses
def barlow_twins(z1, z2, lambd=5e-3, eps=1e-5):
    o = forward(z1, z2, (1, 0, eps, 1.0 / z1.shape[0], 1.0))
    return o["on"] + lambd * o["off"]


def vicreg(x, y, sim=25.0, std=25.0, cov=1.0, eps=1e-4):
    n, p = x.shape
    ox, oy = forward(x, None, VICREG(n)), forward(y, None, VICREG(n))
    inv = ((x - y) ** 2).mean()
    v = torch.relu(1 - torch.sqrt(ox["var_x"] + eps)).mean() / 2 + torch.relu(1 - torch.sqrt(oy["var_x"] + eps)).mean() / 2
    return sim * inv + std * v + cov * (ox["off"] / p + oy["off"] / p)


# ---------------------------------------------------------------------------------------------- inputs
def random_cols(n, p, seed, device="cpu", dtype=torch.float32):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(n, p, generator=g, device=device, dtype=dtype)


def offset_cols(n, p, seed, mean=100.0, device="cpu", dtype=torch.float32):
    """columns with mean 100 and standard deviation 1: the centring cancels two digits"""
    return random_cols(n, p, seed, device, dtype) + mean


def correlated_cols(n, p, seed, rho=0.99, device="cpu", dtype=torch.float32):
    """columns u + sigma e_j with 1 / (1 + sigma^2) = rho: every pair of columns at a correlation of about rho"""
    g = torch.Generator(device=device).manual_seed(seed)
    u = torch.randn(n, 1, generator=g, device=device, dtype=dtype)
    sigma = (1.0 / rho - 1.0) ** 0.5
    return u + sigma * torch.randn(n, p, generator=g, device=device, dtype=dtype)
