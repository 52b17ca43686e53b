"""References for bvc.simclr.nt_xent_loss (csrc/ntxent.hip), dense torch in the dtype of their inputs: the tests pass float64 (the
reference) and float32 (the comparator of the GPU bars).  tests/test_ntxent_ref.py pins them on the CPU.

    zn_i = f_i / max(|f_i|, eps),  s_ij = zn_i . zn_j / T,  P(i) = { j != i : g_j == g_i >= 0 },  c_i = |P(i)|,
    D_i = log sum_{k != i} exp(s_ik),  l_i = D_i - (1 / c_i) sum_{j in P(i)} s_ij  (0 when c_i = 0),  loss = sum l_i / max(1, m)

  forward          l, D, c, loss, m by dense ops (differentiable: the reference gradient is autograd's);
  weighted_grad    d (sum_i w_i l_i) / d f by autograd, w_i dropped where c_i = 0;
  closed_grad      the same by the closed form the kernel implements (G, E = G + G^T, dzn = E zn / T, normalisation backward);
  scales           per output element the float64 sum of the magnitudes of its terms, and the terms A, S of eps_row;
  bf16=True        the bf16-operand model: zn rounded to bf16 wherever it enters a matrix product.
"""
import torch

EPS = 1e-8


def normalise(f, eps=EPS):
    return f / f.norm(dim=1, keepdim=True).clamp_min(eps)


def _operand(zn, bf16):
    return zn.to(torch.bfloat16).to(zn.dtype) if bf16 else zn


def positives(g):
    """bool [n][n]: j in P(i)"""
    n = g.shape[0]
    same = (g[:, None] == g[None, :]) & (g[:, None] >= 0)
    return same & ~torch.eye(n, dtype=torch.bool, device=g.device)


def forward(f, g, T, eps=EPS, bf16=False):
    """dict: row_loss [n], lse [n], npos [n] (int64), loss, m, s [n][n]"""
    n = f.shape[0]
    zn = _operand(normalise(f, eps), bf16)
    s = zn @ zn.t() / T
    eye = torch.eye(n, dtype=torch.bool, device=f.device)
    pos = positives(g)
    c = pos.sum(1)
    if n > 1:
        D = torch.logsumexp(s.masked_fill(eye, float("-inf")), dim=1)
        possum = torch.where(pos, s, torch.zeros_like(s)).sum(1)
        row = torch.where(c > 0, D - possum / c.clamp_min(1).to(f.dtype), torch.zeros_like(D))
    else:       # a single row: an empty sum (D = -inf), no positives
        D = torch.full((n,), float("-inf"), dtype=f.dtype, device=f.device)
        row = f.sum(1) * 0
    m = (c > 0).sum()
    return {"row_loss": row, "lse": D, "npos": c, "loss": row.sum() / m.clamp_min(1).to(f.dtype), "m": m, "s": s}


def mean_weights(g, gout=1.0, dtype=torch.float64):
    """w_i of the mean: gout / max(1, m) where c_i > 0, else 0"""
    c = positives(g).sum(1)
    return torch.where(c > 0, torch.full((g.shape[0],), float(gout), dtype=dtype, device=g.device) / max(1, int((c > 0).sum())),
                       torch.zeros(g.shape[0], dtype=dtype, device=g.device))


def weighted_grad(f, g, T, w, eps=EPS):
    """autograd's d (sum_i w_i l_i) / d f"""
    if f.shape[0] < 2:
        return torch.zeros_like(f)
    x = f.detach().clone().requires_grad_(True)
    out = forward(x, g, T, eps)
    (out["row_loss"] * w.to(f.dtype)).sum().backward()
    return x.grad


def closed_grad(f, g, T, w, eps=EPS, bf16=False):
    """G_ij = w_i (exp(s_ij - D_i) - [j in P(i)] / c_i), E = G + G^T, dzn = E zn / T, df = inv (dzn - zn (zn . dzn)) or dzn / eps"""
    n = f.shape[0]
    if n < 2:
        return torch.zeros_like(f)
    nrm = f.norm(dim=1, keepdim=True)
    inv = 1 / nrm.clamp_min(eps)
    zn = f * inv
    zo = _operand(zn, bf16)
    out = forward(f, g, T, eps, bf16)
    pos = positives(g)
    c = out["npos"]
    w = torch.where(c > 0, w.to(f.dtype), torch.zeros_like(out["lse"]))
    eye = torch.eye(n, dtype=torch.bool, device=f.device)
    G = w[:, None] * (torch.exp(out["s"] - out["lse"][:, None]) - pos.to(f.dtype) / c.clamp_min(1).to(f.dtype)[:, None])
    G = G.masked_fill(eye, 0.0)
    dzn = (G + G.t()) @ zo / T
    return torch.where(nrm > eps, inv * (dzn - zn * (zn * dzn).sum(1, keepdim=True)), dzn / eps)


def scales(f, g, T, w, eps=EPS):
    """float64 magnitudes of f (float64 in): dict with
    row_loss [n] = max(1, |D_i| + mean_{P(i)} |s_ij|) (the lse term carries an absolute error whatever its value: the floor of 1);
    df [n][p] = inv_i (a_id + |zn_id| sum_d |zn_id| a_id), a = (|G| + |G|^T) |zn| / T with |G|_ij = |w_i| (p_ij + [j in P(i)] / c_i);
    A [n] = max |s_ik - D_i| over k != i with exp(s_ik - D_i) >= 2^-30;  S [n] = max_{k != i} sum_d |zn_id zn_kd| / T."""
    n = f.shape[0]
    out = forward(f, g, T, eps)
    nrm = f.norm(dim=1, keepdim=True)
    inv = 1 / nrm.clamp_min(eps)
    zn = f * inv
    eye = torch.eye(n, dtype=torch.bool, device=f.device)
    pos = positives(g)
    c = out["npos"]
    cf = c.clamp_min(1).to(f.dtype)
    if n < 2:
        z = torch.zeros(n, dtype=f.dtype, device=f.device)
        return {"row_loss": z + 1, "df": torch.zeros_like(f), "A": z, "S": z}
    d = out["s"] - out["lse"][:, None]
    p = torch.exp(d).masked_fill(eye, 0.0)
    w = torch.where(c > 0, w.to(f.dtype), torch.zeros_like(out["lse"]))
    Gm = w.abs()[:, None] * (p + pos.to(f.dtype) / cf[:, None])
    a = (Gm + Gm.t()) @ zn.abs() / T
    sdf = torch.where(nrm > eps, inv * (a + zn.abs() * (zn.abs() * a).sum(1, keepdim=True)), a / eps)
    meanpos = torch.where(pos, out["s"].abs(), torch.zeros_like(d)).sum(1) / cf
    A = torch.where((p >= 2.0 ** -30) & ~eye, d.abs(), torch.zeros_like(d)).amax(1)
    S = (zn.abs() @ zn.abs().t() / T).masked_fill(eye, 0.0).amax(1)
    return {"row_loss": (out["lse"].abs() + meanpos).clamp_min(1.0), "df": sdf, "A": A, "S": S}


def eps_row(sc):
    """2^-23 (2 + A_i + S_i): a score is a sum of p products of f32 numbers, each rounded once (relative 2^-24 of sum |zn zn| / T = S,
    twice for the two roundings of the operands' normalisation), and the exponential of s - D is good to 1 ulp of its value, which
    is a relative 2^-23 of a number whose logarithm moved by 2^-24 (|s| + |D|) <= 2^-23 (A + S); 2 covers the roundings of the sum
    and of the logarithm."""
    return 2.0 ** -23 * (2 + sc["A"] + sc["S"])


def bars(ref, t32, scale, eps_rel):
    """Element bar = scale x max(4 x the worst relative-to-scale error of the comparator, eps_rel), floor 4 ulp of the reference.
    Returns (bar, worst comparator error relative to scale)."""
    from tests import rowops_ref as RR
    nz = scale > 0
    wt = float(((t32.double() - ref).abs()[nz] / scale[nz]).max()) if bool(nz.any()) else 0.0
    bar = torch.maximum(torch.maximum(torch.full_like(scale, 4 * wt), eps_rel.expand_as(scale)) * scale, 4 * RR.ulp32(ref))
    return bar, wt


# ---------------------------------------------------------------------------------------------- inputs
def random_rows(n, p, seed, device="cpu", dtype=torch.float32):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(n, p, generator=g, device=device, dtype=dtype)


def correlated_rows(n, p, seed, cos=0.99, device="cpu", dtype=torch.float32):
    """rows u + sigma e_i with 1 / (1 + sigma^2) = cos: every pair at a cosine of about `cos` (what a trunk produces early on)"""
    g = torch.Generator(device=device).manual_seed(seed)
    u = torch.randn(1, p, generator=g, device=device, dtype=dtype)
    sigma = (1.0 / cos - 1.0) ** 0.5
    return u + sigma * torch.randn(n, p, generator=g, device=device, dtype=dtype)


def masked_cross_entropy(f, T, eps=EPS):
    """SimCLR's NT-Xent of two view-major views, written as cross-entropy over the scores with the diagonal masked and the target
    (i + B) mod 2B"""
    import torch.nn.functional as F
    n = f.shape[0]
    zn = normalise(f, eps)
    s = (zn @ zn.t() / T).masked_fill(torch.eye(n, dtype=torch.bool, device=f.device), float("-inf"))
    return F.cross_entropy(s, (torch.arange(n, device=f.device) + n // 2) % n)


def supcon_l_out(f, labels, T, eps=EPS):
    """SupCon's L_out written literally (Khosla et al. 2020, eq. 2): loops over anchors and their positives"""
    zn = normalise(f, eps)
    n = f.shape[0]
    total, m = f.new_zeros(()), 0
    for i in range(n):
        P = [j for j in range(n) if j != i and int(labels[j]) == int(labels[i]) and int(labels[i]) >= 0]
        if not P:
            continue
        den = sum(torch.exp(zn[i] @ zn[a] / T) for a in range(n) if a != i)
        total = total - sum(torch.log(torch.exp(zn[i] @ zn[j] / T) / den) for j in P) / len(P)
        m += 1
    return total / max(1, m)
