"""References for bvc.dino.prototype_ce (csrc/proto_ce.hip), dense torch in the dtype of their inputs: the tests pass float64 (the
reference) and float32 (the comparator of the GPU bars).  tests/test_proto_ce_ref.py pins them on the CPU.

    xsn_i = xs_i / max(|xs_i|, eps),  wsn_k = vs_k / |vs_k| (0 for a zero row),  xtn, wtn likewise,
    s_ik = xsn_i . wsn_k / tau_s,  t_ik = (xtn_i . wtn_k - center_k) / tau_t,
    Ls_i = log sum_k exp(s_ik),  Lt_i = log sum_k exp(t_ik),  q_ik = exp(t_ik - Lt_i),
    l_i = Ls_i - sum_k q_ik s_ik,  loss = sum_i l_i / m,  bc_k = (1 / m) sum_i xtn_i . wtn_k

  forward          l, Ls, Lt, loss, bc by dense ops (differentiable in xs and vs: the reference gradient is autograd's);
  weighted_grad    d (sum_i w_i l_i) / d (xs, vs) by autograd;
  closed_grad      the same by the closed forms the kernels implement;
  scales           per output element the float64 sum of the magnitudes of its terms, and the terms of eps_row;
  online           l, Ls, Lt by the five-number recurrence of the forward kernel over any tile order and split;
  bf16=True        the bf16-operand model: the four normalised operands rounded to bf16 wherever they enter a matrix product;
  dino_double_loop, center_update_original, DinoLossRef, mlp_forward: the original's loss module and head, restated.
"""
import torch

EPS = 1e-12


def _operand(z, bf16):
    return z.to(torch.bfloat16).to(z.dtype) if bf16 else z


def normalise_rows(x, eps=EPS):
    return x / x.norm(dim=1, keepdim=True).clamp_min(eps)


def normalise_protos(v):
    """v_k / |v_k|, 0 for a zero row (no direction; the op refuses it by a flag and scores it 0)"""
    n = v.norm(dim=1, keepdim=True)
    return torch.where(n > 0, v / n.clamp_min(torch.finfo(v.dtype).tiny), torch.zeros_like(v))


def forward(xs, vs, xt, vt, center, tau_s, tau_t, eps=EPS, bf16=False):
    """dict: row_loss, lse_s, lse_t [m], loss, batch_center [K], zero_protos, s, t, q [m][K]"""
    xsn, xtn = _operand(normalise_rows(xs, eps), bf16), _operand(normalise_rows(xt, eps), bf16)
    wsn, wtn = _operand(normalise_protos(vs), bf16), _operand(normalise_protos(vt), bf16)
    c = torch.zeros(vs.shape[0], dtype=xs.dtype, device=xs.device) if center is None else center.reshape(-1).to(xs.dtype)
    raw_t = xtn @ wtn.t()
    s = xsn @ wsn.t() / tau_s
    t = (raw_t - c) / tau_t
    Ls, Lt = torch.logsumexp(s, dim=1), torch.logsumexp(t, dim=1)
    q = torch.exp(t - Lt[:, None])
    row = Ls - (q * s).sum(1)
    zero = int((vs.norm(dim=1) == 0).sum()) + int((vt.norm(dim=1) == 0).sum())
    return {"row_loss": row, "lse_s": Ls, "lse_t": Lt, "loss": row.sum() / xs.shape[0], "batch_center": raw_t.mean(0),
            "zero_protos": zero, "s": s, "t": t, "q": q}


def weighted_grad(xs, vs, xt, vt, center, tau_s, tau_t, w, eps=EPS):
    """autograd's d (sum_i w_i l_i) / d xs, d vs; the teacher side is constant"""
    x = xs.detach().clone().requires_grad_(True)
    v = vs.detach().clone().requires_grad_(True)
    out = forward(x, v, xt.detach(), vt.detach(), None if center is None else center.detach(), tau_s, tau_t, eps)
    (out["row_loss"] * w.to(xs.dtype)).sum().backward()
    return x.grad, v.grad


def closed_grad(xs, vs, xt, vt, center, tau_s, tau_t, w, eps=EPS, bf16=False):
    """dS = w (exp(s - Ls) - q) / tau_s, dxsn = dS wsn, dwsn = dS^T xsn, then the two normalisations backwards"""
    out = forward(xs, vs, xt, vt, center, tau_s, tau_t, eps, bf16)
    nx = xs.norm(dim=1, keepdim=True)
    nv = vs.norm(dim=1, keepdim=True)
    invx = 1 / nx.clamp_min(eps)
    xsn, wsn = xs * invx, normalise_protos(vs)
    dS = w.to(xs.dtype)[:, None] * (torch.exp(out["s"] - out["lse_s"][:, None]) - out["q"]) / tau_s
    dxsn = dS @ _operand(wsn, bf16)
    dwsn = dS.t() @ _operand(xsn, bf16)
    dxs = torch.where(nx > eps, invx * (dxsn - xsn * (xsn * dxsn).sum(1, keepdim=True)), dxsn / eps)
    invv = torch.where(nv > 0, 1 / nv.clamp_min(torch.finfo(vs.dtype).tiny), torch.zeros_like(nv))
    dvs = invv * (dwsn - wsn * (wsn * dwsn).sum(1, keepdim=True))
    return dxs, dvs


def scales(xs, vs, xt, vt, center, tau_s, tau_t, w, eps=EPS):
    """float64 magnitudes (float64 in): dict with
    row_loss [m] = max(1, |Ls_i| + sum_k q_ik |s_ik|) (the lse term carries an absolute error whatever its value: the floor of 1);
    dxs [m][p] = inv_i (a_id + |xsn_id| sum_d |xsn_id| a_id), a = |dS| |wsn| with |dS|_ik = |w_i| (exp(s_ik - Ls_i) + q_ik) / tau_s
    (a / eps where the clamp is active);  dvs [K][p] likewise with a = |dS|^T |xsn|;
    batch_center [K] = 2 + mean_i sum_d |xtn_id wtn_kd|;
    As, At [m] = max |s_ik - Ls_i|, max |t_ik - Lt_i| over the terms whose softmax weight is >= 2^-30;
    Ss, St [m] = max_k sum_d |xsn_id wsn_kd| / tau_s, max_k (sum_d |xtn_id wtn_kd| + |center_k|) / tau_t."""
    out = forward(xs, vs, xt, vt, center, tau_s, tau_t, eps)
    nx, nv = xs.norm(dim=1, keepdim=True), vs.norm(dim=1, keepdim=True)
    invx = 1 / nx.clamp_min(eps)
    xsn, wsn = (xs * invx).abs(), normalise_protos(vs).abs()
    xtn, wtn = normalise_rows(xt, eps).abs(), normalise_protos(vt).abs()
    c = torch.zeros(vs.shape[0], dtype=xs.dtype, device=xs.device) if center is None else center.reshape(-1).to(xs.dtype).abs()
    ds, dt = out["s"] - out["lse_s"][:, None], out["t"] - out["lse_t"][:, None]
    ps = torch.exp(ds)
    dSm = w.to(xs.dtype).abs()[:, None] * (ps + out["q"]) / tau_s
    ax, av = dSm @ wsn, dSm.t() @ xsn
    sdx = torch.where(nx > eps, invx * (ax + xsn * (xsn * ax).sum(1, keepdim=True)), ax / eps)
    invv = torch.where(nv > 0, 1 / nv.clamp_min(torch.finfo(vs.dtype).tiny), torch.zeros_like(nv))
    sdv = invv * (av + wsn * (wsn * av).sum(1, keepdim=True))
    zero = torch.zeros_like(ds)
    return {"row_loss": (out["lse_s"].abs() + (out["q"] * out["s"].abs()).sum(1)).clamp_min(1.0), "dxs": sdx, "dvs": sdv,
            "batch_center": 2 + xtn.mean(0) @ wtn.t(),
            "As": torch.where(ps >= 2.0 ** -30, ds.abs(), zero).amax(1), "At": torch.where(out["q"] >= 2.0 ** -30, dt.abs(), zero).amax(1),
            "Ss": (xsn @ wsn.t() / tau_s).amax(1), "St": ((xtn @ wtn.t() + c) / tau_t).amax(1)}


def eps_row(sc):
    """2^-23 (2 + As_i + Ss_i + At_i + St_i).  A score is a chain of p f32 products: its error is at most 2^-24 per rounding of
    sum_d |x_id w_kd| / tau <= S (2^-23 S with the roundings of the two normalised operands; the centre's subtraction and the
    division by tau_t are inside St).  exp(s - L) of a 1-ulp hardware exponential is off by a relative 2^-23 plus the error of its
    argument, 2^-24 |s - L| <= 2^-23 A for the subtraction and the score error above.  The row loss Ls_i - sum_k q_ik s_ik carries the
    student's share through Ls_i and s_ik and the teacher's through q_ik, whose sum against |s_ik| is inside the element's scale; the
    2 covers the roundings of the sums and of the logarithm.  1 / tau_s and 1 / tau_t stand where NT-Xent has 1 / T."""
    return 2.0 ** -23 * (2 + sc["As"] + sc["Ss"] + sc["At"] + sc["St"])


def bars(ref, t32, scale, eps_rel):
    """Element bar = scale x max(4 x the worst relative-to-scale error of the comparator, eps_rel), floor 4 ulp of the reference.
    Returns (bar, worst comparator error relative to scale)."""
    from tests import ntxent_ref
    return ntxent_ref.bars(ref, t32, scale, eps_rel)


# ---------------------------------------------------------------------------------------------- the forward kernel's recurrence
def online(s, t, tile_order, splits, tile=128, lanes=4):
    """l, Ls, Lt of score rows s, t [m][K] by the kernel's scheme: the tiles of K, visited in tile_order, are cut into `splits`
    contiguous ranges; within a tile every one of `lanes` lanes owns an interleaved share of the columns and keeps
    (max_s, sum_s, max_t, sum_t, a = sum exp(t - max_t) s), rescaled when a maximum moves; lanes, then splits, are merged in
    ascending order.  Empty ranges are legal."""
    m, K = s.shape
    ninf = torch.full((m,), float("-inf"), dtype=s.dtype)

    def empty():
        return [ninf.clone(), torch.zeros(m, dtype=s.dtype), ninf.clone(), torch.zeros(m, dtype=s.dtype), torch.zeros(m, dtype=s.dtype)]

    def scale_of(old, new):
        return torch.where(old == float("-inf"), torch.zeros_like(old), torch.exp(old - new))

    def merge(parts):
        Ms = torch.stack([p[0] for p in parts]).amax(0)
        Mt = torch.stack([p[2] for p in parts]).amax(0)
        out = [Ms, torch.zeros(m, dtype=s.dtype), Mt, torch.zeros(m, dtype=s.dtype), torch.zeros(m, dtype=s.dtype)]
        for p in parts:
            out[1] = out[1] + scale_of(p[0], Ms) * p[1]
            out[3] = out[3] + scale_of(p[2], Mt) * p[3]
            out[4] = out[4] + scale_of(p[2], Mt) * p[4]
        return out

    ntiles = len(tile_order)
    split_parts = []
    for sp in range(splits):
        lane_state = [empty() for _ in range(lanes)]
        for ti in range(ntiles * sp // splits, ntiles * (sp + 1) // splits):
            k0 = tile_order[ti] * tile
            for ln in range(lanes):
                if k0 + ln >= min(k0 + tile, K):
                    continue          # a lane whose share of the tile is all padding keeps its state
                cols = torch.arange(k0 + ln, min(k0 + tile, K), lanes)
                st = lane_state[ln]
                ss, tt = s[:, cols], t[:, cols]
                ns, nt = torch.maximum(st[0], ss.amax(1)), torch.maximum(st[2], tt.amax(1))
                et = torch.exp(tt - nt[:, None])
                st[1] = st[1] * scale_of(st[0], ns) + torch.exp(ss - ns[:, None]).sum(1)
                st[3] = st[3] * scale_of(st[2], nt) + et.sum(1)
                st[4] = st[4] * scale_of(st[2], nt) + (et * ss).sum(1)
                st[0], st[2] = ns, nt
        split_parts.append(merge(lane_state))
    Ms, Lsum, Mt, Ltsum, A = merge(split_parts)
    Ls, Lt = Ms + torch.log(Lsum), Mt + torch.log(Ltsum)
    return Ls - A / Ltsum, Ls, Lt


# ---------------------------------------------------------------------------------------------- the original's module, restated
def logits(x, v, eps=EPS):
    """what the original's head returns: the normalised bottleneck rows through the weight-normalised last layer with gain 1"""
    return normalise_rows(x, eps) @ normalise_protos(v).t()


def dino_double_loop(student_out, teacher_out, center, student_temp, teacher_temp, ncrops, nteacher=2):
    """DINOLoss.forward of the original (main_dino.py) over logits: chunked student and teacher outputs, the double loop over
    (iq, v) with v == iq skipped, the mean over the terms"""
    import torch.nn.functional as F
    student_chunks = (student_out / student_temp).chunk(ncrops)
    q_chunks = F.softmax((teacher_out - center) / teacher_temp, dim=-1).detach().chunk(nteacher)
    total, n_terms = 0, 0
    for iq, q in enumerate(q_chunks):
        for v in range(len(student_chunks)):
            if v == iq:
                continue
            total = total + torch.sum(-q * F.log_softmax(student_chunks[v], dim=-1), dim=-1).mean()
            n_terms += 1
    return total / n_terms


def center_update_original(center, teacher_outs, momentum):
    """update_center of the original over the teacher logits of every rank: sum over the rows, all-reduced (sum), divided by
    len(teacher_output) * world_size"""
    world = len(teacher_outs)
    batch_center = sum(t.sum(dim=0, keepdim=True) for t in teacher_outs) / (teacher_outs[0].shape[0] * world)
    return center * momentum + batch_center * (1 - momentum)


def teacher_temp_schedule(warmup_teacher_temp, teacher_temp, warmup_teacher_temp_epochs, nepochs):
    import numpy as np
    return np.concatenate((np.linspace(warmup_teacher_temp, teacher_temp, warmup_teacher_temp_epochs),
                           np.ones(nepochs - warmup_teacher_temp_epochs) * teacher_temp))


def mlp_forward(x, params, nlayers):
    """the head's MLP: Linear -> GELU (exact erf) -> ... -> Linear, in the dtype of its inputs; params keyed as DINOHead's"""
    import torch.nn.functional as F
    if nlayers == 1:
        return F.linear(x, params["mlp.weight"], params["mlp.bias"])
    for i in range(nlayers):
        x = F.linear(x, params[f"mlp.{2 * i}.weight"], params[f"mlp.{2 * i}.bias"])
        if i < nlayers - 1:
            x = F.gelu(x)
    return x


# ---------------------------------------------------------------------------------------------- inputs
def random_rows(n, p, seed, device="cpu", dtype=torch.float32):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(n, p, generator=g, device=device, dtype=dtype)


def problem(m, K, p, seed, device="cpu", dtype=torch.float32, teacher_noise=0.5):
    """xs, vs, xt, vt: the teacher side is the student side plus noise, as an EMA teacher on another view is"""
    xs, vs = random_rows(m, p, seed, device, dtype), random_rows(K, p, seed + 1, device, dtype)
    xt = xs + teacher_noise * random_rows(m, p, seed + 2, device, dtype)
    vt = vs + 0.1 * random_rows(K, p, seed + 3, device, dtype)
    return xs, vs, xt, vt
