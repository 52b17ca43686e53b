"""float64 references for the layer-wise optimisers (bvc_amd/optim.py ``LARS`` / ``LAMB``), straight from their update rules, with a
multi-step driver (parameter groups, steps a GradScaler skips, gradient-norm clipping) and the flat stand-in module the GPU tests
step.  Host arithmetic only: nothing here calls the library.

    LARS   d = g + weight_decay w;  q = trust_coefficient ||w|| / ||d|| if adapt and ||w|| > 0 and ||d|| > 0 else 1;  d = q d
           buf = momentum buf + d;  w -= lr (d + momentum buf if nesterov else buf)
    LAMB   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + weight_decay w
           r = ||w|| / ||u|| if adapt and ||w|| > 0 and ||u|| > 0 else 1;  w -= lr r u

The stand-in holds the tensor sizes 33 x 7, 129, 64 x 64, a frozen tensor of 10 (no gradient), 5, 1, 1023, 49157 and then the seven live
sizes once more in reverse order: fourteen live tensors.  49157 = 3 x 16384 + 5, so that tensor spans four items of the norm pass with
a ragged last one, and 49 blocks of the apply pass; segments begin at offsets that are no multiples of four, quads straddle segment
boundaries, a 1024-element block holds several segments, and a one-element tensor and a frozen stretch are present."""
import numpy as np
import torch

F64 = torch.float64
LIVE = [(33, 7), (129,), (64, 64), (5,), (1,), (1023,), (49157,)]
SHAPES = LIVE[:3] + [None] + LIVE[3:] + LIVE[::-1]      # None: the frozen tensor
FROZEN = 10
LARS_DEFAULTS = dict(momentum=0.9, weight_decay=0.0, trust_coefficient=0.001, nesterov=False, adapt=True, maximize=False)
LAMB_DEFAULTS = dict(betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, adapt=True, maximize=False)


def _ratio(nw, nx, coef, adapt):
    return coef * nw / nx if adapt and nw > 0 and nx > 0 else 1.0


def lars_step(w, g, buf, *, lr, momentum=0.9, weight_decay=0.0, trust_coefficient=0.001, nesterov=False, adapt=True, maximize=False):
    """One LARS step of one tensor in float64 -> (w, buf, (||w||, ||d||, q)); `g` is the unscaled (and clipped) gradient."""
    w, g, buf = w.to(F64), g.to(F64), buf.to(F64)
    if maximize:
        g = -g
    d = g + weight_decay * w
    nw, nd = float(w.norm()), float(d.norm())
    q = _ratio(nw, nd, trust_coefficient, adapt)
    d = q * d
    buf = momentum * buf + d
    w = w - lr * (d + momentum * buf if nesterov else buf)
    return w, buf, (nw, nd, q)


def lamb_step(w, g, m, v, t, *, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, adapt=True, maximize=False):
    """LAMB step number `t` (1 for the first) of one tensor in float64 -> (w, m, v, (||w||, ||u||, r))."""
    w, g, m, v = w.to(F64), g.to(F64), m.to(F64), v.to(F64)
    if maximize:
        g = -g
    b1, b2 = betas
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    u = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps) + weight_decay * w
    nw, nu = float(w.norm()), float(u.norm())
    r = _ratio(nw, nu, 1.0, adapt)
    return w - lr * r * u, m, v, (nw, nu, r)


class Driver:
    """Several steps of LARS (kind "lars") or LAMB ("lamb") over a list of tensors in float64.

    `groups`: dicts of hyper-parameters with "params" = indices into `tensors`; missing keys take the optimiser's defaults (``lr``
    has none for LARS).  step(grads): `grads` are the UNSCALED gradients, one per tensor; with `max_grad_norm` = c they are multiplied
    by clip_coef = min(1, c / (norm + 1e-6)), norm over all tensors, first.  step(grads, skip=True) is the step a GradScaler skips:
    nothing moves, no step count advances.  After a step: `.w`, `.buf` (LARS) or `.m`, `.v` (LAMB), `.t` (LAMB: steps per group),
    `.stats` (per tensor (||w||, ||d|| or ||u||, ratio)), `.grad_norm`, `.clip_coef`."""

    def __init__(self, kind, tensors, groups, max_grad_norm=None):
        assert kind in ("lars", "lamb")
        self.kind, self.max_grad_norm = kind, max_grad_norm
        self.w = [t.detach().to("cpu", F64).clone() for t in tensors]
        self.groups = [dict(LARS_DEFAULTS if kind == "lars" else LAMB_DEFAULTS, **g) for g in groups]
        self.buf = [torch.zeros_like(w) for w in self.w]
        self.m, self.v = [torch.zeros_like(w) for w in self.w], [torch.zeros_like(w) for w in self.w]
        self.t = [0] * len(self.groups)
        self.stats = [(0.0, 0.0, 1.0)] * len(self.w)
        self.grad_norm, self.clip_coef = 0.0, 1.0

    def step(self, grads, skip=False):
        if skip:
            return
        grads = [g.detach().to("cpu", F64).reshape(w.shape) for g, w in zip(grads, self.w)]
        if self.max_grad_norm is not None:
            owned = [i for g in self.groups for i in g["params"]]
            self.grad_norm = float(torch.sqrt(sum((grads[i] ** 2).sum() for i in owned)))
            self.clip_coef = min(1.0, self.max_grad_norm / (self.grad_norm + 1e-6))
            grads = [g * self.clip_coef for g in grads]
        for gi, group in enumerate(self.groups):
            hyper = {k: v for k, v in group.items() if k not in ("params", "lr_scale", "name")}
            self.t[gi] += 1
            for i in group["params"]:
                if self.kind == "lars":
                    self.w[i], self.buf[i], self.stats[i] = lars_step(self.w[i], grads[i], self.buf[i], **hyper)
                else:
                    self.w[i], self.m[i], self.v[i], self.stats[i] = lamb_step(self.w[i], grads[i], self.m[i], self.v[i], self.t[gi], **hyper)


class FlatStandIn:
    """What the optimisers need of a flat module (flat.py): `_flat`, `_flat_grad`, `_shadow_base()`, membership of flat._MODULES.
    `alloc(n, dtype)` (default torch.zeros on `device`) hands out the four buffers: the GPU tests pass one that puts guard bands
    around them.  With a shadow, it starts as the bf16 image of the parameters - what a forward leaves behind."""

    def __init__(self, bvc, device, seed=0, shadow=False, alloc=None, shapes=SHAPES):
        alloc = alloc or (lambda n, dtype: torch.zeros(n, dtype=dtype, device=device))
        gen = torch.Generator().manual_seed(seed)
        n = sum(FROZEN if s is None else int(np.prod(s)) for s in shapes)
        self._flat, self._flat_grad = alloc(n, torch.float32), alloc(n, torch.float32)
        self._flat.copy_(torch.randn(n, generator=gen))
        self._flat_grad.zero_()
        self._shadow = None
        if shadow:
            self._shadow = alloc(n, torch.bfloat16)
            self._shadow.copy_(self._flat.to(torch.bfloat16))
        self.live, self.offsets, o = [], [], 0
        self.frozen = None
        for s in shapes:
            k = FROZEN if s is None else int(np.prod(s))
            p = torch.nn.Parameter(self._flat[o:o + k].view(s or (k,)), requires_grad=s is not None)
            if s is None:
                self.frozen, self.frozen_at = p, (o, o + k)
            else:
                p.grad = self._flat_grad[o:o + k].view(s)
                self.live.append(p)
                self.offsets.append((o, o + k))
            o += k
        self.n = n
        bvc.flat._MODULES.add(self)

    def _shadow_base(self):
        return None if self._shadow is None else self._shadow.data_ptr()

    def split(self, flat):
        """A flat tensor of the buffer's length -> the live tensors' stretches, in order."""
        return [flat[a:b] for a, b in self.offsets]
