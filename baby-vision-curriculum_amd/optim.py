"""Fused SGD / Adam / AdamW for flat parameter buffers: ONE HIP launch per flat module, whatever the parameter groups.

Parameters that live in a flat module's buffer (flat.py) with their gradients in its flat gradient buffer are updated by one
launch over the whole buffer: a static device table cuts it into segments owned by a parameter group (or by none: frozen
parameters), the groups' hyper-parameters travel per call (``bvc_op_sgd_step_segments`` / ``bvc_op_adam_step_segments``,
include/bvc.h).  The reference's JEPA optimiser (pretraining/predictive/helper.py:123-147: four groups, biases and 1-D tensors
with ``weight_decay`` 0) thereby costs two launches - encoder buffer, predictor buffer - like a single group does.  Parameters
outside any flat buffer (an ordinary ``nn.Linear`` head) take one launch per run of memory-adjacent parameters of a group.

More groups than the by-value struct carries (``_lib.OPT_MAX_GROUPS``) - layer-wise learning-rate decay makes ``2 * (layers + 2)`` of
them, ``layer_decay_param_groups`` below - keep the one launch per flat module: the hyper-parameters then sit in a device table with
one row per group (``bvc_op_sgd_step_table`` / ``bvc_op_adam_step_table``, up to ``_lib.OPT_TABLE_MAX_GROUPS`` groups), filled per
step by one small writer launch per 64 groups.

Same constructor and update rule as ``torch.optim.SGD`` (the reference builds
``torch.optim.SGD(xmodel.parameters(), lr, weight_decay, momentum, nesterov=True)`` at
pretraining/generative/pretrain_videomae.py:187-189) and the same ``state_dict`` layout
(``momentum_buffer`` per parameter).  Works with ``torch.amp.GradScaler``: it advertises
``_step_supports_amp_scaling`` so the scaler hands over its device-side ``grad_scale`` / ``found_inf``
and the step neither unscales in a separate pass nor synchronises with the host
(``scaler.step(optimizer)`` at pretrain_videomae.py:313 is unchanged).

``max_grad_norm=c`` (keyword-only, on all three classes) clips the gradients by their global norm as
``torch.nn.utils.clip_grad_norm_(params, c)`` before the step would, without a pass of its own: one read-only launch pair per flat
buffer gives the squared norm of the segments this optimiser owns (``bvc_op_grad_sqnorm_items``; ``bvc.amp.GradScaler`` takes its inf
check from that same read), ``bvc_op_clip_finalize`` turns the squares into ``{total_norm, clip_coef, scale / clip_coef}`` on the
device, and the step calls are handed the address of the last where they were handed the scale's - the kernels that divide by the scale
thereby clip too.  ``optimizer.grad_norm`` / ``optimizer.clip_coef`` are 0-d device views of the last step's values.  Immediate forms:
``clip_grad_norm_`` (torch's signature) and ``grad_norms(module)`` (per-parameter norms in one launch pair).  DESIGN.md
"Gradient-norm clipping".

``LARS`` and ``LAMB`` scale every parameter tensor's update by a ratio of norms (``adaptive_param_groups`` makes the usual two groups:
1-D tensors and biases neither decay nor adapt).  The segment table has one segment per tensor and the gradient-norm work list cuts
it into items, so a step is one library call per flat module (``bvc_op_lars_step_table`` / ``bvc_op_lamb_step_table``: a pass that
leaves per-item sums of squares, a per-segment reduction to ``{||w||, ||d||, ratio}``, the apply pass), for any number of groups; runs
of parameters outside flat buffers go through the same entry points.  ``optimizer.trust_ratios()`` gives the last step's ratios as
0-d device views.  DESIGN.md "Layer-wise trust ratios".
"""
import ctypes

import torch

from . import _lib
from . import flat as _flat


def _owner(p):
    """The flat module whose buffer holds parameter `p` with its gradient at the same offset of the flat gradient buffer."""
    if p.grad is None or not p.is_cuda:
        return None
    ptr = p.data_ptr()
    for m in list(_flat._MODULES):
        f, g = getattr(m, "_flat", None), getattr(m, "_flat_grad", None)
        if f is None or g is None or not f.is_cuda:
            continue
        base = f.data_ptr()
        if base <= ptr < base + 4 * f.numel() and p.grad.data_ptr() == g.data_ptr() + (ptr - base) and ptr + 4 * p.numel() <= base + 4 * f.numel():
            return m
    return None


class _Plan:
    """Segment table of one flat module for one optimiser: device arrays + the parameters per group, built once."""

    def __init__(self, module, items, table=False):
        # items: [(offset in elements, parameter, group index)]; table: stepped through the device-table entry points
        items = sorted(items, key=lambda t: t[0])
        self.module, self.items, self.table = module, items, table
        self.host = None       # table path: the ctypes arrays the hyper-parameters are handed over in, the device table
        f = module._flat
        self.n = f.numel()
        self.base, self.gbase = f.data_ptr(), module._flat_grad.data_ptr()
        starts, groups, pos = [], [], 0
        for off, prm, gi in items:
            if off < pos:
                raise _lib.BvcError("overlapping parameters in a flat buffer")
            if off > pos:
                starts.append(pos); groups.append(-1)
            starts.append(off); groups.append(gi)
            pos = off + prm.numel()
        if pos < self.n:
            starts.append(pos); groups.append(-1)
        starts.append(self.n)
        dev = f.device
        self.nseg = len(groups)
        self.starts, self.groups = starts, groups      # the host copy of the table (the gradient-norm work list is cut from it)
        self.norm = None       # _NormTable of this table, built by the first clipped step
        self.seg_start = torch.tensor(starts, dtype=torch.int64, device=dev)
        self.seg_group = torch.tensor(groups, dtype=torch.int32, device=dev)
        nblk = (self.n + 1023) // 1024
        firsts = torch.arange(nblk, dtype=torch.int64, device=dev) * 1024
        self.blk_seg = (torch.searchsorted(self.seg_start, firsts, right=True) - 1).to(torch.int32)
        self.state = None      # optimiser-specific flat state
        self.lw = None         # LARS / LAMB: the _Range of this table (work list, group table, partials, seg_stats)


def _build_plans(param_groups):
    """-> (plans, loose): plans = one _Plan per flat module that owns parameters of this optimiser; loose = {group index: [parameters
    outside any flat buffer]}.  More groups than the table carries: everything is loose (a launch per adjacent run, as before)."""
    loose, per_module = {}, {}
    if len(param_groups) > _lib.OPT_MAX_GROUPS:
        return [], {gi: [p for p in g["params"] if p.grad is not None] for gi, g in enumerate(param_groups)}
    for gi, group in enumerate(param_groups):
        for p in group["params"]:
            if p.grad is None:
                continue
            if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_cuda:
                raise _lib.BvcError("the bvc optimisers handle f32 CUDA parameters only")
            m = _owner(p)
            if m is None:
                loose.setdefault(gi, []).append(p)
            else:
                per_module.setdefault(id(m), (m, []))[1].append(((p.data_ptr() - m._flat.data_ptr()) // 4, p, gi))
    return [_Plan(m, items) for m, items in per_module.values()], loose


def _build_table_plans(param_groups, owner=_owner):
    """As _build_plans for more than _lib.OPT_MAX_GROUPS groups: one table _Plan (group index = index into param_groups) per flat
    module that owns parameters of this optimiser; loose carries only groups that have parameters outside flat buffers.
    `owner` finds a parameter's flat module (tests pass their own for buffers that are not on a GPU)."""
    if len(param_groups) > _lib.OPT_TABLE_MAX_GROUPS:
        raise _lib.BvcError(f"{len(param_groups)} parameter groups: the device table carries {_lib.OPT_TABLE_MAX_GROUPS}")
    loose, per_module = {}, {}
    for gi, group in enumerate(param_groups):
        for p in group["params"]:
            if p.grad is None:
                continue
            m = owner(p)
            if m is None:
                loose.setdefault(gi, []).append(p)     # (checked for f32 CUDA where the runs are formed)
                continue
            if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                raise _lib.BvcError("the bvc optimisers handle f32 CUDA parameters only")
            per_module.setdefault(id(m), (m, []))[1].append(((p.data_ptr() - m._flat.data_ptr()) // 4, p, gi))
    return [_Plan(m, items, table=True) for m, items in per_module.values()], loose


def _choose_plans(param_groups):
    """By-value plans up to _lib.OPT_MAX_GROUPS groups (unchanged), table plans up to _lib.OPT_TABLE_MAX_GROUPS, above that the
    per-run path for everything (what _build_plans answers)."""
    if _lib.OPT_MAX_GROUPS < len(param_groups) <= _lib.OPT_TABLE_MAX_GROUPS:
        return _build_table_plans(param_groups)
    return _build_plans(param_groups)


def _table_host(ngroups, reals, ctype, flags, device):
    """What a table plan keeps between steps: one ctypes array of `ngroups` entries per hyper-parameter (the library reads them
    before the call returns and passes them on as kernel arguments) and the device table of 8 floats per group it writes."""
    host = {n: (ctype * ngroups)() for n in reals}
    host.update({n: (ctypes.c_int32 * ngroups)() for n in flags})
    host["table"] = torch.zeros(8 * ngroups, dtype=torch.float32, device=device)
    return host


def _plans_key(param_groups):
    key = []
    for g in param_groups:
        ps = g["params"]
        if not ps:
            key.append(0)
            continue
        # (the count of parameters that HAVE a gradient is part of the key: a parameter frozen after the table was built - .grad None,
        #  torch skips it - must drop out of its segment, or the kernel would keep stepping it on the stale contents of the flat buffer)
        key.append((len(ps), ps[0].data_ptr(), ps[-1].data_ptr(),
                    ps[0].grad.data_ptr() if ps[0].grad is not None else 0,
                    ps[-1].grad.data_ptr() if ps[-1].grad is not None else 0,
                    sum(1 for p in ps if p.grad is not None)))
    return tuple(key)


def _plans_still_valid(cached, key):
    """The key moved although nothing the plans depend on did: gradients of parameters OUTSIDE flat buffers are fresh autograd
    allocations every step, and where one of them is the first or last parameter of a group its address is part of the key.  True
    if the groups are the same lists as before (lengths, first / last parameter, number of gradients) and every parameter of every
    plan still sits, with its gradient, where the plan has it; then the plans - and the flat optimiser state that hangs on them - stay."""
    old_key, plans, loose = cached
    if len(old_key) != len(key):
        return False
    for a, b in zip(old_key, key):
        if (a == 0) != (b == 0) or (a != 0 and (a[0], a[1], a[2], a[5]) != (b[0], b[1], b[2], b[5])):
            return False
    for plan in plans:
        f, g = plan.module._flat, plan.module._flat_grad
        if f is None or g is None or f.data_ptr() != plan.base or g.data_ptr() != plan.gbase:
            return False
        for off, p, _gi in plan.items:
            if p.grad is None or p.data_ptr() != plan.base + 4 * off or p.grad.data_ptr() != plan.gbase + 4 * off:
                return False
    return all(p.grad is not None for ps in loose.values() for p in ps)


# ---------------------------------------------------------------------------------------------- gradient norms
def _checked_max_grad_norm(value):
    if value is None:
        return None
    value = float(value)
    if value != value or value < 0.0:
        raise ValueError(f"max_grad_norm must be a non-negative number or None, not {value}")
    return value


def grad_norm_work_list(seg_start, seg_group):
    """The work list of the gradient-norm pass for a segment table (``bvc_grad_norm_items_host``; host only, no GPU):
    -> (items: int64 CPU tensor [nitems][3] of (start, length, segment), seg_first_item: int64 CPU tensor [nseg + 1])."""
    raw, first = _work_list_raw(seg_start, seg_group)
    return torch.stack([raw[:, 0], raw[:, 1] & 0xFFFFFFFF, raw[:, 1] >> 32], dim=1), first


def _work_list_raw(seg_start, seg_group):
    """-> (the bvc_norm_item array as an int64 CPU tensor [nitems][2], seg_first_item)"""
    nseg = len(seg_group)
    if len(seg_start) != nseg + 1:
        raise _lib.BvcError("a segment table has one more start than segments")
    L = _lib.lib()
    starts, groups = torch.tensor(list(seg_start), dtype=torch.int64), torch.tensor(list(seg_group), dtype=torch.int32)
    first, n = torch.zeros(nseg + 1, dtype=torch.int64), ctypes.c_int64()
    _lib.check(L.bvc_grad_norm_items_host(starts.data_ptr(), groups.data_ptr(), nseg, None, 0, first.data_ptr(), ctypes.byref(n)),
               "bvc_grad_norm_items_host")
    raw = torch.zeros((n.value, 2), dtype=torch.int64)
    if n.value:
        _lib.check(L.bvc_grad_norm_items_host(starts.data_ptr(), groups.data_ptr(), nseg, raw.data_ptr(), n.value, first.data_ptr(),
                                              ctypes.byref(n)), "bvc_grad_norm_items_host")
    return raw, first


class _NormTable:
    """The gradient-norm work list of one segment table on a device, with the f64 item partials the pass writes: static, built once."""

    def __init__(self, seg_start, seg_group, device):
        raw, first = _work_list_raw(seg_start, seg_group)
        self.nseg, self.nitems = len(seg_group), raw.shape[0]
        self.items, self.first = raw.to(device), first.to(device)
        self.partial = torch.zeros(max(self.nitems, 1), dtype=torch.float64, device=device)

    def launch(self, L, base, total, found_inf, stream, seg_out=None, as_norm=0):
        """One launch pair over the range at address `base`: the total (squared) norm to address `total`, per segment to `seg_out`."""
        _lib.check(L.bvc_op_grad_sqnorm_items(base, self.items.data_ptr() if self.nitems else None, self.nitems, self.first.data_ptr(),
                                              self.nseg, self.partial.data_ptr(), seg_out, total, as_norm, found_inf, stream),
                   "bvc_op_grad_sqnorm_items")


_RUN_TABLES = {}     # (elements, device) -> the one-segment _NormTable of a plain contiguous range (launches of one stream share it)


def _run_table(n, device):
    hit = _RUN_TABLES.get((n, device))
    if hit is None:
        hit = _RUN_TABLES[(n, device)] = _NormTable([0, n], [0], device)
    return hit


class SGD(torch.optim.Optimizer):
    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False,
                 max_grad_norm=None):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("invalid hyper-parameter")
        self.max_grad_norm = _checked_max_grad_norm(max_grad_norm)
        self._clip = None    # clipping: the device scalars and the squares of the last norm pass
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize)
        super().__init__(params, defaults)
        self._runs = {}   # group index -> (key, runs) for parameters outside flat buffers
        self._plans = None   # (key, plans, loose)

    _make_plans = staticmethod(_choose_plans)      # (LARS / LAMB below: table plans for any number of groups)

    def _get_plans(self):
        key = _plans_key(self.param_groups)
        if self._plans is not None and self._plans[0] != key and _plans_still_valid(self._plans, key):
            self._plans = (key, self._plans[1], self._plans[2])
        if self._plans is None or self._plans[0] != key:
            plans, loose = self._make_plans(self.param_groups)
            self._plans = (key, plans, loose)
            self._runs = {}
        return self._plans[1], self._plans[2]

    # ---- gradient-norm clipping (max_grad_norm=): the clip rides on the scale pointer of the step calls, no kernel of theirs changes
    def _clip_device(self):
        for g in self.param_groups:
            for p in g["params"]:
                return p.device
        raise _lib.BvcError("an optimiser without parameters has no gradient norm")

    def _clip_buffers(self):
        """{out: device f32 {total_norm, clip_coef, eff_scale}, sq: one square per flat buffer / loose run, nranges, tag}"""
        if self._clip is None:
            dev = self._clip_device()
            self._clip = {"out": torch.zeros(3, dtype=torch.float32, device=dev), "sq": torch.zeros(8, dtype=torch.float32, device=dev),
                          "nranges": 0, "tag": None}
        return self._clip

    @property
    def grad_norm(self):
        """0-d device view: the unscaled gradient norm of the last step before clipping (nonfinite where the gradients were).  No sync."""
        return self._clip_buffers()["out"][0]

    @property
    def clip_coef(self):
        """0-d device view: the coefficient the last step multiplied the gradients by (1 = the clip was inactive).  No sync."""
        return self._clip_buffers()["out"][1]

    def _grad_sq(self, found_inf=None, tag=None):
        """Squared gradient norm of every plan (its owned segments: one launch pair over the plan's segment table) and of every loose
        run (one launch pair each) into the `sq` buffer; `found_inf` (a device scalar) gets GradScaler's inf check out of the same
        read.  `tag` marks the squares as taken for the step a scaler is about to make (bvc.amp.GradScaler, which withdraws the tag when
        its step() returns)."""
        L, stream = _lib.lib(), _lib.current_stream_ptr()
        plans, loose = self._get_plans()
        runs = [run for gi, ps in loose.items() for run in self._group_runs(gi, ps)]
        c = self._clip_buffers()
        dev = c["out"].device
        if any(pl.module._flat.device != dev for pl in plans) or any(run[0].device != dev for run in runs):
            raise _lib.BvcError("max_grad_norm needs all parameters of the optimiser on one device")
        nr = len(plans) + len(runs)
        if c["sq"].numel() < nr:
            c["sq"] = torch.zeros(2 * nr, dtype=torch.float32, device=dev)
        sq, fi = c["sq"].data_ptr(), found_inf.data_ptr() if found_inf is not None else None
        for i, plan in enumerate(plans):
            if plan.norm is None:
                plan.norm = _NormTable(plan.starts, plan.groups, dev)
            plan.norm.launch(L, plan.gbase, sq + 4 * i, fi, stream)
        for i, run in enumerate(runs, len(plans)):
            _run_table(sum(p.numel() for p in run), dev).launch(L, run[0].grad.data_ptr(), sq + 4 * i, fi, stream)
        c["nranges"], c["tag"] = nr, tag
        return c

    def _clip_scale(self, L, stream, grad_scale, gs):
        """-> the address the step calls divide the gradients by: eff_scale = scale / clip_coef of this step's norm.  The squares
        bvc.amp.GradScaler left for this very step are consumed (they are of the scaled gradients: only together with the scale),
        otherwise the norms are taken here."""
        c = self._clip
        if c is None or c["tag"] is None or grad_scale is None:
            c = self._grad_sq()
        c["tag"] = None
        if c["nranges"] == 0:
            return gs
        _lib.check(L.bvc_op_clip_finalize(c["sq"].data_ptr(), c["nranges"], self.max_grad_norm, gs, c["out"].data_ptr(), stream),
                   "bvc_op_clip_finalize")
        return c["out"].data_ptr() + 8

    def _plan_momentum(self, plan):
        """One flat momentum buffer per flat module; the per-parameter ``momentum_buffer`` entries are views into it."""
        if plan.state is None:
            flat = torch.zeros(plan.n, dtype=torch.float32, device=plan.module._flat.device)
            fresh = {}
            for off, p, gi in plan.items:
                st = self.state[p]
                old = st.get("momentum_buffer")
                if old is not None:   # e.g. after load_state_dict, or a run-wise buffer of an earlier layout
                    flat[off:off + p.numel()].copy_(old.reshape(-1))
                else:
                    fresh[gi] = True
                st["momentum_buffer"] = flat[off:off + p.numel()].view(p.shape)
            plan.state = (flat, fresh)
        return plan.state

    @staticmethod
    def _contiguous_runs(params):
        """Maximal runs of parameters that are adjacent in memory with equally adjacent gradients."""
        items = sorted((p for p in params if p.grad is not None), key=lambda p: p.data_ptr())
        runs, cur = [], []
        for p in items:
            if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_cuda:
                raise _lib.BvcError("bvc SGD handles f32 CUDA parameters only")
            if cur:
                q = cur[-1]
                if (q.data_ptr() + q.numel() * 4 == p.data_ptr() and q.grad.data_ptr() + q.numel() * 4 == p.grad.data_ptr()):
                    cur.append(p)
                    continue
                runs.append(cur)
            cur = [p]
        if cur:
            runs.append(cur)
        return runs

    def _group_runs(self, gi, ps):
        if not ps:      # a group without gradients (the fallback for more groups than any table carries lists every group)
            return []
        key = (len(ps), ps[0].data_ptr(), ps[-1].data_ptr(),
               ps[0].grad.data_ptr() if ps[0].grad is not None else 0,
               ps[-1].grad.data_ptr() if ps[-1].grad is not None else 0)
        hit = self._runs.get(gi)
        if hit is None or hit[0] != key:
            hit = (key, self._contiguous_runs(ps))
            self._runs[gi] = hit
        return hit[1]

    def _momentum_buffer(self, run):
        """One flat buffer per run; per-parameter ``momentum_buffer`` entries are views into it."""
        first = run[0]
        st = self.state[first]
        flat = st.get("_flat_momentum")
        n = sum(p.numel() for p in run)
        fresh = False
        if flat is None or flat.numel() != n:
            # zeros: with dampening == 0 the regular update of a zero buffer IS torch's first step (buf = g), and a
            # step skipped by GradScaler (found_inf) leaves a well-defined buffer behind
            flat = torch.zeros(n, dtype=torch.float32, device=first.device)
            have = all("momentum_buffer" in self.state[p] and self.state[p]["momentum_buffer"] is not None for p in run)
            o = 0
            for p in run:
                if have:   # e.g. after load_state_dict: adopt the loaded per-parameter buffers
                    flat[o:o + p.numel()].copy_(self.state[p]["momentum_buffer"].reshape(-1))
                self.state[p]["momentum_buffer"] = flat[o:o + p.numel()].view(p.shape)
                o += p.numel()
            st["_flat_momentum"] = flat
            fresh = not have
        return flat, fresh

    def _step_table(self, plan, L, gs, fi, found_inf, stream):
        """One flat module with more groups than the by-value struct carries: the hyper-parameters go as plain host arrays, the
        library stores them into the plan's device table (one row per group) and steps the buffer with one launch."""
        ng = len(self.param_groups)
        if plan.host is None:
            plan.host = _table_host(ng, ("lr", "momentum", "dampening", "weight_decay"), ctypes.c_float,
                                    ("nesterov", "first_step", "maximize"), plan.module._flat.device)
        H = plan.host
        need_buf = any(g["momentum"] != 0 for g in self.param_groups)
        flat, fresh = self._plan_momentum(plan) if need_buf else (None, {})
        for gi, g in enumerate(self.param_groups):
            H["lr"][gi], H["momentum"][gi], H["dampening"][gi], H["weight_decay"][gi] = float(g["lr"]), float(g["momentum"]), float(g["dampening"]), float(g["weight_decay"])
            H["nesterov"][gi], H["maximize"][gi] = int(g["nesterov"]), int(g["maximize"])
            # torch's first step sets buf = g without dampening; only matters when dampening != 0
            H["first_step"][gi] = int(bool(fresh.get(gi)) and g["dampening"] != 0 and found_inf is None)
        _lib.check(L.bvc_op_sgd_step_table(
            plan.base, plan.gbase, flat.data_ptr() if flat is not None else None, plan.n, plan.seg_start.data_ptr(),
            plan.seg_group.data_ptr(), plan.blk_seg.data_ptr(), plan.nseg, ng, H["lr"], H["momentum"], H["dampening"], H["weight_decay"],
            H["nesterov"], H["first_step"], H["maximize"], H["table"].data_ptr(), gs, fi, 1, _flat.shadow_for(plan.base, plan.n), stream),
            "bvc_op_sgd_step_table")
        if fresh:
            plan.state = (flat, {})

    def load_state_dict(self, state_dict):
        """torch's, then the cached plans and runs are dropped: their flat state lives outside ``self.state``, the next step rebuilds
        it from the loaded per-parameter tensors (a rollback or a resume into an optimiser that has already stepped)."""
        super().load_state_dict(state_dict)
        self._plans = None
        self._runs = {}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale = getattr(self, "grad_scale", None)
        found_inf = getattr(self, "found_inf", None)
        L = _lib.lib()
        stream = _lib.current_stream_ptr()
        gs = grad_scale.data_ptr() if grad_scale is not None else None
        fi = found_inf.data_ptr() if found_inf is not None else None
        plans, loose = self._get_plans()
        if self.max_grad_norm is not None:
            gs = self._clip_scale(L, stream, grad_scale, gs)
        for plan in plans:
            if plan.table:
                self._step_table(plan, L, gs, fi, found_inf, stream)
                continue
            G = _lib.SgdGroupsC()
            G.ngroups = len(self.param_groups)
            need_buf = any(g["momentum"] != 0 for g in self.param_groups)
            flat, fresh = self._plan_momentum(plan) if need_buf else (None, {})
            for gi, g in enumerate(self.param_groups):
                G.lr[gi], G.momentum[gi], G.dampening[gi], G.weight_decay[gi] = float(g["lr"]), float(g["momentum"]), float(g["dampening"]), float(g["weight_decay"])
                G.nesterov[gi], G.maximize[gi] = int(g["nesterov"]), int(g["maximize"])
                # torch's first step sets buf = g without dampening; only matters when dampening != 0
                G.first_step[gi] = int(bool(fresh.get(gi)) and g["dampening"] != 0 and found_inf is None)
            _lib.check(L.bvc_op_sgd_step_segments(
                plan.base, plan.gbase, flat.data_ptr() if flat is not None else None, plan.n, plan.seg_start.data_ptr(),
                plan.seg_group.data_ptr(), plan.blk_seg.data_ptr(), plan.nseg, ctypes.byref(G), gs, fi, 1,
                _flat.shadow_for(plan.base, plan.n), stream), "bvc_op_sgd_step_segments")
            if fresh:
                plan.state = (flat, {})
        for gi, ps in loose.items():
            group = self.param_groups[gi]
            for run in self._group_runs(gi, ps):
                n = sum(p.numel() for p in run)
                buf_ptr, first = None, 0
                if group["momentum"] != 0:
                    flat, fresh = self._momentum_buffer(run)
                    # torch's first step sets buf = g without dampening; only matters when dampening != 0
                    buf_ptr, first = flat.data_ptr(), int(fresh and group["dampening"] != 0 and found_inf is None)
                _lib.check(L.bvc_op_sgd_step(
                    run[0].data_ptr(), run[0].grad.data_ptr(), buf_ptr, n, float(group["lr"]), float(group["momentum"]),
                    float(group["dampening"]), float(group["weight_decay"]), int(group["nesterov"]), first,
                    int(group["maximize"]), gs, fi, 1, _flat.shadow_for(run[0].data_ptr(), n), stream), "bvc_op_sgd_step")
        return loss

    def state_dict(self):
        # shallow copies: super().state_dict() hands out the LIVE per-parameter dicts, popping from them would drop the flat
        # state of the running optimiser (reallocation + host sync on the next step)
        sd = super().state_dict()
        sd["state"] = {k: {n: v for n, v in st.items() if not n.startswith("_flat_")} for k, st in sd["state"].items()}
        return sd


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's constructor, update rule and state layout (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter;
    the reference builds Adam / AdamW(betas=(0.9, 0.95)) at pretrain_videomae.py:190-193), as one HIP launch per flat module (per
    contiguous run for parameters outside flat buffers).  The step count lives on the device so that a step skipped by GradScaler
    does not advance it."""
    _step_supports_amp_scaling = True
    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, maximize=False,
                 max_grad_norm=None):
        if amsgrad:
            raise NotImplementedError("amsgrad is not implemented (the reference does not use it)")
        self.max_grad_norm = _checked_max_grad_norm(max_grad_norm)
        self._clip = None
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=maximize))
        self._runs = {}
        self._plans = None

    _contiguous_runs = staticmethod(SGD._contiguous_runs)
    _group_runs = SGD._group_runs
    _get_plans, _make_plans = SGD._get_plans, staticmethod(_choose_plans)
    _clip_device, _clip_buffers, _grad_sq, _clip_scale = SGD._clip_device, SGD._clip_buffers, SGD._grad_sq, SGD._clip_scale
    grad_norm, clip_coef = SGD.grad_norm, SGD.clip_coef

    def load_state_dict(self, state_dict):
        """As SGD.load_state_dict: the cached flat state is dropped, the next step adopts the loaded ``step`` / ``exp_avg`` / ``exp_avg_sq``."""
        super().load_state_dict(state_dict)
        self._plans = None
        self._runs = {}

    def _plan_state(self, plan):
        """Flat exp_avg / exp_avg_sq per flat module, the per-group step scalars (3 per group) and the f64 upload scratch."""
        if plan.state is None:
            dev = plan.module._flat.device
            m, v = torch.zeros(plan.n, dtype=torch.float32, device=dev), torch.zeros(plan.n, dtype=torch.float32, device=dev)
            # (a table plan has a row of step scalars for every group of the optimiser and needs no upload scratch)
            state = torch.zeros(3 * (len(self.param_groups) if plan.table else _lib.OPT_MAX_GROUPS), dtype=torch.float32, device=dev)
            hyper = None if plan.table else torch.zeros(3 * _lib.OPT_MAX_GROUPS, dtype=torch.float64, device=dev)
            for off, p, gi in plan.items:
                st = self.state[p]
                k = p.numel()
                if "exp_avg" in st:    # after load_state_dict, or state of an earlier layout: adopt it (a group shares one step count)
                    m[off:off + k].copy_(st["exp_avg"].reshape(-1))
                    v[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
                    state[3 * gi] = float(st["step"])
                st["exp_avg"], st["exp_avg_sq"] = m[off:off + k].view(p.shape), v[off:off + k].view(p.shape)
                st["step"] = state[3 * gi]
            plan.state = (m, v, state, hyper)
        return plan.state

    def _run_state(self, run):
        first = run[0]
        st = self.state[first]
        flat = st.get("_flat_adam")
        n = sum(p.numel() for p in run)
        if flat is None or flat[0].numel() != n:
            dev = first.device
            m, v = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
            state3 = torch.zeros(3, dtype=torch.float32, device=dev)
            have = all("exp_avg" in self.state[p] for p in run)
            if have:    # after load_state_dict: adopt the loaded per-parameter state (all parameters share one step count)
                state3[0] = float(self.state[first]["step"])
            o = 0
            for p in run:
                k = p.numel()
                if have:
                    m[o:o + k].copy_(self.state[p]["exp_avg"].reshape(-1))
                    v[o:o + k].copy_(self.state[p]["exp_avg_sq"].reshape(-1))
                self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"] = m[o:o + k].view(p.shape), v[o:o + k].view(p.shape)
                self.state[p]["step"] = state3[0]
                o += k
            flat = (m, v, state3)
            st["_flat_adam"] = flat
        return flat

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale = getattr(self, "grad_scale", None)
        found_inf = getattr(self, "found_inf", None)
        gs = grad_scale.data_ptr() if grad_scale is not None else None
        fi = found_inf.data_ptr() if found_inf is not None else None
        L = _lib.lib()
        stream = _lib.current_stream_ptr()
        plans, loose = self._get_plans()
        if self.max_grad_norm is not None:
            gs = self._clip_scale(L, stream, grad_scale, gs)
        for plan in plans:
            m, v, state, hyper = self._plan_state(plan)
            if plan.table:
                ng = len(self.param_groups)
                if plan.host is None:
                    plan.host = _table_host(ng, ("lr", "beta1", "beta2", "eps", "weight_decay"), ctypes.c_double,
                                            ("decoupled", "maximize"), plan.module._flat.device)
                H = plan.host
                for gi, g in enumerate(self.param_groups):
                    b1, b2 = g["betas"]
                    H["lr"][gi], H["beta1"][gi], H["beta2"][gi], H["eps"][gi], H["weight_decay"][gi] = float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"])
                    H["decoupled"][gi], H["maximize"][gi] = int(self._decoupled), int(g["maximize"])
                _lib.check(L.bvc_op_adam_step_table(
                    plan.base, plan.gbase, m.data_ptr(), v.data_ptr(), plan.n, plan.seg_start.data_ptr(), plan.seg_group.data_ptr(),
                    plan.blk_seg.data_ptr(), plan.nseg, ng, H["lr"], H["beta1"], H["beta2"], H["eps"], H["weight_decay"], H["decoupled"],
                    H["maximize"], state.data_ptr(), H["table"].data_ptr(), gs, fi, 1, _flat.shadow_for(plan.base, plan.n), stream),
                    "bvc_op_adam_step_table")
                continue
            G = _lib.AdamGroupsC()
            G.ngroups = len(self.param_groups)
            for gi, g in enumerate(self.param_groups):
                b1, b2 = g["betas"]
                G.lr[gi], G.beta1[gi], G.beta2[gi], G.eps[gi], G.weight_decay[gi] = float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"])
                G.decoupled[gi], G.maximize[gi] = int(self._decoupled), int(g["maximize"])
            _lib.check(L.bvc_op_adam_step_segments(
                plan.base, plan.gbase, m.data_ptr(), v.data_ptr(), plan.n, plan.seg_start.data_ptr(), plan.seg_group.data_ptr(),
                plan.blk_seg.data_ptr(), plan.nseg, ctypes.byref(G), state.data_ptr(), hyper.data_ptr(), gs, fi, 1,
                _flat.shadow_for(plan.base, plan.n), stream), "bvc_op_adam_step_segments")
        for gi, ps in loose.items():
            group = self.param_groups[gi]
            b1, b2 = group["betas"]
            for run in self._group_runs(gi, ps):
                n = sum(p.numel() for p in run)
                m, v, state3 = self._run_state(run)
                _lib.check(L.bvc_op_adam_prepare(state3.data_ptr(), float(group["lr"]), float(b1), float(b2), fi, stream),
                           "bvc_op_adam_prepare")
                _lib.check(L.bvc_op_adam_step(
                    run[0].data_ptr(), run[0].grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, float(group["lr"]), float(b1), float(b2),
                    float(group["eps"]), float(group["weight_decay"]), int(self._decoupled), int(group["maximize"]),
                    state3.data_ptr(), gs, fi, 1, _flat.shadow_for(run[0].data_ptr(), n), stream), "bvc_op_adam_step")
        return loss

    def state_dict(self):
        # shallow copies: super().state_dict() hands out the LIVE per-parameter dicts, popping from them would drop the flat
        # state of the running optimiser (reallocation + host sync on the next step)
        sd = super().state_dict()
        sd["state"] = {k: {n: v for n, v in st.items() if not n.startswith("_flat_")} for k, st in sd["state"].items()}
        return sd


class AdamW(Adam):
    """torch.optim.AdamW: decoupled weight decay, default 1e-2."""
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 max_grad_norm=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         max_grad_norm=max_grad_norm)


# ---------------------------------------------------------------------------------------------- layer-wise trust ratios: LARS, LAMB
class _Range:
    """What one call of ``bvc_op_lars_step_table`` / ``bvc_op_lamb_step_table`` works on: a segment table with one segment per
    parameter tensor (a flat module's, or that of a run of parameters outside flat buffers), its work list, and the device buffers
    the caller owns: the group table, the f64 item partials and ``seg_stats`` [nseg][3] = {||w||, ||d|| or ||u||, ratio}."""

    def __init__(self, opt, starts, groups, ngroups, device, tables=None):
        self.n, self.nseg, self.ngroups = int(starts[-1]), len(groups), ngroups
        if tables is None:
            seg_start = torch.tensor(starts, dtype=torch.int64, device=device)
            firsts = torch.arange((self.n + 1023) // 1024, dtype=torch.int64, device=device) * 1024
            tables = (seg_start, torch.tensor(groups, dtype=torch.int32, device=device),
                      (torch.searchsorted(seg_start, firsts, right=True) - 1).to(torch.int32))
        self.seg_start, self.seg_group, self.blk_seg = tables
        raw, first = _work_list_raw(starts, groups)
        self.nitems = raw.shape[0]
        self.items, self.first = raw.to(device), first.to(device)
        self.table = opt._zeros(8 * ngroups, torch.float32, device)
        self.partial = opt._zeros(2 * max(self.nitems, 1), torch.float64, device)
        self.stats = opt._zeros(3 * self.nseg, torch.float32, device).view(self.nseg, 3)
        self.stats[:, 2] = 1.0
        self.owned = [s for s, g in enumerate(groups) if g >= 0]      # the segment of the k-th parameter in address order
        self.host = None       # the ctypes arrays the hyper-parameters are handed over in


def _views_alias(flat, views):
    """True if the per-parameter state tensors `views` are, in order, the consecutive stretches of `flat`.  Gradients of parameters
    outside flat buffers are fresh allocations every step, so memory-adjacent runs can join and part from one step to the next: the
    flat state a run's first parameter kept from an earlier grouping is only good while the per-parameter views still point into it."""
    at = flat.data_ptr()
    for v in views:
        if v is None or v.data_ptr() != at:
            return False
        at += 4 * v.numel()
    return True


class _LayerwiseOptimizer(torch.optim.Optimizer):
    """What LARS and LAMB share: one library call per flat module and per run of parameters outside flat buffers, through the
    segment-table entry points for ANY number of groups (there is no by-value twin); the plan cache, the GradScaler protocol and
    ``max_grad_norm`` of the other optimisers; ``trust_ratios()``."""
    _step_supports_amp_scaling = True
    _make_plans = staticmethod(_build_table_plans)
    _contiguous_runs = staticmethod(SGD._contiguous_runs)
    _group_runs, _get_plans = SGD._group_runs, SGD._get_plans
    _clip_device, _clip_buffers, _grad_sq, _clip_scale = SGD._clip_device, SGD._clip_buffers, SGD._grad_sq, SGD._clip_scale
    grad_norm, clip_coef = SGD.grad_norm, SGD.clip_coef

    @staticmethod
    def _zeros(n, dtype, device):
        """Every device buffer the step kernels write is allocated here (tests put guard bands around them)."""
        return torch.zeros(n, dtype=dtype, device=device)

    def _setup(self, max_grad_norm):
        self.max_grad_norm = _checked_max_grad_norm(max_grad_norm)
        self._clip = None
        self._runs = {}
        self._plans = None

    def load_state_dict(self, state_dict):
        """As SGD.load_state_dict: the cached flat state is dropped, the next step adopts the loaded per-parameter tensors."""
        super().load_state_dict(state_dict)
        self._plans = None
        self._runs = {}

    def state_dict(self):
        # shallow copies, as SGD.state_dict: the live per-parameter dicts keep their flat state
        sd = super().state_dict()
        sd["state"] = {k: {n: v for n, v in st.items() if not n.startswith("_flat_")} for k, st in sd["state"].items()}
        return sd

    def _plan_range(self, plan):
        if plan.lw is None:
            plan.lw = _Range(self, plan.starts, plan.groups, len(self.param_groups), plan.module._flat.device,
                             (plan.seg_start, plan.seg_group, plan.blk_seg))
        return plan.lw

    def _run_range(self, run):
        """The table of a run outside flat buffers: one segment per parameter, all of group 0 of a one-group table."""
        st = self.state[run[0]]
        sizes = tuple(p.numel() for p in run)
        R = st.get("_flat_range")
        if R is None or R.sizes != sizes:
            starts = [0]
            for k in sizes:
                starts.append(starts[-1] + k)
            R = st["_flat_range"] = _Range(self, starts, [0] * len(sizes), 1, run[0].device)
            R.sizes = sizes
        return R

    def trust_ratios(self):
        """``{parameter: 0-d device view of the trust ratio the last step applied to it}`` (1 before the first step, for a group with
        ``adapt=False`` and where the rule falls back: a zero tensor, a zero update).  No sync; the views alias ``seg_stats``."""
        out = {}
        plans, loose = self._get_plans()
        for plan in plans:
            R = self._plan_range(plan)
            for s, (_off, p, _gi) in zip(R.owned, plan.items):
                out[p] = R.stats[s, 2]
        for gi, ps in loose.items():
            for run in self._group_runs(gi, ps):
                R = self._run_range(run)
                for s, p in enumerate(run):
                    out[p] = R.stats[s, 2]
        return out

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale = getattr(self, "grad_scale", None)
        found_inf = getattr(self, "found_inf", None)
        gs = grad_scale.data_ptr() if grad_scale is not None else None
        fi = found_inf.data_ptr() if found_inf is not None else None
        L = _lib.lib()
        stream = _lib.current_stream_ptr()
        plans, loose = self._get_plans()
        if self.max_grad_norm is not None:
            gs = self._clip_scale(L, stream, grad_scale, gs)
        everyone = range(len(self.param_groups))
        for plan in plans:
            self._launch(L, self._plan_range(plan), plan.base, plan.gbase, everyone, self._plan_state(plan), gs, fi, stream)
        for gi, ps in loose.items():
            for run in self._group_runs(gi, ps):
                self._launch(L, self._run_range(run), run[0].data_ptr(), run[0].grad.data_ptr(), (gi,), self._run_state(gi, run), gs, fi,
                             stream)
        return loss


class LARS(_LayerwiseOptimizer):
    """Layer-wise adaptive rate scaling in the form of SimCLR's and MAE's LARS, per parameter tensor ``w`` with gradient ``g``::

        d = g + weight_decay * w
        q = trust_coefficient * ||w|| / ||d||   if adapt and ||w|| > 0 and ||d|| > 0, else 1
        buf = momentum * buf + q * d ;  w -= lr * (q * d + momentum * buf  if nesterov else  buf)

    ``adapt`` is a per-group key (default True); with ``adapt=False`` a group is plain momentum SGD - what biases and norm parameters
    get (``adaptive_param_groups``).  State: ``momentum_buffer`` per parameter, views of one flat buffer per flat module.  One
    ``bvc_op_lars_step_table`` call per flat module and step (include/bvc.h "Layer-wise trust ratios")."""

    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0, trust_coefficient=0.001, nesterov=False, *, maximize=False,
                 max_grad_norm=None):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0 or trust_coefficient < 0.0:
            raise ValueError("invalid hyper-parameter")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum")
        self._setup(max_grad_norm)
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, trust_coefficient=trust_coefficient,
                                      nesterov=nesterov, adapt=True, maximize=maximize))

    def _plan_state(self, plan):
        """One flat momentum buffer per flat module; the per-parameter ``momentum_buffer`` entries are views into it."""
        if not any(g["momentum"] != 0 for g in self.param_groups):
            return None
        if plan.state is None:
            flat = self._zeros(plan.n, torch.float32, plan.module._flat.device)
            for off, p, _gi in plan.items:
                st, k = self.state[p], p.numel()
                if st.get("momentum_buffer") is not None:      # after load_state_dict: adopt the loaded buffer
                    flat[off:off + k].copy_(st["momentum_buffer"].reshape(-1))
                st["momentum_buffer"] = flat[off:off + k].view(p.shape)
            plan.state = flat
        return plan.state

    def _run_state(self, gi, run):
        if self.param_groups[gi]["momentum"] == 0:
            return None
        st, n = self.state[run[0]], sum(p.numel() for p in run)
        flat = st.get("_flat_momentum")
        if flat is None or flat.numel() != n or not _views_alias(flat, [self.state[p].get("momentum_buffer") for p in run]):
            flat, o = self._zeros(n, torch.float32, run[0].device), 0
            for p in run:
                k = p.numel()
                if self.state[p].get("momentum_buffer") is not None:
                    flat[o:o + k].copy_(self.state[p]["momentum_buffer"].reshape(-1))
                self.state[p]["momentum_buffer"] = flat[o:o + k].view(p.shape)
                o += k
            st["_flat_momentum"] = flat
        return flat

    def _launch(self, L, R, base, gbase, gids, buf, gs, fi, stream):
        if R.host is None:
            R.host = {n: (ctypes.c_float * R.ngroups)() for n in ("lr", "momentum", "weight_decay", "trust_coefficient")}
            R.host.update({n: (ctypes.c_int32 * R.ngroups)() for n in ("nesterov", "adapt", "maximize")})
        H = R.host
        for j, gi in enumerate(gids):
            g = self.param_groups[gi]
            H["lr"][j], H["momentum"][j], H["weight_decay"][j] = float(g["lr"]), float(g["momentum"]), float(g["weight_decay"])
            H["trust_coefficient"][j] = float(g["trust_coefficient"])
            H["nesterov"][j], H["adapt"][j], H["maximize"][j] = int(g["nesterov"]), int(g.get("adapt", True)), int(g["maximize"])
        _lib.check(L.bvc_op_lars_step_table(
            base, gbase, buf.data_ptr() if buf is not None else None, R.n, R.seg_start.data_ptr(), R.seg_group.data_ptr(),
            R.blk_seg.data_ptr(), R.nseg, R.items.data_ptr() if R.nitems else None, R.nitems, R.first.data_ptr(), R.ngroups, H["lr"],
            H["momentum"], H["weight_decay"], H["trust_coefficient"], H["nesterov"], H["adapt"], H["maximize"], R.table.data_ptr(),
            R.partial.data_ptr(), R.stats.data_ptr(), gs, fi, 1, _flat.shadow_for(base, R.n), stream), "bvc_op_lars_step_table")


class LAMB(_LayerwiseOptimizer):
    """LAMB (You et al. 2020) with bias correction, per parameter tensor ``w`` with gradient ``g``::

        m = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g*g
        u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + weight_decay * w
        r = ||w|| / ||u||   if adapt and ||w|| > 0 and ||u|| > 0, else 1 ;  w -= lr * r * u

    ``adapt`` is a per-group key (default True); with ``adapt=False`` a group is AdamW.  State as ``bvc.optim.Adam``: ``step`` (one
    count per group, on the device: a step GradScaler skips does not advance it), ``exp_avg``, ``exp_avg_sq``.  One
    ``bvc_op_lamb_step_table`` call per flat module and step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, *, maximize=False, max_grad_norm=None):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid hyper-parameter")
        self._setup(max_grad_norm)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, adapt=True, maximize=maximize))

    def _adopt(self, params_at, n, ngroups, device):
        """Flat exp_avg / exp_avg_sq over `n` elements and 3 step scalars per group, {step, 1 / (1 - b1^step), 1 / sqrt(1 - b2^step)};
        loaded per-parameter state is adopted (a group shares one step count), the per-parameter entries become views."""
        m, v = self._zeros(n, torch.float32, device), self._zeros(n, torch.float32, device)
        state = self._zeros(3 * ngroups, torch.float32, device)
        for off, p, row in params_at:
            st, k = self.state[p], p.numel()
            if "exp_avg" in st:
                m[off:off + k].copy_(st["exp_avg"].reshape(-1))
                v[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
                state[3 * row] = float(st["step"])
            st["exp_avg"], st["exp_avg_sq"] = m[off:off + k].view(p.shape), v[off:off + k].view(p.shape)
            st["step"] = state[3 * row]
        return m, v, state

    def _plan_state(self, plan):
        if plan.state is None:
            plan.state = self._adopt(plan.items, plan.n, len(self.param_groups), plan.module._flat.device)
        return plan.state

    def _run_state(self, gi, run):
        st, n = self.state[run[0]], sum(p.numel() for p in run)
        flat = st.get("_flat_lamb")
        if (flat is None or flat[0].numel() != n or not _views_alias(flat[0], [self.state[p].get("exp_avg") for p in run])
                or any(self.state[p]["step"].data_ptr() != flat[2].data_ptr() for p in run)):
            at, o = [], 0
            for p in run:
                at.append((o, p, 0))
                o += p.numel()
            flat = st["_flat_lamb"] = self._adopt(at, n, 1, run[0].device)
        return flat

    def _launch(self, L, R, base, gbase, gids, flat, gs, fi, stream):
        if R.host is None:
            R.host = {n: (ctypes.c_double * R.ngroups)() for n in ("lr", "beta1", "beta2", "eps", "weight_decay")}
            R.host.update({n: (ctypes.c_int32 * R.ngroups)() for n in ("adapt", "maximize")})
        H = R.host
        for j, gi in enumerate(gids):
            g = self.param_groups[gi]
            H["lr"][j], H["beta1"][j], H["beta2"][j] = float(g["lr"]), float(g["betas"][0]), float(g["betas"][1])
            H["eps"][j], H["weight_decay"][j] = float(g["eps"]), float(g["weight_decay"])
            H["adapt"][j], H["maximize"][j] = int(g.get("adapt", True)), int(g["maximize"])
        m, v, state = flat
        _lib.check(L.bvc_op_lamb_step_table(
            base, gbase, m.data_ptr(), v.data_ptr(), R.n, R.seg_start.data_ptr(), R.seg_group.data_ptr(), R.blk_seg.data_ptr(), R.nseg,
            R.items.data_ptr() if R.nitems else None, R.nitems, R.first.data_ptr(), R.ngroups, H["lr"], H["beta1"], H["beta2"], H["eps"],
            H["weight_decay"], H["adapt"], H["maximize"], state.data_ptr(), R.table.data_ptr(), R.partial.data_ptr(), R.stats.data_ptr(),
            gs, fi, 1, _flat.shadow_for(base, R.n), stream), "bvc_op_lamb_step_table")


def adaptive_param_groups(model, weight_decay, no_adapt=()):
    """The usual LARS / LAMB exclusion as two parameter groups: 1-D tensors, ``*.bias`` and the names in ``no_adapt`` get
    ``weight_decay=0, adapt=False`` (group ``no_adapt``: plain momentum SGD / AdamW), the rest the given decay and ``adapt=True``
    (group ``adapt``).  Parameters with ``requires_grad=False`` are left out."""
    skip = set(no_adapt)
    adapted, plain = [], []
    for name, p in model.named_parameters():
        if p.requires_grad:
            (plain if p.ndim <= 1 or name.endswith(".bias") or name in skip else adapted).append(p)
    return [{"name": "adapt", "params": adapted, "weight_decay": weight_decay, "adapt": True},
            {"name": "no_adapt", "params": plain, "weight_decay": 0.0, "adapt": False}]


# ---------------------------------------------------------------------------------------------- layer-wise learning-rate decay
def _layer_ids(model):
    """-> ({parameter name: layer id}, L) with id 0 for the embeddings, i + 1 for encoder layer i and L + 1 for everything after."""
    import re
    from .jepa import VisionTransformer
    from .videomae import VideoMAEForVideoClassification
    names = [n for n, _ in model.named_parameters()]
    if isinstance(model, VideoMAEForVideoClassification):
        layer, emb = re.compile(r"videomae\.encoder\.layer\.(\d+)\."), "videomae.embeddings."
        depth = int(model.config.num_hidden_layers)
        ids = {}
        for n in names:
            hit = layer.match(n)
            ids[n] = 0 if n.startswith(emb) else int(hit.group(1)) + 1 if hit else depth + 1
        return ids, depth
    if isinstance(model, VisionTransformer):
        layer = re.compile(r"blocks\.(\d+)\.")
        depth = 1 + max(int(layer.match(n).group(1)) for n in names if layer.match(n))
        ids = {}
        for n in names:
            hit = layer.match(n)
            if n == "pos_embed" or n.startswith("patch_embed."):
                ids[n] = 0
            elif hit:
                ids[n] = int(hit.group(1)) + 1
            elif n.startswith("norm."):
                ids[n] = depth + 1
            else:
                raise ValueError(f"layer_decay_param_groups: no layer id for parameter {n!r}")
        return ids, depth
    raise TypeError(f"layer_decay_param_groups: {type(model).__name__} is neither VideoMAEForVideoClassification nor a JEPA encoder")


def layer_decay_param_groups(model, lr, weight_decay, layer_decay, no_weight_decay=()):
    """Parameter groups for fine-tuning with layer-wise learning-rate decay, for ``bvc.optim.AdamW`` (or ``torch.optim.AdamW``).

    With L encoder layers, the embeddings have layer id 0, encoder layer i has id i + 1, everything after the encoder (final norm,
    ``fc_norm``, ``classifier``) has id L + 1; a parameter of layer id k trains at ``lr * layer_decay ** (L + 1 - k)``.  Each layer is
    split in two: 1-D tensors, ``*.bias`` and the names in ``no_weight_decay`` get ``weight_decay`` 0, the rest the given value.
    That is up to ``2 * (L + 2)`` groups (``layer_{k}_decay`` / ``layer_{k}_no_decay``; empty ones are left out), each with its
    ``lr_scale`` so that a schedule can rescale them (``set_base_lr``).  Parameters with ``requires_grad=False`` are left out."""
    ids, depth = _layer_ids(model)
    skip = set(no_weight_decay)
    groups = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        k = ids[name]
        plain = p.ndim == 1 or name.endswith(".bias") or name in skip
        key = (k, plain)
        if key not in groups:
            scale = float(layer_decay) ** (depth + 1 - k)
            groups[key] = {"name": f"layer_{k}_{'no_decay' if plain else 'decay'}", "lr_scale": scale, "lr": lr * scale,
                           "weight_decay": 0.0 if plain else weight_decay, "params": []}
        groups[key]["params"].append(p)
    return [groups[key] for key in sorted(groups, key=lambda t: (t[0], t[1]))]


def set_base_lr(optimizer, lr):
    """Sets every group's ``lr`` to ``lr * group["lr_scale"]`` (1 where a group has none): the one line a warm-up or cosine schedule
    needs on top of ``layer_decay_param_groups``."""
    for g in optimizer.param_groups:
        g["lr"] = lr * g.get("lr_scale", 1.0)


# ---------------------------------------------------------------------------------------------- the immediate forms
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` (same signature, same return value) for torch optimisers, or for gradients that are to be
    clipped before they are logged; the ``bvc.optim`` optimisers clip inside their step (``max_grad_norm=``) at no extra pass.

    f32 CUDA gradients with ``norm_type == 2``: one launch pair per run of memory-adjacent parameters (a whole flat module is one
    run), one launch for the clip values on the device, one in-place scaling per run that writes nothing while the clip is inactive;
    no host synchronisation unless ``error_if_nonfinite``.  Anything else goes to torch's function."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = list(parameters)
    with_grad = [p for p in params if p.grad is not None]
    fast = bool(with_grad) and float(norm_type) == 2.0 and all(
        p.is_cuda and p.dtype == torch.float32 and p.grad.dtype == torch.float32 and p.grad.device == with_grad[0].device
        and p.grad.is_contiguous() and p.is_contiguous() for p in with_grad)
    if not fast:
        return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite, foreach=foreach)
    max_norm = _checked_max_grad_norm(max_norm)
    dev = with_grad[0].device
    L = _lib.lib()
    runs = SGD._contiguous_runs(with_grad)
    sq, out = torch.zeros(len(runs), dtype=torch.float32, device=dev), torch.zeros(3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = _lib.current_stream_ptr()
        sizes = [sum(p.numel() for p in run) for run in runs]
        for i, (run, n) in enumerate(zip(runs, sizes)):
            _run_table(n, dev).launch(L, run[0].grad.data_ptr(), sq.data_ptr() + 4 * i, None, stream)
        _lib.check(L.bvc_op_clip_finalize(sq.data_ptr(), len(runs), max_norm, None, out.data_ptr(), stream), "bvc_op_clip_finalize")
        if error_if_nonfinite and not bool(torch.isfinite(out[0])):      # (the one case that waits for the device)
            raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it cannot be "
                               "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                               "`error_if_nonfinite=False`")
        for run, n in zip(runs, sizes):
            _lib.check(L.bvc_op_scale_by_dev(run[0].grad.data_ptr(), n, out.data_ptr() + 4, stream), "bvc_op_scale_by_dev")
    return out[0]


def grad_norms(module):
    """Per-parameter gradient norms of a module in ONE launch pair and without a host synchronisation:
    ``{state-dict name: 0-d device view}`` for every parameter that has a gradient, and ``"total"``.  The gradients are taken as one
    segment table in address order - a flat module's gradient buffer is one stretch of it, gradients outside it are further
    segments, the memory between them belongs to nobody - so the work list is rebuilt only when a gradient has moved.  The views
    alias one device tensor that the next call for the same module overwrites."""
    named = [(n, p) for n, p in module.named_parameters() if p.grad is not None]
    if not named:
        raise _lib.BvcError("grad_norms: no parameter of the module has a gradient")
    dev = named[0][1].grad.device
    for n, p in named:
        g = p.grad
        if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.device == dev):
            raise _lib.BvcError(f"grad_norms: the gradient of {n} is not a contiguous f32 tensor on {dev}")
    named.sort(key=lambda t: t[1].grad.data_ptr())
    key = tuple((p.grad.data_ptr(), p.numel()) for _, p in named)
    cache = getattr(module, "_bvc_grad_norms", None)
    if cache is None or cache[0] != key:
        base, starts, groups, where, pos = key[0][0], [], [], {}, 0
        for (name, _p), (ptr, k) in zip(named, key):
            off = (ptr - base) // 4
            if off < pos or (ptr - base) % 4:
                raise _lib.BvcError(f"grad_norms: the gradient of {name} overlaps another one")
            if off > pos:
                starts.append(pos); groups.append(-1)
            where[name] = len(groups)
            starts.append(off); groups.append(0)
            pos = off + k
        starts.append(pos)
        table = _NormTable(starts, groups, dev)
        cache = (key, table, where, torch.zeros(table.nseg + 1, dtype=torch.float32, device=dev))
        module._bvc_grad_norms = cache
    _key, table, where, out = cache
    with torch.cuda.device(dev):
        table.launch(_lib.lib(), key[0][0], out.data_ptr() + 4 * table.nseg, None, _lib.current_stream_ptr(), seg_out=out.data_ptr(), as_norm=1)
    norms = {name: out[i] for name, i in where.items()}
    norms["total"] = out[table.nseg]
    return norms
