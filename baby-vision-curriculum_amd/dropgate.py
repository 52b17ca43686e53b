"""Stochastic depth and hidden dropout: the host side of the gate on a layer's two residual branches (include/bvc.h, bvc_branch_drop).

The gates follow ``module.training`` alone, as ``nn.Dropout`` and the reference's ``drop_path(x, p, self.training)``
(pretraining/predictive/vision_transformer.py:145-153) do.  Randomness comes from torch's generator of the model's device, without a
host sync: the stochastic-depth draws are one ``torch.rand`` on the device, the hidden-dropout mask is a function of the generator's
seed and of a counter range reserved from its offset (host-side state, taken by value) - so ``torch.manual_seed(s)`` reproduces a
run.  Ranks that share a seed share masks, exactly as with torch's own dropout under DistributedDataParallel.
"""
import ctypes

import torch

from . import _lib


def drop_path_schedule(drop_path_rate, depth):
    """Per-layer rates, ``[x.item() for x in torch.linspace(0, drop_path_rate, depth)]`` (vision_transformer.py:332): layer 0 never
    drops, and a one-layer stack drops nothing."""
    return [x.item() for x in torch.linspace(0, float(drop_path_rate), int(depth))]


def path_scale_from_uniform(u, rates, keep=None):
    """``drop_path``'s arithmetic on uniform draws ``u`` [depth, 2, samples]: floor(keep + u) / keep with keep = 1 - rate, i.e. 0 for a
    dropped sample and 1 / keep for a kept one; exactly 1 where the rate is 0 (the reference skips the branch gate there).
    ``keep``: the [depth, 1, 1] tensor of 1 - rate already on ``u``'s device (a caller that draws every step keeps it)."""
    if keep is None:
        keep = (1.0 - torch.tensor(rates, dtype=torch.float32)).to(u.device).view(-1, 1, 1)
    scale = torch.floor(keep + u) / keep
    return torch.where(keep >= 1.0, torch.ones_like(scale), scale).contiguous()


def take_counter_range(device):
    """(seed, offset) of torch's generator for ``device``; the offset advances by 4 so that the next taker gets another range."""
    gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
    seed, offset = int(gen.initial_seed()), int(gen.get_offset())
    gen.set_offset(offset + 4)
    return seed, offset


class BranchGate:
    """What one gated module owns: rates, and what the last gated forward used (``scale`` = ``model.drop_path_scale``, ``state`` =
    ``model.dropout_state``)."""

    def __init__(self, depth, drop_path_rate=0.0, hidden_p=0.0):
        self.depth, self.drop_path_rate, self.hidden_p = int(depth), float(drop_path_rate), float(hidden_p)
        for name, v in (("drop_path_rate", self.drop_path_rate), ("hidden_dropout_prob", self.hidden_p)):
            if not 0.0 <= v < 1.0:
                raise ValueError(f"{name}={v} must lie in [0, 1)")
        self.rates = drop_path_schedule(self.drop_path_rate, self.depth)
        self.scale, self.state = None, None
        self._keep = {}      # device -> [depth, 1, 1] tensor of 1 - rate (uploaded once)

    def __deepcopy__(self, memo):
        return BranchGate(self.depth, self.drop_path_rate, self.hidden_p)

    @property
    def enabled(self):
        return self.drop_path_rate > 0.0 or self.hidden_p > 0.0

    def arm(self, set_drop, ctx, device, samples, rows_per_sample):
        """Draw the gates of one forward and hand them to the library context (``set_drop`` = its bvc_*_set_drop)."""
        scale = None
        if self.drop_path_rate > 0.0:
            keep = self._keep.get(device)
            if keep is None:
                keep = self._keep[device] = (1.0 - torch.tensor(self.rates, dtype=torch.float32)).to(device).view(-1, 1, 1)
            scale = path_scale_from_uniform(torch.rand((self.depth, 2, samples), dtype=torch.float32, device=device), self.rates, keep)
        seed, offset = take_counter_range(device) if self.hidden_p > 0.0 else (0, 0)
        d = _lib.branch_drop(self.hidden_p, seed, offset, scale, rows_per_sample)
        _lib.check(set_drop(ctx, ctypes.byref(d), int(samples), _lib.current_stream_ptr()), "set_drop")
        self.scale, self.state = scale, (seed, offset, self.hidden_p)


def dropout_mask(seed, offset, layer, branch, rows, cols, p, device):
    """The keep mask (uint8, 1 = kept) [rows, cols] of one branch as the kernels evaluate it (bvc_op_dropout_mask)."""
    out = torch.empty((rows, cols), dtype=torch.uint8, device=device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().bvc_op_dropout_mask(int(seed), int(offset), int(layer), int(branch), int(rows), int(cols), float(p), out.data_ptr(),
                                                  _lib.current_stream_ptr()), "bvc_op_dropout_mask")
    return out


def dropout_mask_host(seed, offset, layer, branch, rows, cols, p):
    """The same mask from the generator's host twin (bvc_dropout_mask_host): no GPU needed."""
    out = torch.empty((rows, cols), dtype=torch.uint8)
    _lib.check(_lib.lib().bvc_dropout_mask_host(int(seed), int(offset), int(layer), int(branch), int(rows), int(cols), float(p), out.data_ptr()),
               "bvc_dropout_mask_host")
    return out
