"""The gradient-norm kernels on raw tensors through the C ABI (include/bvc.h "gradient-norm clipping"): the segmented squared norm with
its fixed-order reduce and the inf check on the same read, the clip values on the device, the in-place scaling by a device scalar.

One buffer for every norm test, laid out to hit each path of the item kernel:

    [0, 1)            owned, a single element
    [1, 4)            hole, filled with NaN
    [4, 7)            owned, unaligned start, shorter than a vector
    [7, 7 + 1025)     owned, starts 3 elements before a 16-byte boundary
    next 4            hole holding +Inf
    next 3 cap + 5    owned: three full items (whole vectors only while the base is 16-byte aligned) and one of 5 elements
    last 3001..3004   owned, unaligned start, ends at n with n % 4 == 3

Every owned segment is drawn at its own magnitude - once balanced, so that each contributes a comparable share to the total and a
dropped or doubled segment moves the total by tens of percent, once spread over 1e-4 .. 1e3, where the per-segment sums catch it.

The bar is derived, not tuned.  The relative error of a sum of n non-negative f32 terms is at most (depth + 1) 2^-24 when every term
passes through at most `depth` rounded additions and its square is rounded once; a kernel whose longest serial chain is S terms and
that adds the rest as a tree has depth <= S + ceil(log2(n / S)) + 1, which gives (S + ceil(log2(n / S)) + 2) 2^-24.  S is exported
(bvc_op_grad_norm_chain).  This library's kernel stays well inside it: above the per-thread f32 chain it adds in f64.  A norm, the
square root of such a sum, gets half the bar."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_util as G   # noqa: E402

bvc = G.bvc
dev = torch.device("cuda:0")
U = 2.0 ** -24


def _lib():
    return bvc._lib.lib()


def _bar(n, chain):
    return (chain + max(0, math.ceil(math.log2(max(n, 1) / chain))) + 2) * U


class _Layout:
    def __init__(self, mags, seed=0):
        L = _lib()
        self.cap, self.chain = L.bvc_op_grad_norm_item_cap(), L.bvc_op_grad_norm_chain()
        cap = self.cap
        lengths = [1, 3, 3, 1025, 4, 3 * cap + 5, 3001]
        lengths[-1] += (3 - sum(lengths)) % 4
        self.groups = [0, -1, 1, 0, -1, 2, 1]
        self.starts = [0] + list(np.cumsum(lengths))
        self.n = int(self.starts[-1])
        assert self.n % 4 == 3 and self.starts[2] == 4 and self.starts[3] == 7 and self.starts[5] % 4 == 0 and self.starts[6] % 4 == 1
        gen = torch.Generator().manual_seed(seed)
        x = torch.zeros(self.n)
        owned = [s for s, g in enumerate(self.groups) if g >= 0]
        assert len(mags) == len(owned)
        for s, mag in zip(owned, mags):
            a, b = self.starts[s], self.starts[s + 1]
            # (segments shorter than a vector get fixed values: their share of the total must not hang on one random draw)
            x[a:b] = (torch.randn(b - a, generator=gen) if b - a >= 4 else torch.tensor([1.0, -0.75, 1.25][:b - a])) * mag
        x[self.starts[1]:self.starts[2]] = float("nan")
        x[self.starts[4]:self.starts[5]] = float("inf")
        self.host = x
        self.owned = owned
        # the float64 reference of the same f32 values: computed once, shared, never changed
        self.seg_ref = [float(x[self.starts[s]:self.starts[s + 1]].double().square().sum()) if g >= 0 else 0.0 for s, g in enumerate(self.groups)]
        self.total_ref = sum(self.seg_ref)
        self.n_owned = sum(self.starts[s + 1] - self.starts[s] for s in owned)
        items, first = bvc.optim.grad_norm_work_list(self.starts, self.groups)
        self.table = bvc.optim._NormTable(self.starts, self.groups, dev)
        assert self.table.nitems == items.shape[0] == 1 + 1 + 1 + 4 + 1

    def run(self, x, found=None, as_norm=0):
        """-> (seg [nseg], total [1], item partials) of the range at x's address"""
        t = self.table
        seg, total = torch.full((t.nseg,), -1.0, device=dev), torch.full((1,), -1.0, device=dev)
        t.launch(_lib(), x.data_ptr(), total.data_ptr(), found.data_ptr() if found is not None else None, G.stream(), seg_out=seg.data_ptr(),
                 as_norm=as_norm)
        torch.cuda.synchronize()
        return seg.cpu(), total.cpu(), t.partial[:t.nitems].clone().cpu()


BALANCED = (1e3, 5e2, 30.0, 4.0, 17.0)      # every segment contributes 6e5 .. 1e6 to the total
SPREAD = (1e-4, 1e-2, 1.0, 1e2, 1e3)
_LAYOUTS = {}


def _layout(kind):
    if kind not in _LAYOUTS:
        _LAYOUTS[kind] = _Layout(BALANCED if kind == "balanced" else SPREAD, seed=1 if kind == "balanced" else 2)
    return _LAYOUTS[kind]


def _check(lay, seg, total, half=False):
    scale = 0.5 if half else 1.0
    for s, g in enumerate(lay.groups):
        ref = math.sqrt(lay.seg_ref[s]) if half else lay.seg_ref[s]
        if g < 0:
            assert float(seg[s]) == 0.0, f"unowned segment {s}: {float(seg[s])}"
            continue
        n = lay.starts[s + 1] - lay.starts[s]
        rel = abs(float(seg[s]) - ref) / ref
        bar = scale * _bar(n, lay.chain)
        print(f"segment {s} n={n}: rel {rel:.3e} bar {bar:.3e}")
        assert rel <= bar, f"segment {s} (n={n}): rel {rel:.3e} > {bar:.3e}"
    ref = math.sqrt(lay.total_ref) if half else lay.total_ref
    rel = abs(float(total[0]) - ref) / ref
    bar = scale * _bar(lay.n_owned, lay.chain)
    print(f"total n={lay.n_owned}: rel {rel:.3e} bar {bar:.3e}")
    assert rel <= bar, f"total: rel {rel:.3e} > {bar:.3e}"


@pytest.mark.parametrize("kind", ["balanced", "spread"])
def test_segmented_squared_norm_against_float64(kind):
    lay = _layout(kind)
    x = lay.host.to(dev)
    assert x.data_ptr() % 16 == 0
    found = torch.zeros((), device=dev)
    seg, total, part = lay.run(x, found)
    _check(lay, seg, total)
    assert float(found) == 0.0                      # the NaN and +Inf holes are inside no item
    if kind == "balanced":                          # a dropped or doubled segment would be far outside the bar
        assert min(lay.seg_ref[s] for s in lay.owned) / lay.total_ref > 1000 * _bar(lay.n_owned, lay.chain)
    # two calls: identical bits, partials included
    seg2, total2, part2 = lay.run(x, found)
    assert torch.equal(seg.view(torch.int32), seg2.view(torch.int32)) and torch.equal(total.view(torch.int32), total2.view(torch.int32))
    assert torch.equal(part.view(torch.int64), part2.view(torch.int64))
    # the norms themselves (as_norm): half the bar
    seg, total, _ = lay.run(x, None, as_norm=1)
    _check(lay, seg, total, half=True)
    # without seg_sq: the total alone, the same bits
    only = torch.full((1,), -1.0, device=dev)
    lay.table.launch(_lib(), x.data_ptr(), only.data_ptr(), None, G.stream())
    torch.cuda.synchronize()
    assert torch.equal(only.cpu().view(torch.int32), total2.view(torch.int32))


def test_found_inf_sees_owned_elements_only():
    lay = _layout("balanced")
    x = lay.host.to(dev)
    found = torch.zeros((), device=dev)
    lay.run(x, found)
    assert float(found) == 0.0
    # one owned element each: in the single-element segment, in a head, in a vector of a full item, in the last tail
    for at in (0, lay.starts[3], lay.starts[5] + lay.cap + 77, lay.n - 1):
        for poison in (float("inf"), float("-inf"), float("nan")):
            y = x.clone()
            y[at] = poison
            found.zero_()
            lay.run(y, found)
            assert float(found) == 1.0, (at, poison)
    found.fill_(1.0)
    lay.run(x, found)
    assert float(found) == 1.0                      # never cleared


def test_base_pointer_offset_by_one_element():
    lay = _layout("balanced")
    room = torch.zeros(lay.n + 1, device=dev)
    y = room[1:]
    y.copy_(lay.host)
    assert y.data_ptr() % 16 == 4
    found = torch.zeros((), device=dev)
    seg, total, _ = lay.run(y, found)
    _check(lay, seg, total)
    assert float(found) == 0.0


def _finalize(sq, max_norm, scale):
    out = torch.full((3,), -1.0, device=dev)
    sq_d = torch.tensor(sq, dtype=torch.float32, device=dev)
    gs = torch.tensor([scale], dtype=torch.float32, device=dev) if scale is not None else None
    bvc._lib.check(_lib().bvc_op_clip_finalize(G.ptr(sq_d), len(sq), max_norm, G.ptr(gs), G.ptr(out), G.stream()), "bvc_op_clip_finalize")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("scale", [None, 65536.0, 3.0])
def test_clip_finalize(scale):
    f = np.float32
    s = f(1.0) if scale is None else f(scale)
    sq = [f(2.5) * s * s, f(0.75) * s * s, f(6.0) * s * s]                 # three ranges; total norm ~ 3.04 after unscaling
    norm = f(np.sqrt(f(np.sum(np.asarray(sq, dtype=np.float64))))) / s       # the f32 formula (the three squares are added exactly first)
    # below max_norm: the clip is inactive, exactly
    out = _finalize(sq, 5.0, scale)
    assert abs(out[0] - norm) <= 2 * np.spacing(norm)
    assert out[1] == f(1.0) and out[2] == s
    # above max_norm
    out = _finalize(sq, 1.0, scale)
    coef = f(1.0) / (norm + f(1e-6))
    assert coef < 1.0
    assert abs(out[0] - norm) <= 2 * np.spacing(norm)                        # device sqrt and divide: within an ulp each
    assert abs(out[1] - coef) <= 4 * np.spacing(coef)
    assert abs(out[2] - s / out[1]) <= 2 * np.spacing(s / out[1])             # eff_scale is scale / clip_coef of the very coefficient reported
    # a nonfinite square propagates as in torch: norm inf -> coefficient 0; norm NaN -> NaN (torch's clamp keeps a NaN)
    out = _finalize([f(1.0), f(np.inf), f(1.0)], 1.0, scale)
    assert np.isinf(out[0]) and out[1] == 0.0
    out = _finalize([f(1.0), f(np.nan), f(1.0)], 1.0, scale)
    assert np.isnan(out[0]) and np.isnan(out[1]) and np.isnan(out[2])
    # max_norm 0 and inf
    assert _finalize(sq, 0.0, scale)[1] == 0.0
    assert _finalize(sq, float("inf"), scale)[1] == 1.0
    assert _lib().bvc_op_clip_finalize(None, 0, ctypes.c_float(-1.0), None, None, G.stream()) != 0


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_scale_by_dev(offset):
    n = 4 * 256 * 9 + 3                                 # more than one block, a tail
    gen = torch.Generator().manual_seed(offset)
    host = torch.randn(n, generator=gen)
    host[5], host[6] = -0.0, float("inf")
    room = torch.zeros(n + offset, device=dev)
    x = room[offset:]
    x.copy_(host)
    one, c = torch.ones((), device=dev), torch.tensor(0.3371, device=dev)
    L = _lib()
    bvc._lib.check(L.bvc_op_scale_by_dev(G.ptr(x), n, G.ptr(one), G.stream()), "bvc_op_scale_by_dev")
    torch.cuda.synchronize()
    assert torch.equal(x.cpu().view(torch.int32), host.view(torch.int32))                  # a coefficient of 1: untouched
    bvc._lib.check(L.bvc_op_scale_by_dev(G.ptr(x), n, G.ptr(c), G.stream()), "bvc_op_scale_by_dev")
    torch.cuda.synchronize()
    want = host * torch.tensor(0.3371)
    assert torch.equal(x.cpu().view(torch.int32), want.view(torch.int32))
    assert offset == 0 or float(room[offset - 1]) == 0.0                                    # nothing before the range
