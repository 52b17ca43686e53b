"""bvc_op_topk (csrc/retrieval.hip, through the C ABI) and bvc.retrieval: the k nearest f32 keys of every f32 query.

Reference, model, inputs and the tie-aware comparison: tests/retrieval_ref.py (pinned on the CPU by tests/test_retrieval_ref.py).
Operands, outputs and workspace are carved from an attention_ref.Arena (NaN-reading guard bands on both sides of each, checked after
every call); the outputs are pre-filled with a poison (index -12345, value NaN) and every one of the Q x k slots must have been
written.  Every figure is printed and logged (gpu_util.log_parity) before anything is asserted.

Bars, per case:
  tau = ROW_BAR x the worst |model32 - scores64| of the case's own inputs, ROW_BAR = 2.5 (the project's ratio,
    tests/test_gpu_attention_edges.py): check_topk with that tau - membership, completeness, no duplicates, values, order.
    The model is evaluated on every query where that is cheap and on the first 64 (16 for the 20 000-key case) otherwise.
  every value within retrieval_ref.value_cap of its float64 distance.  For cosine that is the issue's derivable D 2^-23 from D = 5
    on; two mendings, both derived in value_cap's docstring: below D = 5 the nine rounded operations outside the dot chain outweigh
    D 2^-23 (at D = 1 it would be one ulp of 1.0), so the cap there is (2 D + 7) 2^-24; and for the Euclidean metric, whose operands
    are not unit vectors, the bound is taken in the units of the expanded d2 and carried through the square root (a close pair at
    D = 1 has |d2 error| / 2 d far above D 2^-23 in ANY float32 evaluation of that formula, the model included).
  at most 10 % of a case's queries ambiguous (checked for every case here with the model alone on the CPU: 0 everywhere but the grid's 768 x 4097 x
    300 Euclidean case with 5 of 300, its 1280 x 4097 x 300 cosine case with 1 of 300, and the two clustered cases with 1 and 0 of 128).
  Cosine at D = 1 has scores of +-1 only - every query is ambiguous at any seed - so the grid pairs D = 1 with cosine only where
  all keys are returned (N = 1) and otherwise with the Euclidean metric.
The order the op guarantees is (value ascending, index ascending) on the returned bits; see csrc/retrieval.hip.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():   # collected on the CPU box, run on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import attention_ref as AR   # noqa: E402
from tests import gpu_util as G   # noqa: E402
from tests import retrieval_ref as R   # noqa: E402

L = G.L
dev = "cuda"
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
ROW_BAR = 2.5
POISON = -12345
METRIC = {"cosine": 0, "euclidean": 1}

_cache = {}


def _case(kind, Q, N, D, seed, metric, rows=None):
    """Inputs, float64 scores and the model's error of a case, computed once and shared (never modified)."""
    key = (kind, Q, N, D, seed, metric)
    if key not in _cache:
        if kind == "gauss":
            q, k = R.gaussian(Q, N, D, seed)
            yq = yk = None
        elif kind == "clusters":
            q, k, yq, yk = R.clustered(Q, N, D, seed)
        else:
            q, k = R.small_integers(Q, N, D, seed)
            yq = yk = None
        if rows is None:
            rows = Q if Q * N * D <= 1.3e8 else 64
        for a in (q, k):
            a.setflags(write=False)
        _cache[key] = dict(q=q, k=k, yq=yq, yk=yk, s=R.scores64(q, k, metric), model=R.model_error(q, k, metric, rows), metric=metric)
    return _cache[key]


def _topk(q, k, kk, metric, key_splits=0, ldq=None, ldk=None, chunks=None, repeat=1):
    """bvc_op_topk on guarded memory; returns (idx, val) as numpy arrays.  `chunks`: key counts of an accumulate loop."""
    Q, D = q.shape
    N = k.shape[0]
    ldq, ldk = ldq or D, ldk or D
    parts = [(0, N)] if chunks is None else [(sum(chunks[:i]), c) for i, c in enumerate(chunks)]
    assert sum(c for _, c in parts) == N
    nbytes = max(L.lib().bvc_op_topk_workspace(Q, c, D, kk, key_splits) for _, c in parts)
    assert nbytes > 0
    A = AR.Arena(dev, q=((Q, ldq), F32), k=((N, ldk), F32), idx=((Q, kk), I32), val=((Q, kk), F32), ws=((nbytes,), U8))
    for name, src in (("q", q), ("k", k)):
        A[name].fill_(float("nan"))           # the padding columns read as NaN
        A[name][:, :D].copy_(torch.from_numpy(src.copy()))
    out = None
    for _ in range(repeat):
        A["idx"].fill_(POISON)
        A["val"].fill_(float("nan"))
        for i, (start, count) in enumerate(parts):
            L.check(L.lib().bvc_op_topk(G.ptr(A["q"]), ldq, ctypes.c_void_p(A["k"][start:].data_ptr()), ldk, Q, count, D, kk,
                                        METRIC[metric], key_splits, start, 0 if i == 0 else 1, G.ptr(A["idx"]), G.ptr(A["val"]),
                                        G.ptr(A["ws"]), G.stream()), "bvc_op_topk")
        torch.cuda.synchronize()
        idx, val = A["idx"].cpu().numpy(), A["val"].cpu().numpy()
        A.check()
        assert (idx != POISON).all() and not np.isnan(val).any(), "an output slot was not written"
        assert np.array_equal(A["q"][:, :D].cpu().numpy(), q) and np.array_equal(A["k"][:, :D].cpu().numpy(), k), "operand changed"
        if out is not None:
            assert np.array_equal(out[0], idx) and np.array_equal(out[1].view(np.int32), val.view(np.int32)), "two runs differ"
        out = (idx, val)
    return out


def _hold(label, idx, val, c, kk):
    """Figures first (printed and logged), then check_topk, the cap and the ambiguity condition."""
    q, k, s, metric = c["q"], c["k"], c["s"], c["metric"]
    Q, N = s.shape
    tau = ROW_BAR * c["model"]
    m = min(kk, N)
    safe = np.clip(idx[:, :m].astype(np.int64), 0, N - 1)
    err = np.abs(val[:, :m].astype(np.float64) - R.distance(np.take_along_axis(s, safe, 1), metric))
    worst = float(err.max())
    cap = float((err / np.take_along_axis(R.value_cap(q, k, metric), safe, 1)).max())
    amb = int(R.ambiguous(s, kk, tau).sum())
    ratio = worst / c["model"] if c["model"] > 0 else (0.0 if worst == 0 else float("inf"))
    G.log_parity(f"retrieval {label} {metric} Q{Q} N{N} D{q.shape[1]} k{kk}: value error {worst:.2e} / model {c['model']:.2e} = {ratio:.2f}; "
                 f"error / cap {cap:.3f}; ambiguous {amb} of {Q}")
    got_amb, _ = R.check_topk(idx, val, q, k, kk, metric, tau, s)
    assert got_amb == amb
    assert cap <= 1.0, f"a value is {cap:.2f} x its derivable worst case"
    assert amb <= 0.1 * Q, f"{amb} of {Q} queries ambiguous: choose another seed"
    return amb


# --------------------------------------------------------------------------- 1. grid
GRID = [(1, 1, 1, 1, "cosine"), (1, 49, 5, 50, "euclidean"), (1, 50, 127, 64, "euclidean"), (3, 1, 5, 5, "cosine"),
        (3, 1000, 129, 5, "euclidean"), (31, 1, 129, 50, "euclidean"), (31, 127, 127, 1, "cosine"), (32, 1, 300, 64, "cosine"),
        (32, 128, 1, 50, "euclidean"), (33, 49, 300, 64, "euclidean"), (33, 129, 5, 1, "cosine"), (100, 1000, 129, 50, "cosine"),
        (100, 127, 300, 5, "euclidean"), (384, 4097, 127, 64, "cosine"), (384, 128, 129, 50, "euclidean"),
        (768, 4097, 300, 50, "euclidean"), (768, 129, 5, 5, "cosine"), (1280, 4097, 300, 64, "cosine"), (1280, 1, 1, 1, "euclidean"),
        (1280, 50, 5, 50, "cosine")]


def test_grid_covers_every_axis_value_twice():
    for axis, values in ((0, {1, 3, 31, 32, 33, 100, 384, 768, 1280}), (1, {1, 49, 50, 127, 128, 129, 1000, 4097}),
                         (2, {1, 5, 127, 129, 300}), (3, {1, 5, 50, 64})):
        seen = [g[axis] for g in GRID]
        assert set(seen) == values and all(seen.count(v) >= 2 for v in values), axis
    pairs = {(g[1], g[3]) for g in GRID}
    assert {(1, 5), (1, 50), (1, 64), (49, 50), (49, 64), (50, 64)} <= pairs      # every N < k pairing
    assert {"cosine", "euclidean"} == {g[4] for g in GRID}


@pytest.mark.parametrize("i", range(len(GRID)), ids=[f"D{g[0]}-N{g[1]}-Q{g[2]}-k{g[3]}-{g[4][:3]}" for g in GRID])
def test_topk_grid(i):
    D, N, Q, kk, metric = GRID[i]
    c = _case("gauss", Q, N, D, 1000 + i, metric)
    idx, val = _topk(c["q"], c["k"], kk, metric)
    _hold("grid", idx, val, c, kk)
    if N < kk:
        assert (idx[:, N:] == -1).all() and np.isposinf(val[:, N:]).all()


# --------------------------------------------------------------------------- 2. clustered inputs, the score and the classifier
@pytest.mark.parametrize("D,kk,seed", [(768, 50, 3), (384, 64, 4)])
def test_clustered_topk_nn_score_and_knn_predict(D, kk, seed):
    Q, N = 128, 4097
    c = _case("clusters", Q, N, D, seed, "cosine")
    idx, val = _topk(c["q"], c["k"], kk, "cosine")
    amb = _hold("clusters", idx, val, c, kk)
    xq, xk = torch.from_numpy(c["q"].copy()).to(dev), torch.from_numpy(c["k"].copy()).to(dev)
    got = G.bvc.retrieval.nn_score(xk, torch.from_numpy(c["yk"]), xq, torch.from_numpy(c["yq"]).to(dev), ks=R.KS)
    want = R.hits(R.ranking64(c["s"])[:, :max(R.KS)], c["yk"], c["yq"])
    hits = {k: int(round(got[k] * Q)) for k in R.KS}
    G.log_parity(f"retrieval nn_score clusters D{D}: hits {hits} / float64 {want}; ambiguous {amb}")
    assert all(isinstance(v, float) for v in got.values())
    assert all(abs(hits[k] - want[k]) <= amb for k in R.KS)
    clear = ~R.ambiguous(c["s"], 20, ROW_BAR * c["model"])
    for T in (None, 0.07):
        pred = G.bvc.retrieval.knn_predict(xk, c["yk"], xq, k=20, num_classes=10, temperature=T).cpu().numpy()
        ref = R.vote64(c["s"], c["yk"], 20, 10, T)
        G.log_parity(f"retrieval knn_predict clusters D{D} T{T}: {int((pred != ref).sum())} of {Q} differ, {int((~clear).sum())} ambiguous at k = 20")
        assert pred.dtype == np.int64 and (pred[clear] == ref[clear]).all()


# --------------------------------------------------------------------------- 3. exact case
@pytest.mark.parametrize("D", [33, 768])
def test_exact_integers_pin_ties_and_indices(D):
    Q, N, kk = 129, 1000, 50
    c = _case("ints", Q, N, D, 50 + D, "euclidean", rows=1)
    idx, val = _topk(c["q"], c["k"], kk, "euclidean")
    want = R.ranking64(c["s"])[:, :kk]
    d = -np.take_along_axis(c["s"], want, 1)
    ties = int((d[:, 1:] == d[:, :-1]).sum())
    ulp = np.spacing(np.maximum(d, 2.0 ** -126).astype(np.float32)).astype(np.float64)
    off = float((np.abs(val.astype(np.float64) - d) / ulp).max())
    G.log_parity(f"retrieval exact D{D}: {int((idx != want).sum())} indices differ from the float64 ranking ({ties} tied neighbours); "
                 f"values {off:.2f} ulp from sqrt")
    assert ties > Q, "the case must be full of ties"
    assert np.array_equal(idx, want)
    assert off <= 2.0


# --------------------------------------------------------------------------- 4. duplicates
def test_duplicate_keys_carry_equal_bits_and_ascending_indices():
    Q, M, D, kk = 129, 200, 100, 50
    q, base = R.gaussian(Q, M, D, 77)
    where = np.random.RandomState(78).permutation(3 * M)      # key row j is a copy of base row where[j] % M
    k = base[where % M]
    idx, val = _topk(q, k, kk, "cosine")
    group = where[idx] % M
    bad_bits = bad_order = 0
    for i in range(Q):
        for g in np.unique(group[i]):
            at = np.nonzero(group[i] == g)[0]
            bad_bits += len(set(val[i, at].view(np.int32).tolist())) != 1
            copies = np.sort(np.nonzero(where % M == g)[0])
            bad_order += not np.array_equal(idx[i, at], copies[:len(at)])      # ascending, and the smallest ones at the cut
    G.log_parity(f"retrieval duplicates: {bad_bits} groups with unequal bits, {bad_order} groups out of index order")
    assert bad_bits == 0 and bad_order == 0
    c = dict(q=q, k=k, s=R.scores64(q, k, "cosine"), model=R.model_error(q, k, "cosine", Q), metric="cosine")
    tau = ROW_BAR * c["model"]
    R.check_topk(idx, val, q, k, kk, "cosine", tau, c["s"])


# --------------------------------------------------------------------------- 5. splits and chunks
def test_splits_chunks_and_runs_give_the_same_bits():
    Q, N, D, kk = 300, 4097, 768, 50
    c = _case("gauss", Q, N, D, 5, "cosine", rows=64)
    base = _topk(c["q"], c["k"], kk, "cosine", key_splits=1, repeat=2)
    _hold("splits", base[0], base[1], c, kk)
    assert L.lib().bvc_op_topk_splits(Q, N, D, kk) == 7
    for label, kw in [(f"key_splits {s}", dict(key_splits=s)) for s in (2, 3, 7, 8, 33, 0)] + \
                     [("chunks 1 + 1000 + 3096", dict(chunks=(1, 1000, 3096))), ("chunks, 3 splits", dict(chunks=(1, 1000, 3096), key_splits=3))]:
        idx, val = _topk(c["q"], c["k"], kk, "cosine", **kw)
        same = np.array_equal(idx, base[0]) and np.array_equal(val.view(np.int32), base[1].view(np.int32))
        G.log_parity(f"retrieval {label}: {'same bits' if same else 'DIFFERENT'} as key_splits 1")
        assert same, label
    xq, xk = torch.from_numpy(c["q"].copy()).to(dev), torch.from_numpy(c["k"].copy()).to(dev)
    out = None
    for start, stop in ((0, 1), (1, 1001), (1001, N)):
        out = G.bvc.retrieval.topk(xq, xk[start:stop], kk, out=out, key_base=start)
    assert np.array_equal(out[1].cpu().numpy(), base[0]) and np.array_equal(out[0].cpu().numpy().view(np.int32), base[1].view(np.int32))


# --------------------------------------------------------------------------- 6. strides and layout
@pytest.mark.parametrize("D,pad", [(768, 4), (768, 5), (33, 3)])
def test_strides_and_views(D, pad):
    Q, N, kk = 129, 1000, 50
    c = _case("gauss", Q, N, D, 600 + D, "cosine", rows=64)
    dense = _topk(c["q"], c["k"], kk, "cosine")
    _hold(f"dense (strides pad {pad})", dense[0], dense[1], c, kk)
    idx, val = _topk(c["q"], c["k"], kk, "cosine", ldq=D + pad, ldk=D + 2 * pad)
    assert np.array_equal(idx, dense[0]) and np.array_equal(val.view(np.int32), dense[1].view(np.int32))
    wide = torch.full((Q, D + 8), float("nan"), device=dev)
    wide[:, 4:4 + D] = torch.from_numpy(c["q"].copy()).to(dev)
    wk = torch.full((N, D + pad), float("nan"), device=dev)
    wk[:, :D] = torch.from_numpy(c["k"].copy()).to(dev)
    dist, ind = G.bvc.retrieval.topk(wide[:, 4:4 + D], wk[:, :D], kk)
    assert dist.dtype == F32 and ind.dtype == I32 and dist.shape == ind.shape == (Q, kk)
    assert np.array_equal(ind.cpu().numpy(), dense[0]) and np.array_equal(dist.cpu().numpy().view(np.int32), dense[1].view(np.int32))
    # other float dtypes are cast; a transposed operand goes through .contiguous()
    d64, i64 = G.bvc.retrieval.topk(torch.from_numpy(c["q"].copy()).to(dev).double(), torch.from_numpy(c["k"].copy()).to(dev).t().contiguous().t(), kk)
    assert np.array_equal(i64.cpu().numpy(), dense[0]) and np.array_equal(d64.cpu().numpy().view(np.int32), dense[1].view(np.int32))


# --------------------------------------------------------------------------- 7. zero rows
def test_zero_rows_have_cosine_distance_one():
    q, k = R.gaussian(5, 40, 48, 9)
    q[0] = 0
    k[3] = 0
    idx, val = _topk(q, k, 40, "cosine")
    assert not np.isnan(val).any()
    assert (val[0] == 1.0).all() and np.array_equal(idx[0], np.arange(40))      # all tied: the order is the index order
    assert (val[idx == 3] == 1.0).all() and (idx == 3).sum() == 5
    R.check_topk(idx, val, q, k, 40, "cosine", ROW_BAR * R.model_error(q, k, "cosine"))


# --------------------------------------------------------------------------- 8. one larger shape
def test_larger_gallery_with_automatic_splits():
    Q, N, D, kk = 300, 20000, 768, 50
    c = _case("gauss", Q, N, D, 8, "cosine", rows=16)
    assert L.lib().bvc_op_topk_splits(Q, N, D, kk) == 32
    idx, val = _topk(c["q"], c["k"], kk, "cosine")
    _hold("larger", idx, val, c, kk)


# --------------------------------------------------------------------------- 9. refusals
def test_invalid_arguments_launch_nothing():
    q, k = R.gaussian(4, 16, 8, 1)
    A = AR.Arena(dev, q=((4, 8), F32), k=((16, 8), F32), idx=((4, 2), I32), val=((4, 2), F32), ws=((1 << 16,), U8))
    A["q"].copy_(torch.from_numpy(q)); A["k"].copy_(torch.from_numpy(k))
    A["idx"].fill_(POISON); A["val"].fill_(-7.0); A["ws"].fill_(0x5A)
    P = {n: G.ptr(A[n]) for n in ("q", "k", "idx", "val", "ws")}

    def call(q=P["q"], ldq=8, keys=P["k"], ldk=8, Q=4, N=16, D=8, k=2, metric=0, splits=0, base=0, acc=0, idx=P["idx"], val=P["val"], ws=P["ws"]):
        return L.lib().bvc_op_topk(q, ldq, keys, ldk, Q, N, D, k, metric, splits, base, acc, idx, val, ws, G.stream())

    for kw in (dict(k=65), dict(k=0), dict(Q=0), dict(N=0), dict(D=-3), dict(q=None), dict(keys=None), dict(idx=None), dict(val=None),
               dict(ws=None), dict(ldq=7), dict(ldk=7), dict(base=2 ** 31 - 8)):
        assert call(**kw) == -1 and L.lib().bvc_last_error(), kw      # BVC_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((A["idx"] == POISON).all()) and bool((A["val"] == -7.0).all()) and bool((A["ws"] == 0x5A).all()), "a refused call wrote"
    A.check()
    assert call() == 0
    torch.cuda.synchronize()
    R.check_topk(A["idx"].cpu().numpy(), A["val"].cpu().numpy(), q, k, 2, "cosine", ROW_BAR * R.model_error(q, k, "cosine"))
    A.check()
