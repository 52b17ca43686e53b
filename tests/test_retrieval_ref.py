"""CPU: tests/retrieval_ref.py held to the notebook's own ingredients (sklearn cosine_distances / euclidean_distances + argsort + the
label loop of notebooks/EvaluateEmbeddings.ipynb get_nn_score), the float32 model against the float64 scores (the figures the GPU
bars of tests/test_gpu_retrieval.py are multiples of), and the host side of bvc.retrieval / bvc_op_topk: imports, argument checks,
the split choice and the workspace size.  Nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from tests import retrieval_ref as R

CASES = [("gauss", 129, 1000, 100, 50, 2), ("gauss", 64, 4097, 768, 50, 1), ("clusters", 64, 4097, 768, 50, 3), ("clusters", 64, 2049, 384, 64, 4)]


def _inputs(kind, Q, N, D, seed):
    if kind == "gauss":
        q, k = R.gaussian(Q, N, D, seed)
        r = np.random.RandomState(seed + 1)
        return q, k, r.randint(0, 10, Q), r.randint(0, 10, N)
    return R.clustered(Q, N, D, seed)


def _notebook_hits(dist, y_train, y_test, ks):
    """get_nn_score's loop: argsort of the distance row, the first k labels, `in`."""
    out = {k: 0 for k in ks}
    for i in range(dist.shape[0]):
        order = np.argsort(dist[i])
        for k in ks:
            out[k] += int(y_test[i] in y_train[order[:k]])
    return out


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("kind,Q,N,D,kk,seed", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" for c in CASES])
def test_reference_is_sklearn(kind, Q, N, D, kk, seed, metric):
    pw = pytest.importorskip("sklearn.metrics.pairwise")
    q, k, yq, yk = _inputs(kind, Q, N, D, seed)
    fn = pw.cosine_distances if metric == "cosine" else pw.euclidean_distances
    dist = fn(q.astype(np.float64), k.astype(np.float64))
    s = R.scores64(q, k, metric)
    # sklearn's Euclidean form is the float64 expansion: its own cancellation error is ~1e-16 |x|^2 / d
    tol = 1e-12 if metric == "cosine" else 1e-12 * D
    err = float(np.abs(R.distance(s, metric) - dist).max())
    print(f"{kind} {Q}x{N}x{D} {metric}: |reference - sklearn| {err:.2e}")
    assert err <= tol
    amb = int(R.ambiguous(s, kk, 1e-11).sum())      # queries whose k-th place sklearn's last bits could decide
    got = R.hits(R.ranking64(s)[:, :max(R.KS)], yk, yq)
    want = _notebook_hits(dist, yk, yq, R.KS)
    if amb == 0:
        assert got == want
    else:
        assert all(abs(got[x] - want[x]) <= amb for x in R.KS)


def test_zero_rows_follow_sklearn_normalize():
    pw = pytest.importorskip("sklearn.metrics.pairwise")
    q, k = R.gaussian(4, 9, 16, 7)
    q[1] = 0
    k[3] = 0
    d = R.distance(R.scores64(q, k, "cosine"), "cosine")
    assert np.abs(d - pw.cosine_distances(q.astype(np.float64), k.astype(np.float64))).max() <= 1e-12
    assert (d[1] == 1).all() and (d[:, 3] == 1).all()
    m = R.distance(R.model32(q, k, "cosine"), "cosine")
    assert (m[1] == 1).all() and (m[:, 3] == 1).all()


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("kind,Q,N,D,kk,seed", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" for c in CASES])
def test_model_against_float64(kind, Q, N, D, kk, seed, metric):
    """The model's own error, its ambiguous queries at tau = 2.5 x that error, and the model's ranking through check_topk."""
    q, k, _, _ = _inputs(kind, Q, N, D, seed)
    s = R.scores64(q, k, metric)
    m = R.model32(q, k, metric)
    err = float(np.abs(m - s).max())
    tau = 2.5 * err
    order = np.argsort(-m, axis=1, kind="stable")[:, :kk]
    val = R.distance(np.take_along_axis(m, order, 1), metric).astype(np.float32)
    amb, worst = R.check_topk(order.astype(np.int32), val, q, k, kk, metric, tau, s)
    cap = float((np.abs(m - s) / R.value_cap(q, k, metric)).max())
    print(f"{kind} {Q}x{N}x{D} k{kk} {metric}: model error {err:.2e}, {amb} of {Q} ambiguous, error / cap {cap:.3f}")
    assert 0 < err < 1e-4 and amb <= 0.1 * Q and cap <= 1.0


def test_check_topk_rejects_wrong_results():
    q, k = R.gaussian(8, 200, 32, 11)
    s = R.scores64(q, k, "cosine")
    order = R.ranking64(s)[:, :10].astype(np.int32)
    val = R.distance(np.take_along_axis(s, order.astype(np.int64), 1), "cosine").astype(np.float32)
    assert R.check_topk(order, val, q, k, 10, "cosine", 1e-6, s)[0] == 0
    bad = order.copy()
    bad[3, 9] = R.ranking64(s)[3, 150]
    with pytest.raises(AssertionError, match="below the k-th best"):
        R.check_topk(bad, val, q, k, 10, "cosine", 1e-6, s)
    bad = order.copy()
    bad[2, 4] = bad[2, 5]
    with pytest.raises(AssertionError, match="twice"):
        R.check_topk(bad, val, q, k, 10, "cosine", 1e-6, s)
    with pytest.raises(AssertionError, match="from its float64 distance"):
        R.check_topk(order, val + np.float32(1e-3), q, k, 10, "cosine", 1e-6, s)
    with pytest.raises(AssertionError, match="decrease"):
        R.check_topk(order[:, ::-1].copy(), val[:, ::-1].copy(), q, k, 10, "cosine", 1e-6, s)
    q2, k2 = R.small_integers(4, 100, 8, 5)
    s2 = R.scores64(q2, k2, "euclidean")
    o2 = R.ranking64(s2)[:, :20].astype(np.int32)
    v2 = (-np.take_along_axis(s2, o2.astype(np.int64), 1)).astype(np.float32)
    R.check_topk(o2, v2, q2, k2, 20, "euclidean", 1e-6, s2)
    tied = np.nonzero(v2[0, 1:] == v2[0, :-1])[0]
    assert tied.size, "the integer case must contain ties"
    o3 = o2.copy()
    j = int(tied[0])
    o3[0, j], o3[0, j + 1] = o2[0, j + 1], o2[0, j]
    with pytest.raises(AssertionError, match="descending indices"):
        R.check_topk(o3, v2, q2, k2, 20, "euclidean", 1e-6, s2)
    assert R.hits(np.array([[0, 1], [2, -1]]), np.array([5, 6, 7]), np.array([6, 9]), ks=(1, 2)) == {1: 0, 2: 1}


# ------------------------------------------------------------------ the package and the C ABI, host side only
@pytest.fixture(scope="module")
def bvc():
    ge.build()
    return ge.load_package()


def test_retrieval_module_and_argument_checks(bvc):
    ret = bvc.retrieval
    assert callable(ret.topk) and callable(ret.nn_score) and callable(ret.knn_predict) and ret.MAX_K == 64
    x = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="GPU"):
        ret.topk(x, x, 2)
    with pytest.raises(ValueError, match="outside 1 .. 64"):
        ret.topk(x, x, 65)
    with pytest.raises(ValueError, match="outside 1 .. 64"):
        ret.topk(x, x, 0)
    with pytest.raises(ValueError, match="metric"):
        ret.topk(x, x, 2, metric="manhattan")
    with pytest.raises(ValueError, match="2-D"):
        ret.topk(torch.zeros(4), x, 2)
    with pytest.raises(ValueError, match="floating"):
        ret.topk(torch.zeros(4, 8, dtype=torch.int32), x, 2)
    with pytest.raises(ValueError, match="negative"):
        ret.topk(x, x, 2, key_base=-1)
    with pytest.raises(ValueError, match="ks"):
        ret.nn_score(x, torch.zeros(4, dtype=torch.long), x, torch.zeros(4, dtype=torch.long), ks=(1, 65))
    with pytest.raises(ValueError, match="integer labels"):
        ret.nn_score(x, torch.zeros(4), x, torch.zeros(4, dtype=torch.long))
    with pytest.raises(ValueError, match="temperature"):
        ret.knn_predict(x, torch.zeros(4, dtype=torch.long), x, temperature=0.1, metric="euclidean")
    with pytest.raises(ValueError, match="splits"):
        ret.splits(0, 1, 1, 1)


def test_split_choice_and_workspace(bvc):
    lib = bvc._lib.lib()
    # cost of s splits = ceil(query tiles x s / 256 CUs) x (key tiles per split + 8), each split at least 4 key tiles, at most 64
    # 300 queries are 3 tiles, 4097 keys 33 tiles: up to 8 splits, 7 and 8 both leave 5 tiles per split - the smaller wins
    assert lib.bvc_op_topk_splits(300, 4097, 768, 50) == 7 == bvc.retrieval.splits(300, 4097, 768, 50)
    assert lib.bvc_op_topk_splits(300, 20000, 768, 50) == 32      # 157 key tiles: 5 per split from 32 splits on
    assert lib.bvc_op_topk_splits(24777, 168913, 768, 50) == 9    # 194 query tiles x 9 = 6.8 rounds of 256: the last one nearly full
    assert lib.bvc_op_topk_splits(1, 1, 1, 1) == 1
    assert lib.bvc_op_topk_splits(2048, 16384, 768, 20) == 16     # 16 query tiles x 16 = one full round

    def ws(Q, N, D, k, s):
        return lib.bvc_op_topk_workspace(Q, N, D, k, s)

    def al(n):
        return (n + 255) // 256 * 256

    assert ws(300, 4097, 768, 50, 1) == al(1200) + al(4097 * 4) + 300 * 50 * 8
    assert ws(300, 4097, 768, 50, 0) == al(1200) + al(4097 * 4) + 7 * 300 * 50 * 8
    assert ws(300, 4097, 768, 50, 33) == ws(300, 4097, 768, 50, 1000)      # capped at the 33 key tiles
    assert ws(300, 4097, 768, 65, 1) == -1 and b"k 65" in lib.bvc_last_error()
    assert lib.bvc_op_topk_splits(300, 0, 768, 50) == -1 and b"non-positive" in lib.bvc_last_error()


def test_op_topk_refuses_invalid_arguments_before_any_launch(bvc):
    lib = bvc._lib.lib()
    INVALID = -1      # BVC_ERR_INVALID (include/bvc.h)
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(q=p, ldq=8, keys=p, ldk=8, Q=4, N=4, D=8, k=2, metric=0, splits=0, base=0, acc=0, idx=p, val=p, ws=p):
        return lib.bvc_op_topk(q, ldq, keys, ldk, Q, N, D, k, metric, splits, base, acc, idx, val, ws, None)

    for kw, text in ((dict(k=65), b"k 65"), (dict(k=0), b"k 0"), (dict(Q=0), b"non-positive"), (dict(N=-1), b"non-positive"),
                     (dict(D=0), b"non-positive"), (dict(q=None), b"null"), (dict(keys=None), b"null"), (dict(idx=None), b"null"),
                     (dict(val=None), b"null"), (dict(ws=None), b"null"), (dict(ldq=7), b"stride"), (dict(ldk=7), b"stride"),
                     (dict(base=2 ** 31 - 4), b"overflows"), (dict(metric=2), b"metric"), (dict(splits=-1), b"key_splits")):
        rc = call(**kw)
        assert rc == INVALID and text in lib.bvc_last_error(), (kw, rc, lib.bvc_last_error())
