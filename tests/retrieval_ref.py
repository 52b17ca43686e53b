"""Reference, float32 model, inputs and the tie-aware comparison for the retrieval tests  --  TEST INFRASTRUCTURE ONLY (numpy).

Imported by tests/test_retrieval_ref.py (CPU: pins what is defined here against sklearn, the notebook's own ingredients) and
tests/test_gpu_retrieval.py (bvc_op_topk / bvc.retrieval).  Nothing here touches the library.

A "score" is what the ranking maximises: the cosine similarity, or minus the Euclidean distance.  `distance(score, metric)` is what
the op returns: 1 - score, or -score.  Scores and distances of one metric have the same unit, so one `tau` serves both.
"""
import numpy as np

KS = (1, 5, 10, 20, 50)


def distance(score, metric):
    return 1.0 - score if metric == "cosine" else -score


def scores64(q, k, metric):
    """float64 [Q][N] scores of float32 operands; norms and normalisation in float64."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    if metric == "cosine":
        qn, kn = np.sqrt((q * q).sum(1)), np.sqrt((k * k).sum(1))
        qi = np.divide(1.0, qn, out=np.zeros_like(qn), where=qn > 0)      # a zero row: inverse norm 0, score 0, distance 1
        ki = np.divide(1.0, kn, out=np.zeros_like(kn), where=kn > 0)
        return (q * qi[:, None]) @ (k * ki[:, None]).T
    assert metric == "euclidean", metric
    d2 = ((q[:, None, :] - k[None, :, :]) ** 2).sum(-1) if q.shape[0] * k.shape[0] * q.shape[1] <= 1 << 24 else None
    if d2 is None:      # too large for the direct form: float64 expansion, clamped (its error ~1e-16 |x|^2 is far below any tau)
        d2 = np.maximum((q * q).sum(1)[:, None] + (k * k).sum(1)[None, :] - 2.0 * (q @ k.T), 0.0)
    return -np.sqrt(d2)


def _fma32(acc, a, b):
    """float32(acc + a * b) with one rounding to float64 in between: the product of two float32 is exact in float64."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def _sumsq32(x):
    s = np.zeros(x.shape[0], np.float32)
    for d in range(x.shape[1]):
        s = _fma32(s, x[:, d], x[:, d])
    return s


def model32(q, k, metric):
    """[Q][N] scores (float64 images of float32 results): the computation of the op in float32 with a d-ordered accumulation - acc = f32(acc + q[:, d] k[:, d])
    for d = 0 .. D-1 - and float32 norms; cosine (dot * 1/|k|) * 1/|q| and 1 - score, Euclidean sqrt(max(|q|^2 + |k|^2 - 2 dot, 0)),
    every operation rounded to float32.  This is the float32 evaluation the kernel is allowed to be; its distance from scores64 is
    what the GPU bars are multiples of."""
    q, k = np.asarray(q, np.float32), np.asarray(k, np.float32)
    dot = np.zeros((q.shape[0], k.shape[0]), np.float32)
    for d in range(q.shape[1]):
        dot = _fma32(dot, q[:, d][:, None], k[:, d][None, :])
    qq, kk = _sumsq32(q), _sumsq32(k)
    one = np.float32(1.0)
    if metric == "cosine":
        with np.errstate(divide="ignore"):
            qi = np.where(qq > 0, one / np.sqrt(qq), np.float32(0)).astype(np.float32)
            ki = np.where(kk > 0, one / np.sqrt(kk), np.float32(0)).astype(np.float32)
        s = (dot * ki[None, :]) * qi[:, None]
        return 1.0 - (one - s).astype(np.float64)      # the score as the returned float32 distance 1 - s carries it
    assert metric == "euclidean", metric
    d2 = np.maximum(_fma32(qq[:, None] + kk[None, :], np.float32(-2.0) * np.ones_like(dot), dot), np.float32(0))
    return -np.sqrt(d2).astype(np.float64)


def model_error(q, k, metric, rows=64):
    """Worst |model32 - scores64| over the first `rows` queries: the unit of a case's tau."""
    return float(np.abs(model32(q[:rows], k, metric) - scores64(q[:rows], k, metric)).max())


def ranking64(s):
    """Indices [Q][N] by score descending, ties to the smaller index (stable sort)."""
    return np.argsort(-s, axis=1, kind="stable")


def hits(indices, y_train, y_test, ks=KS):
    """{k: number of queries whose label is among the labels of their first k neighbours} (indices < 0 = no neighbour)."""
    indices, y_train, y_test = np.asarray(indices), np.asarray(y_train), np.asarray(y_test)
    lab = np.where(indices >= 0, y_train[np.maximum(indices, 0)], -1 - np.abs(y_test).max())
    same = lab == y_test[:, None]
    return {k: int(same[:, :k].any(1).sum()) for k in ks}


def vote64(s, y_train, kk, num_classes, temperature=None):
    """The float64 kNN vote [Q]: majority label of the kk best (ties in score to the smaller index), optionally weighted by
    exp(score / T); ties between classes to the smaller class id."""
    order = ranking64(s)[:, :kk]
    votes = np.zeros((s.shape[0], num_classes))
    for i in range(s.shape[0]):
        w = np.ones(order.shape[1]) if temperature is None else np.exp(s[i, order[i]] / temperature)
        np.add.at(votes[i], np.asarray(y_train)[order[i]], w)
    return votes.argmax(1)


def ambiguous(s, kk, tau):
    """bool [Q]: the query has a key other than the kk-th best itself within tau of the kk-th best score."""
    n = s.shape[1]
    if n <= kk:
        return np.zeros(s.shape[0], bool)
    top = -np.sort(-s, axis=1)
    sk = top[:, kk - 1]
    return (np.abs(s - sk[:, None]) <= tau).sum(1) > 1


def check_topk(idx, val, q, k, kk, metric, tau, s=None):
    """The tie-aware comparison of a result (idx int [Q][kk], val f32 [Q][kk]) with the float64 scores `s` of (q, k):
      every returned index has s >= s_k - tau (s_k: the kk-th best score of the query); every key with s > s_k + tau is returned;
      no index twice; val[j] within tau of the float64 distance of idx[j]; val non-decreasing along the row and idx ascending where
      two neighbouring val are bit-equal; with N < kk the slots from N on hold -1 / +inf.
    Returns (number of ambiguous queries, worst |val - float64 distance|)."""
    idx, val = np.asarray(idx), np.asarray(val)
    s = scores64(q, k, metric) if s is None else s
    Q, N = s.shape
    assert idx.shape == (Q, kk) and val.shape == (Q, kk), (idx.shape, val.shape, Q, kk)
    assert val.dtype == np.float32 and idx.dtype == np.int32
    m = min(kk, N)
    assert (idx[:, m:] == -1).all() and np.isposinf(val[:, m:]).all(), "slots past the number of keys must hold -1 / +inf"
    got, gv = idx[:, :m].astype(np.int64), val[:, :m]
    assert (got >= 0).all() and (got < N).all(), f"index outside 0 .. {N - 1}"
    assert not np.isnan(gv).any(), "NaN among the values"
    srt = np.sort(got, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "an index was returned twice"
    top = -np.sort(-s, axis=1)
    sk = top[:, m - 1]
    sg = np.take_along_axis(s, got, axis=1)
    low = (sg < sk[:, None] - tau)
    assert not low.any(), f"{int(low.sum())} returned keys score more than tau = {tau:.2e} below the k-th best (worst by {float((sk[:, None] - sg).max()):.2e})"
    must = s > sk[:, None] + tau
    have = np.zeros_like(must)
    np.put_along_axis(have, got, True, axis=1)
    missed = must & ~have
    assert not missed.any(), f"{int(missed.sum())} keys more than tau above the k-th best score were not returned"
    err = np.abs(gv.astype(np.float64) - distance(sg, metric))
    worst = float(err.max())
    assert worst <= tau, f"a value is {worst:.3e} from its float64 distance, tau = {tau:.2e}"
    bits = gv.view(np.int32)
    assert (gv[:, 1:] >= gv[:, :-1]).all(), "values decrease along a row"
    tie = bits[:, 1:] == bits[:, :-1]
    assert (got[:, 1:][tie] > got[:, :-1][tie]).all(), "bit-equal neighbouring values with descending indices"
    return int(ambiguous(s, kk, tau).sum()), worst


def value_cap(q, k, metric):
    """The derivable worst case of a value's error, [Q][N] float64, u = 2^-24 (every float32 operation: relative error <= u).
    Cosine: D 2^-23 = 2 D u, the issue's bound of a length-D float32 dot product of unit vectors, normalisation included, from
    D = 5 on.  Below that the operations outside the chains outweigh it (at D = 1 it would be one ulp of 1.0 for nine rounded
    operations): the dot chain D u, each inverse norm D u / 2 (its chain, halved by the root) + 2 u (root, reciprocal), two
    multiplications 2 u, the subtraction u - (2 D + 7) u in all, which is the cap for D < 5.
    Euclidean operands are not unit vectors, so the bound is taken in the units of the expanded d2 = |q|^2 + |k|^2 - 2 q.k: the two
    squared-norm chains D u |q|^2 and D u |k|^2, their sum u (|q|^2 + |k|^2), the dot chain 2 D u |q| |k| <= D u (|q|^2 + |k|^2):
    |d2 error| <= E = (D + 1) 2^-23 (|q|^2 + |k|^2).  Carried through the clamp and the square root it is the larger of
    sqrt(d^2 + E) - d and d - sqrt(max(d^2 - E, 0)) (the first where d^2 < E, the second elsewhere), plus the root's own rounding."""
    D = q.shape[1]
    if metric == "cosine":
        return np.full((q.shape[0], k.shape[0]), (2 * D if D >= 5 else 2 * D + 7) * 2.0 ** -24)
    q64, k64 = np.asarray(q, np.float64), np.asarray(k, np.float64)
    E = (D + 1) * 2.0 ** -23 * ((q64 * q64).sum(1)[:, None] + (k64 * k64).sum(1)[None, :])
    d = -scores64(q, k, metric)
    up = np.sqrt(d * d + E)
    return np.maximum(up - d, d - np.sqrt(np.maximum(d * d - E, 0.0))) + 2.0 ** -23 * up


# ------------------------------------------------------------------ inputs
def gaussian(Q, N, D, seed):
    r = np.random.RandomState(seed)
    return r.randn(Q, D).astype(np.float32), r.randn(N, D).astype(np.float32)


def clustered(Q, N, D, seed, classes=10):
    """Ten Gaussian cluster centres with unit noise: (q, k, y_test, y_train)."""
    r = np.random.RandomState(seed)
    c = r.randn(classes, D)
    yk, yq = r.randint(0, classes, N), r.randint(0, classes, Q)
    return ((c[yq] + r.randn(Q, D)).astype(np.float32), (c[yk] + r.randn(N, D)).astype(np.float32), yq.astype(np.int64), yk.astype(np.int64))


def small_integers(Q, N, D, seed):
    """Integers in [-3, 3], the keys drawn from 40 distinct rows so that many collide: every product, sum and d2 is exact in f32."""
    r = np.random.RandomState(seed)
    pool = r.randint(-3, 4, (40, D))
    k = pool[r.randint(0, 40, N)]
    return r.randint(-3, 4, (Q, D)).astype(np.float32), k.astype(np.float32)
