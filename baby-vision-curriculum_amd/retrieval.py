"""Embedding retrieval on the GPU: fused f32 top-k (bvc_op_topk, csrc/retrieval.hip), the reference's kNN score and a kNN classifier.

``nn_score`` is ``get_nn_score`` / ``topk_retrieval`` of the reference's notebooks/EvaluateEmbeddings.ipynb (sklearn
``cosine_distances`` + ``argsort`` + a label loop on the host) on embeddings that are already on the device: no [Q][N] matrix
is stored, and the label arithmetic runs on the [Q][max k] result with plain torch ops.
"""
import torch

from . import _lib

METRICS = {"cosine": 0, "euclidean": 1}
MAX_K = 64


def _metric(metric):
    if metric not in METRICS:
        raise ValueError(f"metric {metric!r}: 'cosine' or 'euclidean'")
    return METRICS[metric]


def _rows(t, name):
    """f32, last dimension dense; returns (tensor, row stride in elements)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"{name} must be a 2-D tensor [rows][D]")
    if not t.is_floating_point():
        raise ValueError(f"{name} must be a floating-point tensor, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be on the GPU (there is no CPU path)")
    if t.dtype != torch.float32:
        t = t.float()
    if t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < t.shape[1]) or t.shape[0] <= 1 and not t.is_contiguous():
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def splits(Q, N, D, k):
    """What ``key_splits=0`` resolves to for this shape (bvc_op_topk_splits)."""
    s = _lib.lib().bvc_op_topk_splits(int(Q), int(N), int(D), int(k))
    if s < 0:
        raise ValueError(f"splits: {_lib.lib().bvc_last_error().decode()}")
    return s


def topk(queries, keys, k, metric="cosine", *, key_splits=0, out=None, key_base=0):
    """(distances f32 [Q][k], indices int32 [Q][k]): for every row of ``queries`` [Q][D] the ``k`` (<= 64) nearest rows of
    ``keys`` [N][D], best first; cosine distance ``1 - q.k / (|q| |k|)`` or Euclidean distance.  Among bit-equal distances the
    smaller index comes first; with fewer than ``k`` keys the remaining slots hold index -1 and distance inf.

    ``out=(distances, indices)`` of an earlier call (same queries, metric and ``k``, other keys) merges this call's keys into it in
    place and returns it; the indices reported are ``key_base`` + row.  A gallery in chunks is then a loop of calls, with the bits
    of one call over the whole gallery.  Runs on the current stream; ``key_splits=0`` lets the library choose."""
    m = _metric(metric)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k = {k} outside 1 .. {MAX_K}")
    if int(key_splits) < 0 or int(key_base) < 0:
        raise ValueError("key_splits and key_base must not be negative")
    queries, ldq = _rows(queries, "queries")
    keys, ldk = _rows(keys, "keys")
    if keys.device != queries.device:
        raise ValueError("queries and keys must be on the same device")
    Q, D = queries.shape
    N = keys.shape[0]
    if keys.shape[1] != D:
        raise ValueError(f"queries have {D} columns, keys {keys.shape[1]}")
    if Q < 1 or N < 1 or D < 1:
        raise ValueError(f"empty operand: queries {tuple(queries.shape)}, keys {tuple(keys.shape)}")
    if int(key_base) + N > 2 ** 31 - 1:
        raise ValueError("key_base + N exceeds int32")
    if out is None:
        dist = torch.empty(Q, k, dtype=torch.float32, device=queries.device)
        idx = torch.empty(Q, k, dtype=torch.int32, device=queries.device)
    else:
        dist, idx = out
        for t, dt, what in ((dist, torch.float32, "distances"), (idx, torch.int32, "indices")):
            if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.shape == (Q, k) and t.is_contiguous() and t.device == queries.device):
                raise ValueError(f"out: {what} must be a contiguous {dt} tensor [{Q}][{k}] on the queries' device")
    L = _lib.lib()
    nbytes = L.bvc_op_topk_workspace(Q, N, D, k, int(key_splits))
    if nbytes < 0:
        raise _lib.BvcError(f"bvc_op_topk_workspace: {L.bvc_last_error().decode()}")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=queries.device)
    with torch.cuda.device(queries.device):
        _lib.check(L.bvc_op_topk(queries.data_ptr(), ldq, keys.data_ptr(), ldk, Q, N, D, k, m, int(key_splits), int(key_base),
                                 0 if out is None else 1, idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), _lib.current_stream_ptr()),
                   "bvc_op_topk")
    return dist, idx


def _labels(y, device, name):
    y = torch.as_tensor(y)
    if y.dim() != 1 or y.is_floating_point() or y.dtype == torch.bool:
        raise ValueError(f"{name} must be a 1-D tensor of integer labels (encode other labels first)")
    return y.to(device=device, dtype=torch.int64)


def _neighbour_labels(x_train, y_train, x_test, k, metric):
    if x_train.shape[0] != y_train.shape[0]:
        raise ValueError(f"{x_train.shape[0]} train embeddings, {y_train.shape[0]} train labels")
    dist, idx = topk(x_test, x_train, k, metric)
    found = idx >= 0
    return dist, y_train[idx.clamp(min=0).long()], found


def nn_score(x_train, y_train, x_test, y_test, ks=(1, 5, 10, 20, 50), metric="cosine"):
    """{k: accuracy}: a test row is a hit at ``k`` when its label is among the labels of its ``k`` nearest train rows (the
    reference's get_nn_score).  One top-k at max(ks); the label gather and the running "any" are torch ops on [Q][max k]."""
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1 or max(ks) > MAX_K:
        raise ValueError(f"ks {ks}: every k in 1 .. {MAX_K}")
    _metric(metric)
    if not (isinstance(x_test, torch.Tensor) and isinstance(x_train, torch.Tensor)):
        raise ValueError("x_train and x_test must be tensors on the GPU")
    y_train = _labels(y_train, x_train.device, "y_train")
    y_test = _labels(y_test, x_test.device, "y_test")
    if x_test.shape[0] != y_test.shape[0]:
        raise ValueError(f"{x_test.shape[0]} test embeddings, {y_test.shape[0]} test labels")
    _, lab, found = _neighbour_labels(x_train, y_train, x_test, max(ks), metric)
    hit = ((lab == y_test[:, None]) & found).cummax(dim=1).values            # [Q][max k]: hit within the first j + 1
    acc = hit[:, [k - 1 for k in ks]].float().mean(dim=0).tolist()         # the one synchronisation
    return {k: a for k, a in zip(ks, acc)}


def knn_predict(x_train, y_train, x_test, k=20, num_classes=None, temperature=None, metric="cosine"):
    """int64 [Q]: the majority label of the ``k`` nearest train rows; with ``temperature`` the votes weigh exp(score / T) on cosine
    scores (the usual kNN monitor).  Ties between classes go to the smaller class id."""
    m = _metric(metric)
    if temperature is not None and (m != 0 or not float(temperature) > 0):
        raise ValueError("temperature needs the cosine metric and a positive value")
    if not (isinstance(x_test, torch.Tensor) and isinstance(x_train, torch.Tensor)):
        raise ValueError("x_train and x_test must be tensors on the GPU")
    y_train = _labels(y_train, x_train.device, "y_train")
    if num_classes is None:
        num_classes = int(y_train.max()) + 1
    dist, lab, found = _neighbour_labels(x_train, y_train, x_test, int(k), metric)
    if temperature is None:
        w = found.to(torch.float64)
    else:
        w = torch.where(found, torch.exp((1.0 - dist.double()) / float(temperature)), torch.zeros((), dtype=torch.float64, device=dist.device))
    votes = torch.zeros(x_test.shape[0], int(num_classes), dtype=torch.float64, device=dist.device)
    votes.scatter_add_(1, lab, w)
    best = votes.max(dim=1, keepdim=True).values
    return (votes == best).int().argmax(dim=1)      # the first (smallest) class among the best
