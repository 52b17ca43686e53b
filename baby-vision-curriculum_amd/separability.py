"""Linear separability score on the GPU: StandardScaler + one-vs-rest squared-hinge linear SVM on device embeddings.

``separability_score`` is ``get_separability_score(..., method='svm')`` of the reference's notebooks/EvaluateEmbeddings.ipynb
(sklearn ``make_pipeline(StandardScaler(), LinearSVC(random_state=0, tol=1e-4))``, fit and scored on the host) on embeddings that
are already on the device.  Per class c, with y = +1 on its rows and -1 elsewhere, xs the standardised row and C = 1, LinearSVC
minimises

    f_c(w, b) = 1/2 (|w|^2 + b^2) + C sum_i max(0, 1 - y_i (w . xs_i + b))^2

- liblinear appends a constant feature 1, so the intercept IS regularised.  f_c is strongly convex: the optimum is a property of the
data, and ``fit`` finds it with a truncated Newton method (conjugate-gradient inner iterations, as liblinear's primal solver),
batched over all classes: every function / gradient evaluation is one GRAD pass and every CG step of every class one HESSVEC pass
of bvc_op_linear_pass (csrc/separability.hip), which reads each row of ``x`` once and never stores the standardised matrix.
Two classes train ONE column (positive class = the larger label), as sklearn does.

``method='sgd'`` (sklearn's SGDClassifier with an unseeded shuffle) is a stochastic approximate minimiser whose result changes
from run to run: there is nothing to be equal to, and it is not provided.
"""
import math
import warnings

import numpy as np
import torch

from . import _lib

GRAD, HESSVEC, DECISION = 0, 1, 2
MAX_COLUMNS = 1024      # columns per bvc_op_linear_pass call; more classes are a loop over class chunks
MAX_D = 1343


def _rows(t, name):
    """f32, last dimension dense; returns (tensor, row stride in elements)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"{name} must be a 2-D tensor [rows][D]")
    if not t.is_floating_point():
        raise ValueError(f"{name} must be a floating-point tensor, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be on the GPU (there is no CPU path)")
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name} is empty: {tuple(t.shape)}")
    if t.shape[1] > MAX_D:
        raise ValueError(f"{name} has {t.shape[1]} columns; at most {MAX_D}")
    if t.dtype != torch.float32:
        t = t.float()
    if t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < t.shape[1]) or t.shape[0] <= 1 and not t.is_contiguous():
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def _labels(y, name):
    """A 1-D int64 tensor (on whatever device ``y`` lives) of integer labels; anything else is refused."""
    if not isinstance(y, torch.Tensor):
        arr = np.asarray(y)
        if arr.dtype.kind not in "iu":
            raise ValueError(f"{name} must hold integer labels, got {arr.dtype} (encode other labels first)")
        y = torch.from_numpy(arr.astype(np.int64))
    if y.dim() != 1 or y.is_floating_point() or y.is_complex() or y.dtype == torch.bool:
        raise ValueError(f"{name} must be a 1-D tensor of integer labels (encode other labels first)")
    return y.to(torch.int64)


def _encode(y, classes, name):
    """int32 positions of the labels in the sorted ``classes``; a label that is not among them is refused."""
    classes = classes.to(y.device)
    pos = torch.searchsorted(classes, y).clamp(max=classes.numel() - 1)
    if not bool((classes[pos] == y).all()):
        raise ValueError(f"{name} holds a label that the training labels do not have")
    return pos.to(torch.int32)


class LinearSVMFit:
    """What ``fit`` returns.  ``coef`` f32 [K or 1][D] and ``intercept`` f32 [K or 1] in standardised coordinates (sklearn's
    ``clf[-1].coef_`` / ``intercept_``); ``mean``, ``scale`` f32 [D] (StandardScaler's; ``inv_scale`` is what the kernel multiplies by);
    ``classes`` the sorted unique labels; ``n_iter`` outer iterations per column, ``grad_norm`` the final |grad f_c| and
    ``threshold`` the stopping threshold per column, ``converged`` bool per column; ``history`` f64 [iterations + 1][columns], the
    evaluated f_c - 1/2 |w|^2 in float64 plus C times the pass's float32 loss - of the weights after every outer iteration, as
    evaluated (non-increasing up to the rounding of that loss: see _solve); ``iterates`` (with ``keep_iterates=True``) f32
    [iterations + 1][columns][D + 1], those weights; ``passes`` = (GRAD passes, HESSVEC passes)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Passes:
    """The three modes of bvc_op_linear_pass on one (x, labels, mean, inv_std), looping over chunks of MAX_COLUMNS columns."""

    def __init__(self, x, ldx, labels, mean, inv_std, columns, class0, C):
        self.x, self.ldx, self.labels, self.mean, self.inv_std = x, int(ldx), labels, mean, inv_std
        self.n, self.D = x.shape
        self.K, self.class0, self.C = int(columns), int(class0), float(C)
        self._ws = {}

    def _workspace(self, L, K, mode):
        nbytes = L.bvc_op_linear_pass_workspace(self.n, self.D, K, mode)
        if nbytes < 0:
            raise _lib.BvcError(f"bvc_op_linear_pass_workspace: {L.bvc_last_error().decode()}")
        key = max(nbytes, 8)
        if self._ws.get("n", 0) < key:
            self._ws = {"n": key, "t": torch.empty((key + 7) // 8, dtype=torch.int64, device=self.x.device)}
        return self._ws["t"]

    def _call(self, mode, W, V=None, out_G=None, out_loss=None, out_pred=None, out_dec=None):
        L = _lib.lib()
        p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        with torch.cuda.device(self.x.device):
            for k0 in range(0, self.K, MAX_COLUMNS):
                k1 = min(k0 + MAX_COLUMNS, self.K)
                ws = self._workspace(L, k1 - k0, mode)
                sl = lambda t: None if t is None else t[k0:k1]      # noqa: E731
                _lib.check(L.bvc_op_linear_pass(self.x.data_ptr(), self.ldx, p(self.labels), self.mean.data_ptr(), self.inv_std.data_ptr(),
                                                p(sl(W)), p(sl(V)), self.n, self.D, k1 - k0, self.class0 + k0, mode, self.C,
                                                p(sl(out_G)), p(sl(out_loss)), p(out_pred), p(out_dec), ws.data_ptr(),
                                                _lib.current_stream_ptr()), "bvc_op_linear_pass")

    def grad(self, W):
        G = torch.empty_like(W)
        loss = torch.empty(self.K, dtype=torch.float32, device=W.device)
        self._call(GRAD, W, out_G=G, out_loss=loss)
        return loss, G

    def hessvec(self, W, V):
        G = torch.empty_like(W)
        self._call(HESSVEC, W, V, out_G=G)
        return G

    def decision(self, W, want_values=False):
        """(column of the largest decision value int32 [n] - for one column z > 0 -, decision values f32 [n][K] or None)"""
        dev = self.x.device
        if self.K <= MAX_COLUMNS:
            pred = torch.empty(self.n, dtype=torch.int32, device=dev)
            dec = torch.empty(self.n, self.K, dtype=torch.float32, device=dev) if want_values else None
            self._call(DECISION, W, out_pred=pred, out_dec=dec)
            return pred, dec
        parts, scratch = [], torch.empty(self.n, dtype=torch.int32, device=dev)      # class chunks: the values, then the first maximum
        for k0 in range(0, self.K, MAX_COLUMNS):
            sub = _Passes(self.x, self.ldx, None, self.mean, self.inv_std, min(MAX_COLUMNS, self.K - k0), 0, self.C)
            d = torch.empty(self.n, sub.K, dtype=torch.float32, device=dev)
            sub._call(DECISION, W[k0:k0 + sub.K], out_pred=scratch, out_dec=d)
            parts.append(d)
        dec = torch.cat(parts, dim=1)
        return (dec == dec.max(dim=1, keepdim=True).values).int().argmax(dim=1).to(torch.int32), (dec if want_values else None)


def colstats(x):
    """(mean f32 [D], inv_std f32 [D]) of the rows of ``x``: StandardScaler's statistics (population variance; a column whose
    variance is exactly 0 gets scale 1), float64 sums in a fixed order (bvc_op_colstats)."""
    x, ldx = _rows(x, "x")
    n, D = x.shape
    mean = torch.empty(D, dtype=torch.float32, device=x.device)
    inv_std = torch.empty(D, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().bvc_op_colstats(x.data_ptr(), ldx, n, D, mean.data_ptr(), inv_std.data_ptr(), _lib.current_stream_ptr()),
                   "bvc_op_colstats")
    return mean, inv_std


def _solve(ev, columns, width, pos, n, C, tol, max_iter, cg_max, keep_iterates=False):
    """Truncated Newton on ``columns`` independent problems at once.  ``ev.grad(W)`` -> (loss [K], G [K][width]) and
    ``ev.hessvec(W, V)`` -> G are the data terms; vectors are [K][width] device tensors (f32 where the kernel reads them, f64 for
    the solver's own sums), per-class scalars [K] device tensors.  One read-back per outer iteration: whether any class is still
    active, and how many CG steps the last direction needed (the next CG budget).

    Line search by re-evaluation: three trial points w + t d per class (t = step, 0.9 step, step / 4), one GRAD pass each.  A class
    moves to the first trial at which the slope grad f_c(w + t d) . d is still <= 0 - f_c is convex, so f_c is lower there - and
    otherwise to the trial with the lowest evaluated f below its current one; else it stays.  Both tests read float32 results of
    the pass, so "non-increasing" holds up to their rounding: with a slope error of at most e (|G error| . |d|) convexity gives
    f_c(w + t d) <= f_c(w) + t e, and the f test can be wrong by the error of two evaluated losses.  ``history`` is the EVALUATED f
    (1/2 |w|^2 in float64 + C x the pass's float32 loss) of every iterate, unclamped: where the slope decided it may tick up by a
    rounding of the loss.  ``keep_iterates`` also returns the weights after every outer iteration ([iterations + 1][K][width] f32), so
    that f_c can be evaluated independently.  The first trial of the next iteration is four times the accepted t (at most 1), a
    16th after a failure."""
    dev = pos.device
    f64 = torch.float64
    W = torch.zeros(columns, width, dtype=torch.float32, device=dev)
    passes = [0, 0]

    def value_grad(W):
        loss, G = ev.grad(W)
        passes[0] += 1
        Wd = W.double()
        return 0.5 * (Wd * Wd).sum(1) + C * loss.double(), Wd + G.double()

    f, g = value_grad(W)
    gnorm = g.norm(dim=1)
    small = torch.clamp(torch.minimum(pos, n - pos), min=1).to(f64)
    thr = tol * small / n * gnorm                  # liblinear: eps * max(min(pos, neg), 1) / n * |grad f(0)|
    step = torch.ones(columns, dtype=f64, device=dev)
    stalled = torch.zeros(columns, dtype=torch.bool, device=dev)
    active = gnorm > thr
    n_iter = torch.zeros(columns, dtype=torch.int64, device=dev)
    history = [f]
    iterates = [W] if keep_iterates else None
    zero = torch.zeros((), dtype=f64, device=dev)
    budget = min(8, cg_max)
    used = torch.zeros((), dtype=torch.int64, device=dev)
    for _ in range(int(max_iter)):
        any_active, last = torch.stack([active.any().to(torch.int64), used]).tolist()      # the one read-back
        if not any_active:
            break
        if last >= budget:
            budget = min(2 * budget, cg_max)
        # conjugate gradients on (I + data term) d = -g, every class with its own step lengths; a class is frozen once
        # |r| <= 0.1 |g| (liblinear's inner rule)
        d = torch.zeros(columns, width, dtype=f64, device=dev)
        r = torch.where(active[:, None], -g, zero)
        p = r.clone()
        rs = (r * r).sum(1)
        stop = (0.1 * gnorm) ** 2
        steps = torch.zeros(columns, dtype=torch.int64, device=dev)
        for _j in range(budget):
            live = active & (rs > stop)
            Hp = p + ev.hessvec(W, p.float()).double()
            passes[1] += 1
            pHp = (p * Hp).sum(1)
            live = live & (pHp > 0)
            alpha = torch.where(live, rs / torch.where(live, pHp, torch.ones_like(pHp)), zero)
            d = d + alpha[:, None] * p
            r = r - alpha[:, None] * Hp
            rs_new = (r * r).sum(1)
            beta = torch.where(live, rs_new / torch.where(live, rs, torch.ones_like(rs)), zero)
            p = torch.where(live[:, None], r + beta[:, None] * p, p)
            rs = torch.where(live, rs_new, rs)
            steps = steps + live
        used = steps.max()
        # line search: three trial points per class along d, one GRAD pass each.  f_c is convex, so along d the slope
        # phi'(t) = grad f_c(w + t d) . d only grows: a trial whose slope is still <= 0 lies below f_c(w) - a test that float32
        # resolves where the difference of two f no longer does (near the optimum a Newton step lowers f by less than one
        # rounding of the loss).  The first such trial wins (0.9 of the step: the CG direction ends where the model's slope is 0, and
        # 0.9 of it keeps a tenth of the initial slope, clear of the rounding); failing that the lowest f below the current one.
        base = W.double()
        t0 = torch.where(active, step, zero)
        done = torch.zeros_like(active)
        best_f, best_W, best_g, best_t = f, W, g, torch.zeros_like(step)
        for mult in (1.0, 0.9, 0.25):
            trial = (base + (t0 * mult)[:, None] * d).float()
            f_t, g_t = value_grad(trial)
            by_slope = active & ~done & ((g_t * d).sum(1) <= 0)
            better = by_slope | (active & ~done & (f_t < best_f))
            best_W = torch.where(better[:, None], trial, best_W)
            best_g = torch.where(better[:, None], g_t, best_g)
            best_f = torch.where(better, f_t, best_f)      # the evaluated value, also where the slope decided
            best_t = torch.where(better, t0 * mult, best_t)
            done = done | by_slope
        take = best_t > 0
        W, f, g = best_W, best_f, best_g
        # the next first trial: four times the accepted step (at most 1), or a 16th of this one's after a failure
        step = torch.where(take, torch.clamp(4.0 * best_t, max=1.0), step / 16.0)
        stalled = stalled | (active & ~take & (step < 2.0 ** -20))
        gnorm = g.norm(dim=1)
        n_iter = n_iter + active
        active = (gnorm > thr) & ~stalled
        history.append(f)
        if keep_iterates:
            iterates.append(W)
    extra = dict(iterates=torch.stack(iterates)) if keep_iterates else {}
    return W, dict(n_iter=n_iter, grad_norm=gnorm, threshold=thr, converged=gnorm <= thr, history=torch.stack(history), passes=tuple(passes), **extra)


def _check_fit_inputs(x, y, C, tol):
    if not (float(C) > 0 and float(tol) > 0):
        raise ValueError("C and tol must be positive")
    y = _labels(y, "y_train")
    classes = torch.unique(y)      # sorted, as LabelEncoder
    if classes.numel() < 2:
        raise ValueError(f"the training labels hold {classes.numel()} class; at least two are needed")
    x, ldx = _rows(x, "x_train")
    if x.shape[0] != y.shape[0]:
        raise ValueError(f"{x.shape[0]} train embeddings, {y.shape[0]} train labels")
    return x, ldx, y, classes


def fit(x_train, y_train, C=1.0, tol=1e-4, max_iter=100, cg_max=16, keep_iterates=False):
    """Fit StandardScaler + LinearSVC(C, tol) on device embeddings ``x_train`` [n][D] (any float dtype, cast to f32; strided rows
    are taken as they are) and integer labels ``y_train`` [n]; returns a LinearSVMFit.  ``cg_max`` caps the CG steps (HESSVEC passes)
    of one outer iteration.  Class c stops when
    |grad f_c| <= tol * max(min(pos_c, neg_c), 1) / n * |grad f_c(0)| (liblinear's rule).  A class that has not met it after
    ``max_iter`` outer iterations, or whose line search can no longer lower f_c in float32, has ``converged`` False and a warning.
    ``keep_iterates=True`` keeps the weights of every outer iteration in the result (``iterates``)."""
    x, ldx, y, classes = _check_fit_inputs(x_train, y_train, C, tol)
    dev = x.device
    n, D = x.shape
    code = _encode(y, classes, "y_train").to(dev)
    K = classes.numel()
    columns, class0 = (1, 1) if K == 2 else (K, 0)
    mean, inv_std = colstats(x)
    counts = torch.bincount(code.long(), minlength=K)[class0:class0 + columns]
    ev = _Passes(x, ldx, code, mean, inv_std, columns, class0, C)
    W, info = _solve(ev, columns, D + 1, counts, n, float(C), float(tol), max_iter, int(cg_max), bool(keep_iterates))
    converged = info["converged"]
    if not bool(converged.all()):
        bad = [int(classes[class0 + i]) for i in torch.nonzero(~converged).flatten().tolist()]
        warnings.warn(f"separability.fit: class(es) {bad} did not reach the stopping threshold (max_iter = {max_iter}); "
                      "the weights are the best found", RuntimeWarning, stacklevel=2)
    return LinearSVMFit(coef=W[:, :D].contiguous(), intercept=W[:, D].contiguous(), weights=W, mean=mean, inv_scale=inv_std,
                        scale=1.0 / inv_std, classes=classes.to(dev), C=float(C), tol=float(tol), **info)


def decision_function(model, x):
    """f32 [n][K or 1]: w_c . xs + b_c of every row (sklearn's decision_function; one column for two classes)."""
    x, ldx = _rows(x, "x")
    if x.shape[1] != model.mean.numel():
        raise ValueError(f"x has {x.shape[1]} columns, the model {model.mean.numel()}")
    ev = _Passes(x, ldx, None, model.mean, model.inv_scale, model.weights.shape[0], 0, model.C)
    return ev.decision(model.weights, want_values=True)[1]


def predict(model, x):
    """int64 [n]: the label with the largest decision value (ties to the smaller label); two classes: the larger label where z > 0."""
    x, ldx = _rows(x, "x")
    if x.shape[1] != model.mean.numel():
        raise ValueError(f"x has {x.shape[1]} columns, the model {model.mean.numel()}")
    ev = _Passes(x, ldx, None, model.mean, model.inv_scale, model.weights.shape[0], 0, model.C)
    col, _ = ev.decision(model.weights)
    return model.classes[col.long()]


def score(model, x, y):
    """Accuracy (a Python float) of ``predict(model, x)`` against the integer labels ``y``."""
    y = _labels(y, "y")
    pred = predict(model, x)
    if pred.shape[0] != y.shape[0]:
        raise ValueError(f"{pred.shape[0]} embeddings, {y.shape[0]} labels")
    return float((pred == y.to(pred.device)).double().mean())


def separability_score(x_train, y_train, x_test=None, y_test=None, method="svm", ret_preds=False, test_size=0.33, generator=None, **fit_args):
    """(train_score, test_score[, preds, y_test]): the reference's get_separability_score with method='svm'.

    Without a test set the train rows are split by a permutation drawn from ``generator`` (torch.randperm; the first
    ceil(test_size * n) rows of it are the test set).  This is NOT sklearn's ``train_test_split(random_state=42)`` permutation: the
    split is reproducible under a seeded generator, not equal to the notebook's.  ``method='sgd'`` raises NotImplementedError."""
    if method == "sgd":
        raise NotImplementedError("method='sgd' is sklearn's SGDClassifier with an unseeded shuffle: a stochastic approximate fit whose "
                                  "result changes from run to run, so there is no defined result to compute; use method='svm' "
                                  "(LinearSVC), which the notebook accepts as well")
    if method != "svm":
        raise ValueError(f"method {method!r}: 'svm'")
    y_train = _labels(y_train, "y_train")
    if (x_test is None) != (y_test is None):
        raise ValueError("x_test and y_test go together")
    if x_test is None:
        if not (isinstance(x_train, torch.Tensor) and x_train.dim() == 2 and x_train.shape[0] == y_train.shape[0]):
            raise ValueError("x_train must be a 2-D tensor with one row per label")
        n = y_train.shape[0]
        n_test = int(math.ceil(float(test_size) * n))
        if not 0 < n_test < n:
            raise ValueError(f"test_size {test_size} leaves an empty side ({n} rows)")
        perm = torch.randperm(n, generator=generator, device=generator.device if generator is not None else "cpu")
        test, train = perm[:n_test], perm[n_test:]
        y_test, y_train = y_train[test.to(y_train.device)], y_train[train.to(y_train.device)]
        x_test, x_train = x_train[test.to(x_train.device)], x_train[train.to(x_train.device)]
    else:
        y_test = _labels(y_test, "y_test")
    classes = torch.unique(y_train)
    if classes.numel() < 2:
        raise ValueError(f"the training labels hold {classes.numel()} class; at least two are needed")
    _encode(y_test, classes, "y_test")
    model = fit(x_train, y_train, **fit_args)
    train_score = score(model, x_train, y_train)
    preds = predict(model, x_test)
    if preds.shape[0] != y_test.shape[0]:
        raise ValueError(f"{preds.shape[0]} test embeddings, {y_test.shape[0]} test labels")
    y_test = y_test.to(preds.device)
    test_score = float((preds == y_test).double().mean())
    return (train_score, test_score, preds, y_test) if ret_preds else (train_score, test_score)
