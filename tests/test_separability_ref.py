"""CPU pins of tests/separability_ref.py (the reference the GPU tests of bvc.separability are measured against), the conditions
those tests rely on, and the host-side argument checks of bvc.separability that need no GPU.

  gradient64 against central finite differences; hessvec64 against a gradient difference on margin-safe inputs;
  solve64 against sklearn's LinearSVC(tol=1e-10, max_iter=200000) behind StandardScaler, primal and dual, within 1e-6;
  the single column of a two-class problem and its sign; the ambiguity shares and the margin gaps the GPU cases assume;
  the batched solver of bvc.separability on a float32 numpy stand-in of the pass (the solver itself is device-agnostic torch).
"""
import warnings

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from tests import separability_ref as S

SOLVER = list(S.SOLVER_CASES)


def _problem(n, D, K, seed):
    x, labels = S.clustered(n, D, K, seed)
    xs1, _, _ = S.standardise64(x)
    return xs1, S.signs(labels, K)


def test_standardise_is_standardscaler_and_keeps_constant_columns():
    x, _ = S.clustered(257, 7, 3, 1, constant_column=2)
    xs1, mean, scale = S.standardise64(x)
    assert scale[2] == 1.0 and (xs1[:, 2] == 0).all() and (xs1[:, -1] == 1).all()
    live = [0, 1, 3, 4, 5, 6]
    assert np.allclose(xs1[:, live].mean(0), 0, atol=1e-12) and np.allclose(xs1[:, live].std(0), 1, atol=1e-12)
    sk = pytest.importorskip("sklearn.preprocessing")
    ref = sk.StandardScaler().fit(x.astype(np.float64))
    assert np.allclose(ref.mean_, mean, rtol=1e-12) and np.allclose(ref.scale_, scale, rtol=1e-12)


def test_gradient_matches_finite_differences():
    xs1, y = _problem(60, 5, 3, 2)
    W = S.random_weights(3, 5, 3).astype(np.float64)
    g = S.gradient64(W, xs1, y)
    h = 1e-6
    for c in range(3):
        for d in range(6):
            E = np.zeros_like(W)
            E[c, d] = h
            fd = (S.objective64(W + E, xs1, y)[c] - S.objective64(W - E, xs1, y)[c]) / (2 * h)
            assert abs(fd - g[c, d]) <= 1e-6 * max(1.0, abs(g[c, d])), (c, d, fd, g[c, d])


def test_hessvec_matches_a_gradient_difference_away_from_the_kinks():
    x, labels, mean, inv_std, W, V = S.margin_safe(80, 6, 3, 4, gap=1e-2)
    xs1, y = S.apply64(x, mean, inv_std), S.signs(labels, 3)
    W, V = W.astype(np.float64), V.astype(np.float64)
    h = 1e-6 / np.abs(xs1 @ V.T).max()      # no margin changes sign along the way
    fd = (S.gradient64(W + h * V, xs1, y) - S.gradient64(W - h * V, xs1, y)) / (2 * h)
    hv = S.hessvec64(W, V, xs1, y)
    assert np.abs(fd - hv).max() <= 1e-6 * np.abs(hv).max()


@pytest.mark.parametrize("name", SOLVER)
@pytest.mark.parametrize("dual", [False, True])
def test_solve64_is_linearsvc(name, dual):
    svm = pytest.importorskip("sklearn.svm")
    c = S.solver_case(name)
    xs = c["xs1"][:, :-1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = svm.LinearSVC(random_state=0, tol=1e-10, max_iter=200000, dual=dual).fit(xs, c["labels"])
    assert clf.coef_.shape == (c["columns"], xs.shape[1])
    err = max(np.abs(clf.coef_ - c["W"][:, :-1]).max(), np.abs(clf.intercept_ - c["W"][:, -1]).max())
    assert err <= 1e-6, err
    assert np.array_equal(clf.classes_[S.predict64(c["W"], c["xs1_test"])], clf.predict(c["xs1_test"][:, :-1]))


def test_two_classes_train_one_column_for_the_larger_label():
    c = S.solver_case("binary200x64")
    assert c["W"].shape == (1, 65) and c["class0"] == 1
    assert ((c["y"][:, 0] > 0) == (c["labels"] == 1)).all()
    pred = S.predict64(c["W"], c["xs1"])
    assert (pred == c["labels"]).mean() > 0.9      # positive decision value = the larger label


@pytest.mark.parametrize("name", SOLVER)
def test_solver_cases_have_no_ambiguous_held_out_rows(name):
    """The fit test lets a held-out row go either way when its optimum top-two gap is below separability_ref.flip_bound with
    |dw| = stopping threshold + |G cap|_2, at most 5 % of the rows.  The solver cases are well separated (the gap of a separable
    one-vs-rest optimum is about 2): no held-out row of any case has a gap below 1e-3, and none is below the bound."""
    c = S.solver_case(name)
    z = c["xs1_test"] @ c["W"].T
    gap = S.top_two_gap(z)
    dw = S.stopping_threshold(c["xs1"], c["y"]) + np.linalg.norm(S.grad_cap(c["W"], c["xs1"], c["y"]), axis=1)
    bound = S.flip_bound(z, dw, c["xs1_test"])
    print(name, "smallest gap", gap.min(), "largest bound", bound.max(), "share", (gap < bound).mean())
    assert (gap < 1e-3).sum() == 0
    assert (gap < bound).mean() <= 0.05


# the shapes of the GPU tests' DECISION and HESSVEC cases (tests/test_gpu_separability.py imports these lists)
DECISION_CASES = [(257, 64, 10, 21), (33, 768, 174, 22), (257, 3, 3, 23), (31, 1280, 33, 24), (257, 192, 2, 25)]
HESSVEC_CASES = [(1, 1, 3, 31), (31, 3, 2, 32), (33, 64, 10, 33), (257, 192, 33, 34), (33, 768, 101, 35), (31, 1280, 174, 36), (257, 64, 3, 37)]


@pytest.mark.parametrize("n,D,K,seed", DECISION_CASES)
def test_decision_cases_are_rarely_ambiguous(n, D, K, seed):
    x, labels = S.clustered(n, D, K, seed)
    mean, inv_std = S.stats32(x)
    cols = 1 if K == 2 else K
    W = S.random_weights(cols, D, seed + 1)
    xs1 = S.apply64(x, mean, inv_std)
    z = xs1 @ W.astype(np.float64).T
    cap = S.z_cap(xs1, W)
    amb = S.top_two_gap(z) < 2.0 * cap.max(1)
    assert amb.mean() <= 0.10, amb.mean()


@pytest.mark.parametrize("n,D,K,seed", HESSVEC_CASES)
def test_hessvec_cases_have_no_margin_within_the_z_cap(n, D, K, seed):
    cols, class0 = (1, 1) if K == 2 else (K, 0)
    x, labels, mean, inv_std, W, V = S.margin_safe(n, D, cols, seed, class0=class0)
    xs1 = S.apply64(x, mean, inv_std)
    m = S.margins64(W, xs1, S.signs(labels, cols, class0))
    assert (np.abs(m) > 4.0 * S.z_cap(xs1, W)).all()


def test_model32_is_within_its_caps_of_the_reference():
    x, labels = S.clustered(70, 19, 5, 41, constant_column=3)
    mean, inv_std = S.stats32(x)
    W = S.random_weights(5, 19, 42)
    xs1, y = S.apply64(x, mean, inv_std), S.signs(labels, 5)
    tile, splits = 32, 2
    rr = S.ranges(70, tile, splits)
    m = S.model32("grad", x, labels, mean, inv_std, W, tile_rows=tile, splits=splits)
    assert (np.abs(m["z"] - xs1 @ W.astype(np.float64).T) <= S.z_cap(xs1, W)).all()
    assert (np.abs(m["loss"] - S.loss64(W, xs1, y)) <= S.loss_cap(W, xs1, y, rr)).all()
    assert (np.abs(m["G"] - S.datagrad64(W, xs1, y)) <= S.grad_cap(W, xs1, y, 1.0, rr)).all()
    assert S.ranges(70, 32, 2) == [(0, 32), (32, 70)] and S.ranges(5, 16, 1) == [(0, 5)]


# ------------------------------------------------------------------ bvc.separability on the host
@pytest.fixture(scope="module")
def sep():
    ge.build()
    return ge.load_package().separability


class _HostPasses:
    """A numpy stand-in of the GRAD and HESSVEC passes for the device-agnostic solver: float32 (BLAS order) or float64 results."""

    def __init__(self, xs1, y, dtype=np.float32):
        self.xs, self.y, self.dtype = xs1.astype(dtype), y.astype(dtype), dtype

    def grad(self, W):
        W = W.numpy().astype(self.dtype)
        mp = np.maximum(1.0 - self.y * (self.xs @ W.T), 0).astype(self.dtype)
        return torch.from_numpy((mp * mp).sum(0)), torch.from_numpy(((-2.0 * self.y * mp).T @ self.xs).astype(self.dtype))

    def hessvec(self, W, V):
        W, V = W.numpy().astype(self.dtype), V.numpy().astype(self.dtype)
        on = (1.0 - self.y * (self.xs @ W.T)) > 0
        return torch.from_numpy(((2.0 * on * (self.xs @ V.T)).T @ self.xs).astype(self.dtype))


class _ModelPasses:
    """The passes as separability_ref.model32 computes them: float32 in the op's own order (tile_rows, splits)."""

    def __init__(self, x, labels, mean, inv_std, class0, tile_rows, splits):
        self.a = (x, labels, mean, inv_std)
        self.kw = dict(class0=class0, tile_rows=tile_rows, splits=splits)

    def grad(self, W):
        m = S.model32("grad", *self.a, W.numpy(), **self.kw)
        return torch.from_numpy(m["loss"]), torch.from_numpy(m["G"])

    def hessvec(self, W, V):
        return torch.from_numpy(S.model32("hessvec", *self.a, W.numpy(), V.numpy(), **self.kw)["G"])


@pytest.mark.parametrize("name", SOLVER)
def test_batched_newton_reaches_the_threshold(sep, name):
    c = S.solver_case(name)
    n, D1 = c["xs1"].shape
    pos = torch.from_numpy((c["y"] > 0).sum(0))
    W, info = sep._solve(_HostPasses(c["xs1"], c["y"]), c["columns"], D1, pos, n, 1.0, 1e-4, 100, 16)
    thr = S.stopping_threshold(c["xs1"], c["y"])
    assert bool(info["converged"].all()) and np.allclose(info["threshold"].numpy(), thr, rtol=1e-5)
    g = np.linalg.norm(S.gradient64(W.numpy(), c["xs1"], c["y"]), axis=1)
    print(name, "iterations", info["n_iter"].tolist(), "passes", info["passes"], "gradient / threshold", (g / thr).max())
    assert (g <= 1.5 * thr).all()
    assert np.linalg.norm(W.numpy() - c["W"], axis=1).max() <= 1.5 * thr.max()      # strong convexity, modulus 1
    assert "iterates" not in info and info["history"].shape == (int(info["n_iter"].max()) + 1, c["columns"])


@pytest.mark.parametrize("name", SOLVER)
def test_no_accepted_step_raises_f_with_an_exact_pass(sep, name):
    """The solver's logic alone: with float64 passes every accepted iterate, evaluated independently (objective64), lies at or
    below its predecessor - up to the float32 rounding of the iterate itself (separability_ref.rise_allowance, exact_pass)."""
    c = S.solver_case(name)
    n, D1 = c["xs1"].shape
    pos = torch.from_numpy((c["y"] > 0).sum(0))
    W, info = sep._solve(_HostPasses(c["xs1"], c["y"], np.float64), c["columns"], D1, pos, n, 1.0, 1e-4, 100, 16, keep_iterates=True)
    it = info["iterates"].numpy()
    assert it.shape[0] == info["history"].shape[0] and np.array_equal(it[-1], W.numpy()) and not it[0].any()
    rise, share, lowered = S.worst_rise(it, c["xs1"], c["y"], exact_pass=True)
    print(name, "largest rise", rise, "as a share of the allowance", share, "steps that lowered f", lowered)
    assert share <= 1.0 and lowered >= int(info["n_iter"].sum()) // 2
    h = info["history"].numpy()      # evaluated by the pass: here float64, so the record itself is non-increasing to 1e-12
    assert (h[1:] <= h[:-1] + 1e-12 * np.maximum(h[:-1], 1.0)).all()
    assert np.allclose(h, np.stack([S.objective64(w, c["xs1"], c["y"]) for w in it]), rtol=1e-12)


def test_no_accepted_step_raises_f_beyond_the_float32_allowance(sep):
    """With float32 passes in the op's own order the same holds up to the derived allowance: slope error x step + two loss caps."""
    n, D, K = 120, 12, 3
    x, labels = S.clustered(n, D, K, 91, sep=1.0)      # overlapping classes: the active sets keep changing
    mean, inv_std = S.stats32(x)
    xs1, y = S.apply64(x, mean, inv_std), S.signs(labels, K)
    tile, splits = 32, 2
    pos = torch.from_numpy((y > 0).sum(0))
    W, info = sep._solve(_ModelPasses(x, labels, mean, inv_std, 0, tile, splits), K, D + 1, pos, n, 1.0, 1e-4, 100, 16, keep_iterates=True)
    rise, share, lowered = S.worst_rise(info["iterates"].numpy(), xs1, y, rr=S.ranges(n, tile, splits))
    print("largest rise", rise, "as a share of the allowance", share, "steps that lowered f", lowered, "iterations", info["n_iter"].tolist())
    assert bool(info["converged"].all())
    assert share <= 1.0 and lowered >= int(info["n_iter"].sum()) // 2


def test_host_side_argument_checks(sep):
    x = torch.zeros(6, 4)
    y = torch.tensor([0, 1, 2, 0, 1, 2])
    with pytest.raises(NotImplementedError, match="svm"):
        sep.separability_score(x, y, x, y, method="sgd")
    with pytest.raises(ValueError, match="method"):
        sep.separability_score(x, y, x, y, method="ridge")
    with pytest.raises(ValueError, match="integer"):
        sep.separability_score(x, y.float(), x, y)
    with pytest.raises(ValueError, match="integer"):
        sep.separability_score(x, ["a", "b", "c", "a", "b", "c"], x, y)
    with pytest.raises(ValueError, match="integer"):
        sep.fit(x, np.array([0.0, 1.0, 2.0, 0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="at least two"):
        sep.fit(x, torch.zeros(6, dtype=torch.int64))
    with pytest.raises(ValueError, match="at least two"):
        sep.separability_score(x, torch.zeros(6, dtype=torch.int64), x, y)
    with pytest.raises(ValueError, match="do not have"):
        sep.separability_score(x, y, x, torch.tensor([0, 1, 3, 0, 1, 2]))
    with pytest.raises(ValueError, match="on the GPU"):
        sep.fit(x, y)
    with pytest.raises(ValueError, match="go together"):
        sep.separability_score(x, y, x_test=x)
    with pytest.raises(ValueError, match="positive"):
        sep.fit(x, y, C=0.0)
    with pytest.raises(ValueError, match="empty side"):
        sep.separability_score(x, y, test_size=0.0)
