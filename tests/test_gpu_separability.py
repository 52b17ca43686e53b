"""bvc_op_colstats / bvc_op_linear_pass (csrc/separability.hip, through the C ABI) and bvc.separability: StandardScaler + LinearSVC on
device embeddings.

Reference, float32 model, inputs and caps: tests/separability_ref.py (pinned on the CPU by tests/test_separability_ref.py, which also
checks the conditions assumed here: the ambiguity shares of the DECISION and fit cases and the margin gaps of the HESSVEC cases).
Operands, outputs and workspace are carved from an attention_ref.Arena (NaN-reading guard bands on both sides of each, checked after
every call); padding columns of strided operands hold NaN; the outputs are pre-filled with a poison and every slot must have been
written.  Every figure is printed and logged (gpu_util.log_parity) before anything is asserted.

Bars, per case and per output (z, loss, G):
  every element's |kernel - float64| at most ROW_BAR = 2.5 (the project's ratio) x the worst |model32 - float64| of the case's own
    inputs - the model follows the op's order (d-ordered chain for z, the op's row ranges for the row sums), so the ratio is
    about 1 - and within its derived cap (separability_ref.z_cap / loss_cap / grad_cap / hess_cap).
The float64 reference of a pass takes the pass's own float32 operands (x, mean, inv_std, W, V) exactly.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():   # collected on the CPU box, run on the GPU box
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import attention_ref as AR   # noqa: E402
from tests import gpu_util as G   # noqa: E402
from tests import separability_ref as S   # noqa: E402
from tests.test_separability_ref import DECISION_CASES, HESSVEC_CASES   # noqa: E402

L = G.L
dev = "cuda"
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
ROW_BAR = 2.5
POISON = -12345
MODE = {"grad": 0, "hessvec": 1, "decision": 2}
sep = G.bvc.separability


def _layout(n, D, K):
    lib = L.lib()
    return lib.bvc_op_linear_pass_tile_rows(D), lib.bvc_op_linear_pass_splits(n, D, K)


def _pass(mode, x, labels, mean, inv_std, W, V=None, class0=0, C=1.0, ldx=None, want_dec=True, repeat=1):
    """bvc_op_linear_pass on guarded memory; returns dict(G, loss, pred, dec) of numpy arrays (those the mode writes)."""
    n, D = x.shape
    K = W.shape[0]
    ldx = ldx or D
    nbytes = L.lib().bvc_op_linear_pass_workspace(n, D, K, MODE[mode])
    assert nbytes > 0
    A = AR.Arena(dev, x=((n, ldx), F32), labels=((n,), I32), mean=((D,), F32), inv_std=((D,), F32), W=((K, D + 1), F32), V=((K, D + 1), F32),
                 G=((K, D + 1), F32), loss=((K,), F32), pred=((n,), I32), dec=((n, K), F32), ws=((nbytes,), U8))
    A["x"].fill_(float("nan"))           # the padding columns read as NaN
    A["x"][:, :D].copy_(torch.from_numpy(x.copy()))
    A["labels"].copy_(torch.from_numpy(np.asarray(labels, np.int32).copy()))
    for name, src in (("mean", mean), ("inv_std", inv_std), ("W", W), ("V", V if V is not None else np.zeros_like(W))):
        A[name].copy_(torch.from_numpy(np.asarray(src, np.float32).copy()))
    out = None
    for _ in range(repeat):
        for name in ("G", "loss", "dec"):
            A[name].fill_(float("nan"))
        A["pred"].fill_(POISON)
        dec = mode == "decision"
        L.check(L.lib().bvc_op_linear_pass(G.ptr(A["x"]), ldx, G.ptr(A["labels"]), G.ptr(A["mean"]), G.ptr(A["inv_std"]), G.ptr(A["W"]),
                                           G.ptr(A["V"]) if mode == "hessvec" else None, n, D, K, class0, MODE[mode], C,
                                           None if dec else G.ptr(A["G"]), G.ptr(A["loss"]) if mode == "grad" else None,
                                           G.ptr(A["pred"]) if dec else None, G.ptr(A["dec"]) if dec and want_dec else None,
                                           G.ptr(A["ws"]), G.stream()), "bvc_op_linear_pass")
        torch.cuda.synchronize()
        got = {k: A[k].cpu().numpy() for k in ("G", "loss", "pred", "dec")}
        A.check()
        if dec:
            assert (got["pred"] != POISON).all(), "a prediction was not written"
            assert not want_dec or not np.isnan(got["dec"]).any(), "a decision value was not written"
            assert want_dec or np.isnan(got["dec"]).all(), "decision values written without being asked for"
        else:
            assert not np.isnan(got["G"]).any(), "an element of G was not written"
            assert mode != "grad" or not np.isnan(got["loss"]).any(), "a loss was not written"
        assert np.array_equal(A["x"][:, :D].cpu().numpy(), x) and np.array_equal(A["W"].cpu().numpy(), np.asarray(W, np.float32)), "operand changed"
        if out is not None:
            for k in got:
                assert np.array_equal(out[k].view(np.int32), got[k].view(np.int32)), f"two runs differ in {k}"
        out = got
    return out


def _bar(label, what, got, ref, model, cap):
    """Figures first, then: every element within ROW_BAR x the model's worst error, and within its cap."""
    err = np.abs(got.astype(np.float64) - ref)
    merr = float(np.abs(model.astype(np.float64) - ref).max())
    worst = float(err.max())
    ratio = worst / merr if merr > 0 else (0.0 if worst == 0 else float("inf"))
    with np.errstate(divide="ignore", invalid="ignore"):
        capr = float(np.nanmax(np.where(err > 0, err / cap, 0.0)))
    G.log_parity(f"separability {label} {what}: error {worst:.2e} / model {merr:.2e} = {ratio:.2f}; error / cap {capr:.3f}")
    return ratio, capr


def _hold(results):
    for ratio, capr in results:
        assert ratio <= ROW_BAR, f"kernel error is {ratio:.2f} x the model's"
        assert capr <= 1.0, f"a value is {capr:.2f} x its derivable worst case"


# --------------------------------------------------------------------------- 1. column statistics
@pytest.mark.parametrize("n", [1, 2, 257])
@pytest.mark.parametrize("D", [1, 3, 64, 770])
def test_colstats(n, D):
    r = np.random.RandomState(100 * n + D)
    x = (r.randn(n, D) * np.exp(r.randn(D))[None, :] + 3.0 * r.randn(D)[None, :]).astype(np.float32)
    x[:, 0] = (1e3 + 1e-2 * r.randn(n)).astype(np.float32)       # mean 1e3, standard deviation 1e-2
    if D >= 3:
        x[:, 1] = 3.25                                            # constant: scale exactly 1
    ldx = D + 3
    A = AR.Arena(dev, x=((n, ldx), F32), mean=((D,), F32), inv_std=((D,), F32))
    A["x"].fill_(float("nan"))
    A["x"][:, :D].copy_(torch.from_numpy(x))
    A["mean"].fill_(float("nan")); A["inv_std"].fill_(float("nan"))
    L.check(L.lib().bvc_op_colstats(G.ptr(A["x"]), ldx, n, D, G.ptr(A["mean"]), G.ptr(A["inv_std"]), G.stream()), "bvc_op_colstats")
    torch.cuda.synchronize()
    mean, inv = A["mean"].cpu().numpy(), A["inv_std"].cpu().numpy()
    A.check()
    assert not np.isnan(mean).any() and not np.isnan(inv).any(), "a statistic was not written"
    _, m64, s64 = S.standardise64(x)
    # one rounding of a float64 result: relative error at most u (and 1e-12 for the order of the float64 sums; the variance of the
    # 1e3 +- 1e-2 column is a sum of squared deviations from the float64 mean, not a difference of large sums)
    em = float((np.abs(mean - m64) / np.maximum(np.abs(m64), 1e-30)).max())
    es = float((np.abs(inv * s64 - 1.0)).max())
    G.log_parity(f"separability colstats n{n} D{D}: mean relative error {em:.2e}, inv_std relative error {es:.2e} (bar {S.U * 1.01 + 1e-12:.2e})")
    assert em <= S.U * 1.01 + 1e-12 and es <= S.U * 1.01 + 1e-12
    if D >= 3 or n == 1:
        assert inv[1 if D >= 3 else 0] == 1.0
    if n == 1:
        assert (inv == 1.0).all() and np.array_equal(mean, x[0])
    dense, _ = sep.colstats(torch.from_numpy(x).to(dev))
    assert np.array_equal(dense.cpu().numpy(), mean)


# --------------------------------------------------------------------------- 2. GRAD
# (n, D, K, options): every value of n in {1, 31, 33, 257}, D in {1, 3, 64, 192, 768, 1280} and K in {2, 3, 10, 33, 101, 174} at
# least twice; both tile heights (32 rows to D = 831, 16 above), all three accumulator widths (D + 1 <= 256, <= 832, <= 1344),
# one and several row ranges, one and several class chunks, the row, column and class tails.
GRAD_GRID = [(1, 1, 2, ""), (1, 64, 10, ""), (1, 768, 174, ""), (1, 1280, 3, ""), (31, 1, 3, ""), (31, 3, 33, ""), (31, 192, 2, "zero"),
             (31, 768, 10, "stride"), (31, 1280, 101, ""), (33, 1, 10, "zero"), (33, 3, 174, ""), (33, 64, 2, "stride"), (33, 192, 101, ""),
             (33, 768, 33, "empty"), (33, 1280, 174, ""), (257, 1, 33, ""), (257, 3, 3, "empty"), (257, 3, 101, "zero"), (257, 64, 10, ""),
             (257, 64, 174, "stride"), (257, 192, 3, ""), (257, 192, 33, "zero"), (257, 192, 174, "empty"), (257, 768, 2, ""),
             (257, 768, 10, "zero"), (257, 768, 101, ""), (257, 1280, 2, "empty"), (257, 1280, 10, "stride"), (257, 1280, 33, ""),
             (1, 3, 101, "zero")]


def test_grad_grid_covers_every_axis_value_twice():
    for axis, values in ((0, {1, 31, 33, 257}), (1, {1, 3, 64, 192, 768, 1280}), (2, {2, 3, 10, 33, 101, 174})):
        seen = [g[axis] for g in GRAD_GRID]
        assert set(seen) == values and all(seen.count(v) >= 2 for v in values), axis
    assert {g[3] for g in GRAD_GRID} == {"", "zero", "stride", "empty"}
    lib = L.lib()
    assert {lib.bvc_op_linear_pass_tile_rows(g[1]) for g in GRAD_GRID} == {16, 32}
    assert {min(lib.bvc_op_linear_pass_splits(*g[:3]), 2) for g in GRAD_GRID} == {1, 2}


def _columns(K):
    return (1, 1) if K == 2 else (K, 0)


@pytest.mark.parametrize("i", range(len(GRAD_GRID)), ids=[f"n{g[0]}-D{g[1]}-K{g[2]}{'-' + g[3] if g[3] else ''}" for g in GRAD_GRID])
def test_grad_pass(i):
    n, D, K, opt = GRAD_GRID[i]
    cols, class0 = _columns(K)
    x, labels = S.clustered(n, D, K, 2000 + i, constant_column=1 if D >= 3 else None, empty_class=opt == "empty")
    mean, inv_std = S.stats32(x)
    W = np.zeros((cols, D + 1), np.float32) if opt == "zero" else S.random_weights(cols, D, 3000 + i)
    tile, splits = _layout(n, D, cols)
    rr = S.ranges(n, tile, splits)
    got = _pass("grad", x, labels, mean, inv_std, W, class0=class0, ldx=D + 5 if opt == "stride" else None)
    xs1, y = S.apply64(x, mean, inv_std), S.signs(labels, cols, class0)
    m = S.model32("grad", x, labels, mean, inv_std, W, class0=class0, tile_rows=tile, splits=splits)
    label = f"grad n{n} D{D} K{K} {opt}".strip()
    res = [_bar(label, "loss", got["loss"], S.loss64(W, xs1, y), m["loss"], S.loss_cap(W, xs1, y, rr)),
           _bar(label, "G", got["G"], S.datagrad64(W, xs1, y), m["G"], S.grad_cap(W, xs1, y, 1.0, rr))]
    _hold(res)
    if opt == "zero":
        assert np.array_equal(got["loss"], np.full(cols, n, np.float32))      # every margin is exactly 1
    if opt == "empty" and cols > 1:
        assert (y[:, cols - 1] < 0).all()      # the class without a positive row is in the case


def test_grad_pass_with_another_C():
    n, D, K = 33, 64, 3
    x, labels = S.clustered(n, D, K, 71)
    mean, inv_std = S.stats32(x)
    W = S.random_weights(K, D, 72)
    tile, splits = _layout(n, D, K)
    got = _pass("grad", x, labels, mean, inv_std, W, C=0.3)
    xs1, y = S.apply64(x, mean, inv_std), S.signs(labels, K)
    m = S.model32("grad", x, labels, mean, inv_std, W, C=0.3, tile_rows=tile, splits=splits)
    C32 = float(np.float32(0.3))
    _hold([_bar("grad C0.3", "G", got["G"], S.datagrad64(W, xs1, y, C32), m["G"], S.grad_cap(W, xs1, y, C32, S.ranges(n, tile, splits)))])


# --------------------------------------------------------------------------- 3. HESSVEC
@pytest.mark.parametrize("n,D,K,seed", HESSVEC_CASES)
def test_hessvec_pass(n, D, K, seed):
    cols, class0 = _columns(K)
    x, labels, mean, inv_std, W, V = S.margin_safe(n, D, cols, seed, class0=class0)
    tile, splits = _layout(n, D, cols)
    rr = S.ranges(n, tile, splits)
    got = _pass("hessvec", x, labels, mean, inv_std, W, V, class0=class0)
    xs1, y = S.apply64(x, mean, inv_std), S.signs(labels, cols, class0)
    m = S.model32("hessvec", x, labels, mean, inv_std, W, V, class0=class0, tile_rows=tile, splits=splits)
    _hold([_bar(f"hessvec n{n} D{D} K{K}", "G", got["G"], S.datahess64(W, V, xs1, y), m["G"], S.hess_cap(W, V, xs1, y, 1.0, rr))])
    zero = _pass("hessvec", x, labels, mean, inv_std, W, np.zeros_like(V), class0=class0)
    assert (zero["G"] == 0).all(), "V = 0 must give exactly 0"


# --------------------------------------------------------------------------- 4. DECISION
@pytest.mark.parametrize("n,D,K,seed", DECISION_CASES)
def test_decision_pass(n, D, K, seed):
    cols, _ = _columns(K)
    x, labels = S.clustered(n, D, K, seed)
    mean, inv_std = S.stats32(x)
    W = S.random_weights(cols, D, seed + 1)
    got = _pass("decision", x, labels, mean, inv_std, W)
    xs1 = S.apply64(x, mean, inv_std)
    z = xs1 @ W.astype(np.float64).T
    cap = S.z_cap(xs1, W)
    m = S.model32("decision", x, labels, mean, inv_std, W)
    res = _bar(f"decision n{n} D{D} K{K}", "z", got["dec"], z, m["z"], cap)
    clear = S.top_two_gap(z) >= 2.0 * cap.max(1)
    G.log_parity(f"separability decision n{n} D{D} K{K}: {int((~clear).sum())} of {n} rows ambiguous, "
                 f"{int((got['pred'] != S.predict64(W, xs1)).sum())} predictions differ from float64")
    _hold([res])
    assert (~clear).mean() <= 0.10
    assert np.array_equal(got["pred"][clear], S.predict64(W, xs1)[clear])
    assert np.array_equal(got["pred"], S.first_max(got["dec"])), "pred is not the first maximum of the returned values"
    quiet = _pass("decision", x, labels, mean, inv_std, W, want_dec=False)
    assert np.array_equal(quiet["pred"], got["pred"])


def test_decision_exact_tie_goes_to_the_smaller_class():
    n, D, K = 40, 5, 7
    r = np.random.RandomState(5)
    x = r.randint(-3, 4, (n, D)).astype(np.float32)
    mean, inv_std = np.zeros(D, np.float32), np.ones(D, np.float32)
    W = r.randint(-2, 3, (K, D + 1)).astype(np.float32)      # small integers: every z is exact
    W[5] = W[2]                                               # classes 2 and 5 always tie
    W[2, D] = W[5, D] = 100.0                                 # and are the largest
    got = _pass("decision", x, np.zeros(n, np.int32), mean, inv_std, W)
    assert np.array_equal(got["dec"].astype(np.float64), S.apply64(x, mean, inv_std) @ W.astype(np.float64).T)
    assert (got["pred"] == 2).all()


# --------------------------------------------------------------------------- 5. reproducibility
def test_two_runs_give_the_same_bits():
    """The entry point exposes no split or grid parameter: the row ranges are a function of (n, D, K) alone."""
    n, D, K = 257, 192, 10
    x, labels = S.clustered(n, D, K, 81)
    mean, inv_std = S.stats32(x)
    W = S.random_weights(K, D, 82)
    a = _pass("grad", x, labels, mean, inv_std, W, repeat=2)
    G.bvc.use_deterministic_algorithms(True)
    try:
        b = _pass("grad", x, labels, mean, inv_std, W)
    finally:
        G.bvc.use_deterministic_algorithms(False)
    assert torch.equal(torch.from_numpy(a["G"]), torch.from_numpy(b["G"])) and torch.equal(torch.from_numpy(a["loss"]), torch.from_numpy(b["loss"]))
    assert L.lib().bvc_op_linear_pass_splits(n, D, K) == 9


def test_class_chunks_of_the_host_loop_give_the_bits_of_one_call(monkeypatch):
    """More columns than one call takes are a host loop over class chunks (bvc.separability.MAX_COLUMNS); with the limit lowered to
    32 a 101-class problem runs as 4 calls with class0 = 0, 32, 64, 96.  Both forms cut the 33 rows into the same two row ranges, so
    every output must have the bits of the single call; a wrong class0 of a chunk would change its signs and with them loss and G."""
    n, D, K = 33, 64, 101
    assert L.lib().bvc_op_linear_pass_splits(n, D, K) == L.lib().bvc_op_linear_pass_splits(n, D, 32) == L.lib().bvc_op_linear_pass_splits(n, D, 5) == 2
    x, _ = S.clustered(n, D, K, 61)
    labels = np.random.RandomState(62).permutation(K)[:n].astype(np.int32)      # labels in every chunk, 33 distinct classes
    mean, inv_std = S.stats32(x)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    W, V = t(S.random_weights(K, D, 63)), t(S.random_weights(K, D, 64))

    def run():
        ev = sep._Passes(t(x), D, t(labels), t(mean), t(inv_std), K, 0, 1.0)
        loss, Gr = ev.grad(W)
        pred, dec = ev.decision(W, want_values=True)
        return loss, Gr, ev.hessvec(W, V), pred, dec, ev.decision(W)[0]

    one = run()
    monkeypatch.setattr(sep, "MAX_COLUMNS", 32)
    many = run()
    for a, b, what in zip(one, many, ("loss", "G", "hessvec", "pred", "dec", "pred alone")):
        assert a.dtype == b.dtype and torch.equal(a, b), what
    xs1, y = S.apply64(x, mean, inv_std), S.signs(labels, K)
    Wn = W.cpu().numpy()
    assert (np.abs(many[1].cpu().numpy() - S.datagrad64(Wn, xs1, y)) <= S.grad_cap(Wn, xs1, y, 1.0, S.ranges(n, 32, 2))).all()
    assert np.array_equal(many[3].cpu().numpy(), S.first_max(many[4].cpu().numpy()))


# --------------------------------------------------------------------------- 6. fit
_fits = {}


def _fit(name):
    if name not in _fits:
        c = S.solver_case(name)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)      # a convergence warning fails the case
            model = sep.fit(torch.from_numpy(c["x"].copy()).to(dev), torch.from_numpy(c["labels"].astype(np.int64)), keep_iterates=True)
        mean, inv = model.mean.cpu().numpy(), model.inv_scale.cpu().numpy()
        xs1 = S.apply64(c["x"], mean, inv)
        _fits[name] = dict(model=model, xs1=xs1, xs1_test=S.apply64(c["x_test"], mean, inv), W_star=S.solve64(xs1, c["y"]))
    return _fits[name]


@pytest.mark.parametrize("name", list(S.SOLVER_CASES))
def test_fit(name):
    c, f = S.solver_case(name), _fit(name)
    model, xs1 = f["model"], f["xs1"]
    n, D = c["x"].shape
    W = model.weights.cpu().numpy()
    assert W.shape == (c["columns"], D + 1) and model.coef.shape == (c["columns"], D) and model.intercept.shape == (c["columns"],)
    assert np.array_equal(model.classes.cpu().numpy(), np.arange(c["K"]))
    assert np.allclose(model.mean.cpu().numpy(), S.stats32(c["x"])[0], rtol=2.0 ** -23, atol=0)
    tile, splits = _layout(n, D, c["columns"])
    thr = S.stopping_threshold(xs1, c["y"])
    capn = np.linalg.norm(S.grad_cap(W, xs1, c["y"], 1.0, S.ranges(n, tile, splits)), axis=1)
    g = np.linalg.norm(S.gradient64(W, xs1, c["y"]), axis=1)
    dist = np.linalg.norm(W.astype(np.float64) - f["W_star"], axis=1)
    hist = model.history.cpu().numpy()
    G.log_parity(f"separability fit {name}: iterations {model.n_iter.tolist()}, passes {model.passes}; float64 |grad| / (threshold + cap) "
                 f"{float((g / (thr + capn)).max()):.3f} (threshold {thr.max():.2e}, cap {capn.max():.2e}); |w - w*| / bound {float((dist / (thr + capn)).max()):.3f}")
    assert bool(model.converged.all())
    assert (g <= thr + capn).all()
    assert (dist <= thr + capn).all()      # strong convexity with modulus 1: |w - w*| <= |grad f(w)|
    # every f_c non-increasing: evaluated in float64 at the weights of every outer iteration, a step may raise f_c by at most the
    # derived allowance of separability_ref.rise_allowance (the float32 slope's error x the step + two loss caps)
    it = model.iterates.cpu().numpy()
    rr = S.ranges(n, tile, splits)
    rise, share, lowered = S.worst_rise(it, xs1, c["y"], 1.0, rr)
    f64 = np.stack([S.objective64(w, xs1, c["y"]) for w in it])
    G.log_parity(f"separability fit {name}: largest float64 f(next) - f(previous) over the accepted steps {rise:.3e} (share of the allowance "
                 f"{share:.3f}), {lowered} steps lowered f; largest rise of the evaluated history {float((hist[1:] - hist[:-1]).max()):.3e}")
    assert it.shape == hist.shape + (D + 1,) and np.array_equal(it[-1], W) and hist.shape[1] == c["columns"]
    assert share <= 1.0 and lowered >= int(model.n_iter.sum()) // 2
    caps = np.stack([S.loss_cap(w, xs1, c["y"], rr) for w in it[:: max(1, len(it) // 4)]])      # the history is the evaluated f
    assert (np.abs(hist - f64)[:: max(1, len(it) // 4)] <= caps + 1e-12 * f64[:: max(1, len(it) // 4)]).all()
    assert np.allclose(model.threshold.cpu().numpy(), thr, rtol=1e-4)
    # held-out predictions against the float64 optimum's
    z = f["xs1_test"] @ f["W_star"].T
    clear = S.top_two_gap(z) >= S.flip_bound(z, thr + capn, f["xs1_test"])
    pred = sep.predict(model, torch.from_numpy(c["x_test"].copy()).to(dev)).cpu().numpy()
    want = S.predict64(f["W_star"], f["xs1_test"])
    G.log_parity(f"separability fit {name}: {int((pred != want).sum())} of {S.HELD_OUT} held-out predictions differ, {int((~clear).sum())} rows within the bound")
    assert pred.dtype == np.int64 and (~clear).mean() <= 0.05
    assert np.array_equal(pred[clear], want[clear])


# --------------------------------------------------------------------------- 7. the score
def test_separability_score_matches_the_float64_pipeline():
    name = "257x64x10"
    c, f = S.solver_case(name), _fit(name)
    xtr, xte = torch.from_numpy(c["x"].copy()).to(dev), torch.from_numpy(c["x_test"].copy()).to(dev)
    ytr, yte = torch.from_numpy(c["labels"].astype(np.int64)), torch.from_numpy(c["labels_test"].astype(np.int64))
    out = sep.separability_score(xtr, ytr, xte, yte)
    assert isinstance(out, tuple) and len(out) == 2 and all(isinstance(v, float) for v in out)
    tile, splits = _layout(*c["x"].shape, c["columns"])
    W = f["model"].weights.cpu().numpy()
    dw = S.stopping_threshold(f["xs1"], c["y"]) + np.linalg.norm(S.grad_cap(W, f["xs1"], c["y"], 1.0, S.ranges(c["x"].shape[0], tile, splits)), axis=1)
    want, slack = [], []
    for xs1, lab in ((f["xs1"], c["labels"]), (f["xs1_test"], c["labels_test"])):
        z = xs1 @ f["W_star"].T
        want.append(float((S.first_max(z) == lab).mean()))
        slack.append(float((S.top_two_gap(z) < S.flip_bound(z, dw, xs1)).mean()))      # rows that may go either way
    G.log_parity(f"separability score {name}: {out} / float64 {tuple(want)}, shares within the bound {tuple(slack)}")
    assert abs(out[0] - want[0]) <= slack[0] + 1e-12 and abs(out[1] - want[1]) <= slack[1] + 1e-12 and slack[1] <= 0.05
    full = sep.separability_score(xtr, ytr, xte, yte.to(dev), ret_preds=True)
    assert len(full) == 4 and full[:2] == out and full[2].shape == (S.HELD_OUT,) and torch.equal(full[3].cpu(), yte)
    # bf16 input is cast (the rounded embeddings are another problem: only the shape of the answer is checked)
    b = sep.separability_score(xtr.bfloat16(), ytr, xte.bfloat16(), yte)
    assert len(b) == 2 and 0.0 <= b[1] <= 1.0
    # shifted labels come back as labels
    shifted = sep.separability_score(xtr, ytr * 3 + 7, xte, yte * 3 + 7, ret_preds=True)
    assert shifted[:2] == out and torch.equal(shifted[2], full[2] * 3 + 7)
    # strided rows
    wide = torch.full((c["x"].shape[0], c["x"].shape[1] + 3), float("nan"), device=dev)
    wide[:, :c["x"].shape[1]] = xtr
    assert sep.separability_score(wide[:, :c["x"].shape[1]], ytr, xte, yte) == out


def test_separability_score_splits_reproducibly_and_refuses_what_it_cannot_do():
    c = S.solver_case("300x16x3")
    x, y = torch.from_numpy(c["x"].copy()).to(dev), torch.from_numpy(c["labels"].astype(np.int64))
    a = sep.separability_score(x, y, generator=torch.Generator().manual_seed(3), ret_preds=True)
    b = sep.separability_score(x, y, generator=torch.Generator().manual_seed(3), ret_preds=True)
    assert a[:2] == b[:2] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and a[3].shape == (99,)      # ceil(0.33 * 300)
    with pytest.raises(NotImplementedError):
        sep.separability_score(x, y, x, y, method="sgd")
    with pytest.raises(ValueError):
        sep.separability_score(x, y.float(), x, y)
    with pytest.raises(ValueError):
        sep.separability_score(x, [str(int(v)) for v in y], x, y)
    with pytest.raises(ValueError):
        sep.separability_score(x, y, x, y + 1)      # label 3 is not among the training labels
    with pytest.raises(ValueError):
        sep.separability_score(x, torch.zeros_like(y), x, y)
    with pytest.raises(ValueError):
        sep.fit(x.cpu(), y)


# --------------------------------------------------------------------------- 8. refusals
def test_invalid_arguments_launch_nothing():
    n, D, K = 8, 4, 3
    x, labels = S.clustered(n, D, K, 1)
    mean, inv_std = S.stats32(x)
    W = S.random_weights(K, D, 2)
    A = AR.Arena(dev, x=((n, D), F32), labels=((n,), I32), mean=((D,), F32), inv_std=((D,), F32), W=((K, D + 1), F32), G=((K, D + 1), F32),
                 loss=((K,), F32), pred=((n,), I32), ws=((1 << 16,), U8))
    for name, src in (("x", x), ("labels", labels), ("mean", mean), ("inv_std", inv_std), ("W", W)):
        A[name].copy_(torch.from_numpy(src.copy()))
    A["G"].fill_(-7.0); A["loss"].fill_(-7.0); A["pred"].fill_(POISON); A["ws"].fill_(0x5A)
    P = {k: G.ptr(A[k]) for k in ("x", "labels", "mean", "inv_std", "W", "G", "loss", "pred", "ws")}

    def call(x=P["x"], ldx=D, labels=P["labels"], mean=P["mean"], inv_std=P["inv_std"], W=P["W"], V=P["W"], n=n, D=D, K=K, class0=0, mode=0, C=1.0,
             G_=P["G"], loss=P["loss"], pred=P["pred"], ws=P["ws"]):
        return L.lib().bvc_op_linear_pass(x, ldx, labels, mean, inv_std, W, V, n, D, K, class0, mode, C, G_, loss, pred, None, ws, G.stream())

    for kw in (dict(x=None), dict(labels=None), dict(mean=None), dict(inv_std=None), dict(W=None), dict(G_=None), dict(loss=None), dict(ws=None),
               dict(ldx=D - 1), dict(n=0), dict(D=0), dict(K=0), dict(n=-2), dict(K=1025), dict(D=1344), dict(mode=3), dict(mode=-1),
               dict(mode=1, V=None), dict(mode=2, pred=None), dict(C=0.0)):
        assert call(**kw) == -1 and L.lib().bvc_last_error(), kw      # BVC_ERR_INVALID
    lib = L.lib()
    assert lib.bvc_op_linear_pass_workspace(0, 4, 3, 0) == -1 and lib.bvc_op_linear_pass_workspace(8, 4, 3, 5) == -1
    assert lib.bvc_op_linear_pass_workspace(8, 1344, 3, 0) == -1 and lib.bvc_op_linear_pass_workspace(8, 4, 1025, 0) == -1
    assert lib.bvc_op_colstats(None, D, n, D, P["mean"], P["inv_std"], G.stream()) == -1
    assert lib.bvc_op_colstats(P["x"], D - 1, n, D, P["mean"], P["inv_std"], G.stream()) == -1
    assert lib.bvc_op_colstats(P["x"], D, 0, D, P["mean"], P["inv_std"], G.stream()) == -1
    torch.cuda.synchronize()
    assert bool((A["G"] == -7.0).all()) and bool((A["loss"] == -7.0).all()) and bool((A["pred"] == POISON).all()) and bool((A["ws"] == 0x5A).all()), \
        "a refused call wrote"
    assert np.array_equal(A["mean"].cpu().numpy(), mean)
    A.check()
    assert call() == 0
    torch.cuda.synchronize()
    A.check()
    xs1, y = S.apply64(x, mean, inv_std), S.signs(labels, K)
    assert (np.abs(A["G"].cpu().numpy() - S.datagrad64(W, xs1, y)) <= S.grad_cap(W, xs1, y)).all()
