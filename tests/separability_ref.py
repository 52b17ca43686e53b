"""Reference, float32 model, inputs and caps for the linear-separability tests  --  TEST INFRASTRUCTURE ONLY (numpy).

Imported by tests/test_separability_ref.py (CPU: pins what is defined here against finite differences and sklearn) and
tests/test_gpu_separability.py (bvc_op_colstats / bvc_op_linear_pass / bvc.separability).  Nothing here touches the library.

Conventions: `xs1` is the standardised matrix with a column of ones appended, [n][D + 1]; `W` is [K][D + 1] with the intercept in
the last column; `y` is the sign matrix [n][K], +1 where the row's label is the column's class.  For two classes there is ONE column,
that of the larger label (sklearn's convention).  Per class the objective is
    f(w) = 1/2 |w|^2 + C sum_i max(0, 1 - y_i w.xs1_i)^2           (the intercept is part of w: it is regularised, as in liblinear).
The "data terms" are what bvc_op_linear_pass returns: loss = sum_i max(0, 1 - y z)^2 and G = the gradient / Hessian-vector product
without the regulariser's + W / + V.
"""
import numpy as np

U = 2.0 ** -24      # unit roundoff of float32: every f32 operation has relative error <= U


# ------------------------------------------------------------------ float64 reference
def standardise64(x):
    """(xs1 [n][D + 1], mean [D], scale [D]): StandardScaler in float64 - population variance, scale 1 where it is exactly 0."""
    x = np.asarray(x, np.float64)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    scale = np.where(var > 0, np.sqrt(np.where(var > 0, var, 1.0)), 1.0)
    return apply64(x, mean, 1.0 / scale), mean, scale


def apply64(x, mean, inv_std):
    """xs1 in float64 from GIVEN statistics (the float32 operands of the pass, taken exactly)."""
    x = np.asarray(x, np.float64)
    return np.concatenate([(x - np.asarray(mean, np.float64)) * np.asarray(inv_std, np.float64), np.ones((x.shape[0], 1))], 1)


def signs(labels, columns, class0=0):
    """y [n][columns]: +1 where labels == class0 + column, else -1."""
    return np.where(np.asarray(labels)[:, None] == class0 + np.arange(columns)[None, :], 1.0, -1.0)


def margins64(W, xs1, y):
    return 1.0 - y * (xs1 @ np.asarray(W, np.float64).T)


def loss64(W, xs1, y):
    return (np.maximum(margins64(W, xs1, y), 0.0) ** 2).sum(0)


def datagrad64(W, xs1, y, C=1.0):
    a = -2.0 * C * y * np.maximum(margins64(W, xs1, y), 0.0)
    return a.T @ xs1


def datahess64(W, V, xs1, y, C=1.0):
    a = 2.0 * C * (margins64(W, xs1, y) > 0) * (xs1 @ np.asarray(V, np.float64).T)
    return a.T @ xs1


def objective64(W, xs1, y, C=1.0):
    W = np.asarray(W, np.float64)
    return 0.5 * (W * W).sum(1) + C * loss64(W, xs1, y)


def gradient64(W, xs1, y, C=1.0):
    return np.asarray(W, np.float64) + datagrad64(W, xs1, y, C)


def hessvec64(W, V, xs1, y, C=1.0):
    return np.asarray(V, np.float64) + datahess64(W, V, xs1, y, C)


def solve64(xs1, y, C=1.0, gtol=1e-10, max_iter=200):
    """The minimisers W [K][D + 1] of every f_c, by Newton's method with the dense generalised Hessian I + 2 C Xa^T Xa (Xa: the active
    rows) and step halving, to |grad f_c| <= gtol.  f_c is piecewise quadratic and strongly convex: Newton ends in finitely many
    steps once the active set is that of the optimum."""
    n, D1 = xs1.shape
    W = np.zeros((y.shape[1], D1))
    for c in range(y.shape[1]):
        yc = y[:, c:c + 1]
        w = np.zeros((1, D1))
        for _ in range(max_iter):
            g = gradient64(w, xs1, yc, C)[0]
            if np.linalg.norm(g) <= gtol:
                break
            act = margins64(w, xs1, yc)[:, 0] > 0
            xa = xs1[act]
            d = np.linalg.solve(np.eye(D1) + 2.0 * C * xa.T @ xa, -g)
            f0, t = objective64(w, xs1, yc, C)[0], 1.0
            while objective64(w + t * d, xs1, yc, C)[0] > f0 + 1e-4 * t * (g @ d) and t > 1e-12:
                t *= 0.5
            w = w + t * d
        assert np.linalg.norm(gradient64(w, xs1, yc, C)[0]) <= gtol, "solve64 did not converge"
        W[c] = w[0]
    return W


def first_max(z):
    """Column of the largest value of each row (the first among equal ones); one column: z > 0."""
    return (z[:, 0] > 0).astype(np.int64) if z.shape[1] == 1 else z.argmax(1)


def predict64(W, xs1):
    return first_max(xs1 @ np.asarray(W, np.float64).T)


def top_two_gap(z):
    """Per row the distance between the two largest decision values; one column: 2 |z| (the distance to the other side)."""
    if z.shape[1] == 1:
        return 2.0 * np.abs(z[:, 0])
    s = np.sort(z, axis=1)
    return s[:, -1] - s[:, -2]


def flip_bound(z, dw, xs1):
    """Per row: a prediction can differ from that of the weights behind `z` only if the top-two gap is below this.  With
    |w_c - w*_c| <= dw[c], a decision value moves by at most dw[c] |(xs, 1)|, so the order of the two largest can change only when
    their gap is below (dw[first] + dw[second]) |(xs, 1)| - 2 |dw|_bound |(xs, 1)| with the two classes' own bounds; one column:
    z changes sign only if 2 |z| < 2 dw |(xs, 1)|."""
    norm = np.linalg.norm(xs1, axis=1)
    if z.shape[1] == 1:
        return 2.0 * dw[0] * norm
    order = np.argsort(z, axis=1)
    return (dw[order[:, -1]] + dw[order[:, -2]]) * norm


# ------------------------------------------------------------------ float32 model of the pass
def _fma32(acc, a, b):
    """float32(acc + a * b) with one rounding to float64 in between: the product of two float32 is exact in float64."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def xs32(x, mean, inv_std):
    """[n][D + 1] float32: (x - mean) * inv_std with two float32 roundings, then the constant 1."""
    x = np.asarray(x, np.float32)
    v = ((x - np.asarray(mean, np.float32)[None, :]).astype(np.float32) * np.asarray(inv_std, np.float32)[None, :]).astype(np.float32)
    return np.concatenate([v, np.ones((x.shape[0], 1), np.float32)], 1)


def z32(xs, W):
    """[n][K] float32: z = fma(xs[d], w[d], z) for d = 0 .. D in that order, from 0 (the op's first product, bit for bit)."""
    W = np.asarray(W, np.float32)
    z = np.zeros((xs.shape[0], W.shape[0]), np.float32)
    for d in range(xs.shape[1]):
        z = _fma32(z, xs[:, d][:, None], W[:, d][None, :])
    return z


def ranges(n, tile_rows, splits):
    """The row ranges of the op: `splits` contiguous runs of whole tiles of `tile_rows` rows."""
    tiles = (n + tile_rows - 1) // tile_rows
    return [(min(n, tiles * s // splits * tile_rows), min(n, tiles * (s + 1) // splits * tile_rows)) for s in range(splits)]


def _rowsum32(a, xs, n_ranges):
    """[K][D + 1] float32: per range one fma chain over its rows in ascending order from 0; the ranges added in ascending order."""
    total = None
    for lo, hi in n_ranges:
        acc = np.zeros((a.shape[1], xs.shape[1]), np.float32)
        for r in range(lo, hi):
            acc = _fma32(acc, a[r][:, None], xs[r][None, :])
        total = acc if total is None else (total + acc).astype(np.float32)
    return total


def model32(mode, x, labels, mean, inv_std, W, V=None, C=1.0, class0=0, tile_rows=32, splits=1):
    """The float32 evaluation the op is allowed to be, in the op's own order: standardisation with two roundings, z as the d-ordered
    fma chain, the element-wise stage in float32, and row sums as one fma chain per row range, ranges added in order.
    Returns dict(z, loss, G) for 'grad', dict(z, G) for 'hessvec', dict(z) for 'decision' (float32 arrays)."""
    xs = xs32(x, mean, inv_std)
    W = np.asarray(W, np.float32)
    z = z32(xs, W)
    if mode == "decision":
        return dict(z=z)
    y = signs(labels, W.shape[0], class0).astype(np.float32)
    m = (np.float32(1.0) - y * z).astype(np.float32)
    on = m > 0
    rr = ranges(x.shape[0], tile_rows, splits)
    if mode == "grad":
        a = np.where(on, ((np.float32(-2.0) * np.float32(C) * y) * m).astype(np.float32), np.float32(0))
        mm = np.where(on, m, np.float32(0))
        loss = None
        for lo, hi in rr:
            acc = np.zeros(W.shape[0], np.float32)
            for r in range(lo, hi):
                acc = _fma32(acc, mm[r], mm[r])
            loss = acc if loss is None else (loss + acc).astype(np.float32)
        return dict(z=z, loss=loss, G=_rowsum32(a, xs, rr))
    assert mode == "hessvec", mode
    zv = z32(xs, V)
    a = np.where(on, ((np.float32(2.0) * np.float32(C)) * zv).astype(np.float32), np.float32(0))
    return dict(z=z, G=_rowsum32(a, xs, rr))


# ------------------------------------------------------------------ caps
# Every cap is first order in u = 2^-24, times 1.01 for the higher orders.  A recursive float32 sum s_j = fl(s_(j-1) + t_j) rounds
# each PARTIAL SUM once, so its error is at most u sum_j |s_j|: the caps use these running sums (evaluated in float64) instead
# of the coarser (number of terms) x sum |t_j|, which at D = 192 would be an order of magnitude wider than any float32 evaluation.
def _running(t, axis):
    """sum over the chain of |partial sum| along `axis`"""
    return np.abs(np.cumsum(t, axis=axis)).sum(axis)


def z_cap(xs1, W):
    """[n][K]: worst case of |z_f32 - z_64|.  Each standardised entry carries two roundings, |xs_f32 - xs| <= 2 u |xs| (x, mean
    and inv_std are exact operands; the subtraction and the multiplication round once each), which moves z by at most 2 u S,
    S = sum_d |xs1_d| |w_d| (intercept column included).  The chain z = fma(xs_d, w_d, z) over the D + 1 columns rounds each
    partial sum once: u sum_j |s_j| with s_j = sum_(d <= j) xs1_d w_d.  Together u (sum_j |s_j| + 2 S) - for operands of one sign
    that is the familiar (D + 3) u S, and never more."""
    W = np.asarray(W, np.float64)
    out = np.empty((xs1.shape[0], W.shape[0]))
    for k0 in range(0, W.shape[0], 8):
        t = xs1[:, None, :] * W[None, k0:k0 + 8, :]
        out[:, k0:k0 + 8] = _running(t, 2) + 2.0 * np.abs(t).sum(2)
    return 1.01 * U * out


def _margin_move(m, ez):
    """Worst case of |max(0, m_f32) - max(0, m)|: m = 1 - y z is one rounding on top of z's error, e_m = e_z + u (|m| + e_z), and
    max(0, .) is 1-Lipschitz; a row whose margin is below -e_m is inactive in both evaluations and moves by nothing, one in
    between by at most m + e_m."""
    em = ez + U * (np.abs(m) + ez)
    return np.minimum(em, np.maximum(m + em, 0.0))


def _row_chain(a, xs1, rr):
    """[K][D + 1]: sum of |partial sum| over the op's row chains of sum_i a_i xs1_id - per range (lo, hi) of `rr` the chain restarts
    at 0 and runs over its rows in order; then the ranges' totals are added in order (one rounding per addition)."""
    out = np.zeros((a.shape[1], xs1.shape[1]))
    for k0 in range(0, a.shape[1], 8):
        c = np.cumsum(a[:, k0:k0 + 8, None] * xs1[:, None, :], axis=0)
        for s, (lo, hi) in enumerate(rr):
            if hi <= lo:
                continue
            base = c[lo - 1] if lo > 0 else 0.0
            out[k0:k0 + 8] += np.abs(c[lo:hi] - base).sum(0)
            if s > 0:
                out[k0:k0 + 8] += np.abs(c[hi - 1])
    return out


def loss_cap(W, xs1, y, rr=None):
    """[K]: worst case of the loss error.  With e_m = _margin_move, a term t = max(0, m)^2 moves by at most e_m (2 max(0, m) + e_m) -
    this covers rows whose margin changes sign.  The chain fma(m, m, loss) and the sum of the ranges round non-negative partial
    sums, each at most the whole sum: at most (n + ranges) u sum_i t_i."""
    rr = rr or [(0, xs1.shape[0])]
    m = margins64(W, xs1, y)
    em = _margin_move(m, z_cap(xs1, W))
    mp = np.maximum(m, 0.0)
    move = em * (2.0 * mp + em)
    return 1.01 * (move.sum(0) + (xs1.shape[0] + len(rr)) * U * (mp ** 2 + move).sum(0))


def grad_cap(W, xs1, y, C=1.0, rr=None):
    """[K][D + 1]: worst case of the error of G = sum_i a_i xs1_id, a = -2 C y max(0, m).  |a_f32 - a| <= 2 C e_m + u |a| (e_m =
    _margin_move, which contains z's cap and through it D; the factor -2 C y is exact for C a power of two and costs one more u
    otherwise, which the 2 u |a| below covers), |xs_f32 - xs| <= 2 u |xs|, and the chains over the rows round their partial sums:
      cap = sum_i (2 C e_m,i + 4 u |a_i|) |xs1_id|  +  u sum over the row chains of |partial sum|      (`rr`: the op's row ranges)."""
    rr = rr or [(0, xs1.shape[0])]
    m = margins64(W, xs1, y)
    em = _margin_move(m, z_cap(xs1, W))
    a = -2.0 * C * y * np.maximum(m, 0.0)
    return 1.01 * ((2.0 * C * em + 4.0 * U * np.abs(a)).T @ np.abs(xs1) + U * _row_chain(a, xs1, rr))


def hess_cap(W, V, xs1, y, C=1.0, rr=None):
    """[K][D + 1]: the same for a = 2 C [m > 0] z(V), VALID ONLY where no margin is within z_cap of 0 (the indicator is then the
    float64 one; margin_safe inputs): |a_f32 - a| <= 2 C e_z(V) + u |a|."""
    rr = rr or [(0, xs1.shape[0])]
    on = margins64(W, xs1, y) > 0
    a = 2.0 * C * on * (xs1 @ np.asarray(V, np.float64).T)
    ea = 2.0 * C * on * z_cap(xs1, V)
    return 1.01 * ((ea + 4.0 * U * np.abs(a)).T @ np.abs(xs1) + U * _row_chain(a, xs1, rr))


def rise_allowance(W_old, W_new, xs1, y, C=1.0, rr=None, exact_pass=False):
    """[K]: how far f_c(W_new) may lie ABOVE f_c(W_old), both evaluated exactly, when the solver accepted the step on results of the
    pass.  The solver accepts on one of two tests.  (1) Slope: the computed grad f_c(W_new) . d <= 0.  The gradient is W_new (exact)
    plus the pass's G, whose error is at most grad_cap, so the true slope is at most e = sum_d grad_cap_d |d_d|; f_c is convex, so
    f_c(W_new) <= f_c(W_old) + t e = f_c(W_old) + sum_d grad_cap_d |W_new - W_old|_d.  W_new is the float32 rounding of W_old + t d,
    which turns the direction by at most u |W_new| per coordinate: + u sum_d |grad f_c(W_new)|_d |W_new|_d.  (2) Value: evaluated
    f(W_new) below evaluated f(W_old), each C x loss_cap from the truth.  The allowance is the sum of both, as the test does not
    know which one decided.  `exact_pass`: the pass is float64 (caps 0); only the rounding of W_new and of float64 itself is left."""
    W_old, W_new = np.asarray(W_old, np.float64), np.asarray(W_new, np.float64)
    turn = U * (np.abs(gradient64(W_new, xs1, y, C)) * np.abs(W_new)).sum(1)
    if exact_pass:
        return turn + 1e-12 * np.maximum(objective64(W_old, xs1, y, C), 1.0)
    slope = (grad_cap(W_new, xs1, y, C, rr) * np.abs(W_new - W_old)).sum(1)
    return turn + slope + C * (loss_cap(W_old, xs1, y, rr) + loss_cap(W_new, xs1, y, rr))


def worst_rise(iterates, xs1, y, C=1.0, rr=None, exact_pass=False):
    """(largest f_c(next) - f_c(previous) over the iterates [steps + 1][K][D + 1] in float64, largest such rise as a share of its
    rise_allowance, number of steps that lowered f): what "every f_c is non-increasing" means for a solver that reads float32."""
    iterates = np.asarray(iterates, np.float64)
    f = np.stack([objective64(w, xs1, y, C) for w in iterates])
    rise, share, lowered = -np.inf, 0.0, 0
    for i in range(1, len(iterates)):
        moved = (iterates[i] != iterates[i - 1]).any(1)
        if not moved.any():
            continue
        up = (f[i] - f[i - 1])[moved]
        allow = rise_allowance(iterates[i - 1], iterates[i], xs1, y, C, rr, exact_pass)[moved]
        rise = max(rise, float(up.max()))
        share = max(share, float((np.maximum(up, 0.0) / allow).max()))
        lowered += int((up < 0).sum())
    return rise, share, lowered


# ------------------------------------------------------------------ inputs
def clustered(n, D, K, seed, sep=2.0, constant_column=None, empty_class=False, informative=None):
    """(x f32 [n][D], labels int32 [n]): K Gaussian clusters with unit noise, then a per-column scale (log-normal) and offset, so
    that standardisation matters.  `constant_column`: that column is 3.25 everywhere.  `empty_class`: no row has label K - 1.
    `informative`: the cluster centres differ in the first that many columns only (the others are noise)."""
    r = np.random.RandomState(seed)
    m = D if informative is None else min(D, informative)
    centres = np.zeros((K, D))
    centres[:, :m] = r.randn(K, m) * sep / np.sqrt(max(m, 1)) * 2.0
    labels = r.randint(0, K - 1 if empty_class and K > 1 else K, n)
    if not empty_class and n >= K:
        labels[:K] = np.arange(K)      # every class present
    x = (centres[labels] + r.randn(n, D)) * np.exp(0.7 * r.randn(D))[None, :] + 5.0 * r.randn(D)[None, :]
    if constant_column is not None:
        x[:, constant_column] = 3.25
    return x.astype(np.float32), labels.astype(np.int32)


def stats32(x):
    """float32 (mean, inv_std) as bvc_op_colstats defines them: float64 statistics rounded once."""
    _, mean, scale = standardise64(x)
    return mean.astype(np.float32), (1.0 / scale).astype(np.float32)


def random_weights(K, D, seed, scale=0.3):
    r = np.random.RandomState(seed)
    return (r.randn(K, D + 1) * scale / np.sqrt(D + 1)).astype(np.float32) * np.float32(3.0)


def margin_safe(n, D, K, seed, gap=1e-3, class0=0):
    """(x, labels, mean, inv_std, W, V): clustered rows in which every margin 1 - y z at W is at least `gap` from 0.  The statistics
    are those of the first draw and stay fixed (they are operands of the pass, not recomputed); a row with a margin inside the gap
    is drawn again."""
    x, labels = clustered(n, D, K if K > 1 else 2, seed)
    mean, inv_std = stats32(x)
    W, V = random_weights(K, D, seed + 1), random_weights(K, D, seed + 2, scale=1.0)
    r = np.random.RandomState(seed + 3)
    for _ in range(100):
        m = margins64(W, apply64(x, mean, inv_std), signs(labels, K, class0))
        bad = np.nonzero((np.abs(m) < gap).any(1))[0]
        if bad.size == 0:
            return x, labels, mean, inv_std, W, V
        x[bad] = (x[bad] + (r.randn(bad.size, D) / inv_std[None, :]).astype(np.float32)).astype(np.float32)
    raise AssertionError("margin_safe: could not clear the gap")


# the solver cases of the issue: (n, D, K, seed); 200 further rows of the same draw are held out
SOLVER_CASES = {"300x16x3": (300, 16, 3, 11), "257x64x10": (257, 64, 10, 12), "500x192x5": (500, 192, 5, 13), "binary200x64": (200, 64, 2, 14)}
HELD_OUT = 200
_solved = {}


def solver_case(name):
    """dict(x, labels (train), x_test, labels_test, xs1, xs1_test, y, W (the float64 optimum), columns, class0, mean, scale), computed once."""
    if name not in _solved:
        n, D, K, seed = SOLVER_CASES[name]
        x, labels = clustered(n + HELD_OUT, D, K, seed, sep=16.0, informative=16)
        xs1, mean, scale = standardise64(x[:n])
        columns, class0 = (1, 1) if K == 2 else (K, 0)
        y = signs(labels[:n], columns, class0)
        for a in (x, labels):
            a.setflags(write=False)
        _solved[name] = dict(x=x[:n], labels=labels[:n], x_test=x[n:], labels_test=labels[n:], xs1=xs1, xs1_test=apply64(x[n:], mean, 1.0 / scale),
                             y=y, W=solve64(xs1, y), columns=columns, class0=class0, mean=mean, scale=scale, K=K)
    return _solved[name]


def stopping_threshold(xs1, y, tol=1e-4):
    """[K]: tol * max(min(pos, neg), 1) / n * |grad f(0)| (liblinear's rule)."""
    n = xs1.shape[0]
    pos = (y > 0).sum(0)
    g0 = np.linalg.norm(gradient64(np.zeros((y.shape[1], xs1.shape[1])), xs1, y), axis=1)
    return tol * np.maximum(np.minimum(pos, n - pos), 1) / n * g0
