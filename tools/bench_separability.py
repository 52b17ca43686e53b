"""bvc.separability against torch on one MI355X, at the sizes of the reference's evaluation:

    python tools/bench_separability.py [--shapes ssv2,ssv2-easy10,ucf101,vith-10] [--fit ucf101,ssv2,ssv2-easy10] [--out FILE]
                                       [--sklearn ucf101] [--sklearn-seconds 150]

Two kinds of JSON lines.
  "pass": one GRAD evaluation (bvc_op_linear_pass mode 0: loss and gradient of K one-vs-rest squared-hinge problems from ONE read of
    X, standardised on load) against torch's f32 form on the same GPU - the standardised copy and the sign matrix made once outside
    the timed region, then Xs @ W.T, the element-wise stage and A.T @ Xs.  Same process, order ours / torch / ours again (A / B / A'),
    HIP events around each of 10 calls after 3 warm-ups; median, min and max of each, so drift between A and A' shows.  FLOP are
    counted as 4 n (D + 1) K; the share of the 157.3 TFLOP/s f32 matrix peak follows, and "share_of_hbm_peak" is n D 4 bytes - ONE
    read of X, which is what the pass fetches for K <= 32; with more classes it reads X ceil(K / 32) times and how much of that
    reaches HBM is not measured here - over the time and 8 TB/s.  "colstats" is bvc_op_colstats alone, timed the same way.
  "fit": bvc.separability.fit end to end (column statistics included), wall clock after a synchronise; outer iterations and passes.
    sklearn's LinearSVC on the host is timed in a child process at the shapes named by --sklearn (default ucf101) if sklearn
    imports, with --sklearn-seconds as its limit; otherwise the line says that it was not measured."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402

SHAPES = {"ssv2": (168913, 768, 174), "ssv2-easy10": (168913, 768, 10), "ucf101": (9537, 768, 101), "vith-10": (25000, 1280, 10)}
PEAK_TF, PEAK_TBS = 157.3, 8.0
WARMUP, CALLS = 3, 10


def _time(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _stats(ms):
    return {"ms": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def _data(n, D, K, seed=1234):
    """Clustered embeddings: K class centres (0.15 per coordinate) with unit noise, a per-column scale and offset."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    y = torch.randint(0, K, (n,), device="cuda", generator=gen)
    centres = 0.15 * torch.randn(K, D, device="cuda", generator=gen)
    x = torch.randn(n, D, device="cuda", generator=gen) + centres[y]
    x = x * torch.exp(0.5 * torch.randn(D, device="cuda", generator=gen)) + torch.randn(D, device="cuda", generator=gen)
    return x, y


SKLEARN_CHILD = """
import sys, time, numpy as np
from sklearn.pipeline import make_pipeline
from sklearn.preprocessing import StandardScaler
from sklearn.svm import LinearSVC
d = np.load(sys.argv[1])
t = time.time()
make_pipeline(StandardScaler(), LinearSVC(random_state=0, tol=1e-4)).fit(d["x"], d["y"])
print(time.time() - t)
"""


def _sklearn_seconds(x, y, limit):
    try:
        import sklearn  # noqa: F401
    except ImportError:
        return "not measured: sklearn does not import here"
    import tempfile
    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "xy.npz")
        np.savez(path, x=x.cpu().numpy(), y=y.cpu().numpy())
        try:
            r = subprocess.run([sys.executable, "-c", SKLEARN_CHILD, path], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            return f"not finished within {limit} s"
    return round(float(r.stdout.strip().splitlines()[-1]), 2) if r.returncode == 0 else "failed: " + r.stderr.strip()[-200:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ssv2,ssv2-easy10,ucf101,vith-10")
    ap.add_argument("--fit", default="ucf101,ssv2-easy10,ssv2")
    ap.add_argument("--sklearn", default="ucf101")
    ap.add_argument("--sklearn-seconds", type=int, default=150)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_separability: no GPU (there is nothing to measure without one)")
    ge.build()
    bvc = ge.load_package()
    sep, L, lib = bvc.separability, bvc._lib, bvc._lib.lib()
    out = open(args.out, "w") if args.out else None      # one run, one file: a rerun replaces it

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name in [s for s in args.shapes.split(",") if s]:
        n, D, K = SHAPES[name]
        x, y = _data(n, D, K)
        mean, inv_std = sep.colstats(x)
        W = 0.05 * torch.randn(K, D + 1, device="cuda")
        ev = sep._Passes(x, D, y.to(torch.int32), mean, inv_std, K, 0, 1.0)
        stats_ms = _time(lambda: sep.colstats(x))
        ours_a = _time(lambda: ev.grad(W))
        xs1 = torch.cat([(x - mean) * inv_std, torch.ones(n, 1, device="cuda")], dim=1)
        sign = torch.where(y[:, None] == torch.arange(K, device="cuda")[None, :], 1.0, -1.0)

        def torch_form():
            m = torch.clamp(1.0 - sign * (xs1 @ W.t()), min=0.0)
            return (m * m).sum(0), (-2.0 * sign * m).t() @ xs1

        tm = _time(torch_form)
        ours_b = _time(lambda: ev.grad(W))
        loss, G = ev.grad(W)
        tl, tG = torch_form()
        med = statistics.median(ours_a + ours_b)
        flop, nbytes = 4.0 * n * (D + 1) * K, 4.0 * n * D
        emit({"kind": "pass", "shape": name, "n": n, "D": D, "K": K, "splits": lib.bvc_op_linear_pass_splits(n, D, K),
              "ours_A": _stats(ours_a), "torch_B": _stats(tm), "ours_A2": _stats(ours_b), "ms": round(med, 3), "colstats": _stats(stats_ms),
              "tflops": round(flop / med / 1e9, 1), "share_of_f32_matrix_peak": round(flop / med / 1e9 / PEAK_TF, 3),
              "share_of_hbm_peak": round(nbytes / med / 1e9 / PEAK_TBS, 3), "torch_over_ours": round(statistics.median(tm) / med, 2),
              "G_relative_difference_to_torch": float((G - tG).norm() / tG.norm()), "loss_relative_difference_to_torch": float(((loss - tl) / tl).abs().max())})
        del xs1, sign, ev, x, tG, G
        torch.cuda.empty_cache()

    for name in [s for s in args.fit.split(",") if s]:
        n, D, K = SHAPES[name]
        x, y = _data(n, D, K)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sep.fit(x[:2048], y[:2048] % 3, max_iter=2)      # warm the library and the allocator (two iterations do not converge)
        torch.cuda.synchronize()
        t = time.time()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            model = sep.fit(x, y)
        torch.cuda.synchronize()
        secs = time.time() - t
        t = time.time()
        acc = sep.score(model, x, y)
        torch.cuda.synchronize()
        rec = {"kind": "fit", "shape": name, "n": n, "D": D, "K": K, "seconds": round(secs, 3), "outer_iterations_max": int(model.n_iter.max()),
               "grad_passes": model.passes[0], "hessvec_passes": model.passes[1], "converged": int(model.converged.sum()), "columns": int(model.converged.numel()),
               "warnings": len(caught), "train_accuracy": round(acc, 4), "score_seconds": round(time.time() - t, 3),
               "sklearn_linearsvc_seconds": _sklearn_seconds(x, y, args.sklearn_seconds) if name in args.sklearn.split(",") else "not measured"}
        emit(rec)
        del x, y, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
