"""The gradient-norm pass alone against the inf check it replaces, on the flat gradient buffer of a VideoMAE classifier (one MI355X):

    python tools/bench_grad_norm.py [--arch base] [--iters 50] [--rounds 3]

Three read-only passes over the same buffer of random f32 values, timed by device events over `iters` back-to-back calls, the three
alternating `rounds` times: `bvc_op_nonfinite_check` (GradScaler's inf check), `bvc_op_grad_sqnorm_items` with found_inf over the
per-parameter segment table an optimiser plan has (norm + inf check, the launch pair), and the same over a one-segment table.  One JSON
line: microseconds per call of every round and the read rate of the best round (buffer bytes / time)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="base", choices=["small", "base", "large", "huge"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    ge.build()
    bvc = ge.load_package()
    dev = torch.device("cuda:0")
    m = bvc.VideoMAEForVideoClassification(bvc.videomae_config(args.arch, num_labels=400))
    n = m._numel
    starts = [off for _name, off, _shape in m._layout] + [n]
    assert starts == sorted(starts) and starts[0] == 0
    x = torch.randn(n, generator=torch.Generator().manual_seed(0)).to(dev)
    L, lib = bvc._lib, bvc._lib.lib()
    found, total = torch.zeros((), device=dev), torch.zeros(1, device=dev)
    per_param = bvc.optim._NormTable(starts, [0] * (len(starts) - 1), dev)
    whole = bvc.optim._NormTable([0, n], [0], dev)
    stream = L.current_stream_ptr()

    def inf_check():
        L.check(lib.bvc_op_nonfinite_check(x.data_ptr(), n, found.data_ptr(), stream), "bvc_op_nonfinite_check")

    passes = {"nonfinite_check": inf_check,
              "sqnorm_per_parameter": lambda: per_param.launch(lib, x.data_ptr(), total.data_ptr(), found.data_ptr(), stream),
              "sqnorm_one_segment": lambda: whole.launch(lib, x.data_ptr(), total.data_ptr(), found.data_ptr(), stream)}
    for fn in passes.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in passes}
    for _ in range(args.rounds):
        for k, fn in passes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            b.synchronize()
            us[k].append(round(1e3 * a.elapsed_time(b) / args.iters, 2))
    ref = float(x.double().square().sum())
    print(json.dumps({"metric": "gradient-norm pass against the inf check, one read of the flat gradient buffer", "arch": args.arch,
                      "elements": n, "mbytes": round(4 * n / 1e6, 1), "segments": per_param.nseg, "items": per_param.nitems,
                      "us_per_call": us, "tb_per_s_best": {k: round(4 * n / min(v) / 1e6, 2) for k, v in us.items()},
                      "found_inf": float(found), "sq_rel_err": abs(float(total) - ref) / ref}), flush=True)


if __name__ == "__main__":
    main()
