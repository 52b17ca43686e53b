"""bvc.simclr.nt_xent_loss against the same loss composed in torch f32, on one MI355X:

    python tools/bench_ntxent.py [--shapes 512x128,2048x768,8192x768,8192x2048] [--out FILE]

Per shape one JSON line (ms: HIP events around each of 10 calls after 3 warm-ups, median):
  op_fwd_ms, op_bwd_ms   bvc_op_ntxent_fwd / _bwd through the C ABI, with their TFLOP/s (2 n^2 p forward, 4 n^2 p backward) and the share
                         of the 157.3 TFLOP/s f32 matrix peak;
  fused_ms               nt_xent_loss forward + backward through autograd (two view-major views, T = 0.1);
  torch_ms               the same loss in torch f32: F.normalize, mm, diagonal-masked logsumexp, autograd - what a user has without
                         the op; max_abs_diff of the two losses and the largest gradient difference relative to the largest gradient;
  info_nce_ms            for orientation only: bvc.simclr.info_nce_loss forward + backward at the same shape (another loss - one
                         logsumexp over the whole matrix, tridiagonal positives - on bf16 operands)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402

PEAK_TFLOPS = 157.3
WARMUP, CALLS = 3, 10
T = 0.1


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
    return round(statistics.median(ms), 4)


def torch_nt_xent(f, eye, target):
    zn = F.normalize(f, dim=1, eps=1e-8)
    s = (zn @ zn.t() / T).masked_fill(eye, float("-inf"))
    return (torch.logsumexp(s, dim=1) - s.gather(1, target[:, None])[:, 0]).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x128,2048x768,8192x768,8192x2048")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ntxent: no GPU (there is nothing to measure without one)")
    ge.build()
    bvc = ge.load_package()
    L, lib, S = bvc._lib, bvc._lib.lib(), bvc.simclr
    out = open(args.out, "a") if args.out else None
    for shape in args.shapes.split(","):
        n, p = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device="cuda").manual_seed(1234)
        f = torch.randn(n, p, device="cuda", generator=gen)
        row_loss, lse, stats = torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(2, device="cuda")
        npos = torch.empty(n, dtype=torch.int32, device="cuda")
        w = torch.full((n,), 1.0 / n, device="cuda")
        df = torch.empty(n, p, device="cuda")
        ws = torch.empty(lib.bvc_op_ntxent_workspace(n, p, 0, 0) // 4, device="cuda")
        st = L.current_stream_ptr()

        def op_fwd():
            L.check(lib.bvc_op_ntxent_fwd(f.data_ptr(), p, None, 2, n, p, T, 1e-8, 0, row_loss.data_ptr(), lse.data_ptr(), npos.data_ptr(),
                                          stats.data_ptr(), ws.data_ptr(), st), "fwd")

        def op_bwd():
            L.check(lib.bvc_op_ntxent_bwd(f.data_ptr(), p, None, 2, n, p, T, 1e-8, lse.data_ptr(), npos.data_ptr(), w.data_ptr(), 0, 0,
                                          df.data_ptr(), p, ws.data_ptr(), st), "bwd")

        rec = {"shape": shape, "n": n, "p": p, "T": T, "splits": lib.bvc_op_ntxent_splits(n, p), "block_rows": lib.bvc_op_ntxent_block_rows(n, p),
               "workspace_MB": round(ws.numel() * 4 / 2 ** 20, 1)}
        rec["op_fwd_ms"] = _time(op_fwd)
        rec["op_bwd_ms"] = _time(op_bwd)
        gflop = 2.0 * n * n * p / 1e9
        rec["op_fwd_tflops"] = round(gflop / rec["op_fwd_ms"], 1)
        rec["op_bwd_tflops"] = round(2 * gflop / rec["op_bwd_ms"], 1)
        rec["op_fwd_share_of_peak"] = round(rec["op_fwd_tflops"] / PEAK_TFLOPS, 3)
        rec["op_bwd_share_of_peak"] = round(rec["op_bwd_tflops"] / PEAK_TFLOPS, 3)
        del ws

        x = f.clone().requires_grad_(True)
        eye = torch.eye(n, dtype=torch.bool, device="cuda")
        target = (torch.arange(n, device="cuda") + n // 2) % n

        def step(loss_fn):
            x.grad = None
            loss = loss_fn(x)
            loss.backward()
            return loss

        rec["fused_ms"] = _time(lambda: step(lambda t: S.nt_xent_loss(t, T)))
        lf, gf = float(step(lambda t: S.nt_xent_loss(t, T))), x.grad.clone()
        rec["torch_ms"] = _time(lambda: step(lambda t: torch_nt_xent(t, eye, target)))
        lt, gt = float(step(lambda t: torch_nt_xent(t, eye, target))), x.grad.clone()
        rec["fused_tflops"] = round(3 * gflop / rec["fused_ms"], 1)
        rec["fused_share_of_peak"] = round(rec["fused_tflops"] / PEAK_TFLOPS, 3)
        rec["torch_over_fused"] = round(rec["torch_ms"] / rec["fused_ms"], 2)
        rec["max_abs_diff_loss"] = abs(lf - lt)
        rec["max_rel_diff_grad"] = float((gf - gt).abs().max() / gt.abs().max())
        del eye, target, gf, gt
        if n % 8 == 0 and p % 64 == 0:
            masks = S.make_masks(n // 2, "cuda")
            rec["info_nce_ms"] = _time(lambda: step(lambda t: S.info_nce_loss(T, masks, t)))
            del masks
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del f, x, df
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
