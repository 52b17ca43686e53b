"""Feature-correlation losses on the GPU: the fused op (csrc/xcorr.hip) against the dense torch-f32 form, time and memory.

    python tools/bench_xcorr.py [--shapes 128x2048,512x2048,2048x2048,512x8192,2048x8192] [--out FILE]

One JSON line per shape n x p (two views of p features, Barlow Twins parameters), medians of 10 calls after 3 warm-ups:
  op_fwd_ms, op_bwd_ms   bvc_op_xcorr_fwd / _bwd through the C ABI, with their TFLOP/s (2 n p^2 forward; the backward runs four such
                         products: G and dxh for either operand) and the share of the 157.3 TFLOP/s f32 matrix peak
  fused_ms, torch_ms     barlow_twins_loss forward + backward through autograd, ours and the dense torch-f32 form
  *_peak_MB              torch's peak allocated memory of one forward (fwd) and of one forward + backward (step) beyond the inputs
  workspace_fwd_MB       bvc_op_xcorr_workspace(.., backward=0): what the forward allocates beyond its inputs and outputs
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402

PEAK_TFLOPS = 157.3
WARMUP, CALLS = 3, 10
LAMBD, EPS = 5e-3, 1e-5
MB = 2.0 ** 20


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


def _peak(fn):
    """peak allocated bytes of fn() beyond what is allocated on entry, in MB"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / MB, 1)


def torch_barlow(z1, z2):
    n = z1.shape[0]
    a = (z1 - z1.mean(0)) / torch.sqrt(z1.var(0, unbiased=False) + EPS)
    b = (z2 - z2.mean(0)) / torch.sqrt(z2.var(0, unbiased=False) + EPS)
    c = a.t() @ b / n
    on = torch.diagonal(c).add(-1).pow(2).sum()
    off = c.pow(2).sum() - torch.diagonal(c).pow(2).sum()
    return on + LAMBD * off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x2048,512x2048,2048x2048,512x8192,2048x8192")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_xcorr: no GPU (there is nothing to measure without one)")
    ge.build()
    bvc = ge.load_package()
    L, lib, S = bvc._lib, bvc._lib.lib(), bvc.simclr
    out = open(args.out, "a") if args.out else None
    for shape in args.shapes.split(","):
        n, p = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device="cuda").manual_seed(1234)
        z1 = torch.randn(n, p, device="cuda", generator=gen)
        z2 = z1 + 0.5 * torch.randn(n, p, device="cuda", generator=gen)
        mx, vx, my, vy = (torch.empty(p, device="cuda") for _ in range(4))
        stats = torch.empty(2, device="cuda")
        w = torch.tensor([1.0, LAMBD], device="cuda")
        dx, dy = torch.empty(n, p, device="cuda"), torch.empty(n, p, device="cuda")
        nf, nb = lib.bvc_op_xcorr_workspace(n, p, p, 0, 0, 0), lib.bvc_op_xcorr_workspace(n, p, p, 0, 0, 1)
        ws = torch.empty(max(nf, nb) // 4, device="cuda")
        st = L.current_stream_ptr()
        cfg = (n, p, p, 1, 0, EPS, 1.0 / n, 1.0)

        def op_fwd():
            L.check(lib.bvc_op_xcorr_fwd(z1.data_ptr(), p, z2.data_ptr(), p, *cfg, mx.data_ptr(), vx.data_ptr(), my.data_ptr(), vy.data_ptr(),
                                         stats.data_ptr(), ws.data_ptr(), st), "fwd")

        def op_bwd():
            L.check(lib.bvc_op_xcorr_bwd(z1.data_ptr(), p, z2.data_ptr(), p, *cfg, mx.data_ptr(), vx.data_ptr(), my.data_ptr(), vy.data_ptr(),
                                         w.data_ptr(), None, None, 0, dx.data_ptr(), p, dy.data_ptr(), p, ws.data_ptr(), st), "bwd")

        rec = {"shape": shape, "n": n, "p": p, "block_cols": lib.bvc_op_xcorr_block_cols(n, p, p), "workspace_fwd_MB": round(nf / MB, 1),
               "workspace_bwd_MB": round(nb / MB, 1), "dense_c_MB": round(p * p * 4 / MB, 1)}
        rec["op_fwd_ms"] = _time(op_fwd)
        rec["op_bwd_ms"] = _time(op_bwd)
        gflop = 2.0 * n * p * p / 1e9
        rec["op_fwd_tflops"] = round(gflop / rec["op_fwd_ms"], 1)
        rec["op_bwd_tflops"] = round(4 * gflop / rec["op_bwd_ms"], 1)
        rec["op_fwd_share_of_peak"] = round(rec["op_fwd_tflops"] / PEAK_TFLOPS, 3)
        rec["op_bwd_share_of_peak"] = round(rec["op_bwd_tflops"] / PEAK_TFLOPS, 3)
        del ws, dx, dy

        a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)

        def step(loss_fn):
            a.grad = b.grad = None
            loss = loss_fn(a, b)
            loss.backward()
            return loss

        def fwd_only(loss_fn):
            with torch.no_grad():
                return loss_fn(a, b)

        fused = lambda u, v: S.barlow_twins_loss(u, v, LAMBD, EPS)      # noqa: E731
        rec["fused_ms"] = _time(lambda: step(fused))
        lf, gf = float(step(fused)), a.grad.clone()
        rec["torch_ms"] = _time(lambda: step(torch_barlow))
        lt, gt = float(step(torch_barlow)), a.grad.clone()
        rec["torch_over_fused"] = round(rec["torch_ms"] / rec["fused_ms"], 2)
        rec["rel_diff_loss"] = abs(lf - lt) / abs(lt)
        rec["max_rel_diff_grad"] = float((gf - gt).abs().max() / gt.abs().max())
        del gf, gt
        a.grad = b.grad = None
        rec["fused_fwd_peak_MB"] = _peak(lambda: fwd_only(fused))
        rec["torch_fwd_peak_MB"] = _peak(lambda: fwd_only(torch_barlow))
        rec["fused_step_peak_MB"] = _peak(lambda: step(fused))
        a.grad = b.grad = None
        rec["torch_step_peak_MB"] = _peak(lambda: step(torch_barlow))
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del z1, z2, a, b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
