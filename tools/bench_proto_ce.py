"""bvc.dino.prototype_ce against the same loss composed in torch f32, on one MI355X:

    python tools/bench_proto_ce.py [--shapes 32x65536x256,256x65536x256,1024x65536x256,1024x8192x256] [--out FILE]

Per shape m x K x p one JSON line (ms: HIP events around each of 10 calls after 3 warm-ups, median):
  op_fwd_ms, op_bwd_ms   bvc_op_proto_ce_fwd / _bwd through the C ABI, with their TFLOP/s (4 m K p forward: two products; 8 m K p
                         backward: the dS recompute and two products) and the share of the 157.3 TFLOP/s f32 matrix peak;
  fused_ms               prototype_ce forward + backward through autograd (tau_s 0.1, tau_t 0.04, a centre);
  torch_ms               the same loss in torch f32: F.normalize, mm, softmax / log_softmax, autograd - what a user has without the
                         op; the difference of the two losses and the largest gradient differences relative to the largest gradient;
  workspace_MB, fwd_workspace_MB, outputs_MB, fused_peak_MB, torch_peak_MB
                         the op's workspace (both directions / the forward alone) and outputs, and the peak allocated memory
                         (above the inputs) of one forward + backward of either path."""
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
TAU_S, TAU_T, EPS = 0.1, 0.04, 1e-12


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


def torch_proto_ce(xs, vs, xt, vt, center):
    s = F.normalize(xs, dim=1, eps=EPS) @ F.normalize(vs, dim=1, eps=EPS).t() / TAU_S
    with torch.no_grad():
        q = F.softmax((F.normalize(xt, dim=1, eps=EPS) @ F.normalize(vt, dim=1, eps=EPS).t() - center) / TAU_T, dim=-1)
    return torch.sum(-q * F.log_softmax(s, dim=-1), dim=-1).mean()


def _peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x65536x256,256x65536x256,1024x65536x256,1024x8192x256")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_proto_ce: no GPU (there is nothing to measure without one)")
    ge.build()
    bvc = ge.load_package()
    L, lib, D = bvc._lib, bvc._lib.lib(), bvc.dino
    out = open(args.out, "a") if args.out else None
    for shape in args.shapes.split(","):
        m, K, p = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device="cuda").manual_seed(1234)
        xs, vs = torch.randn(m, p, device="cuda", generator=gen), torch.randn(K, p, device="cuda", generator=gen)
        xt = xs + 0.5 * torch.randn(m, p, device="cuda", generator=gen)
        vt = vs + 0.1 * torch.randn(K, p, device="cuda", generator=gen)
        center = 0.1 * torch.randn(K, device="cuda", generator=gen)
        row_loss, lse_s, lse_t = (torch.empty(m, device="cuda") for _ in range(3))
        stats, bc = torch.empty(2, device="cuda"), torch.empty(K, device="cuda")
        w = torch.full((m,), 1.0 / m, device="cuda")
        dxs, dvs = torch.empty(m, p, device="cuda"), torch.empty(K, p, device="cuda")
        ws = torch.empty(lib.bvc_op_proto_ce_workspace(m, K, p, 0, 0) // 4, device="cuda")
        st = L.current_stream_ptr()

        def op_fwd():
            L.check(lib.bvc_op_proto_ce_fwd(xs.data_ptr(), p, vs.data_ptr(), p, xt.data_ptr(), p, vt.data_ptr(), p, center.data_ptr(), m, K, p,
                                            TAU_S, TAU_T, EPS, 0, row_loss.data_ptr(), lse_s.data_ptr(), lse_t.data_ptr(), stats.data_ptr(),
                                            bc.data_ptr(), ws.data_ptr(), st), "fwd")

        def op_bwd():
            L.check(lib.bvc_op_proto_ce_bwd(xs.data_ptr(), p, vs.data_ptr(), p, xt.data_ptr(), p, vt.data_ptr(), p, center.data_ptr(), m, K, p,
                                            TAU_S, TAU_T, EPS, lse_s.data_ptr(), lse_t.data_ptr(), w.data_ptr(), 0, 0, dxs.data_ptr(), p,
                                            dvs.data_ptr(), p, ws.data_ptr(), st), "bwd")

        outputs = row_loss.numel() * 3 + stats.numel() + bc.numel() + dxs.numel() + dvs.numel()
        rec = {"shape": shape, "m": m, "K": K, "p": p, "tau_s": TAU_S, "tau_t": TAU_T, "splits": lib.bvc_op_proto_ce_splits(m, K, p),
               "block": lib.bvc_op_proto_ce_block(m, K, p), "workspace_MB": round(ws.numel() * 4 / 2 ** 20, 1),
               "fwd_workspace_MB": round(lib.bvc_op_proto_ce_workspace(m, K, p, 0, 128) / 2 ** 20, 1),
               "outputs_MB": round(outputs * 4 / 2 ** 20, 1), "logits_MB": round(m * K * 4 / 2 ** 20, 1)}
        rec["op_fwd_ms"] = _time(op_fwd)
        rec["op_bwd_ms"] = _time(op_bwd)
        gflop = 4.0 * m * K * p / 1e9
        rec["op_fwd_tflops"] = round(gflop / rec["op_fwd_ms"], 1)
        rec["op_bwd_tflops"] = round(2 * gflop / rec["op_bwd_ms"], 1)
        rec["op_fwd_share_of_peak"] = round(rec["op_fwd_tflops"] / PEAK_TFLOPS, 3)
        rec["op_bwd_share_of_peak"] = round(rec["op_bwd_tflops"] / PEAK_TFLOPS, 3)
        del ws, dxs, dvs

        x, v = xs.clone().requires_grad_(True), vs.clone().requires_grad_(True)

        def step(loss_fn):
            x.grad, v.grad = None, None
            loss = loss_fn(x, v)
            loss.backward()
            return loss

        fused = lambda a, b: D.prototype_ce(a, b, xt, vt, center, TAU_S, TAU_T)      # noqa: E731
        plain = lambda a, b: torch_proto_ce(a, b, xt, vt, center)                      # noqa: E731
        rec["fused_ms"] = _time(lambda: step(fused))
        lf, gx, gv = float(step(fused)), x.grad.clone(), v.grad.clone()
        rec["fused_peak_MB"] = _peak_mb(lambda: step(fused))
        rec["torch_ms"] = _time(lambda: step(plain))
        lt = float(step(plain))
        rec["max_abs_diff_loss"] = abs(lf - lt)
        rec["max_rel_diff_dxs"] = float((gx - x.grad).abs().max() / x.grad.abs().max())
        rec["max_rel_diff_dvs"] = float((gv - v.grad).abs().max() / v.grad.abs().max())
        del gx, gv
        rec["torch_peak_MB"] = _peak_mb(lambda: step(plain))
        rec["fused_tflops"] = round(3 * gflop / rec["fused_ms"], 1)
        rec["fused_share_of_peak"] = round(rec["fused_tflops"] / PEAK_TFLOPS, 3)
        rec["torch_over_fused"] = round(rec["torch_ms"] / rec["fused_ms"], 2)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del xs, vs, xt, vt, x, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
