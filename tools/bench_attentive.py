"""bvc.attentive against the same pooler written unfused in torch, on one MI355X, at the encoder shapes 1568 x 768 and 1568 x 1280:

    python tools/bench_attentive.py [--shapes vitb,vith] [--batch 256] [--out FILE]

Per shape one JSON line (ms: HIP events around each of 10 calls after 3 warm-ups, median):
  op_*        bvc_op_attn_pool_fwd, _bwd without dx (the frozen encoder) and _bwd with dx through the C ABI, with the bytes each must move
              (x once; dx once more) at the measured 6.29 TB/s float4 copy rate, and the share of that floor reached;
  fused_*     AttentivePooler.forward, forward + backward to the parameters, and forward + backward with x.requires_grad;
  unfused_*   the same parameters through LayerNorm, a bf16 kv linear over all tokens and scaled_dot_product_attention with one query
              per clip - what a user has without the op;
  max_abs_diff  of the two poolers' outputs (the unfused one rounds K and V to bf16)."""
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

SHAPES = {"vitb": (1568, 768, 12), "vith": (1568, 1280, 16)}
COPY_TBS = 6.29
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
    return round(statistics.median(ms), 4)


def unfused(pooler, x):
    blk, D, H = pooler.cross_attention_block, pooler.embed_dim, pooler.num_heads
    B, N, d = x.shape[0], x.shape[1], D // H
    t = pooler.query_tokens[0, 0]
    xn = F.layer_norm(x, (D,), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps).to(torch.bfloat16)
    kv = F.linear(xn, blk.xattn.kv.weight.to(torch.bfloat16), blk.xattn.kv.bias.to(torch.bfloat16)).view(B, N, 2, H, d)
    k, v = kv[:, :, 0].transpose(1, 2), kv[:, :, 1].transpose(1, 2)
    q = blk.xattn.q(t).to(torch.bfloat16).view(1, H, 1, d).expand(B, H, 1, d)
    o = F.scaled_dot_product_attention(q, k, v).float().reshape(B, D)
    q = t + blk.xattn.proj(o)
    return q + blk.mlp(blk.norm2(q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="vitb,vith")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attentive: no GPU (there is nothing to measure without one)")
    ge.build()
    bvc = ge.load_package()
    L, lib = bvc._lib, bvc._lib.lib()
    out = open(args.out, "a") if args.out else None
    for name in args.shapes.split(","):
        N, D, H = SHAPES[name]
        B = args.batch
        gen = torch.Generator(device="cuda").manual_seed(1234)
        x = torch.randn(B, N, D, device="cuda", generator=gen)
        torch.manual_seed(0)
        pooler = bvc.AttentivePooler(D, H, init_std=0.2).cuda()
        params = list(pooler.parameters())
        u = pooler.folded_queries()[0].detach().contiguous()
        pooled, lse = torch.empty(B, H, D, device="cuda"), torch.empty(B, H, device="cuda")
        dpooled, du, dx = torch.randn(B, H, D, device="cuda", generator=gen), torch.empty(H, D, device="cuda"), torch.empty_like(x)
        ws = torch.empty(lib.bvc_op_attn_pool_workspace(B, N, D, H, 0) // 4, device="cuda")
        st = L.current_stream_ptr()

        def op_fwd():
            L.check(lib.bvc_op_attn_pool_fwd(x.data_ptr(), D, u.data_ptr(), B, N, D, H, 1e-5, 0, pooled.data_ptr(), lse.data_ptr(), ws.data_ptr(), st), "fwd")

        def op_bwd(dxp):
            L.check(lib.bvc_op_attn_pool_bwd(x.data_ptr(), D, u.data_ptr(), pooled.data_ptr(), lse.data_ptr(), dpooled.data_ptr(), B, N, D, H,
                                             1e-5, 0, du.data_ptr(), dxp, D, ws.data_ptr(), st), "bwd")

        xbytes = B * N * D * 4
        floor = xbytes / (COPY_TBS * 1e9)       # ms
        rec = {"shape": name, "B": B, "N": N, "D": D, "H": H, "splits": lib.bvc_op_attn_pool_splits(B, N, D, H), "x_GB": round(xbytes / 1e9, 3),
               "copy_floor_ms": round(floor, 4)}
        rec["op_fwd_ms"] = _time(op_fwd)
        rec["op_bwd_ms"] = _time(lambda: op_bwd(None))
        rec["op_bwd_dx_ms"] = _time(lambda: op_bwd(dx.data_ptr()))
        rec["op_fwd_share_of_floor"] = round(floor / rec["op_fwd_ms"], 3)
        rec["op_bwd_share_of_floor"] = round(floor / rec["op_bwd_ms"], 3)
        rec["op_bwd_dx_share_of_floor"] = round(2 * floor / rec["op_bwd_dx_ms"], 3)

        def step(fn, xin):
            for p in params:
                p.grad = None
            xin.grad = None
            fn(pooler, xin).square().mean().backward()

        xg = x.clone().requires_grad_(True)
        for tag, fn in (("fused", lambda m, t: m(t)), ("unfused", unfused)):
            with torch.no_grad():
                rec[tag + "_fwd_ms"] = _time(lambda: fn(pooler, x))
            rec[tag + "_fwd_bwd_ms"] = _time(lambda: step(fn, x))
            rec[tag + "_fwd_bwd_dx_ms"] = _time(lambda: step(fn, xg))
        with torch.no_grad():
            rec["max_abs_diff"] = float((pooler(x) - unfused(pooler, x)).abs().max())
        rec["unfused_over_fused_fwd"] = round(rec["unfused_fwd_ms"] / rec["fused_fwd_ms"], 2)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del x, xg, dx, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
