"""Embedding-extraction throughput (clips/s) on one MI355X: a VideoMAE encoder (--arch, default base) on all 1568 tokens of
16x224^2 clips, mean-pool + fc_norm (the path benchmarks/compute_embeddings_videomae.py runs between curriculum stages).  Synthetic
clips.  --hidden-states / --attentions request the per-layer outputs; --probs times bvc.attention_probs alone at the encoder's
shape against the same quantity composed in torch (softmax(q @ k^T * scale) in f32) on the same qkv.  One JSON line per batch."""
import argparse, json, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--arch", default="base")
ap.add_argument("--batch", default="16", help="clips per call; a comma-separated list runs each in turn")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--hidden-states", action="store_true", help="output_hidden_states=True")
ap.add_argument("--attentions", action="store_true", help="output_attentions=True")
ap.add_argument("--probs", action="store_true", help="time the attention-probabilities kernel alone against torch's composition")
args = ap.parse_args()
ge.build()
bvc = ge.load_package()
dev = torch.device("cuda:0")
torch.manual_seed(0)
cfg = bvc.videomae_config(args.arch, num_labels=0)
N, D, H, nl = cfg.seq_length, cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers


def timed(fn, warmup, steps):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, out


def bench_probs(B):
    """One layer's probabilities for B clips: N^2 * 4 bytes of stores per head, once for the kernel; torch's composition writes the
    scores, reads them, and writes the softmax."""
    hd = D // H
    g = torch.Generator(device=dev).manual_seed(1)
    qkv = torch.randn(B * N, 3 * D, device=dev, generator=g).to(torch.bfloat16)
    ctx = torch.empty(B * N, D, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B * H, N, device=dev, dtype=torch.float32)
    L = bvc._lib
    L.check(L.lib().bvc_op_attention_fwd(qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), B, N, H, hd, L.current_stream_ptr()), "attention_fwd")
    probs = torch.empty((B, H, N, N), dtype=torch.float32, device=dev)

    def ours():
        L.check(L.lib().bvc_op_attention_probs(qkv.data_ptr(), lse.data_ptr(), probs.data_ptr(), B, N, H, hd, 0.0, L.current_stream_ptr()),
                "attention_probs")
        return probs

    def composed():
        x = qkv.view(B, N, 3, H, hd).permute(2, 0, 3, 1, 4).float()
        return torch.softmax((x[0] @ x[1].transpose(-1, -2)) * hd ** -0.5, dim=-1)

    t_ours, a = timed(ours, args.warmup, args.steps)
    a = a.clone()
    t_torch, b = timed(composed, args.warmup, args.steps)
    nbytes = B * H * N * N * 4
    print(json.dumps({"metric": "attention probabilities, one layer (f32 [B][H][N][N])", "arch": args.arch, "batch": B, "N": N, "heads": H,
                      "head_dim": hd, "bytes": nbytes, "ms": round(1e3 * t_ours, 4), "store_GBps": round(nbytes / t_ours / 1e9, 1),
                      "torch_ms": round(1e3 * t_torch, 4), "torch_over_ours": round(t_torch / t_ours, 2),
                      "max_abs_diff": float((a - b).abs().max())}), flush=True)


m = None if args.probs else bvc.VideoMAEForVideoClassification(cfg).to(dev).eval()
for B in [int(b) for b in str(args.batch).split(",")]:
    if args.probs:
        bench_probs(B)
        continue
    g = torch.Generator().manual_seed(1)
    clips = ((torch.randint(0, 256, (B, 16, 3, 224, 224), generator=g, dtype=torch.uint8).float() / 255 - 0.5) / 0.25).to(dev)
    kw = {}
    if args.hidden_states:
        kw["output_hidden_states"] = True
    if args.attentions:
        kw["output_attentions"] = True
    dt, out = timed(lambda: m(pixel_values=clips, **kw), args.warmup, args.steps)
    # encoder forward on all tokens: patch embed N x 1536 x D + layers x (24 N D^2 + 4 N^2 D)
    gflop = (2 * N * 1536 * D + nl * (24 * N * D ** 2 + 4 * N ** 2 * D)) / 1e9
    line = {"metric": f"embedding clips/s (VideoMAE-{args.arch} encoder, all {N} tokens, bf16)", "value": round(B / dt, 1),
            "batch": B, "ms_per_batch": round(1e3 * dt, 3), "gflop_per_clip": round(gflop, 2),
            "tflops": round(gflop * B / dt / 1e3, 1), "finite": bool(torch.isfinite(out.logits).all()),
            "hidden_states": bool(args.hidden_states), "attentions": bool(args.attentions)}
    if args.attentions:
        line["attentions_bytes"] = bvc.videomae.attentions_nbytes(cfg, B)
        line["rowsum_err"] = float((out.attentions[-1].sum(-1) - 1).abs().max())
    if args.hidden_states:
        line["hidden_states_bytes"] = bvc.videomae.hidden_states_nbytes(cfg, B)
    print(json.dumps(line), flush=True)
    del clips, out
