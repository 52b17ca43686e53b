"""bvc.retrieval.topk against torch on one MI355X, at the sizes of the reference's evaluation (SSv2 embeddings) and of a kNN monitor:

    python tools/bench_retrieval.py [--shapes ssv2,monitor,ssv2-d384,ssv2-d1280] [--data clusters|gauss] [--out FILE]
                                    [--ablation-lib PATH]

Per shape one JSON line: ms per call (HIP events around each of 10 calls after 3 warm-ups; median, min and max), TFLOP/s counted as
2 Q N D, that rate as a share of the 157.3 TFLOP/s f32 matrix peak, the same job done by torch on the same GPU (normalised rows,
`torch.topk` over f32 `q @ k.T` in query chunks of 1 GiB of scores - what a user has without this op and without the host round
trip), and the share of the neighbour sets on which the two agree.  Embeddings: `clusters` = 174 Gaussian class centres with unit
noise (the real case: the survivors of the selection fall off more slowly than on unclustered data), `gauss` = unit normal.

The selection's share of the time comes from one more run with a threshold that accepts nothing.  That switch is not in the
product: it is `bvc_exp_topk_no_select`, which only an experiments build (BVC_EXTRA_HIPCC_FLAGS=-DBVC_EXPERIMENTS) of the library
exports; pass such a build as --ablation-lib (`tools/build_variant.sh exp baby-vision-curriculum_amd/csrc/retrieval.hip
-DBVC_EXPERIMENTS` writes libbvc_hip_exp.so next to the product library).  Without it the share is reported as null (not measured)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402

SHAPES = {"ssv2": (24777, 168913, 768, 50), "monitor": (2048, 16384, 768, 20), "ssv2-d384": (24777, 168913, 384, 50),
          "ssv2-d1280": (24777, 168913, 1280, 50)}
PEAK_TF = 157.3
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


def _embeddings(rows, D, kind, gen, centres):
    x = torch.randn(rows, D, device="cuda", generator=gen)
    if kind == "clusters":
        x += centres[torch.randint(0, centres.shape[0], (rows,), device="cuda", generator=gen)]
    return x


def _torch_topk(q, keys, k):
    qn = torch.nn.functional.normalize(q, dim=1)
    kn = torch.nn.functional.normalize(keys, dim=1)
    rows = max(1, (1 << 30) // (4 * keys.shape[0]))
    vals, idxs = [], []
    for i in range(0, q.shape[0], rows):
        v, j = torch.topk(qn[i:i + rows] @ kn.t(), k, dim=1)
        vals.append(v)
        idxs.append(j)
    return 1.0 - torch.cat(vals), torch.cat(idxs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ssv2,monitor,ssv2-d384,ssv2-d1280")
    ap.add_argument("--data", default="clusters", choices=["clusters", "gauss"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--ablation-lib", default=None)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_retrieval: no GPU (there is nothing to measure without one)")
    ge.build()
    bvc = ge.load_package()
    L, lib = bvc._lib, bvc._lib.lib()
    exp = None
    if args.ablation_lib:
        exp = ctypes.CDLL(args.ablation_lib).bvc_exp_topk_no_select
        exp.restype = ctypes.c_int
        exp.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 4
    out = open(args.out, "a") if args.out else None
    for name in args.shapes.split(","):
        Q, N, D, k = SHAPES[name]
        gen = torch.Generator(device="cuda").manual_seed(1234)
        centres = torch.randn(174, D, device="cuda", generator=gen)
        q, keys = _embeddings(Q, D, args.data, gen, centres), _embeddings(N, D, args.data, gen, centres)
        dist = torch.empty(Q, k, device="cuda")
        idx = torch.empty(Q, k, dtype=torch.int32, device="cuda")
        ws = torch.empty((lib.bvc_op_topk_workspace(Q, N, D, k, 0) + 7) // 8, dtype=torch.int64, device="cuda")
        a = (q.data_ptr(), D, keys.data_ptr(), D, Q, N, D, k, 0, 0)

        def ours():
            L.check(lib.bvc_op_topk(*a, 0, 0, idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), L.current_stream_ptr()), "bvc_op_topk")

        ms = _time(ours)
        got_idx = idx.clone()
        flop = 2.0 * Q * N * D
        med = statistics.median(ms)
        rec = {"shape": name, "Q": Q, "N": N, "D": D, "k": k, "data": args.data, "key_splits": lib.bvc_op_topk_splits(Q, N, D, k),
               "ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "tflops": round(flop / med / 1e9, 1),
               "share_of_f32_matrix_peak": round(flop / med / 1e9 / PEAK_TF, 3), "selection_share": None, "ms_no_select": None}
        if exp is not None:
            d2, i2 = torch.empty_like(dist), torch.empty_like(idx)

            def bare():
                rc = exp(*a, i2.data_ptr(), d2.data_ptr(), ws.data_ptr(), L.current_stream_ptr())
                assert rc == 0, rc

            mb = statistics.median(_time(bare))
            assert bool((i2 == -1).all()), "the ablation accepted something"
            rec["ms_no_select"] = round(mb, 3)
            rec["selection_share"] = round(1.0 - mb / med, 3)
        if not args.no_torch:
            mt = _time(lambda: _torch_topk(q, keys, k))
            _, ti = _torch_topk(q, keys, k)
            same = (torch.sort(ti, dim=1).values == torch.sort(got_idx.long(), dim=1).values).all(dim=1).float().mean()
            rec.update(torch_ms=round(statistics.median(mt), 3), torch_over_ours=round(statistics.median(mt) / med, 2),
                       rows_with_the_same_neighbour_set=round(float(same), 4))
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del q, keys, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
