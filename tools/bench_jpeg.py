"""bvc.jpeg.decode on one MI355X at the loaders' frame sizes:

    python tools/bench_jpeg.py [--sizes 224x224,320x240,640x480] [--batches 256,4096] [--split N|auto] [--chunk 32,64,...]
                               [--step-ms MS] [--out FILE]

Frames are synthetic (a gradient, a low-frequency pattern and mild noise), encoded on the spot at 4:2:0 and quality 90 where PIL
imports - 16 distinct frames per size, tiled to the batch; elsewhere the tiny fixture files of tests/golden/jpeg_decode.json are tiled
and the sizes are ignored.  Every line says which.  Each size runs without a restart interval and with one restart per MCU row.

Per configuration one JSON line:
  stage1_ms / stage2_ms   HIP events around the entropy + IDCT kernel and the upsample + colour kernel alone (medians of 10 calls after
                          3 warm-ups), and the frames/s of each;
  decode_ms               both kernels, events;
  e2e_ms                  a host clock around bvc.jpeg.decode(infos=...) ending in a synchronise: staging into pinned memory, the one
                          copy, both kernels (the parse is timed apart as parse_us_per_frame, one host thread);
  staging_ms              of that, the host's part: descriptors, segments and bytes into the pinned buffer (a JpegClipRing does this
                          in stage(), under the step before);
  split / chunk           --split, --chunk: segments of at least `split` bytes go through the split path (bvc.jpeg.decode(split=,
                          chunk=)), one line per chunk size of the list; split_segments = how many did, rounds_max / fallbacks = the
                          most hand-over rounds of a segment and the segments that fell back (stage1_ms is then everything in front
                          of the colour kernel: routing, both entropy paths, the IDCT kernel and the fall-back launch);
  compressed / decoded MB/s over e2e_ms; lanes = the segments per wave the call chose;
  pil_fps_16_threads      PIL decode of the same files on 16 host threads of the same machine (where PIL imports);
  step_ms                 --step-ms: the time of a 256-clip VideoMAE step from a plain `python bench.py` run, for scale, and whether 4096
                          frames (= 256 clips) decode under one step."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge   # noqa: E402

WARMUP, CALLS, DISTINCT = 3, 10, 16


def _frames(W, H, restart):
    import io
    from PIL import Image
    out = []
    for seed in range(DISTINCT):
        g = np.random.default_rng(seed)
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        a = np.stack([x * 255 / W, y * 255 / H, (x + y) * 255 / (W + H)], -1)
        a += 40 * np.sin(x / (7 + seed))[..., None] * np.cos(y / (11 + seed))[..., None] + g.normal(0, 8, a.shape)
        bio = io.BytesIO()
        kw = dict(restart_marker_rows=1) if restart else {}
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(bio, "JPEG", quality=90, subsampling=2, **kw)
        out.append(bio.getvalue())
    return out


def _events(fn):
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
    return statistics.median(ms)


def _pil_fps(files):
    import io
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image

    def one(f):
        return Image.open(io.BytesIO(f)).convert("RGB").size
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(one, files[:64]))
        t = time.perf_counter()
        list(ex.map(one, files))
        return len(files) / (time.perf_counter() - t)


def run(J, dev, files, source, size, restart, step_ms, have_pil, split=0, chunk=0):
    t = time.perf_counter()
    infos = [J.parse(f) for f in files]
    parse_us = 1e6 * (time.perf_counter() - t) / len(files)
    n = len(files)
    nseg, nbytes = J._sizes(infos)
    decoded = sum(3 * i.width * i.height for i in infos)
    # the two kernels, alone and together, on buffers staged once
    offs, at = [], 0
    for i in infos:
        offs.append(at)
        at += 3 * i.width * i.height
    pack = J._Pack(n, nseg, nbytes)
    host_t = torch.empty(pack.total, dtype=torch.uint8, pin_memory=True)
    t = time.perf_counter()
    ws = J._fill(pack, host_t.numpy(), infos, offs, split)
    staging_ms = 1e3 * (time.perf_counter() - t)
    d = host_t.to(dev)
    out = torch.empty(at, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    work = torch.empty(ws, dtype=torch.uint8, device=dev)
    extra = torch.zeros(n, 2, dtype=torch.int32, device=dev)
    ms = {k: _events(lambda s=s: J._launch(pack, host_t.numpy(), d, out, at, status, work, 0, s, split=split, chunk=chunk, extra=extra))
          for k, s in (("stage1_ms", 1), ("stage2_ms", 2), ("decode_ms", 3))}
    assert not bool(status.any())
    split_segments = sum(J.is_split(int(e - b), split) for i in infos for b, e in i.segments[:, :2]) if split else 0

    def e2e():
        J.decode(None, dev, infos=infos, split=split, chunk=chunk)
        torch.cuda.synchronize()
    for _ in range(2):
        e2e()
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        e2e()
        ts.append(1e3 * (time.perf_counter() - t))
    e2e_ms = statistics.median(ts)
    want = (nseg + 2047) // 2048
    line = dict(bench="jpeg_decode", source=source, size=size, restart="mcu_row" if restart else "none", frames=n, segments=nseg,
                lanes=max(1, min(64, want)), split=split, chunk=chunk, split_segments=split_segments,
                rounds_max=int(extra[:, 1].max()), fallbacks=int(extra[:, 0].sum()), bytes_per_frame=round(nbytes / n), parse_us_per_frame=round(parse_us, 1), staging_ms=round(staging_ms, 3),
                **{k: round(v, 3) for k, v in ms.items()}, stage1_fps=round(1e3 * n / ms["stage1_ms"]), stage2_fps=round(1e3 * n / ms["stage2_ms"]),
                decode_fps=round(1e3 * n / ms["decode_ms"]), e2e_ms=round(e2e_ms, 3), e2e_fps=round(1e3 * n / e2e_ms),
                compressed_MBps=round(nbytes / e2e_ms / 1e3, 1), decoded_MBps=round(decoded / e2e_ms / 1e3, 1),
                pil_fps_16_threads=round(_pil_fps(files)) if have_pil else None, step_ms=step_ms)
    if step_ms and n == 4096:
        line["fits_under_step"] = dict(kernels=ms["decode_ms"] < step_ms, end_to_end=e2e_ms < step_ms)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="224x224,320x240,640x480")
    ap.add_argument("--batches", default="256,4096")
    ap.add_argument("--split", default="0", help='bytes from which a segment takes the split path, or "auto"; 0 = the one-lane path alone')
    ap.add_argument("--chunk", default="0", help="bytes per lane of the split path; a comma-separated list runs each")
    ap.add_argument("--step-ms", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ge.build()
    J = ge.load_package().jpeg
    dev = torch.device("cuda:0")
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    configs = []
    if have_pil:
        for size in args.sizes.split(","):
            W, H = (int(v) for v in size.split("x"))
            for restart in (False, True):
                configs.append(("synthetic, encoded here (PIL)", size, restart, _frames(W, H, restart)))
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import jpeg_ref
        configs.append(("tiled fixture files (no PIL here)", "mixed", None, [c["jpeg"] for c in jpeg_ref.decode_cases()]))
    split = J._split_bytes(args.split if args.split == "auto" else int(args.split))
    chunks = [int(v) for v in args.chunk.split(",")] if split else [0]
    lines = []
    for source, size, restart, distinct in configs:
        for b in (int(v) for v in args.batches.split(",")):
            files = [distinct[i % len(distinct)] for i in range(b)]
            for chunk in chunks:
                line = run(J, dev, files, source, size, restart, args.step_ms, have_pil and chunk == chunks[0], split, chunk)
                print(json.dumps(line), flush=True)
                lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
