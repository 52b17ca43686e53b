"""JPEG frames to uint8 clips on the GPU (include/bvc.h "JPEG decode", csrc/jpeg.h, csrc/jpeg.hip).

The reference's loaders decode one ``.jpg`` per frame on the host (``torchvision.io.read_image`` / ``PIL.Image.open``,
pretraining/generative/homeview.py:255-281): 16 decodes per clip.  Here the dataset hands over the file's BYTES; ``parse`` (plain C++,
no device call: fit for loader workers) turns each into a fixed-size descriptor and a list of independent segments, and ``decode``
/ ``JpegClipRing`` upload the compressed bytes and decode on the device into the planar RGB uint8 frames that ``ClipTransform`` /
``ClipAugment`` take - the same bytes as ``PIL.Image.open(f).convert("RGB")``.

Baseline Huffman files only (8-bit, grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0, one scan); everything else is refused at parse with a
reason (``JpegUnsupported``) and is the caller's to decode on the host.  There is no host fallback in here.

A file without restart markers is one segment, and a segment is one lane's work - unless ``split`` is set: then long segments are cut
into chunks that the lanes of a workgroup decode together (``decode(split=, chunk=)``, ``JpegClipRing(split=, chunk=)``,
``decode_host_split``, ``split_chunks``; DESIGN.md "JPEG decode").  Same bytes, same status bits.
"""

import numpy as np
import torch

from . import _lib

HUFF = np.dtype([("look", "<u2", 256), ("maxcode", "<i4", 18), ("valoff", "<i4", 18), ("huffval", "u1", 256)])
INFO = np.dtype([("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("hs", "<i4"), ("vs", "<i4"), ("mcus_x", "<i4"), ("mcus_y", "<i4"),
                 ("restart_interval", "<i4"), ("scan_begin", "<i4"), ("scan_end", "<i4"), ("nseg", "<i4"), ("reason", "<i4"),
                 ("flags", "<i4"), ("seg_first", "<i4"), ("blob_offset", "<i8"), ("plane_offset", "<i8"), ("tq", "u1", 4), ("td", "u1", 4),
                 ("ta", "u1", 4), ("pad_", "<u4"), ("qt", "<u2", (4, 64)), ("huff", HUFF, 4)])      # bvc_jpeg_info
assert HUFF.itemsize == 912 and INFO.itemsize == 4248
SEG_INTS = 4      # a segment record: first byte, end byte, first MCU, MCU count

REASONS = {1: "not_jpeg", 2: "bad_length", 3: "progressive", 4: "arithmetic", 5: "lossless", 6: "precision", 7: "components", 8: "rgb",
           9: "sampling", 10: "multi_scan", 11: "huffman", 12: "quant", 13: "size", 14: "scan_header", 15: "restart", 16: "header"}
ST_TRUNCATED, ST_BAD_CODE, ST_BAD_RUN, ST_NO_EOI = 1, 2, 4, 8
# the split path (include/bvc.h, bvc_op_jpeg_decode_split): lanes per segment, the smallest and the default chunk in bytes
SPLIT_THREADS, SPLIT_MIN_CHUNK, SPLIT_DEFAULT_CHUNK = 512, 16, 64
# split="auto": the smallest whole-file segment from which the split path beat the one-lane path at 256 AND at 4096 frames by more than
# the spread of the medians (profiles/jpeg_decode_split.txt, second part: 7.4 KB scans of 160 x 160 frames win 6.5x / 1.8x, 6.0 KB scans
# are level at 4096 frames, 3 - 4 KB scans and every restart interval of the table lose there).  The default chunk is that sweep's best.
SPLIT_AUTO_BYTES = 7168


def _split_bytes(split):
    if split == "auto":
        return SPLIT_AUTO_BYTES
    if isinstance(split, bool) or not isinstance(split, int) or split < 0:
        raise ValueError('jpeg: split is 0 (off), a number of bytes or "auto"')
    return split


def _chunk_bytes(chunk):
    if isinstance(chunk, bool) or not isinstance(chunk, int) or (chunk != 0 and chunk < SPLIT_MIN_CHUNK):
        raise ValueError(f"jpeg: chunk is 0 (the default) or at least {SPLIT_MIN_CHUNK} bytes")
    return chunk


def is_split(nbytes, split):
    """whether a segment of ``nbytes`` bytes takes the split path at this ``split``"""
    split = _split_bytes(split)
    return split > 0 and nbytes >= split and 2 * SPLIT_MIN_CHUNK <= nbytes < (1 << 28)


def split_chunks(info, chunk, split=2 * SPLIT_MIN_CHUNK):
    """The (begin, end) byte ranges, offsets into the file, of every chunk of every segment of ``info`` that takes the split path, by
    the rule of include/bvc.h: c = max(chunk, ceil(bytes / SPLIT_THREADS) rounded up to a multiple of 4), chunk j = [begin + j c,
    min(begin + (j + 1) c, end)).  ``split`` defaults to the smallest that splits everything splittable."""
    chunk = _chunk_bytes(chunk)
    out = []
    for b, e in info.segments[:, :2].tolist():
        if is_split(e - b, split):
            c = _lib.lib().bvc_jpeg_split_chunk(e - b, chunk)
            if c < 0:
                _lib.check(c, "bvc_jpeg_split_chunk")
            out.extend((at, min(at + c, e)) for at in range(b, e, c))
    return out


class JpegUnsupported(ValueError):
    """A file the device does not decode; ``reason`` is one of REASONS' names, ``code`` the BVC_JPEG_REFUSE_* value."""

    def __init__(self, code):
        self.code, self.reason = int(code), REASONS.get(int(code), "unknown")
        super().__init__(f"JPEG refused: {self.reason}")


class JpegDecodeError(_lib.BvcError):
    """decode(check=True): some image's status is not 0.  ``status`` is the host copy of the per-image bits."""

    def __init__(self, status):
        self.status = status
        bad = [(i, int(s)) for i, s in enumerate(status.tolist()) if s]
        super().__init__(f"JPEG decode: {len(bad)} damaged image(s), (index, status bits) {bad[:8]}")


class JpegInfo:
    """What parse() found: ``record`` (one INFO element), ``segments`` (int32 [nseg, 4]) and the file's bytes as a uint8 array."""

    def __init__(self, record, segments, data):
        self.record, self.segments, self.data = record, segments, data

    width = property(lambda self: int(self.record["width"][0]))
    height = property(lambda self: int(self.record["height"][0]))
    ncomp = property(lambda self: int(self.record["ncomp"][0]))
    sampling = property(lambda self: (int(self.record["hs"][0]), int(self.record["vs"][0])))
    restart_interval = property(lambda self: int(self.record["restart_interval"][0]))
    flags = property(lambda self: int(self.record["flags"][0]))
    nseg = property(lambda self: int(self.record["nseg"][0]))


def _bytes_of(data):
    if isinstance(data, torch.Tensor):
        data = data.numpy()
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    if a.dtype != np.uint8 or a.ndim != 1:
        raise ValueError("JPEG data must be bytes, a memoryview or a 1-D uint8 array")
    return np.ascontiguousarray(a)


def try_parse(data):
    """parse(), but a refusal is returned (a JpegUnsupported instance), not raised."""
    a = _bytes_of(data)
    L = _lib.lib()
    rec = np.zeros(1, INFO)
    cap = 64
    while True:
        seg = np.empty((cap, SEG_INTS), np.int32)
        rc = L.bvc_jpeg_parse(a.ctypes.data, a.size, rec.ctypes.data, seg.ctypes.data, cap)
        if rc < 0:
            _lib.check(rc, "bvc_jpeg_parse")
        if rc > 0:
            return JpegUnsupported(rc)
        n = int(rec["nseg"][0])
        if n <= cap:
            return JpegInfo(rec, seg[:n], a)
        cap = n


def parse(data):
    """The file's descriptor and segment list (host only, no device call), or JpegUnsupported(reason)."""
    r = try_parse(data)
    if isinstance(r, JpegUnsupported):
        raise r
    return r


class _Frames(list):
    """a list of frames with ``status`` and ``refused``"""


def decode_host(datas):
    """The host twin: a list of uint8 [3, H, W] CPU tensors, with ``.status`` (a list of status bits).  A refused file raises."""
    out = _Frames()
    out.status, out.refused = [], []
    L = _lib.lib()
    for d in datas:
        info = d if isinstance(d, JpegInfo) else parse(d)
        t = torch.empty(3, info.height, info.width, dtype=torch.uint8)
        rc = L.bvc_jpeg_decode_host(info.data.ctypes.data, info.data.size, info.record.ctypes.data, info.segments.ctypes.data, t.data_ptr())
        if rc < 0:
            _lib.check(rc, "bvc_jpeg_decode_host")
        out.append(t)
        out.status.append(rc)
    return out


def decode_host_split(datas, split, chunk=0):
    """The host twin of the split path (the chunk loop, the rounds and the placement in plain C++, lanes one after another): as
    decode_host, and ``.fallback`` / ``.rounds``, lists with per file the split segments that were decoded again whole and the most
    hand-over rounds a segment took."""
    split, chunk = _split_bytes(split), _chunk_bytes(chunk)
    out = _Frames()
    out.status, out.refused, out.fallback, out.rounds = [], [], [], []
    L = _lib.lib()
    extra = np.zeros(2, np.int32)
    for d in datas:
        info = d if isinstance(d, JpegInfo) else parse(d)
        t = torch.empty(3, info.height, info.width, dtype=torch.uint8)
        rc = L.bvc_jpeg_decode_host_split(info.data.ctypes.data, info.data.size, info.record.ctypes.data, info.segments.ctypes.data, split,
                                          chunk, t.data_ptr(), extra.ctypes.data)
        if rc < 0:
            _lib.check(rc, "bvc_jpeg_decode_host_split")
        out.append(t)
        out.status.append(rc)
        out.fallback.append(int(extra[0]))
        out.rounds.append(int(extra[1]))
    return out


def _align16(v):
    return (v + 15) & ~15


class _Pack:
    """One staging buffer for a call: [infos | segments | output offsets | the files' bytes], each part 16-byte aligned, so that the
    whole input crosses in one copy."""

    def __init__(self, n, nseg, nbytes):
        self.n, self.nseg, self.nbytes = n, nseg, nbytes
        self.at_seg = _align16(n * INFO.itemsize)
        self.at_off = _align16(self.at_seg + nseg * SEG_INTS * 4)
        self.at_blob = _align16(self.at_off + n * 8)
        self.total = _align16(self.at_blob + nbytes)

    def views(self, host):
        """numpy views of a host uint8 array of at least .total bytes"""
        return (host[:self.n * INFO.itemsize].view(INFO), host[self.at_seg:self.at_seg + self.nseg * SEG_INTS * 4].view(np.int32),
                host[self.at_off:self.at_off + self.n * 8].view(np.int64), host[self.at_blob:self.at_blob + self.nbytes])


_REFUSED = np.zeros(1, INFO)
_NO_SEGS = np.zeros((0, SEG_INTS), np.int32)
_NO_BYTES = np.zeros(0, np.uint8)


def _fill(pack, host, infos, out_offsets, split=0):
    """infos (JpegInfo or JpegUnsupported per image) into the staging array; returns the workspace bytes (with ``split``, those of the
    split path)"""
    recs, segs, offs, blob = pack.views(host)
    ok = [isinstance(i, JpegInfo) for i in infos]
    np.concatenate([i.record if k else _REFUSED for i, k in zip(infos, ok)], out=recs)
    np.concatenate([i.segments if k else _NO_SEGS for i, k in zip(infos, ok)], out=segs.reshape(-1, SEG_INTS))
    np.concatenate([i.data if k else _NO_BYTES for i, k in zip(infos, ok)], out=blob)
    nseg = np.array([i.segments.shape[0] if k else 0 for i, k in zip(infos, ok)], np.int64)
    size = np.array([i.data.size if k else 0 for i, k in zip(infos, ok)], np.int64)
    recs["seg_first"] = np.cumsum(nseg) - nseg
    recs["blob_offset"] = np.cumsum(size) - size
    if not all(ok):
        recs["reason"] = [0 if k else i.code for i, k in zip(infos, ok)]
    offs[:] = out_offsets
    L = _lib.lib()
    return int((L.bvc_op_jpeg_decode_split_workspace if split else L.bvc_op_jpeg_decode_workspace)(recs.ctypes.data, pack.n))


def _launch(pack, host, dev, out, out_bytes, status, work, lanes, stages=3, split=0, chunk=0, extra=None):
    b = dev.data_ptr()
    h = host.ctypes.data
    if split:
        _lib.check(_lib.lib().bvc_op_jpeg_decode_split(b + pack.at_blob, pack.nbytes, h, b, pack.n, h + pack.at_seg, b + pack.at_seg,
                                                       pack.nseg, h + pack.at_off, b + pack.at_off, out.data_ptr(), out_bytes,
                                                       status.data_ptr(), work.data_ptr() if work is not None else None,
                                                       work.numel() if work is not None else 0, int(lanes), int(stages), int(split),
                                                       int(chunk), extra.data_ptr(), _lib.current_stream_ptr()), "bvc_op_jpeg_decode_split")
        return
    _lib.check(_lib.lib().bvc_op_jpeg_decode(b + pack.at_blob, pack.nbytes, h, b, pack.n, h + pack.at_seg, b + pack.at_seg, pack.nseg,
                                             h + pack.at_off, b + pack.at_off, out.data_ptr(), out_bytes, status.data_ptr(),
                                             work.data_ptr() if work is not None else None, work.numel() if work is not None else 0,
                                             int(lanes), int(stages), _lib.current_stream_ptr()), "bvc_op_jpeg_decode")


def _sizes(infos):
    nseg = sum(i.segments.shape[0] for i in infos if isinstance(i, JpegInfo))
    nbytes = sum(i.data.size for i in infos if isinstance(i, JpegInfo))
    return nseg, nbytes


def decode(datas, device, out=None, infos=None, check=False, lanes=0, split=0, chunk=0):
    """Decode a sequence of JPEG files (bytes / memoryview / 1-D uint8 arrays) on ``device``.

    Returns uint8 [F, 3, H, W] when every decodable file has the same size, else a list of [3, H, W] views into one buffer; either
    carries ``.status`` (int32 [F] on the device: 0, or the ST_* bits of a damaged file, whose bytes are then the host twin's on the
    same input) and ``.refused`` (a host list of (index, reason) for files that parse refuses: their frames are zero - of zero size
    in the list form - and the caller decodes them on the host).  ``infos``: what try_parse() / parse() gave for each file, to keep
    the parse out of this call (loader workers can do it).  ``out``: where to decode to: [F, 3, H, W] uint8, or for mixed sizes a 1-D
    uint8 tensor of at least the frames' bytes.  Descriptors, segments and bytes cross in ONE asynchronous copy out of pinned memory,
    and nothing synchronises - unless ``check`` is set: then the call synchronises once and raises JpegDecodeError on any non-zero
    status.  ``lanes``: segments per wave of the entropy kernel, 0 = chosen by the call.

    ``split``: segments of at least this many bytes - a file without restart markers is ONE segment - are cut into chunks of ``chunk``
    bytes (0 = SPLIT_DEFAULT_CHUNK) that the lanes of a workgroup decode together (DESIGN.md "JPEG decode"); 0, the default, is the
    one-lane path alone, "auto" is SPLIT_AUTO_BYTES.  Same bytes and status either way.  The result also carries ``.fallback`` and
    ``.rounds``, int32 [F] on the device: per file the split segments that turned out damaged and were decoded again by the one-lane
    path, and the most hand-over rounds one of its segments took (zeros without ``split``)."""
    device = torch.device(device)
    split, chunk = _split_bytes(split), _chunk_bytes(chunk)
    if infos is None:
        infos = [try_parse(d) for d in datas]
    infos = list(infos)
    n = len(infos)
    if n < 1:
        raise ValueError("jpeg.decode: nothing to decode")
    refused = [(i, info.reason) for i, info in enumerate(infos) if isinstance(info, JpegUnsupported)]
    shapes = {(i.height, i.width) for i in infos if isinstance(i, JpegInfo)}
    uniform = len(shapes) == 1
    out_offsets, at = [], 0
    if uniform:
        H, W = next(iter(shapes))
        out_offsets = [3 * H * W * i for i in range(n)]
        at = 3 * H * W * n
    else:
        for info in infos:
            out_offsets.append(at)
            at += 3 * info.height * info.width if isinstance(info, JpegInfo) else 0
    given = out is not None
    if not given:
        out = (torch.zeros if refused else torch.empty)(max(at, 1), dtype=torch.uint8, device=device)
    else:
        if out.dtype != torch.uint8 or out.device != device or not out.is_contiguous() or out.numel() < at:
            raise ValueError(f"jpeg.decode: out must be a contiguous uint8 tensor on {device} with at least {at} elements")
        if uniform and tuple(out.shape) != (n, 3, H, W):
            raise ValueError(f"jpeg.decode: out must have shape {(n, 3, H, W)}")
    flat = out.view(-1)
    nseg, nbytes = _sizes(infos)
    pack = _Pack(n, nseg, nbytes)
    host_t = torch.empty(pack.total, dtype=torch.uint8, pin_memory=True)
    host = host_t.numpy()
    ws = _fill(pack, host, infos, out_offsets, split)
    with torch.cuda.device(device):
        dev = torch.empty(pack.total, dtype=torch.uint8, device=device)
        dev.copy_(host_t, non_blocking=True)
        status = torch.empty(n, dtype=torch.int32, device=device)
        work = torch.empty(max(ws, 16), dtype=torch.uint8, device=device)
        extra = (torch.empty if split else torch.zeros)(n, 2, dtype=torch.int32, device=device)
        _launch(pack, host, dev, flat, flat.numel(), status, work, lanes, split=split, chunk=chunk, extra=extra)
    if uniform:
        res = flat[:at].view(n, 3, H, W)
        if refused and given:
            for i, _ in refused:
                res[i].zero_()
    else:
        res = _Frames()
        for i, info in enumerate(infos):
            hw = (info.height, info.width) if isinstance(info, JpegInfo) else (0, 0)
            res.append(flat[out_offsets[i]:out_offsets[i] + 3 * hw[0] * hw[1]].view(3, *hw))
    res.status, res.refused = status, refused
    res.fallback, res.rounds = extra[:, 0], extra[:, 1]
    if check:
        st = status.cpu()      # the one synchronisation
        if bool(st.any()):
            raise JpegDecodeError(st)
    return res


class JpegClipRing:
    """ClipUploadRing for compressed frames: ``stage(datas)`` parses B * T JPEG files (each Hs x Ws) and uploads their bytes on the
    copy stream; ``get()`` makes the current stream wait for that copy, decodes on it and hands out [B, T, 3, Hs, Ws] uint8 with
    ``.status`` (int32 [B * T] on the device); ``release()`` lets the slot be overwritten once everything enqueued so far on the
    current stream has run.  Same event fencing as ClipUploadRing; nothing blocks the host except a full ring and the re-use of a
    pinned staging buffer whose upload has not left the host yet.  ``max_bytes``: capacity for one batch's compressed bytes;
    ``max_segments``: for its restart segments (default: eight per 8 rows of every frame).  ``split`` / ``chunk``: as in decode();
    with ``split`` the workspace is that of the split path (3.25 times the planes) and batches carry ``.fallback`` and ``.rounds``."""

    def __init__(self, shape, device, depth=3, max_bytes=None, max_segments=None, lanes=0, split=0, chunk=0):
        if depth < 2:
            raise ValueError("JpegClipRing: depth must be >= 2 (one slot in use, one in flight)")
        B, T, Hs, Ws = (int(v) for v in shape)
        self.device = torch.device(device)
        self.shape, self.depth, self.lanes = (B, T, Hs, Ws), depth, lanes
        self.split, self.chunk = _split_bytes(split), _chunk_bytes(chunk)
        self.frames = B * T
        self.max_bytes = int(max_bytes) if max_bytes is not None else self.frames * Hs * Ws      # a third of the raw frames
        self.max_segments = int(max_segments) if max_segments is not None else self.frames * 8 * ((Hs + 7) // 8)
        self._cap = _Pack(self.frames, self.max_segments, self.max_bytes).total
        pad = lambda v: (v + 15) // 16 * 16      # noqa: E731
        planes = self.frames * (3 * pad(Hs) * pad(Ws) + 16)
        self._ws_bytes = planes + 4 * self.max_segments
        if self.split:      # flags, rounds and routed records per segment, 4 + 128 bytes per block (bvc_op_jpeg_decode_split_workspace)
            self._ws_bytes += 24 * self.max_segments + planes // 4 + 2 * planes + 128
        self.pinned = [torch.empty(self._cap, dtype=torch.uint8, pin_memory=True) for _ in range(depth)]
        with torch.cuda.device(self.device):
            self.dev = [torch.empty(self._cap, dtype=torch.uint8, device=self.device) for _ in range(depth)]
            self.out = [torch.empty(B, T, 3, Hs, Ws, dtype=torch.uint8, device=self.device) for _ in range(depth)]
            self.status = [torch.empty(self.frames, dtype=torch.int32, device=self.device) for _ in range(depth)]
            self.extra = [torch.zeros(self.frames, 2, dtype=torch.int32, device=self.device) for _ in range(depth)]
            self.work = torch.empty(self._ws_bytes, dtype=torch.uint8, device=self.device)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.ready = [torch.cuda.Event() for _ in range(depth)]
        self.free = [torch.cuda.Event() for _ in range(depth)]
        self._work_done = None      # the one workspace is shared: a get() on another stream waits for the decode before it
        self._packs = [None] * depth
        self._head = self._tail = self._count = 0
        self._out = []
        self._used = [False] * depth
        self.bytes_uploaded = 0

    def can_stage(self):
        return self._count + len(self._out) < self.depth

    def stage(self, datas, infos=None):
        """Enqueue the upload of one batch: B * T files in clip-major order (or B sequences of T).  Returns False when the ring is
        full.  A frame that is not Hs x Ws is a ValueError; a file that parse refuses raises its JpegUnsupported."""
        if not self.can_stage():
            return False
        B, T, Hs, Ws = self.shape
        if infos is None:
            datas = list(datas)
            if datas and isinstance(datas[0], (list, tuple)):
                datas = [f for clip in datas for f in clip]
            infos = [parse(d) for d in datas]
        infos = list(infos)
        if len(infos) != self.frames:
            raise ValueError(f"JpegClipRing.stage: expected {self.frames} frames, got {len(infos)}")
        for i, info in enumerate(infos):
            if isinstance(info, JpegUnsupported):
                raise info
            if (info.height, info.width) != (Hs, Ws):
                raise ValueError(f"JpegClipRing.stage: frame {i} is {info.height} x {info.width}, the ring holds {Hs} x {Ws}")
        nseg, nbytes = _sizes(infos)
        if nseg > self.max_segments or nbytes > self.max_bytes:
            raise ValueError(f"JpegClipRing.stage: {nbytes} bytes in {nseg} segments exceed max_bytes {self.max_bytes} / max_segments "
                             f"{self.max_segments}")
        s = self._head
        if self._used[s]:
            self.ready[s].synchronize()      # the previous upload out of this staging buffer has left the host
        pack = _Pack(self.frames, nseg, nbytes)
        ws = _fill(pack, self.pinned[s].numpy(), infos, [3 * Hs * Ws * i for i in range(self.frames)], self.split)
        assert ws <= self._ws_bytes
        with torch.cuda.stream(self.copy_stream):
            if self._used[s]:
                self.copy_stream.wait_event(self.free[s])
            self.dev[s][:pack.total].copy_(self.pinned[s][:pack.total], non_blocking=True)
            self.ready[s].record(self.copy_stream)
        self._packs[s] = pack
        self._used[s] = True
        self.bytes_uploaded += pack.total
        self._head = (s + 1) % self.depth
        self._count += 1
        return True

    def get(self):
        """[B, T, 3, Hs, Ws] uint8 of the oldest staged batch, decoded on the CURRENT stream after it has waited for the copy."""
        if self._count == 0:
            raise RuntimeError("JpegClipRing.get: nothing staged")
        s = self._tail
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self.ready[s])
        if self._work_done is not None:
            cur.wait_event(self._work_done)
        with torch.cuda.device(self.device):
            _launch(self._packs[s], self.pinned[s].numpy(), self.dev[s], self.out[s], self.out[s].numel(), self.status[s], self.work, self.lanes,
                    split=self.split, chunk=self.chunk, extra=self.extra[s])
        self._work_done = torch.cuda.Event()
        self._work_done.record(cur)
        self._tail = (s + 1) % self.depth
        self._count -= 1
        self._out.append(s)
        res = self.out[s]
        res.status = self.status[s]
        res.fallback, res.rounds = self.extra[s][:, 0], self.extra[s][:, 1]
        return res

    def release(self):
        """The oldest handed-out batch may be overwritten once everything enqueued so far on the current stream has run."""
        if not self._out:
            raise RuntimeError("JpegClipRing.release: nothing to release")
        s = self._out.pop(0)
        self.free[s].record(torch.cuda.current_stream(self.device))
