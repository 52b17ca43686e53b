"""Random erasing for fine-tuning: the host side of the erase inside the patch gather (include/bvc.h, bvc_erase_box).

``RandomErasing`` draws, per clip, what the published VideoMAE fine-tuning recipe draws (``reprob 0.25``, ``mode pixel``, ``count 1``):
whether the clip is erased at all, how many boxes, and each box's area, aspect and place.  It hands back a ``ClipErase`` - a table of
up to four boxes per clip, a seed and a call offset - that ``VideoMAEForVideoClassification.forward(..., erase=)`` gives to the library,
where the patch gather writes the boxes' content (zeros, one normal value per frame and channel, or per-element normal noise, in
normalised space) in place of the source pixels while it reads the clip: the erased clip is never written, uint8 input stays uint8,
and an erased run of pixels is not loaded.  With ``mix=`` armed as well the order is the recipe's: erase each clip, then mix the batch.
The draws are host-side (a ``numpy.random.Generator``), like the mask generators': no device sync.
"""
import math

import numpy as np
import torch

MAX_BOXES = 4                                      # BVC_ERASE_MAX_BOXES
MODES = {"const": 0, "rand": 1, "pixel": 2}


def _mode_code(m):
    if isinstance(m, str):
        if m not in MODES:
            raise ValueError(f"erase mode {m!r} must be one of {sorted(MODES)}")
        return MODES[m]
    return int(m)


class ClipErase:
    """The erasing of one batch: ``boxes`` (int32 [B, n, 4], n <= 4: rows [y0, y1) x columns [x0, x1) of every frame; an empty box
    erases nothing; of overlapping boxes the later one wins) and ``modes`` (int32 [B, n]: 0 const, 1 rand, 2 pixel; names are accepted,
    and one value serves every box) - numpy arrays on the host, readable without a sync - with the ``seed`` and call ``offset`` of the
    noise, and ``table``, the same as the library's device table ([B, n, 5] int32: y0, y1, x0, x1, mode), uploaded in one
    asynchronous copy from pinned memory, or None when built for the CPU."""

    def __init__(self, boxes, modes, seed=0, offset=0, image_size=None, device=None):
        self.boxes = np.ascontiguousarray(boxes, dtype=np.int32)
        if self.boxes.ndim == 2:
            self.boxes = self.boxes[:, None, :]
        if self.boxes.ndim != 3 or self.boxes.shape[2] != 4 or not 1 <= self.boxes.shape[1] <= MAX_BOXES or self.boxes.shape[0] < 1:
            raise ValueError(f"ClipErase: boxes must be [B, n, 4] with 1 <= n <= {MAX_BOXES}, got {tuple(self.boxes.shape)}")
        B, n = self.boxes.shape[:2]
        if isinstance(modes, (str, int)):
            modes = np.full((B, n), _mode_code(modes), dtype=np.int32)
        else:
            flat = [_mode_code(m) for m in np.asarray(modes, dtype=object).reshape(-1)]
            if len(flat) != B * n:
                raise ValueError(f"ClipErase: {len(flat)} modes for {B} clips of {n} boxes")
            modes = np.array(flat, dtype=np.int32).reshape(B, n)
        self.modes = modes
        self.seed, self.offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
        self.image_size = tuple(int(v) for v in image_size) if image_size is not None else None
        self.table = None
        device = torch.device(device) if device is not None else None
        if device is not None and device.type != "cpu":
            host = torch.empty((B, n, 5), dtype=torch.int32, pin_memory=True)      # a pageable copy would make the host wait
            h = host.numpy()
            h[:, :, :4] = self.boxes
            h[:, :, 4] = self.modes
            self.table = host.to(device, non_blocking=True)

    @property
    def batch_size(self):
        return int(self.boxes.shape[0])

    @property
    def num_boxes(self):
        return int(self.boxes.shape[1])

    @property
    def erased(self):
        """bool [B]: the clip has a box that is not empty"""
        return ((self.boxes[:, :, 1] > self.boxes[:, :, 0]) & (self.boxes[:, :, 3] > self.boxes[:, :, 2])).any(axis=1)

    def __repr__(self):
        return (f"ClipErase(batch_size={self.batch_size}, boxes={self.num_boxes}, erased={int(self.erased.sum())}, "
                f"device={self.table.device if self.table is not None else 'cpu'})")


class RandomErasing:
    """Random erasing of a batch of clips, with the interface of the published recipe:

        re = bvc.RandomErasing(probability=0.25, mode="pixel", generator=np.random.default_rng(seed))
        erase = re(B, image_size=(H, W), device=pixels.device)
        out = model(pixel_values=pixels, labels=soft, mix=mix, erase=erase)

    Rules, per clip and in this order of draws:
      * ``random()`` against ``probability``: otherwise the clip keeps no box;
      * count = ``min_count``, or ``integers(min_count, max_count + 1)`` when ``max_count`` is given (at most 4);
      * per box up to 10 attempts of: area = ``uniform(min_area, max_area)`` * H * W / count; aspect =
        exp(``uniform(log min_aspect, log max_aspect)``) with ``max_aspect`` = 1 / ``min_aspect`` by default;
        h = int(round(sqrt(area * aspect))), w = int(round(sqrt(area / aspect))); accepted when h < H and w < W, and then
        top = ``integers(0, H - h + 1)``, left = ``integers(0, W - w + 1)``; ten failures mean no box;
      * a box is the same in every frame of the clip (a cube); the noise is fresh per frame;
      * ``seed`` of the noise is drawn once, at construction (``integers(0, 2**63)``); ``offset`` counts the calls, so every batch
        gets other noise.

    ``device="cpu"`` (or None) yields a ``ClipErase`` without a device table: no library call, no GPU needed."""

    def __init__(self, probability=0.25, mode="pixel", min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, min_count=1,
                 max_count=None, generator=None):
        if not 0.0 <= probability <= 1.0:
            raise ValueError("probability must lie in [0, 1]")
        if not (0.0 < min_area <= max_area <= 1.0) or not min_aspect > 0.0:
            raise ValueError("0 < min_area <= max_area <= 1 and min_aspect > 0 are required")
        self.mode = _mode_code(mode)
        if self.mode not in (0, 1, 2):
            raise ValueError(f"mode {mode!r} unknown")
        max_aspect = 1.0 / min_aspect if max_aspect is None else float(max_aspect)
        lo, hi = sorted((math.log(min_aspect), math.log(max_aspect)))
        self.log_aspect = (lo, hi)
        self.probability, self.min_area, self.max_area = float(probability), float(min_area), float(max_area)
        self.min_count = int(min_count)
        self.max_count = self.min_count if max_count is None else int(max_count)
        self.draw_count = max_count is not None
        if not 1 <= self.min_count <= self.max_count <= MAX_BOXES:
            raise ValueError(f"1 <= min_count <= max_count <= {MAX_BOXES} is required (got {min_count}, {max_count})")
        self.generator = generator if generator is not None else np.random.default_rng()
        self.seed = int(self.generator.integers(0, 2 ** 63))
        self.offset = 0

    def _draw_clip(self, H, W):
        g = self.generator
        boxes = []
        if not g.random() < self.probability:
            return boxes
        count = int(g.integers(self.min_count, self.max_count + 1)) if self.draw_count else self.min_count
        for _ in range(count):
            for _ in range(10):
                area = float(g.uniform(self.min_area, self.max_area)) * H * W / count
                aspect = math.exp(float(g.uniform(*self.log_aspect)))
                h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
                if h < H and w < W:
                    top, left = int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1))
                    boxes.append((top, top + h, left, left + w))
                    break
        return boxes

    def __call__(self, batch_size, image_size, device=None):
        B = int(batch_size)
        H, W = (int(v) for v in image_size)
        tab = np.zeros((B, self.max_count, 4), dtype=np.int32)
        for b in range(B):
            for j, box in enumerate(self._draw_clip(H, W)):
                tab[b, j] = box
        erase = ClipErase(tab, self.mode, seed=self.seed, offset=self.offset, image_size=(H, W), device=device)
        self.offset += 1
        return erase


def erase_noise(seed, offset, kind, B, T, C, H, W, device):
    """The f32 values the gather writes for erased elements (bvc_op_erase_noise): ``kind`` 0 (or "pixel") the per-element noise of a
    whole batch [B, T, C, H, W], ``kind`` 1 (or "rand") the colours [B, T, 4, 4] (box, channel)."""
    from . import _lib
    kind = {"pixel": 0, "rand": 1}.get(kind, kind)
    out = torch.empty((B, T, C, H, W) if int(kind) == 0 else (B, T, 4, 4), dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().bvc_op_erase_noise(int(seed), int(offset), int(kind), int(B), int(T), int(C), int(H), int(W), out.data_ptr(),
                                                 _lib.current_stream_ptr()), "bvc_op_erase_noise")
    return out
