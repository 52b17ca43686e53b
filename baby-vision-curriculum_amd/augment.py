"""Clip transforms on the GPU: resize, crop, flip, colour jitter and grayscale on uint8 frames (include/bvc.h, bvc_frame_aug).

The reference's loaders run these per frame on the host, through torchvision / PIL, between ``read_image`` and the upload
(pretraining/generative/homeview.py:227-231, predictive/homeview.py:118-178, contrastive/homeview.py:120-181).  Here the host only draws
a small table - one entry per OUTPUT frame: source frame, region, resized size, window, flip, jitter stages and factors, gray - and the
library applies it to frames that are already on the device (``ClipUploadRing`` at the loader's stored resolution).  The result is an
ordinary uint8 clip ``[B, T, 3, H, W]`` that every model takes.

    tf = bvc.augment.ClipTransform(224, augs="cjg", crop_scale=(0.08, 1.0), generator=np.random.default_rng(seed))
    clips = tf(ring.upload(host_uint8))            # [B, T, 3, Hs, Ws] uint8 on the device -> [B, T, 3, 224, 224] uint8
    loss = model(clips, ...)

The draws follow torchvision's ``get_params`` rules (``sample_params``) from a ``numpy.random.Generator``; they do NOT reproduce
torchvision's random stream bit for bit (that one is torch's global generator, consumed in torchvision's own order).
``clip_transform_host`` is the same arithmetic compiled for the host: no GPU needed.

``ClipTransform`` stops at these: ``'b'`` (Gaussian blur) and ``RandomRotation`` raise there.  ``ClipAugment`` takes the reference's
whole letter set, ``c j b g o n``: it runs the stage above and then the post stage (include/bvc.h, bvc_frame_post) on its output,

    aug = bvc.ClipAugment(64, augs="cjo", views=2, generator=np.random.default_rng(seed))      # the SimCLR recipe's --augs
    views = aug(ring.upload(host_uint8))           # [B, T, 3, Hs, Ws] -> [2 B, T, 3, 64, 64] uint8

with one ``bvc_frame_post`` per output frame: ``'b'`` is PIL's ``ImageFilter.GaussianBlur`` (three box passes per direction, each
rounded to uint8, in 8.24 fixed point), ``'o'`` RandomHorizontalFlip + PIL's ``Image.rotate(angle, NEAREST)`` (an inverse affine map in
16.16 fixed point).  Both are integer arithmetic restated from Pillow: ``clip_post``, ``clip_post_host`` and PIL give the same bytes.

RandAugment (the ``rand-m7-n4-mstd0.5-inc1`` family of the fine-tuning recipes) is a third stage (include/bvc.h, bvc_frame_randaug):

    ra = bvc.RandAugment("rand-m7-n4-mstd0.5-inc1", generator=np.random.default_rng(seed))
    clips = ra(clips)                              # [B, T, 3, H, W] uint8 on the device -> the same shape
    aug = bvc.ClipAugment(224, augs="c", randaug="rand-m7-n4-mstd0.5-inc1", generator=...)      # or as ClipAugment's last stage

Per clip it draws up to ``num_ops`` of the fifteen PIL operations ``RANDAUG_OPS`` with their parameters (``sample_randaug_params``);
``rand_augment`` applies them, ``rand_augment_host`` is the host twin, and both give the bytes of the PIL calls.
"""
import math

import numpy as np
import torch

from . import _lib

# bvc_frame_aug, 68 bytes
FRAME_AUG = np.dtype([("src", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("Hr", "<i4"), ("Wr", "<i4"),
                      ("oy", "<i4"), ("ox", "<i4"), ("flip", "<i4"), ("nops", "<i4"), ("order", "<i4"), ("factor", "<f4", (4,)),
                      ("gray", "<i4")])
assert FRAME_AUG.itemsize == 68
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
MAX_SCALE = 16      # BVC_AUG_MAX_SCALE
# bvc_frame_post, 44 bytes
FRAME_POST = np.dtype([("blur_r", "<i4"), ("blur_ww", "<u4"), ("blur_fw", "<u4"), ("gray", "<i4"), ("rotate", "<i4"), ("rot", "<i4", (6,))])
assert FRAME_POST.itemsize == 44
MAX_BLUR_RADIUS = 4.0      # BVC_AUG_MAX_BLUR_RADIUS
# bvc_randaug_stage, 36 bytes, and bvc_frame_randaug, 296 bytes
RANDAUG_MAX_OPS = 8        # BVC_RANDAUG_MAX_OPS
RANDAUG_STAGE = np.dtype([("op", "<i4"), ("ival", "<i4"), ("fval", "<f4"), ("aff", "<i4", (6,))])
FRAME_RANDAUG = np.dtype([("nops", "<i4"), ("fill", "u1", (4,)), ("stage", RANDAUG_STAGE, (RANDAUG_MAX_OPS,))])
assert RANDAUG_STAGE.itemsize == 36 and FRAME_RANDAUG.itemsize == 296
RANDAUG_OPS = ("AutoContrast", "Equalize", "Invert", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness",
               "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")


def pack_order(ops):
    """Stage list (op codes in the order they run) -> the table's ``order`` word."""
    word = 0
    for i, op in enumerate(ops):
        word |= int(op) << (4 * i)
    return word


def empty_table(n):
    """n identity-colour entries (no stages, no flip, no gray); geometry fields are zero and must be filled."""
    t = np.zeros(int(n), dtype=FRAME_AUG)
    t["factor"][:, :3] = 1.0
    return t


def _size2(size):
    return (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))


def center_crop_params(frames, src_size, size, resize=None):
    """The VideoMAE geometry, ``Resize(resize) + CenterCrop(size)``, for ``frames`` source frames in order: the whole frame resized so
    that its short side becomes ``resize`` (default: the short side of ``size``, the reference's ``Resize(image_size)``) and its long
    side ``int(resize * long / short)``, as torchvision computes it, then the centred ``size`` window at ``round((Hr - Ho) / 2)``."""
    Hs, Ws = _size2(src_size)
    Ho, Wo = _size2(size)
    S = int(resize) if resize is not None else min(Ho, Wo)
    if Hs <= Ws:
        Hr, Wr = S, int(S * Ws / Hs)
    else:
        Hr, Wr = int(S * Hs / Ws), S
    if Hr < Ho or Wr < Wo:
        raise ValueError(f"center_crop_params: the {Ho} x {Wo} window does not fit the {Hr} x {Wr} resized frame (no padding)")
    t = empty_table(frames)
    t["src"] = np.arange(int(frames))
    t["w"], t["h"], t["Hr"], t["Wr"] = Ws, Hs, Hr, Wr
    t["oy"], t["ox"] = int(round((Hr - Ho) / 2.0)), int(round((Wr - Wo) / 2.0))
    return t


def _crop_box(g, Hs, Ws, scale, ratio):
    """RandomResizedCrop.get_params: ten attempts, then the centre crop at the nearest allowed ratio.  (x0, y0, w, h), fallback?"""
    area = Hs * Ws
    log_r = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target = area * g.uniform(scale[0], scale[1])
        ar = math.exp(g.uniform(log_r[0], log_r[1]))
        w, h = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
        if 0 < w <= Ws and 0 < h <= Hs:
            return int(g.integers(0, Ws - w + 1)), int(g.integers(0, Hs - h + 1)), w, h, False
    in_ratio = Ws / Hs
    if in_ratio < ratio[0]:
        w, h = Ws, int(round(Ws / ratio[0]))
    elif in_ratio > ratio[1]:
        h, w = Hs, int(round(Hs * ratio[1]))
    else:
        w, h = Ws, Hs
    return (Ws - w) // 2, (Hs - h) // 2, w, h, True


def sample_params(batch, frames, src_size, size, augs="cjg", crop_scale=(0.08, 1.0), crop_ratio=(3.0 / 4.0, 4.0 / 3.0),
                  jitter_strength=0.5, jitter_p=0.8, gray_p=0.2, extra_gray_p=0.5, flip=0.0, consistent=True, views=1,
                  generator=None, return_info=False):
    """Draw the table for ``views`` x ``batch`` clips of ``frames`` frames from a source batch ``[batch, frames, 3, Hs, Ws]``: entry
    ``(v * batch + b) * frames + t`` reads source frame ``b * frames + t``, so every view shares the one upload.

    ``augs`` letters, as the reference's ``--augs``:
      'c'  RandomResizedCrop(size, scale=crop_scale): ten attempts at an area uniform in ``crop_scale`` x the frame's with a
           log-uniform aspect ratio in ``crop_ratio``, a uniform position, and the centre-crop fallback; without 'c' the
           Resize + CenterCrop geometry of ``center_crop_params``;
      'j'  the reference's get_color_distortion(s = jitter_strength): with probability ``jitter_p`` a ColorJitter(0.8 s, 0.8 s, 0.8 s,
           0.2 s) - brightness, contrast and saturation factors uniform in [max(0, 1 - 0.8 s), 1 + 0.8 s], a hue shift uniform in
           [-0.2 s, 0.2 s], the four stages in a uniformly random order - then RandomGrayscale(gray_p);
      'g'  a further RandomGrayscale(extra_gray_p) (gray of gray is gray: the two fold into one flag);
      'n'  nothing (ignored).  'b' (blur) and 'o' are refused: they belong to the post stage (``sample_post_params``, ``ClipAugment``).
    ``flip`` is the probability of RandomHorizontalFlip.  ``consistent=True`` draws once per clip and repeats the entry over its
    frames; ``False`` draws per frame, which is what the reference's per-frame ``transform(read_image(fp))`` does.
    With ``return_info`` also a dict of per-entry diagnostics (``fallback``: the crop came from the fallback)."""
    for ch in augs:
        if ch == "b":
            raise ValueError("augs 'b' (Gaussian blur) is not part of this stage: ClipAugment / sample_post_params draw it")
        if ch not in "cjgn":
            raise ValueError(f"augs letter {ch!r} unknown (c, j, g, n; ClipAugment also takes b and o)")
    if not (0 <= crop_scale[0] <= crop_scale[1]) or not (0 < crop_ratio[0] <= crop_ratio[1]):
        raise ValueError("crop_scale / crop_ratio must be ascending ranges")
    if not (0.0 <= flip <= 1.0 and 0.0 <= jitter_p <= 1.0 and 0.0 <= gray_p <= 1.0 and 0.0 <= extra_gray_p <= 1.0):
        raise ValueError("probabilities must lie in [0, 1]")
    s = float(jitter_strength)
    if s < 0 or 0.2 * s > 0.5:
        raise ValueError("jitter_strength must lie in [0, 2.5] (the hue range 0.2 s may not exceed 0.5)")
    g = generator if generator is not None else np.random.default_rng()
    B, T, V = int(batch), int(frames), int(views)
    Hs, Ws = _size2(src_size)
    Ho, Wo = _size2(size)
    table = empty_table(V * B * T)
    fallback = np.zeros(V * B * T, dtype=bool)
    centre = None if "c" in augs else center_crop_params(1, (Hs, Ws), (Ho, Wo))[0]
    lo, hi = max(0.0, 1.0 - 0.8 * s), 1.0 + 0.8 * s

    def draw(e):
        fb = False
        if centre is None:
            e["x0"], e["y0"], e["w"], e["h"], fb = _crop_box(g, Hs, Ws, crop_scale, crop_ratio)
            e["Hr"], e["Wr"], e["oy"], e["ox"] = Ho, Wo, 0, 0
        else:
            for k in ("x0", "y0", "w", "h", "Hr", "Wr", "oy", "ox"):
                e[k] = centre[k]
        gray = False
        if "j" in augs:
            if g.random() < jitter_p:
                e["factor"] = (g.uniform(lo, hi), g.uniform(lo, hi), g.uniform(lo, hi), g.uniform(-0.2 * s, 0.2 * s))
                e["nops"], e["order"] = 4, pack_order(g.permutation(4))
            gray = g.random() < gray_p
        if "g" in augs:
            gray = bool(g.random() < extra_gray_p) or gray
        e["gray"] = int(gray)
        e["flip"] = int(g.random() < flip) if flip > 0 else 0
        return fb

    for v in range(V):
        for b in range(B):
            first = (v * B + b) * T
            for t in range(T):
                i = first + t
                if consistent and t > 0:
                    table[i] = table[first]
                    fallback[i] = fallback[first]
                else:
                    fallback[i] = draw(table[i])
                table[i]["src"] = b * T + t
    return (table, {"fallback": fallback}) if return_info else table


def _check_clips(clips):
    if clips.dtype != torch.uint8 or clips.dim() != 5:
        raise ValueError(f"clips must be uint8 [B, T, C, Hs, Ws], got {clips.dtype} {tuple(clips.shape)}")
    if not clips.is_contiguous():
        raise ValueError("clips must be contiguous")


def _check_table(table):
    t = np.ascontiguousarray(table)
    if t.dtype != FRAME_AUG or t.ndim != 1 or t.shape[0] < 1:
        raise ValueError("table must be a non-empty 1-d array of augment.FRAME_AUG entries")
    return t


def clip_transform_host(frames, table, size):
    """bvc_clip_transform_host: uint8 host frames ``[..., C, Hs, Ws]`` (any leading dims, flattened to F_src) and a table of F_out
    entries -> uint8 ``[F_out, 3, Ho, Wo]``.  No GPU needed."""
    if frames.dtype != torch.uint8 or frames.dim() < 3 or frames.device.type != "cpu":
        raise ValueError("frames must be a uint8 host tensor [..., C, Hs, Ws]")
    frames = frames.contiguous()
    t = _check_table(table)
    C, Hs, Ws = (int(v) for v in frames.shape[-3:])
    Ho, Wo = _size2(size)
    F_src = frames.numel() // max(1, C * Hs * Ws)
    out = torch.empty(t.shape[0], 3, Ho, Wo, dtype=torch.uint8)
    _lib.check(_lib.lib().bvc_clip_transform_host(frames.data_ptr(), F_src, C, Hs, Ws, t.ctypes.data, t.shape[0], Ho, Wo, out.data_ptr()),
               "bvc_clip_transform_host")
    return out


def clip_transform(frames, table, size, out=None):
    """bvc_op_clip_transform on the current stream: uint8 device frames ``[..., C, Hs, Ws]`` and a host table of F_out entries ->
    uint8 ``[F_out, 3, Ho, Wo]`` on the device (``out``: a contiguous uint8 device tensor of that many bytes to write into).  The
    table travels through pinned memory in one asynchronous copy; nothing synchronises."""
    if frames.dtype != torch.uint8 or frames.dim() < 3 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous uint8 tensor [..., C, Hs, Ws]")
    t = _check_table(table)
    C, Hs, Ws = (int(v) for v in frames.shape[-3:])
    Ho, Wo = _size2(size)
    F_src, F_out = frames.numel() // max(1, C * Hs * Ws), t.shape[0]
    L = _lib.lib()
    if frames.device.type != "cuda":
        raise _lib.BvcError("clip_transform runs on the GPU (clip_transform_host is the host twin); there is no CPU fallback")
    if out is None:
        out = torch.empty(F_out, 3, Ho, Wo, dtype=torch.uint8, device=frames.device)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != F_out * 3 * Ho * Wo or out.device != frames.device:
        raise ValueError("out must be a contiguous uint8 tensor of F_out * 3 * Ho * Wo elements on the frames' device")
    with torch.cuda.device(frames.device):
        staging = torch.empty(t.nbytes, dtype=torch.uint8, pin_memory=True)
        staging.numpy()[:] = t.view(np.uint8).reshape(-1)
        table_dev = staging.to(frames.device, non_blocking=True)
        work = torch.empty(max(1, int(L.bvc_op_clip_transform_workspace(F_out, Ho, Wo))), dtype=torch.uint8, device=frames.device)
        _lib.check(L.bvc_op_clip_transform(frames.data_ptr(), F_src, C, Hs, Ws, t.ctypes.data, table_dev.data_ptr(), F_out, Ho, Wo,
                                           out.data_ptr(), work.data_ptr(), _lib.current_stream_ptr()), "bvc_op_clip_transform")
        # the stream still reads these after the call returns: keep the caching allocator from handing them out on another stream
        table_dev.record_stream(torch.cuda.current_stream())
        work.record_stream(torch.cuda.current_stream())
    return out


class ClipTransform:
    """The reference's frame transform as one GPU stage: ``ClipTransform(size, augs)(clips)`` with uint8 device clips
    ``[B, T, 3, Hs, Ws]`` returns uint8 ``[views * B, T, 3, size, size]`` (view-major: the second SimCLR view of clip b is row
    ``B + b``).  Arguments as ``sample_params``; ``augs`` without 'c' (e.g. ``"n"``) gives VideoMAE's Resize + CenterCrop.
    ``rotation`` exists only to refuse: RandomRotation is ``ClipAugment``'s 'o'.  ``last_table`` keeps the table of the last call."""

    def __init__(self, size, augs="cjg", crop_scale=(0.08, 1.0), jitter_strength=0.5, flip=0.0, consistent=True, generator=None,
                 views=1, crop_ratio=(3.0 / 4.0, 4.0 / 3.0), jitter_p=0.8, gray_p=0.2, extra_gray_p=0.5, rotation=None):
        if rotation:
            raise ValueError("rotation (RandomRotation) is not part of ClipTransform: use ClipAugment with augs 'o'")
        if int(views) < 1:
            raise ValueError("views must be >= 1")
        self.size = _size2(size)
        self.views = int(views)
        self.kw = dict(augs=augs, crop_scale=crop_scale, crop_ratio=crop_ratio, jitter_strength=jitter_strength, jitter_p=jitter_p,
                       gray_p=gray_p, extra_gray_p=extra_gray_p, flip=flip, consistent=consistent)
        self.generator = generator if generator is not None else np.random.default_rng()
        sample_params(1, 1, self.size, self.size, generator=np.random.default_rng(0), **self.kw)      # argument errors surface here
        self.last_table = None

    def sample(self, batch, frames, src_size):
        return sample_params(batch, frames, src_size, self.size, views=self.views, generator=self.generator, **self.kw)

    def __call__(self, clips, table=None):
        _check_clips(clips)
        B, T, C, Hs, Ws = (int(v) for v in clips.shape)
        if C != 3:
            raise ValueError(f"clips have {C} channels; the transforms are defined for 3")
        table = self.sample(B, T, (Hs, Ws)) if table is None else table
        self.last_table = table
        return clip_transform(clips, table, self.size).view(-1, T, 3, *self.size)


# ---------------------------------------------------------------- post stage: blur, gray, rotation (bvc_frame_post)
def empty_post_table(n):
    """n identity entries: no blur (``blur_r = -1``), no gray, no rotation."""
    t = np.zeros(int(n), dtype=FRAME_POST)
    t["blur_r"] = -1
    return t


def blur_weights(radius):
    """bvc_aug_blur_weights: PIL's box radius and 8.24 weights ``(r, ww, fw)`` for a Gaussian radius in [0, MAX_BLUR_RADIUS]."""
    import ctypes
    r, ww, fw = ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_uint32()
    _lib.check(_lib.lib().bvc_aug_blur_weights(float(radius), ctypes.byref(r), ctypes.byref(ww), ctypes.byref(fw)), "bvc_aug_blur_weights")
    return int(r.value), int(ww.value), int(fw.value)


def rotation_coeffs(angle, size):
    """The six 16.16 coefficients a0 .. a5 of PIL's ``Image.rotate(angle, NEAREST, expand=False)`` on an ``size`` = (H, W) frame: the
    matrix as Image.rotate builds it (rounded to 15 places, about the centre (W / 2, H / 2)), fixed as ImagingTransform's affine_fixed
    fixes it (the half-pixel offset folded into a2 and a5)."""
    H, W = _size2(size)
    t = -math.radians(float(angle) % 360.0)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
    m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy
    return affine_coeffs(m)


def affine_coeffs(matrix):
    """The six 16.16 coefficients of PIL's ``Image.transform(size, AFFINE, matrix, NEAREST)``: ``matrix`` = (a, b, c, d, e, f) maps output
    (x, y) to source (a x + b y + c, d x + e y + f); fixed as ``rotation_coeffs`` fixes its matrix."""
    m = [float(v) for v in matrix]
    if len(m) != 6 or not all(math.isfinite(v) for v in m):
        raise ValueError("affine_coeffs: six finite values")

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))

    return (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def sample_post_params(batch, frames, size, augs, blur_p=0.5, blur_radius=(0.1, 2.0), degrees=(-90.0, 90.0), extra_gray_p=0.5,
                       consistent=True, views=1, generator=None):
    """Draw the post table for ``views`` x ``batch`` clips of ``frames`` frames of ``size``, entries in ``sample_params``' order.  Per
    clip (per frame with ``consistent=False``), in this order:
      'b'  GaussianBlur(p = blur_p): one draw decides, and if it holds a radius uniform in ``blur_radius``;
      'g'  together with 'b': the further RandomGrayscale(extra_gray_p), here because the reference applies it after the blur
           (without 'b' it folds into stage one's flag and ``sample_params`` draws it);
      'o'  RandomRotation(degrees): always an angle uniform in ``degrees`` (its RandomHorizontalFlip is stage one's ``flip``).
    Other letters of ``c j b g o n`` draw nothing here."""
    for ch in augs:
        if ch not in "cjbgon":
            raise ValueError(f"augs letter {ch!r} unknown (c, j, b, g, o, n)")
    if not (0.0 <= blur_p <= 1.0 and 0.0 <= extra_gray_p <= 1.0):
        raise ValueError("probabilities must lie in [0, 1]")
    if not (0.0 <= blur_radius[0] <= blur_radius[1] <= MAX_BLUR_RADIUS):
        raise ValueError(f"blur_radius must be an ascending range inside [0, {MAX_BLUR_RADIUS}]")
    if not (math.isfinite(degrees[0]) and math.isfinite(degrees[1]) and degrees[0] <= degrees[1]):
        raise ValueError("degrees must be an ascending finite range")
    g = generator if generator is not None else np.random.default_rng()
    B, T, V = int(batch), int(frames), int(views)
    H, W = _size2(size)
    table = empty_post_table(V * B * T)
    for first in range(0, V * B * T, T):
        for t in range(T):
            e = table[first + t]
            if consistent and t > 0:
                table[first + t] = table[first]
                continue
            if "b" in augs:
                if g.random() < blur_p:
                    e["blur_r"], e["blur_ww"], e["blur_fw"] = blur_weights(g.uniform(blur_radius[0], blur_radius[1]))
                if "g" in augs:
                    e["gray"] = int(g.random() < extra_gray_p)
            if "o" in augs:
                e["rotate"], e["rot"] = 1, rotation_coeffs(g.uniform(degrees[0], degrees[1]), (H, W))
    return table


def _check_post(frames, table):
    if frames.dtype != torch.uint8 or frames.dim() < 3 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous uint8 tensor [..., 3, H, W]")
    C, H, W = (int(v) for v in frames.shape[-3:])
    if C != 3:
        raise ValueError(f"frames have {C} channels; the post stage is defined for 3")
    t = np.ascontiguousarray(table)
    F = frames.numel() // max(1, 3 * H * W)
    if t.dtype != FRAME_POST or t.ndim != 1 or t.shape[0] != F or F < 1:
        raise ValueError(f"table must be a 1-d array of augment.FRAME_POST entries, one per frame ({F})")
    return t, F, H, W


def post_needed(table):
    """Whether any entry of a post table blurs, turns gray or rotates."""
    return bool(((table["blur_r"] >= 0) | (table["gray"] != 0) | (table["rotate"] != 0)).any())


def clip_post_host(frames, table):
    """bvc_clip_post_host: uint8 host frames ``[..., 3, H, W]`` and one FRAME_POST entry per frame -> a new tensor of the same shape:
    blur, then gray, then rotation.  No GPU needed."""
    if frames.device.type != "cpu":
        raise ValueError("frames must be a host tensor")
    t, F, H, W = _check_post(frames, table)
    out = torch.empty_like(frames)
    _lib.check(_lib.lib().bvc_clip_post_host(frames.data_ptr(), t.ctypes.data, F, H, W, out.data_ptr()), "bvc_clip_post_host")
    return out


def clip_post(frames, table, out=None):
    """bvc_op_clip_post on the current stream: uint8 device frames ``[..., 3, H, W]`` and a host table with one FRAME_POST entry per
    frame -> uint8 frames of the same shape (``out``: a contiguous uint8 device tensor of as many bytes that shares no memory with
    ``frames``; it is returned as it is).  The table travels through pinned memory in one asynchronous copy; nothing synchronises."""
    t, F, H, W = _check_post(frames, table)
    L = _lib.lib()
    if frames.device.type != "cuda":
        raise _lib.BvcError("clip_post runs on the GPU (clip_post_host is the host twin); there is no CPU fallback")
    if out is None:
        out = torch.empty_like(frames)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != frames.numel() or out.device != frames.device:
        raise ValueError("out must be a contiguous uint8 tensor of as many elements as frames, on their device")
    both = bool(((t["blur_r"] >= 0) | (t["gray"] != 0)).any()) and bool((t["rotate"] != 0).any())
    with torch.cuda.device(frames.device):
        staging = torch.empty(t.nbytes, dtype=torch.uint8, pin_memory=True)
        staging.numpy()[:] = t.view(np.uint8).reshape(-1)
        table_dev = staging.to(frames.device, non_blocking=True)
        # the frames between the two kernels: needed only when the table asks for both
        work = torch.empty(max(4, int(L.bvc_op_clip_post_workspace(F, H, W)) if both else 4), dtype=torch.uint8, device=frames.device)
        _lib.check(L.bvc_op_clip_post(frames.data_ptr(), t.ctypes.data, table_dev.data_ptr(), F, H, W, out.data_ptr(), work.data_ptr(),
                                      _lib.current_stream_ptr()), "bvc_op_clip_post")
        # the stream still reads these after the call returns: keep the caching allocator from handing them out on another stream
        table_dev.record_stream(torch.cuda.current_stream())
        work.record_stream(torch.cuda.current_stream())
    return out


class ClipAugment:
    """The reference's whole ``--augs`` letter set as GPU stages: ``ClipAugment(size, augs)(clips)`` with uint8 device clips
    ``[B, T, 3, Hs, Ws]`` returns uint8 ``[views * B, T, 3, size, size]``, view-major as ``ClipTransform``.  Letters ``c j b g o n``.
    Each call draws the stage-one table with ``sample_params`` first, for the whole batch (letters c, j, n, and g when 'b' is absent;
    ``flip`` defaults to 0.5 with 'o', RandomRotation's companion flip, and to 0 otherwise), then the post table with
    ``sample_post_params``; it runs ``clip_transform`` and, only if some entry blurs, turns gray or rotates, ``clip_post``.  With
    letters from ``c j g n`` alone and the same seed it returns exactly what ``ClipTransform`` returns.  ``last_table`` and
    ``last_post_table`` keep the tables of the last call.

    ``randaug``: ``None`` (the default) draws nothing more and launches nothing more.  A ``RandAugment``, or a config string such as
    ``"rand-m7-n4-mstd0.5-inc1"``, runs as the last stage on the ``[views * B, T, 3, size, size]`` clips: its table is drawn from this
    object's generator after the two others (``sample`` then returns three tables, ``last_randaug_table`` keeps the third)."""

    def __init__(self, size, augs="cjo", crop_scale=(0.08, 1.0), jitter_strength=0.5, flip=None, consistent=True, generator=None,
                 views=1, crop_ratio=(3.0 / 4.0, 4.0 / 3.0), jitter_p=0.8, gray_p=0.2, extra_gray_p=0.5, blur_p=0.5,
                 blur_radius=(0.1, 2.0), degrees=(-90.0, 90.0), randaug=None):
        if int(views) < 1:
            raise ValueError("views must be >= 1")
        for ch in augs:
            if ch not in "cjbgon":
                raise ValueError(f"augs letter {ch!r} unknown (c, j, b, g, o, n)")
        self.size = _size2(size)
        self.views = int(views)
        self.augs = augs
        first = "".join(ch for ch in augs if ch in "cjn" or (ch == "g" and "b" not in augs))
        self.kw = dict(augs=first, crop_scale=crop_scale, crop_ratio=crop_ratio, jitter_strength=jitter_strength, jitter_p=jitter_p,
                       gray_p=gray_p, extra_gray_p=extra_gray_p, flip=(0.5 if "o" in augs else 0.0) if flip is None else flip,
                       consistent=consistent)
        self.post_kw = dict(augs=augs, blur_p=blur_p, blur_radius=blur_radius, degrees=degrees, extra_gray_p=extra_gray_p,
                            consistent=consistent)
        self.generator = generator if generator is not None else np.random.default_rng()
        sample_params(1, 1, self.size, self.size, generator=np.random.default_rng(0), **self.kw)      # argument errors surface here
        sample_post_params(1, 1, self.size, generator=np.random.default_rng(0), **self.post_kw)
        if randaug is not None and not isinstance(randaug, RandAugment):
            randaug = RandAugment(randaug, consistent=consistent)
        self.randaug = randaug
        self.last_table = self.last_post_table = self.last_randaug_table = None

    def sample(self, batch, frames, src_size):
        """(stage-one table, post table) for one batch, drawn in that order from the generator; with ``randaug`` a third table after them"""
        table = sample_params(batch, frames, src_size, self.size, views=self.views, generator=self.generator, **self.kw)
        post = sample_post_params(batch, frames, self.size, views=self.views, generator=self.generator, **self.post_kw)
        if self.randaug is None:
            return table, post
        return table, post, self.randaug.sample(batch, frames, self.size, views=self.views, generator=self.generator)

    def __call__(self, clips, tables=None):
        _check_clips(clips)
        B, T, C, Hs, Ws = (int(v) for v in clips.shape)
        if C != 3:
            raise ValueError(f"clips have {C} channels; the transforms are defined for 3")
        tables = self.sample(B, T, (Hs, Ws)) if tables is None else tuple(tables)
        if len(tables) != (2 if self.randaug is None else 3):
            raise ValueError("tables: (stage-one table, post table), and the RandAugment table when randaug is set")
        table, post = tables[:2]
        self.last_table, self.last_post_table = table, post
        out = clip_transform(clips, table, self.size)
        if post_needed(post):
            out = clip_post(out, post)
        if self.randaug is not None:
            self.last_randaug_table = tables[2]
            out = rand_augment(out, tables[2])
        return out.view(-1, T, 3, *self.size)


# ---------------------------------------------------------------- RandAugment (bvc_frame_randaug)
_RA_ID = {name: i for i, name in enumerate(RANDAUG_OPS)}
_RA_SIGNED = frozenset(("Color", "Contrast", "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"))
_RA_ENHANCE = ("Color", "Contrast", "Brightness", "Sharpness")
_RA_INT_RANGE = {"Posterize": 8, "Solarize": 256, "SolarizeAdd": 110}


def _ra_name(op):
    if isinstance(op, str):
        if op not in _RA_ID:
            raise ValueError(f"RandAugment op {op!r} unknown ({', '.join(RANDAUG_OPS)})")
        return op
    if not 0 <= int(op) < len(RANDAUG_OPS):
        raise ValueError(f"RandAugment op id {op} unknown (0 .. {len(RANDAUG_OPS) - 1})")
    return RANDAUG_OPS[int(op)]


def empty_randaug_table(n):
    """n identity entries: no stages, fill 0."""
    return np.zeros(int(n), dtype=FRAME_RANDAUG)


def randaug_stage(op, param, size):
    """One RANDAUG_STAGE record for ``op`` (a name of RANDAUG_OPS or its id) on frames of ``size`` = (H, W).  ``param`` is PIL's own
    argument: bits (Posterize), threshold (Solarize), the added value (SolarizeAdd), the enhancement factor (Color, Contrast,
    Brightness, Sharpness), the shear factor (ShearX, ShearY: the matrix entry), pixels (TranslateX, TranslateY: the matrix entry),
    degrees (Rotate); ignored by AutoContrast, Equalize and Invert."""
    name = _ra_name(op)
    H, W = _size2(size)
    st = np.zeros((), dtype=RANDAUG_STAGE)
    st["op"] = _RA_ID[name]
    if name in _RA_INT_RANGE:
        if int(param) != param or not 0 <= int(param) <= _RA_INT_RANGE[name]:
            raise ValueError(f"{name}: ival {param!r} outside 0 .. {_RA_INT_RANGE[name]}")
        st["ival"] = int(param)
    elif name in _RA_ENHANCE:
        if not (math.isfinite(param) and param >= 0):
            raise ValueError(f"{name}: fval {param!r} must be finite and >= 0")
        st["fval"] = param
    elif name == "Rotate":
        st["aff"] = rotation_coeffs(param, (H, W))
    elif name in _RA_SIGNED:
        p = float(param)
        st["aff"] = affine_coeffs({"ShearX": (1.0, p, 0.0, 0.0, 1.0, 0.0), "ShearY": (1.0, 0.0, 0.0, p, 1.0, 0.0),
                                   "TranslateX": (1.0, 0.0, p, 0.0, 1.0, 0.0), "TranslateY": (1.0, 0.0, 0.0, 0.0, 1.0, p)}[name])
    return st


def randaug_entry(stages, size, fill=(124, 116, 104)):
    """One FRAME_RANDAUG record from a list of ``(op, param)`` (see ``randaug_stage``), applied in that order."""
    stages = list(stages)
    if len(stages) > RANDAUG_MAX_OPS:
        raise ValueError(f"an entry holds at most {RANDAUG_MAX_OPS} stages, got {len(stages)}")
    e = np.zeros((), dtype=FRAME_RANDAUG)
    e["nops"] = len(stages)
    e["fill"][:3] = [int(v) for v in fill]
    for i, (op, param) in enumerate(stages):
        e["stage"][i] = randaug_stage(op, param, size)
    return e


def _ra_param(name, level, sign, H, W):
    """the "increasing" magnitude maps: level in [0, 1] -> the op's parameter"""
    if name == "Rotate":
        return sign * 30.0 * level
    if name in ("ShearX", "ShearY"):
        return sign * 0.3 * level
    if name == "TranslateX":
        return sign * 0.45 * level * W
    if name == "TranslateY":
        return sign * 0.45 * level * H
    if name in _RA_ENHANCE:
        return max(0.1, 1.0 + sign * 0.9 * level)
    if name == "Posterize":
        return 4 - int(4 * level)
    if name == "Solarize":
        return 256 - int(256 * level)
    if name == "SolarizeAdd":
        return int(110 * level)
    return None


def sample_randaug_params(batch, frames, size, num_ops=4, magnitude=7.0, magnitude_std=0.5, prob=0.5, ops=None, fill=(124, 116, 104),
                          consistent=True, views=1, generator=None):
    """Draw the RandAugment table for ``views`` x ``batch`` clips of ``frames`` frames of ``size``, entries in ``sample_params``' order.
    Per clip (per frame with ``consistent=False``), ``num_ops`` times in turn:
      * an op, uniform with replacement from ``ops`` (names or ids; default all of RANDAUG_OPS);
      * a uniform draw; only below ``prob`` does the op apply - otherwise it adds no stage and nothing more is drawn for it;
      * ``level = clip(normal(magnitude, magnitude_std), 0, 10) / 10``;
      * for the signed ops (the geometric ones and the four enhancers) a sign, negative with probability 1/2.
    Level to parameter, the "increasing" set: Rotate +-30 level degrees; ShearX / ShearY +-0.3 level; TranslateX / TranslateY
    +-0.45 level x W / H pixels (floats); Color, Contrast, Brightness, Sharpness f = max(0.1, 1 +- 0.9 level); Posterize
    bits = 4 - int(4 level); Solarize thresh = 256 - int(256 level); SolarizeAdd add = int(110 level); AutoContrast, Equalize and Invert
    take none.  Pixels that a geometric op leaves uncovered take ``fill`` (r, g, b).

    The draws come from a ``numpy.random.Generator``: the same seed gives the same table, but the stream is this project's own - it is
    not the stream of timm, torchvision or any other library."""
    B, T, V, K = int(batch), int(frames), int(views), int(num_ops)
    if not 0 <= K <= RANDAUG_MAX_OPS:
        raise ValueError(f"num_ops must lie in 0 .. {RANDAUG_MAX_OPS}")
    if not (0.0 <= prob <= 1.0):
        raise ValueError("prob must lie in [0, 1]")
    if not (0.0 <= magnitude <= 10.0 and magnitude_std >= 0.0 and math.isfinite(magnitude_std)):
        raise ValueError("magnitude must lie in [0, 10] and magnitude_std be finite and >= 0")
    names = [_ra_name(op) for op in (RANDAUG_OPS if ops is None else ops)]
    if not names:
        raise ValueError("ops must name at least one op")
    if len(fill) != 3 or not all(0 <= int(v) <= 255 for v in fill):
        raise ValueError("fill must be three values in 0 .. 255")
    g = generator if generator is not None else np.random.default_rng()
    H, W = _size2(size)
    table = empty_randaug_table(V * B * T)
    for first in range(0, V * B * T, T):
        for t in range(T):
            if consistent and t > 0:
                table[first + t] = table[first]
                continue
            stages = []
            for _ in range(K):
                name = names[int(g.integers(0, len(names)))]
                if not g.random() < prob:
                    continue
                level = min(max(float(g.normal(magnitude, magnitude_std)), 0.0), 10.0) / 10.0
                sign = (-1.0 if g.random() < 0.5 else 1.0) if name in _RA_SIGNED else 1.0
                stages.append((name, _ra_param(name, level, sign, H, W)))
            table[first + t] = randaug_entry(stages, (H, W), fill=fill)
    return table


_RA_FIELDS = {"m": "magnitude", "n": "num_ops", "mstd": "magnitude_std", "p": "prob"}


def parse_randaug(config):
    """``"rand-m7-n4-mstd0.5-inc1"`` -> the keyword dict for ``sample_randaug_params`` / ``RandAugment``.  Fields: ``m`` magnitude,
    ``n`` num_ops, ``mstd`` magnitude_std, ``p`` prob, and ``inc1`` (the increasing magnitude maps: the only set there is, so it adds
    nothing).  Any other field - ``inc0`` among them - is refused by name."""
    parts = str(config).split("-")
    if parts[0] != "rand":
        raise ValueError(f"parse_randaug: {config!r} does not start with 'rand'")
    kw = {}
    for part in parts[1:]:
        if part == "inc1":
            continue
        for key in ("mstd", "m", "n", "p"):
            if part.startswith(key) and len(part) > len(key) and (part[len(key)].isdigit() or part[len(key)] == "."):
                try:
                    value = float(part[len(key):])
                except ValueError:
                    raise ValueError(f"parse_randaug: field {part!r} has no number") from None
                kw[_RA_FIELDS[key]] = int(value) if key == "n" and value == int(value) else value
                break
        else:
            raise ValueError(f"parse_randaug: field {part!r} is not supported (m, n, mstd, p, inc1)")
    return kw


def format_randaug(num_ops=4, magnitude=7.0, magnitude_std=0.5, prob=0.5):
    """the config string that ``parse_randaug`` turns back into these keywords"""
    return f"rand-m{magnitude:g}-n{int(num_ops)}-mstd{magnitude_std:g}-p{prob:g}-inc1"


_ra_size_checked = False


def _check_randaug(frames, table):
    global _ra_size_checked
    if not _ra_size_checked:
        n = int(_lib.lib().bvc_frame_randaug_bytes())
        if n != FRAME_RANDAUG.itemsize:
            raise _lib.BvcError(f"bvc_frame_randaug is {n} bytes in the library, FRAME_RANDAUG {FRAME_RANDAUG.itemsize}")
        _ra_size_checked = True
    if frames.dtype != torch.uint8 or frames.dim() < 3 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous uint8 tensor [..., 3, H, W]")
    C, H, W = (int(v) for v in frames.shape[-3:])
    if C != 3:
        raise ValueError(f"frames have {C} channels; RandAugment is defined for 3")
    t = np.ascontiguousarray(table)
    F = frames.numel() // max(1, 3 * H * W)
    if t.dtype != FRAME_RANDAUG or t.ndim != 1 or t.shape[0] != F or F < 1:
        raise ValueError(f"table must be a 1-d array of augment.FRAME_RANDAUG entries, one per frame ({F})")
    return t, F, H, W


def rand_augment_host(frames, table):
    """bvc_clip_randaug_host: uint8 host frames ``[..., 3, H, W]`` and one FRAME_RANDAUG entry per frame -> a new tensor of the same
    shape, every frame through its stages in order.  No GPU needed."""
    if frames.device.type != "cpu":
        raise ValueError("frames must be a host tensor")
    t, F, H, W = _check_randaug(frames, table)
    out = torch.empty_like(frames)
    _lib.check(_lib.lib().bvc_clip_randaug_host(frames.data_ptr(), t.ctypes.data, F, H, W, out.data_ptr()), "bvc_clip_randaug_host")
    return out


def rand_augment(frames, table, out=None, workspace=None):
    """bvc_op_clip_randaug on the current stream: uint8 device frames ``[..., 3, H, W]`` and a host table with one FRAME_RANDAUG entry
    per frame -> uint8 frames of the same shape (``out``: a contiguous uint8 device tensor of as many bytes that shares no memory with
    ``frames``; it is returned as it is.  ``workspace``: a uint8 device tensor of at least ``bvc_op_clip_randaug_workspace`` bytes to
    use instead of a fresh one).  The table travels through pinned memory in one asynchronous copy; nothing synchronises."""
    t, F, H, W = _check_randaug(frames, table)
    L = _lib.lib()
    if frames.device.type != "cuda":
        raise _lib.BvcError("rand_augment runs on the GPU (rand_augment_host is the host twin); there is no CPU fallback")
    if out is None:
        out = torch.empty_like(frames)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != frames.numel() or out.device != frames.device:
        raise ValueError("out must be a contiguous uint8 tensor of as many elements as frames, on their device")
    need = int(L.bvc_op_clip_randaug_workspace(F, H, W)) if bool((t["nops"] != 0).any()) else 4
    if workspace is not None and (workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need or
                                  workspace.device != frames.device):
        raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {need} elements on the frames' device")
    with torch.cuda.device(frames.device):
        staging = torch.empty(t.nbytes, dtype=torch.uint8, pin_memory=True)
        staging.numpy()[:] = t.view(np.uint8).reshape(-1)
        table_dev = staging.to(frames.device, non_blocking=True)
        work = torch.empty(need, dtype=torch.uint8, device=frames.device) if workspace is None else workspace
        _lib.check(L.bvc_op_clip_randaug(frames.data_ptr(), t.ctypes.data, table_dev.data_ptr(), F, H, W, out.data_ptr(), work.data_ptr(),
                                         _lib.current_stream_ptr()), "bvc_op_clip_randaug")
        # the stream still reads these after the call returns: keep the caching allocator from handing them out on another stream
        table_dev.record_stream(torch.cuda.current_stream())
        work.record_stream(torch.cuda.current_stream())
    return out


class RandAugment:
    """RandAugment as one GPU stage: ``RandAugment("rand-m7-n4-mstd0.5-inc1")(clips)`` with uint8 device clips ``[B, T, 3, H, W]``
    returns uint8 clips of the same shape.  ``config`` (see ``parse_randaug``) sets ``num_ops``, ``magnitude``, ``magnitude_std`` and
    ``prob`` over the keyword arguments; the others are ``sample_randaug_params``'.  ``last_table`` keeps the table of the last call."""

    def __init__(self, config=None, num_ops=4, magnitude=7.0, magnitude_std=0.5, prob=0.5, ops=None, fill=(124, 116, 104),
                 consistent=True, generator=None):
        self.kw = dict(num_ops=num_ops, magnitude=magnitude, magnitude_std=magnitude_std, prob=prob, ops=ops, fill=tuple(fill),
                       consistent=consistent)
        if config is not None:
            self.kw.update(parse_randaug(config))
        self.generator = generator if generator is not None else np.random.default_rng()
        sample_randaug_params(1, 1, 8, generator=np.random.default_rng(0), **self.kw)      # argument errors surface here
        self.last_table = None

    def sample(self, batch, frames, size, views=1, generator=None):
        return sample_randaug_params(batch, frames, size, views=views, generator=self.generator if generator is None else generator,
                                     **self.kw)

    def __call__(self, clips, table=None):
        _check_clips(clips)
        B, T, C, H, W = (int(v) for v in clips.shape)
        if C != 3:
            raise ValueError(f"clips have {C} channels; RandAugment is defined for 3")
        table = self.sample(B, T, (H, W)) if table is None else table
        self.last_table = table
        return rand_augment(clips, table)
