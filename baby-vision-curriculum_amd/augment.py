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
    ``last_post_table`` keep the tables of the last call."""

    def __init__(self, size, augs="cjo", crop_scale=(0.08, 1.0), jitter_strength=0.5, flip=None, consistent=True, generator=None,
                 views=1, crop_ratio=(3.0 / 4.0, 4.0 / 3.0), jitter_p=0.8, gray_p=0.2, extra_gray_p=0.5, blur_p=0.5,
                 blur_radius=(0.1, 2.0), degrees=(-90.0, 90.0)):
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
        self.last_table = self.last_post_table = None

    def sample(self, batch, frames, src_size):
        """(stage-one table, post table) for one batch, drawn in that order from the generator"""
        table = sample_params(batch, frames, src_size, self.size, views=self.views, generator=self.generator, **self.kw)
        post = sample_post_params(batch, frames, self.size, views=self.views, generator=self.generator, **self.post_kw)
        return table, post

    def __call__(self, clips, tables=None):
        _check_clips(clips)
        B, T, C, Hs, Ws = (int(v) for v in clips.shape)
        if C != 3:
            raise ValueError(f"clips have {C} channels; the transforms are defined for 3")
        table, post = self.sample(B, T, (Hs, Ws)) if tables is None else tables
        self.last_table, self.last_post_table = table, post
        out = clip_transform(clips, table, self.size)
        if post_needed(post):
            out = clip_post(out, post)
        return out.view(-1, T, 3, *self.size)
