"""Plain numpy / torch restatement of random erasing inside the patch gather (include/bvc.h, bvc_erase_box): the counter function
(Philox4x32-10), the Box-Muller normals in float64 and in the kernel's own f32 arithmetic, and the composition of erased clips."""
import numpy as np
import torch

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TAG_PIXEL, TAG_COLOUR = 0xE0, 0xE1


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of 32-bit counter words (uint64 arrays holding 32-bit values) under one key; returns four uint64
    arrays of 32-bit outputs."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c1, c3, c0, c2 = p1 & MASK, p0 & MASK, n0, n2
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def draws(seed, offset, q, tag):
    """the four outputs of counter {low q, high q | tag << 16, low offset, high offset} under key = the halves of seed; q an array"""
    q = np.asarray(q, dtype=np.uint64)
    seed, offset = int(seed), int(offset)
    return philox4x32_10(q & MASK, (q >> np.uint64(32)) | np.uint64(tag << 16), offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32)


def normals(r, dtype=np.float64):
    """[..., 4] normals of the four outputs r = (r0, r1, r2, r3): lanes 0 / 1 the cos / sin branch of Box-Muller on (r0, r1), lanes
    2 / 3 on (r2, r3); u1 = ((ra >> 8) + 1) 2^-24, u2 = (rb >> 8) 2^-24, z = sqrt(-2 ln u1) {cos, sin}(2 pi u2).  dtype float64 is the
    reference; float32 evaluates the same formula with every operation in f32, as the kernel does."""
    out = []
    for ra, rb in ((r[0], r[1]), (r[2], r[3])):
        u1 = (((ra >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24).astype(dtype)      # exact in f32
        u2 = ((rb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(dtype)
        rad = np.sqrt(dtype(-2.0) * np.log(u1))
        ang = dtype(2.0 * np.pi) * u2
        out += [rad * np.cos(ang), rad * np.sin(ang)]
    return np.stack(out, axis=-1)


def pixel_noise(seed, offset, B, T, C, H, W, dtype=np.float64):
    """[B, T, C, H, W]: element e = (((s T + t) C + c) H + y) W + x takes lane e & 3 of the call with q = e >> 2"""
    n = B * T * C * H * W
    assert n % 4 == 0
    return normals(draws(seed, offset, np.arange(n // 4, dtype=np.uint64), TAG_PIXEL), dtype).reshape(B, T, C, H, W)


def colours(seed, offset, B, T, dtype=np.float64):
    """[B, T, 4 boxes, 4 channels]: e = ((s T + t) 4 + j) 4 + c"""
    return normals(draws(seed, offset, np.arange(B * T * 4, dtype=np.uint64), TAG_COLOUR), dtype).reshape(B, T, 4, 4)


def erase_clips(f32_clips, boxes, modes, noise, colours):
    """f32_clips [B, T, C, H, W]; boxes [B][n] of (y0, y1, x0, x1), modes [B][n] (0 const, 1 rand, 2 pixel); noise [B, T, C, H, W]
    and colours [B, T, 4, 4] f32 tensors.  Box after box, so the later one wins; the same box in every frame."""
    out = f32_clips.to(torch.float32).clone()
    C = out.shape[2]
    for b in range(out.shape[0]):
        for j, (box, mode) in enumerate(zip(boxes[b], modes[b])):
            y0, y1, x0, x1 = (int(v) for v in box)
            if y1 <= y0 or x1 <= x0:
                continue
            if int(mode) == 0:
                out[b, :, :, y0:y1, x0:x1] = 0.0
            elif int(mode) == 1:
                out[b, :, :, y0:y1, x0:x1] = colours[b, :, j, :C].to(out.dtype)[:, :, None, None]
            else:
                out[b, :, :, y0:y1, x0:x1] = noise[b, :, :, y0:y1, x0:x1].to(out.dtype)
    return out
