"""Host-side VideoMAE mask samplers with the interface of pretraining/generative/mask.py: ``Generator((T, H, W), ratio)()``
returns a flat float64 vector of T*H*W zeros (visible) and ones (masked), which the step turns into a bool tensor
(pretrain_videomae.py:294-298).

The draws follow the reference's random stream (one in-place ``shuffle`` of a "visible first, masked last" vector per call)
so that a seeded run reproduces its masks; ``rng`` selects a private ``numpy.random.RandomState`` instead of the global one
the reference uses.  Fixture: tests/golden/tube_mask.json.
"""
import numpy as np


def _shuffled_flags(count, masked, rng):
    """`count` flags, the last `masked` of them set, permuted in place by the chosen generator."""
    flags = (np.arange(count) >= count - masked).astype(np.float64)
    (np.random if rng is None else rng).shuffle(flags)
    return flags


class TubeMaskingGenerator:
    """One spatial mask per clip, repeated over every temporal slot (a "tube")."""

    def __init__(self, input_size, mask_ratio, rng=None):
        slots, rows, cols = input_size
        self.slots, self.per_slot = slots, rows * cols
        self.masked_per_slot = int(mask_ratio * self.per_slot)
        self.rng = rng

    @property
    def total_patches(self):
        return self.slots * self.per_slot

    @property
    def total_masks(self):
        return self.slots * self.masked_per_slot

    def __repr__(self):
        return f"TubeMaskingGenerator({self.total_masks} of {self.total_patches} tokens masked)"

    def __call__(self):
        spatial = _shuffled_flags(self.per_slot, self.masked_per_slot, self.rng)
        return np.broadcast_to(spatial, (self.slots, self.per_slot)).reshape(-1).copy()


class RandomMaskingGenerator:
    """Independent mask over all T*H*W tokens."""

    def __init__(self, input_size, mask_ratio, rng=None):
        dims = input_size if isinstance(input_size, tuple) else (input_size,) * 3
        self.num_patches = int(np.prod(dims))
        self.num_mask = int(mask_ratio * self.num_patches)
        self.rng = rng

    def __repr__(self):
        return f"RandomMaskingGenerator({self.num_mask} of {self.num_patches} tokens masked)"

    def __call__(self):
        return _shuffled_flags(self.num_patches, self.num_mask, self.rng)


class DecoderSubsetGenerator:
    """The masked tokens the decoder reconstructs (``bool_decode_pos`` of VideoMAEForPreTraining.forward): called with a mask from
    ``TubeMaskingGenerator``, it keeps ``int(decode_ratio * masked_per_frame)`` of every temporal slot's masked positions and returns
    the flat vector of T*H*W zeros and ones.  The draw (one ``shuffle`` per slot, from the same generator the tube mask uses) is fresh
    for every slot, so over time every position of a tube is reconstructed, and every clip decodes the same number of tokens.

    This is decoder masking in the sense of VideoMAE V2 (Wang et al., CVPR 2023, section 3.2) but NOT its running-cell generator, whose
    source was not available when this was written; the model accepts any mask that is a subset of the encoder mask with one count per
    clip."""

    def __init__(self, input_size, decode_ratio, rng=None):
        slots, rows, cols = input_size
        if not 0.0 < decode_ratio <= 1.0:
            raise ValueError(f"decode_ratio={decode_ratio} must lie in (0, 1]")
        self.slots, self.per_slot = slots, rows * cols
        self.decode_ratio = decode_ratio
        self.rng = rng

    def __repr__(self):
        return f"DecoderSubsetGenerator({self.decode_ratio} of the masked tokens of each of {self.slots} slots decoded)"

    def __call__(self, mask):
        masked = np.asarray(mask).reshape(self.slots, self.per_slot) != 0
        per_slot = masked.sum(axis=1)
        if not (per_slot == per_slot[0]).all():
            raise ValueError("every temporal slot must mask the same number of positions (a tube mask)")
        keep = int(self.decode_ratio * int(per_slot[0]))
        if keep < 1:
            raise ValueError(f"decode_ratio={self.decode_ratio} keeps none of the {int(per_slot[0])} masked positions of a slot")
        out = np.zeros((self.slots, self.per_slot), dtype=np.float64)
        for t in range(self.slots):
            positions = np.flatnonzero(masked[t])
            out[t, positions[_shuffled_flags(len(positions), keep, self.rng) != 0]] = 1.0
        return out.reshape(-1)
