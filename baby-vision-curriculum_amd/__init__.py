"""bvc_amd -- MI355X-native (gfx950) self-supervised video pre-training step.

The directory is named ``baby-vision-curriculum_amd`` (not importable as such); it is registered under
the alias ``bvc_amd`` by ``__graft_entry__.load_package()``.

Host-side mirror of the model interface the reference's entry points use
(pretraining/generative/pretrain_videomae.py:61-64,301-302): ``VideoMAEConfig`` /
``VideoMAEForPreTraining`` with transformers' state-dict keys, whose arithmetic runs in
``libbvc_hip.so`` (hand-written HIP, C ABI in ``include/bvc.h``).  PyTorch is used for device
memory, streams, the optimiser object and torch.distributed only.
"""
from . import _lib, _ops  # noqa: F401
from ._ops import attention_probs  # noqa: F401
from ._lib import use_deterministic_algorithms, are_deterministic_algorithms_enabled  # noqa: F401
from .videomae import (VideoMAEConfig, VideoMAEForPreTraining, VideoMAEForPreTrainingOutput, VideoMAEForVideoClassification,  # noqa: F401
                       get_config, get_model, VIDEOMAE_ARCHS, videomae_config, soft_target_cross_entropy)
from .mixup import Mixup, ClipMix  # noqa: F401
from .erase import RandomErasing, ClipErase, erase_noise  # noqa: F401
from .mask import TubeMaskingGenerator, RandomMaskingGenerator, DecoderSubsetGenerator  # noqa: F401
from .ddp import DistributedDataParallel  # noqa: F401
from .ddputils import AllReduce  # noqa: F401
from .loggingtools import grad_logger  # noqa: F401
from . import optim, amp  # noqa: F401
from . import dropgate  # noqa: F401
from . import augment  # noqa: F401
from .augment import ClipAugment, ClipTransform  # noqa: F401
from .augment import (FRAME_RANDAUG, RANDAUG_OPS, RandAugment, empty_randaug_table, parse_randaug, rand_augment,  # noqa: F401
                      rand_augment_host, sample_randaug_params)
from . import simclr, distributed, jepa, jepa_mask, checkpoint, launch, comm, probe, retrieval, separability, attentive, xcorr  # noqa: F401
from .attentive import AttentiveClassifier, AttentivePooler, attentive_pool  # noqa: F401
from . import dino  # noqa: F401
from .dino import DINOHead, DINOLoss, dino_loss, prototype_ce, update_teacher  # noqa: F401
from . import input as input_pipeline  # noqa: F401
from .input import ClipUploadRing  # noqa: F401
from . import jpeg  # noqa: F401
from .jpeg import JpegClipRing, JpegUnsupported  # noqa: F401
