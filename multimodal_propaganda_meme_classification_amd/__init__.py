"""MI355X-native dual-encoder fine-tuning path for Subtask-2C meme classification.

Host side is Python (the reference is Python); all arithmetic runs in hand-written HIP kernels
for gfx950 behind the C ABI in include/memehip.h (libmemehip.so).  No CPU fallback.
"""
from . import _lib  # noqa: F401
from ._lib import MemehipError  # noqa: F401
from .config import ImageConfig, Layout, ModelConfig, TextConfig  # noqa: F401
from .model import (Adam, BatchNorm1d, BCEWithLogitsLoss, CrossEntropyLoss, GradScaler, GraphedStep, MultimodalClassifier,  # noqa: F401
                    SigmoidFocalLoss, TextEncoder, balanced_class_weights, flatten_parameters, get_linear_schedule_with_warmup)
from . import fused  # noqa: F401
from .heads import (MCA3, ConcatAttention3, FineTuneMLP, KevinMultimodalClassifier, LinearBNReLU,  # noqa: F401
                    OrganizersMultimodalClassifier, ResNeXt50_32x4d_BH, SEResNeXt50_32x4d_BH, SequencePooling, TextClassifier,
                    TrainerModel)
from .data import HashTokenizer, MultimodalDataset, id2l, l2id, normalize_images, read_data  # noqa: F401
from .train import evaluate, test, train  # noqa: F401
from . import kevin  # noqa: F401
from .kevin import BlipImageCaptioning, KevinMultimodalDataset, blip_caption_fn, kevin_collate  # noqa: F401
from .blip import BlipCaptioner  # noqa: F401
from .resnet import (BasicBlock, Bottleneck, HFResNetForImageClassification, ResNet18, ResNet34, ResNet50, ResNetClassifier,  # noqa: F401
                     ResNeXt50_32x4d, SEModule, SEResNeXt50_32x4d, TowerOptions)
from .convnext import CNBlock, ConvNeXtTiny  # noqa: F401
from .features import dump_features, get_features  # noqa: F401
from . import svm  # noqa: F401
from .svm import SVC  # noqa: F401
from . import baselines  # noqa: F401
from .baselines import run_image_baseline, run_imgbert_baseline  # noqa: F401
